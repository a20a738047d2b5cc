"""The optimizer hyper-parameter record on its way from the updaters to the kernels, without a GPU.

    test_hyper_vec_*          ops.hyper_vec, the one Python packer: order, flags, defaults, unknown keys
    test_header_*             csrc/include/psamd_opt_hyper.h through csrc/tests/opt_hyper_test.cpp, a host
                              program built here under the address and undefined-behaviour sanitizers:
                              the C++ name table against ops.HYPER_FIELDS, the decode of 1..16 field by
                              field, the refusal of a short vector (the program's exit status), and
                              opt_bias_correct against numpy on the float32 betas

Bias correction bounds.  Mode 0 (bc1 / bc2 as given) and mode 2 (1.f / (1.f - beta), three float32 operations
numpy repeats) are compared bit for bit.  Mode 1 is float32(1.0 / (1.0 - pow(beta, step))) in double: two pow
implementations may differ in the last bit of the double, which moves the rounded float32 by one ulp at the
most: 2^-23 relative.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ps_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("lr", "beta1", "beta2", "eps", "wd", "momentum", "dampening", "nesterov", "adamw", "bc1", "bc2", "l1", "l2",
          "fbeta", "ftrl_mode", "gscale")
STEPS = (1, 2, 1000)


def test_hyper_vec_order():
    assert ops.HYPER_FIELDS == FIELDS
    hp = {k: (bool(i % 2) if k in ("nesterov", "adamw") else i + 1) for i, k in enumerate(FIELDS)}
    assert hp["nesterov"] is True and hp["adamw"] is False
    want = [float(i + 1) for i in range(16)]
    want[7], want[8] = 1.0, 0.0
    got = ops.hyper_vec(hp)
    assert got == want and all(type(x) is float for x in got)
    # every flag value at its own position
    assert ops.hyper_vec(dict(hp, nesterov=False, adamw=True))[7:9] == [0.0, 1.0]


def test_hyper_vec_defaults_and_unknown_keys():
    assert ops.hyper_vec({}) == [0.01, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    assert ops.hyper_vec(dict(lr=0.5))[0] == 0.5 and ops.hyper_vec(dict(lr=0.5))[1:] == ops.hyper_vec({})[1:]
    with pytest.raises(TypeError):
        ops.hyper_vec(dict(lr=0.1, learning_rate=0.1))


@pytest.fixture(scope="module")
def header_program(tmp_path_factory):
    """stdout lines of csrc/tests/opt_hyper_test.cpp; its own checks passed (exit status 0)."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++") or shutil.which("g++")
    exe = str(tmp_path_factory.mktemp("opt_hyper") / "opt_hyper_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT}/csrc/include", f"{ROOT}/csrc/tests/opt_hyper_test.cpp", "-o", exe], check=True,
                   timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout + r.stderr[-3000:]
    return r.stdout.splitlines()


def test_header_names_match_python(header_program):
    names = [ln.split()[1:] for ln in header_program if ln.startswith("names")]
    assert names == [list(ops.HYPER_FIELDS)]


def test_header_bias_correction(header_program):
    got = {}
    for ln in header_program:
        if ln.startswith("bias"):
            _, mode, step, b1, b2 = ln.split()
            got[int(mode), int(step)] = np.array([int(b1, 16), int(b2, 16)], dtype=np.uint32).view(np.float32)
    assert sorted(got) == [(m, s) for m in range(3) for s in STEPS]
    betas = np.array([0.9, 0.999], dtype=np.float32)
    one = np.float32(1.0)
    for step in STEPS:
        assert got[0, step].tolist() == [3.0, 5.0]
        mode2 = one / (one - betas)
        assert mode2.dtype == np.float32 and got[2, step].tobytes() == mode2.tobytes()
        mode1 = (1.0 / (1.0 - np.power(betas.astype(np.float64), float(step)))).astype(np.float32).astype(np.float64)
        err = np.abs(got[1, step].astype(np.float64) - mode1) / mode1
        print(f"step {step}: mode 1 relative error {err}")
        assert (err <= 2.0 ** -23).all()
