"""bench.py driver contract, exercised on CPU tensors over gloo (``--device cpu``): the same
torchrun self-launch, barrier-bracketed timed region, MAX-over-ranks elapsed time, per-phase PS
timing and collective probe (``--full``) as the multi-GPU runs, ending in exactly ONE JSON line from
rank 0 with the BASELINE.json metric; a plain run stops at the timed steps, ``--dump-outputs`` writes
what the last of them computed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [1, 2])
def test_bench_json_contract_cpu(world, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", "--gpus", str(world), "--steps", "2",
           "--warmup", "1", "--batch-per-gpu", "2", "--image-size", "32", "--full"]
    out = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=540)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert KEYS <= set(rec)
    baseline = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert rec["metric"] == baseline["metric"]
    assert rec["n_gpus"] == world and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["config"]["model"] == "ResNet-50" and rec["config"]["global_batch"] == 2 * world
    # value is the whole-job rate: global batch x steps / (max over ranks of the timed region)
    assert rec["value"] == pytest.approx(2 * world * 1e3 / rec["ms_per_step"], rel=1e-2)
    # stream policy fields: keyed on ranks sharing a device (CPU ranks never share one)
    assert rec["config"]["ranks_per_device"] == 1
    assert rec["config"]["compute_priority"] == "normal" and rec["config"]["side_stream"] is False
    assert rec["config"]["streams_per_rank"] == 0
    if world > 1:
        assert set(rec["config"]["ps_phase_ms_per_step"]) >= {"push_ms", "serve_ms", "pull_ms"}
        if rec["config"].get("data_plane") == "xgmi":  # mapping mode / self-test / round end reported
            assert {"mode", "self_test", "round_end"} <= set(rec["config"]["plane_info"])


@pytest.mark.timeout(600)
@pytest.mark.parametrize("config,extra", [("dlrm", ["--dlrm-rows", "2000", "--batch-per-gpu", "32"]),
                                          ("ctr-async", ["--batch-per-gpu", "32"]),
                                          ("llama-onebit", ["--tiny", "1", "--batch-per-gpu", "2", "--seq-len", "32"])])
def test_other_bench_configs_build_and_step_cpu(config, extra, tmp_path):
    """Every non-default bench config builds and times a step on CPU (world 1): a config that no
    longer constructs fails here, not on the GPU box."""
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", "--config", config, "--steps", "1",
           "--warmup", "1"] + extra
    out = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=540)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert KEYS <= set(rec) and rec["value"] > 0


def _plain_run(tmp_path, world, extra):
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "PS_AMD_CHECKPOINT_DIR"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", "--gpus", str(world), "--steps", "2",
           "--warmup", "1", "--batch-per-gpu", "2", "--image-size", "32"] + extra
    return subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=540)


@pytest.mark.timeout(600)
def test_plain_run_stops_at_the_timed_steps_cpu(tmp_path):
    """Without ``--full`` a world-2 run reports the headline fields and none of the after-the-timed-
    region measurements; asking for one of them without ``--full`` is a usage error."""
    out = _plain_run(tmp_path, 2, [])
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert KEYS <= set(rec) and rec["steps"] == 2 and rec["ms_per_step"] > 0
    assert not {"ps_phase_ms_per_step", "rccl_probe", "sync_audit"} & set(rec["config"])
    assert "[bench-timing]" not in out.stderr
    bad = _plain_run(tmp_path, 1, ["--timing", "1"])
    assert bad.returncode == 2 and "--full" in bad.stderr and not bad.stdout.strip()


@pytest.mark.timeout(600)
def test_dump_outputs_cpu(tmp_path):
    """``--dump-outputs``: float32 .npy files of the last timed step (loss, logits, parameters,
    BatchNorm statistics), under 64 MB in all, sampled arrays included, and the same arrays from a
    second run with the same arguments."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        out = _plain_run(tmp_path, 1, ["--dump-outputs", str(tmp_path / name)])
        assert out.returncode == 0, out.stderr[-3000:]
        rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
        files = sorted(os.listdir(tmp_path / name))
        arrs = {f[:-4]: np.load(tmp_path / name / f) for f in files}
        assert all(f.endswith(".npy") for f in files) and all(a.dtype == np.float32 for a in arrs.values())
        assert sum(os.path.getsize(tmp_path / name / f) for f in files) <= 64 * 2**20
        assert arrs["logits"].shape == (2, 1000) and np.isfinite(arrs["logits"]).all()
        assert arrs["loss"].shape == () and float(arrs["loss"]) ==pytest.approx(rec["config"]["final_loss"], abs=1e-4)
        assert "param.fc.weight" in arrs and any(k.startswith("buffer.") for k in arrs)
        # ResNet-50's 25.6M parameters exceed the budget: the large arrays are 1-D samples
        assert arrs["param.fc.weight"].ndim == 1 and arrs["param.fc.weight"].size < 2048 * 1000
        dumps.append(arrs)
    assert dumps[0].keys() == dumps[1].keys()
    for k in dumps[0]:
        np.testing.assert_allclose(dumps[0][k], dumps[1][k], rtol=1e-5, atol=1e-6, err_msg=k)
