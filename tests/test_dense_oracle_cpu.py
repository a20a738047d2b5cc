"""The fp64 oracles, builders and checkers of tests/dense_oracle.py, validated without a GPU.

    test                                       what it establishes
    test_fp32_path_fused_opt                   ops.fused_opt (fp32 CPU path) on every build_dense case test_dense_gpu.py launches
                                               (8 sets x n 7 / 8 / 275 / 2051 x fp32 / bf16 g, wout none / bf16 / fp32, gscale_t)
                                               stays within CPU_TOL = half the GPU bound of dense_opt64
    test_fp32_path_fused_opt_grid_wrap_inputs  the same on the two large fused_opt inputs (fused_opt_kernel<.., VEC / !VEC> wraps)
    test_fp32_path_multi                       multi_grad64 + dense_opt64 against ops.fused_opt on the summed sources, on every
                                               segment of fused_opt_multi_kernel / reduce_multi_kernel the GPU file runs
    test_fp32_path_onebit_pack                 C.onebit_pack (CPU) passes check_pack: onebit_pack_kernel<G, E, MOM> cases
    test_fp32_path_onebit_unpack               C.onebit_unpack_reduce (CPU) is bit-exact: onebit_unpack_reduce_kernel<O> cases
    test_fp32_path_onebit_momentum             C.onebit_momentum (CPU): onebit_momentum_kernel<G, E> cases
    test_fp32_path_elementwise                 R.cast_ / axpy_ / reduce_n / lerp / sumsq / clip_factor (CPU): the reduce.hip cases
    test_oracle_*_is_torch_*                   dense_opt64 = torch.optim SGD / Adam / AdamW / Adagrad in fp64, one step
    test_ftrl_by_hand, test_onebit_layout_by_hand, test_multi_grad_by_hand
                                               FTRL both modes, the bit layout, word and chunk boundaries written out
    test_builders_cover_what_they_promise      every condition of the builders
    test_bounds_reject_wrong_variants          eleven wrong versions of the operations each break a checker the GPU file uses

Measured here (max |fp32 path - oracle| / (1 + |oracle|) over w, st0, st1 and every case of the set):

    sgd 3.9e-08   sgd_momentum 8.5e-08   sgd_nesterov 1.2e-07   adam 6.3e-08   adamw 6.1e-08   adagrad 1.1e-07
    ftrl0_dense 3.9e-06   ftrl1_dense 7.2e-08   grid-wrap inputs 1.3e-07   multi-source segments 2.9e-06

All are under 1e-5, FTRL mode 1 (sqrt(n / lr) at lr = 0.05) included, so the GPU bound stays 2e-5 for every set.
"""
import pytest
import torch

from ps_amd import ops
from ps_amd.ops import compress as C
from ps_amd.ops import reduce as R

from . import dense_oracle as do

CPU_TOL = do.OPT_TOL / 2
DT = do.GDTYPES
MEASURED = {}


def _cpu_step(c, w, a, b, g, wout=None, gscale_t=None):
    ops.fused_opt(c["kind"], w, a, b, g, wout=wout, gscale_t=gscale_t, **c["hp"])


def _record(name, got, ref, keep):
    for x, r in zip(got, ref):
        if r is not None:
            MEASURED[name] = max(MEASURED.get(name, 0.0), do.opt_err(x, r, keep))


# ------------------------------------------------------------------------------ fp32 CPU paths
@pytest.mark.parametrize("gdt", ["f32", "bf16"])
@pytest.mark.parametrize("n", do.DENSE_NS)
@pytest.mark.parametrize("hpname", do.DENSE_HP)
def test_fp32_path_fused_opt(hpname, n, gdt):
    for wdt, gs in ((None, None), ("bf16", None), ("f32", torch.tensor([0.75]))):
        c = do.build_dense(hpname, gdt, n, gscale_t=gs)
        w, a, b = (x.clone() if x is not None else None for x in (c["w"], c["st0"], c["st1"]))
        wout = None if wdt is None else torch.full((n,), 9.0, dtype=DT[wdt])
        _cpu_step(c, w, a, b, c["g"], wout, gs)
        ref = do.dense_opt64(c["kind"], c["w"], c["st0"], c["st1"], c["g"], gs, **c["hp"])
        do.check_opt((w, a, b), ref[:3], c["keep"], CPU_TOL)
        _record(hpname, (w, a, b), ref[:3], c["keep"])
        if wout is not None:
            do.check_copy_out(w, wout)
        assert (a is None) == (hpname == "sgd") and (b is None) == (c["kind"] in (do.SGD, do.ADAGRAD))


@pytest.mark.parametrize("aligned", [True, False])
def test_fp32_path_fused_opt_grid_wrap_inputs(aligned):
    c = do.build_dense_wrap(aligned)
    w, a = c["w"].clone(), c["st0"].clone()
    _cpu_step(c, w, a, None, c["g"])
    ref = do.dense_opt64(c["kind"], c["w"], c["st0"], None, c["g"], **c["hp"])
    do.check_opt((w, a, None), ref[:3], c["keep"], CPU_TOL)
    _record("wrap", (w, a, None), ref[:3], c["keep"])


def _multi_cases():
    for src in ("f32", "bf16", "onebit"):
        for nsrc in (1, 2, 16):
            for off, n in do.segments(src):
                yield src, nsrc, off, n, "sgd_momentum"
    for hpname in do.DENSE_HP:
        for src in ("f32", "bf16", "onebit"):
            yield src, 2, 5, do.head_of(5) + 8 * 130 + 5, hpname


def test_fp32_path_multi():
    for src, nsrc, off, n, hpname in _multi_cases():
        c = do.build_multi(src, nsrc, off, n, hpname)
        seg = lambda x: None if x is None else x[off:off + n].clone()  # noqa: E731
        w, a, b = seg(c["master"]), seg(c["st0"]), seg(c["st1"])
        g = c["gsum"].float()
        assert torch.equal(g.double(), c["gsum"])
        _cpu_step(c, w, a, b, g)
        ref = do.multi_opt64(c)
        do.check_opt((w, a, b), ref, c["keep"], CPU_TOL)
        _record("multi", (w, a, b), ref, c["keep"])
        # the project's own decode of the 1-bit form agrees with multi_grad64
        if src == "onebit":
            out = torch.zeros(c["L"])
            C.onebit_unpack_reduce(c["words"], c["scales"], out)
            assert torch.equal(out[off:off + n].double(), c["gsum"])


def test_measured_maxima_are_what_the_docstring_says():
    """Runs after the fp32-path tests of this file (pytest keeps file order); a no-op when run alone."""
    for name, v in MEASURED.items():
        assert v <= 1e-5, (name, v)  # otherwise that set's GPU bound would have to be twice the measured value
    if MEASURED:
        print({k: f"{v:.2g}" for k, v in MEASURED.items()})


@pytest.mark.parametrize("with_mom", [False, True])
@pytest.mark.parametrize("edt", ["f32", "bf16"])
@pytest.mark.parametrize("gdt", ["f32", "bf16"])
@pytest.mark.parametrize("n", do.PACK_NS)
def test_fp32_path_onebit_pack(n, gdt, edt, with_mom):
    c = do.build_pack(n, gdt, edt, with_mom)
    nw, ns = C.packed_sizes(n)
    words, scales = torch.full((nw,), -1, dtype=torch.int64), torch.full((ns,), -1.0)
    err, mom = c["err"].clone(), (c["mom"].clone() if with_mom else None)
    C.onebit_pack(c["g"], err, words, scales, mom, c["beta1"])
    do.check_pack(c, words, scales, err, mom, mom_slack=do.cpu_coef_slack(c["g"], c["beta1"]))


@pytest.mark.parametrize("n,mdt", [(3001, "f32"), (5000, "bf16"), (70000, "f32"), (70000, "bf16")])
def test_pack_margin_on_the_existing_momentum_inputs(n, mdt):
    """The inputs of test_kernels_gpu.py::test_onebit_momentum_pack: at most 4 elements inside the
    rounding margin, so its per-element sign rule compares all but those."""
    torch.manual_seed(n)
    g = torch.randn(n).bfloat16()
    err, mom = (torch.randn(n) * 0.1).to(DT[mdt]), torch.randn(n).to(DT[mdt])
    o = do.onebit_pack64(g, err, mom, 0.9)
    assert int((~do.pack_margin(o, g, err, mom)).sum()) <= 4


@pytest.mark.parametrize("odt", ["f32", "bf16"])
@pytest.mark.parametrize("nworkers", [1, 3])
@pytest.mark.parametrize("n", do.UNPACK_NS)
def test_fp32_path_onebit_unpack(n, nworkers, odt):
    c = do.build_unpack(n, nworkers)
    for acc in (False, True):
        out = c["prev"].to(DT[odt]).clone()
        C.onebit_unpack_reduce(c["words"], c["scales"], out, 0.5, acc)
        ref = do.onebit_unpack64(c["words"], c["scales"], n, 0.5, c["prev"] if acc else None)
        assert torch.equal(out, do.to_dtype(ref, DT[odt]))


@pytest.mark.parametrize("mdt", ["f32", "bf16"])
@pytest.mark.parametrize("gdt", ["f32", "bf16"])
def test_fp32_path_onebit_momentum(gdt, mdt):
    c = do.build_pack(3001, gdt, mdt, True)
    m = c["mom"].clone()
    C.onebit_momentum(c["g"], m, 0.9)
    o = do.onebit_pack64(c["g"], c["err"], c["mom"], 0.9)
    do.check_bounded(m, o["m"], do.mom_bound(o, c["g"], c["mom"], 0.9, mdt == "bf16") + do.cpu_coef_slack(c["g"], 0.9),
                     "momentum")


@pytest.mark.parametrize("ydt", ["f32", "bf16"])
@pytest.mark.parametrize("xdt", ["f32", "bf16"])
@pytest.mark.parametrize("n", do.ELEM_NS + (2056,))
def test_fp32_path_elementwise(n, xdt, ydt):
    c = do.build_elem(n, xdt, ydt)
    y = torch.empty(n, dtype=DT[ydt])
    R.cast_(c["x"], y, 0.3)
    assert torch.equal(y, do.to_dtype(do.cast64(c["x"], 0.3), DT[ydt]))
    y = c["y"].clone()
    R.axpy_(0.3, c["x"], y)
    ref, mag = do.axpy64(0.3, c["x"], c["y"])
    do.check_bounded(y, ref, do.fma_bound(mag, ref, ydt == "bf16"), "axpy")
    y = torch.empty(n, dtype=DT[ydt])
    R.reduce_n(c["xs"], y, 0.25)
    assert torch.equal(y, do.to_dtype(do.reduce_n64(c["xs"], 0.25), DT[ydt]))
    if xdt == "f32":
        w0, w = c["x"], c["y"].float()
        out = torch.empty(n, dtype=DT[ydt])
        R.lerp(w0, w, 0.3, out)
        ref, mag = do.lerp64(w0, w, 0.3)
        # the CPU path forms 1 - s in double: one more 2^-24 of the second term than the kernel's fp32 1.f - sc
        do.check_bounded(out, ref, do.fma_bound(mag, ref, ydt == "bf16") + do.U24 * mag, "lerp")
    sq = R.sumsq(c["x"])
    ref = do.sumsq64(c["x"])
    assert abs(float(sq) - float(ref)) <= 1e-4 * float(ref)
    assert abs(float(R.clip_factor(sq, 1.5)) - do.clip64(ref, 1.5)) <= 1e-4
    assert do.clip64(1e-4, 1.5) == 1.0


# ------------------------------------------------------------------ dense_opt64 vs torch.optim
def _torch_case(hpname, n=41):
    c = do.build_dense(hpname, "f32", n)
    d = lambda x: None if x is None else x.double()  # noqa: E731
    w, a, b, g = d(c["w"]), d(c["st0"]), d(c["st1"]), d(c["g"])
    out = do.dense_opt64(c["kind"], w, a, b, g, **c["hp"])
    p = torch.nn.Parameter(w.clone())
    p.grad = g * c["hp"]["gscale"]
    return c["hp"], p, a, b, out


def _same(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("hpname", ["sgd", "sgd_momentum", "sgd_nesterov"])
def test_oracle_sgd_is_torch_sgd(hpname):
    hp, p, a, _, (w, st0, _, wout) = _torch_case(hpname)
    opt = torch.optim.SGD([p], lr=hp["lr"], momentum=hp.get("momentum", 0.0), dampening=hp.get("dampening", 0.0),
                          nesterov=hp.get("nesterov", False), weight_decay=hp.get("wd", 0.0))
    if a is not None:
        opt.state[p]["momentum_buffer"] = a.clone()
    opt.step()
    _same(w, p.data)
    assert torch.equal(wout, w)
    if a is not None:
        _same(st0, opt.state[p]["momentum_buffer"])
    else:
        assert st0 is None


@pytest.mark.parametrize("hpname", ["adam", "adamw"])
def test_oracle_adam_is_torch_adam(hpname):
    hp, p, a, b, (w, st0, st1, _) = _torch_case(hpname)
    t = 3  # the step the sets' bias corrections stand at
    assert abs(hp["bc1"] - 1 / (1 - 0.9 ** t)) < 1e-12 and abs(hp["bc2"] - 1 / (1 - 0.999 ** t)) < 1e-12
    cls = torch.optim.AdamW if hp.get("adamw") else torch.optim.Adam
    opt = cls([p], lr=hp["lr"], betas=(0.9, 0.999), eps=hp["eps"], weight_decay=hp["wd"])
    opt.state[p].update(step=torch.tensor(float(t - 1)), exp_avg=a.clone(), exp_avg_sq=b.clone())
    opt.step()
    # torch divides by (sqrt(v) / sqrt(bias2) + eps) and multiplies lr / bias1: the same numbers up to fp64 rounding
    torch.testing.assert_close(st0, opt.state[p]["exp_avg"], rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(st1, opt.state[p]["exp_avg_sq"], rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(w, p.data, rtol=1e-9, atol=1e-10)


def test_oracle_adagrad_is_torch_adagrad():
    hp, p, a, _, (w, st0, _, _) = _torch_case("adagrad")
    opt = torch.optim.Adagrad([p], lr=hp["lr"], eps=hp["eps"], weight_decay=hp["wd"])
    opt.state[p]["sum"] = a.clone()
    opt.step()
    _same(w, p.data)
    _same(st0, opt.state[p]["sum"])


# ------------------------------------------------------------------------------ by hand
def test_ftrl_by_hand():
    # lr = alpha = 0.5, l1 = 0.5, l2 = 0, beta = 1, gscale 1; n = 4 -> sqrt(n) = 2
    hp = dict(lr=0.5, l1=0.5, l2=0.0, fbeta=1.0)
    w, z, n, g = (torch.tensor(v, dtype=torch.float64) for v in ([1.0, 1.0], [2.0, 0.25], [4.0, 4.0], [3.0, 0.0]))
    # mode 1: w from (z, n_old): z = 2 -> -(2 - 0.5) / ((0 + (1 + 2)) / 0.5) = -0.25; z = 0.25 <= l1 -> 0
    #   sigma = sqrt(n + g^2) - sqrt(n / alpha) = sqrt(13) - sqrt(8) | 2 - sqrt(8);  z += g - sigma w
    nw, nz, nn, _ = do.dense_opt64(do.FTRL, w, z, n, g, ftrl_mode=1, **hp)
    s8, s13 = 8.0 ** 0.5, 13.0 ** 0.5
    assert torch.allclose(nw, torch.tensor([-0.25, 0.0], dtype=torch.float64), atol=1e-15)
    assert torch.allclose(nz, torch.tensor([2.0 + 3.0 + (s13 - s8) * 0.25, 0.25], dtype=torch.float64), atol=1e-14)
    assert torch.equal(nn, torch.tensor([13.0, 4.0], dtype=torch.float64))
    # mode 0: nn = 13 | 4; sigma = (sqrt(nn) - 2) / 0.5; zn = z + g - sigma w; w from (zn, nn)
    nw, nz, nn, _ = do.dense_opt64(do.FTRL, w, z, n, g, ftrl_mode=0, **hp)
    zn0 = 2.0 + 3.0 - (s13 - 2.0) / 0.5
    assert torch.allclose(nz, torch.tensor([zn0, 0.25], dtype=torch.float64), atol=1e-14)
    assert torch.allclose(nw, torch.tensor([-(zn0 - 0.5) / ((1.0 + s13) / 0.5), 0.0], dtype=torch.float64), atol=1e-14)
    assert torch.equal(nn, torch.tensor([13.0, 4.0], dtype=torch.float64))
    zero, tie = do.ftrl_margin(w, z, n, g, ftrl_mode=1, **hp)
    assert zero.tolist() == [False, True] and not tie.any()
    _, tie = do.ftrl_margin(w, torch.tensor([0.5 + 5e-6, -0.5 + 5e-6], dtype=torch.float64), n, g, ftrl_mode=1, **hp)
    assert tie.all()


def test_onebit_layout_by_hand():
    # n = 11: c = g + e; signs + - + + - - - + | + + -  -> byte 0 = 0b10001101 = 0x8D, byte 1 = 0b011 = 0x03
    g = torch.tensor([1.0, -2.0, 0.5, 0.0, -1.0, -1.0, -3.0, 2.0, 4.0, 1.0, -0.5])
    e = torch.tensor([0.5, 0.0, 0.0, 0.0, 0.5, -1.0, 1.0, 2.0, 0.0, 1.0, 0.0])
    o = do.onebit_pack64(g, e)
    assert o["words"].tolist() == [0x038D]
    cabs = [1.5, 2.0, 0.5, 0.0, 0.5, 2.0, 2.0, 4.0, 4.0, 2.0, 0.5]
    assert abs(float(o["scales"][0]) - sum(cabs) / 11) < 1e-15  # the valid count, not 1024
    sc = sum(cabs) / 11
    assert abs(float(o["err"][0]) - (1.5 - sc)) < 1e-15 and abs(float(o["err"][1]) - (-2.0 + sc)) < 1e-15
    assert abs(float(o["err"][3]) - (0.0 - sc)) < 1e-15  # c == 0 is bit 1
    raw = o["words"].numpy().tobytes()  # little-endian memory: element i at byte i / 8, bit i % 8
    assert raw[0] == 0x8D and raw[1] == 0x03 and not any(raw[2:])
    assert do.unpack_bits(o["words"], 11).int().tolist() == [1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 0]
    # bit 63 is the sign bit of the int64 word
    b = torch.zeros(64, dtype=torch.bool)
    b[63] = True
    assert do.pack_words(b).tolist() == [-2 ** 63]
    # momentum form: m = beta1 m + (1 - beta1) g with the fp32 beta1; c = m + e
    o = do.onebit_pack64(torch.tensor([2.0]), torch.tensor([-1.0]), torch.tensor([1.0]), 0.5)
    assert float(o["m"][0]) == 1.5 and float(o["c"][0]) == 0.5 and float(o["scales"][0]) == 0.5
    assert float(o["err"][0]) == 0.0
    # unpack: mult and accumulate
    words, scales = torch.tensor([[0x038D], [0x0001]]), torch.tensor([[0.5], [0.25]])
    out = do.onebit_unpack64(words, scales, 3, 2.0, torch.tensor([10.0, 10.0, 10.0]))
    assert out.tolist() == [10.0 + 2 * 0.75, 10.0 + 2 * -0.75, 10.0 + 2 * 0.25]


def test_multi_grad_by_hand():
    L = 2048
    words = torch.zeros(2, L // 64, dtype=torch.int64)
    scales = torch.tensor([[0.5, 0.25], [1.0, 0.125]])
    words[0, 0] = 1 << 62          # chunk element 62
    words[0, 1] = 1                # chunk element 64
    words[1, 15] = -2 ** 63        # chunk element 1023 (bit 63 of word 15)
    words[1, 16] = 1               # chunk element 1024
    tot, sumabs = do.multi_grad64([], 61, 5, words, scales)     # elements 61..65: a word boundary
    assert tot.tolist() == [-1.5, -0.5, -1.5, -0.5, -1.5] and sumabs.tolist() == [1.5] * 5
    tot, _ = do.multi_grad64([], 1022, 4, words, scales)        # 1022..1025: a chunk boundary
    assert tot.tolist() == [-1.5, 0.5, -0.125, -0.375]
    a, b = torch.arange(16.0), 100.0 * torch.arange(16.0)
    tot, sumabs = do.multi_grad64([a, -b.to(torch.bfloat16)], 7, 3)
    assert tot.tolist() == [7 - 700.0, 8 - 800.0, 9 - 900.0] and sumabs.tolist() == [707.0, 808.0, 909.0]
    assert [do.head_of(o) for o in range(9)] == [0, 7, 6, 5, 4, 3, 2, 1, 0] and do.head_of(61) == 3


# --------------------------------------------------------------------------------- builders
def test_builders_cover_what_they_promise():
    # every branch of opt_apply has a set
    sets = {k: do.HP_SETS[k] for k in do.DENSE_HP}
    assert sets["sgd"][3].get("momentum", 0) == 0 and do.build_dense("sgd", "f32", 8)["st0"] is None
    assert sets["sgd_momentum"][3]["dampening"] != 0 and not sets["sgd_momentum"][3].get("nesterov")
    assert sets["sgd_nesterov"][3]["nesterov"] and sets["adamw"][3]["adamw"] and not sets["adam"][3].get("adamw")
    assert sets["adam"][3]["wd"] != 0 and sets["adamw"][3]["wd"] != 0 and sets["adagrad"][0] == do.ADAGRAD
    assert sets["ftrl0_dense"][3]["ftrl_mode"] == 0 and sets["ftrl1_dense"][3]["ftrl_mode"] == 1
    # FTRL: the branch shares and the cap on ties, on every dense and multi case
    for hpname in ("ftrl0_dense", "ftrl1_dense"):
        assert do.HP_SETS[hpname][3]["l1"] == 0.5
        for n in do.DENSE_NS:
            for gdt in ("f32", "bf16"):
                c = do.build_dense(hpname, gdt, n)
                zero, tie = do.ftrl_margin(c["w"], c["st0"], c["st1"], c["g"], **c["hp"])
                assert int(tie.sum()) <= do.MAX_TIES and torch.equal(c["keep"], ~tie)
                assert 0 < int(zero.sum()) < n
                if n >= 64:
                    assert 0.1 <= float(zero.double().mean()) <= 0.9
        for src in ("f32", "bf16", "onebit"):
            c = do.build_multi(src, 2, 5, 1048, hpname)
            zero, tie = do.ftrl_margin(c["master"][5:1053], c["st0"][5:1053], c["st1"][5:1053], c["gsum"], **c["hp"])
            assert 0.1 <= float(zero.double().mean()) <= 0.9 and int((~c["keep"]).sum()) <= do.MAX_TIES
    # Adam's cold element
    c = do.build_dense("adamw", "bf16", 7)
    assert float(c["g"][do.ADAM_COLD]) == 0 and float(c["st1"][do.ADAM_COLD]) == 0 and float(c["st0"][do.ADAM_COLD]) > 0
    # segments: all 8 phases at both lengths, the short one, the 1-bit extras
    for src in ("f32", "bf16", "onebit"):
        segs = do.segments(src)
        assert (3, 2) in segs and do.head_of(3) > 2
        assert {o & 7 for o, n in segs if n == do.head_of(o) + 8} == set(range(8))
        assert {o & 7 for o, n in segs if n == do.head_of(o) + 8 * 130 + 5} >= set(range(8))
    assert (61, 3 + 8 * 130 + 5) in do.segments("onebit") and 61 // 64 != (61 + do.head_of(61)) // 64
    assert (1019, 2100) in do.segments("onebit") and 1019 // 1024 == 0 and (1019 + 2099) // 1024 == 3
    assert (61, 1048) not in do.segments("f32")
    # the exact grid sums exactly for 16 sources in any order, in fp32; every source differs
    for src in ("f32", "bf16", "onebit"):
        c = do.build_multi(src, 16, 1019 if src == "onebit" else 3, 2100)
        o, n = c["off"], c["n"]
        if src == "onebit":
            vals = [do.multi_grad64([], o, n, c["words"][s:s + 1], c["scales"][s:s + 1])[0].float() for s in range(16)]
            assert len({float(x) for x in c["scales"][0]}) >= 3  # chunks 0..3 of the segment: different scales
        else:
            vals = [s[o:o + n].float() for s in c["srcs"]]
            assert all(torch.equal(s, s.to(torch.bfloat16).to(s.dtype)) for s in c["srcs"])
        fwd, rev = torch.zeros(n), torch.zeros(n)
        for v in vals:
            fwd += v
        for v in reversed(vals):
            rev += v
        assert torch.equal(fwd, rev) and torch.equal(fwd.double(), c["gsum"])
        for a in range(16):
            for b in range(a):
                assert not torch.equal(vals[a], vals[b])
        # sentinels outside the segment, whole chunks
        for buf in (c["master"], c["st0"]):
            assert buf.numel() % do.CHUNK == 0 and bool((buf[~c["inside"]] == do.SENTINEL).all())
            assert not bool((buf[c["inside"]] == do.SENTINEL).any())
        assert int(c["inside"].sum()) == n and bool(c["inside"][o]) and not bool(c["inside"][o - 1])
    c = do.build_multi("bf16", 2, 5, 1048, wout="bf16")
    assert c["pull"].dtype == torch.bfloat16 and bool((c["pull"] == do.SENTINEL).all())
    # the rounded-sum cases are not exact (their bound is what covers them)
    c = do.build_multi("f32", 16, 3, 1050, exact=False)
    assert not torch.equal(c["gsum"], c["gsum"].float().double())
    # grid wrap sizes leave the 2048-block grid
    assert do.GRID_WRAP_VEC // 8 > 2048 * 256 and do.GRID_WRAP_VEC % 8 == 5
    assert do.GRID_WRAP_SCALAR > 2048 * 256
    assert (do.GRID_WRAP_MULTI - do.head_of(5)) // 8 > 2048 * 256
    # pack: zeros of both signs, an all-zero chunk, the margin cap
    for mom in (False, True):
        c = do.build_pack(3001, "bf16", "bf16", mom)
        o = do.onebit_pack64(c["g"], c["err"], c["mom"], c["beta1"])
        assert float(o["scales"][1]) == 0 and float(o["scales"][0]) > 0 and float(o["scales"][2]) > 0
        assert bool(torch.signbit(o["c"][2])) and float(o["c"][1]) == 0 and bool(o["bits"][1] & o["bits"][2])
        assert 0.3 < float(o["bits"][:1024].double().mean()) < 0.7
    assert do.PACK_NS == (5, 64, 1000, 1024, 1029, 2048, 3001)
    # unpack: exact, and the previous output is not zero
    c = do.build_unpack(3001, 3)
    assert bool((c["prev"] != 0).any()) and c["words"].shape == (3, 47) and c["scales"].shape == (3, 3)


# ----------------------------------------------------------------------------- wrong variants
def _rejects(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def _f32_step(c, hp=None, g=None):
    """The fp32 CPU path on a dense case with other hyper-parameters / another gradient."""
    w, a, b = (x.clone() if x is not None else None for x in (c["w"], c["st0"], c["st1"]))
    ops.fused_opt(c["kind"], w, a, b, c["g"] if g is None else g, **(hp or c["hp"]))
    return w, a, b


def _ref(c):
    return do.dense_opt64(c["kind"], c["w"], c["st0"], c["st1"], c["g"], **c["hp"])[:3]


def test_bounds_reject_wrong_variants():
    tol = do.OPT_TOL
    # 1. bf16 copy-out by truncation
    c = do.build_dense("sgd", "f32", 2051)
    w, _, _ = _f32_step(c)
    do.check_copy_out(w, w.to(torch.bfloat16))
    trunc = (w.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    assert torch.equal(trunc.float(), (w.view(torch.int32) & -65536).view(torch.float32))  # truncation is bf16-exact
    _rejects(do.check_copy_out, w, trunc)
    torch.testing.assert_close(trunc.float(), w, rtol=1e-2, atol=1e-2)  # ... and passes the old 1e-2 comparison
    # 2. Adam eps inside the square root
    for hpname in ("adam", "adamw"):
        c = do.build_dense(hpname, "f32", 275)
        h = do._hp(c["hp"])
        g = c["g"].double() * h["gscale"] + (0 if h["adamw"] else h["wd"] * c["w"].double())
        m = h["beta1"] * c["st0"].double() + (1 - h["beta1"]) * g
        v = h["beta2"] * c["st1"].double() + (1 - h["beta2"]) * g * g
        upd = m * h["bc1"] / torch.sqrt(v * h["bc2"] + h["eps"]) + (h["wd"] * c["w"].double() if h["adamw"] else 0)
        bad = (c["w"].double() - h["lr"] * upd).float()
        do.check_opt(_f32_step(c), _ref(c), c["keep"], tol)
        _rejects(do.check_opt, (bad, m.float(), v.float()), _ref(c), c["keep"], tol)
    # 3. Nesterov and plain momentum swapped; 4. dampening ignored
    for hpname, change in (("sgd_nesterov", dict(nesterov=False)), ("sgd_momentum", dict(nesterov=True)),
                           ("sgd_momentum", dict(dampening=0.0))):
        c = do.build_dense(hpname, "bf16", 275)
        do.check_opt(_f32_step(c), _ref(c), c["keep"], tol)
        _rejects(do.check_opt, _f32_step(c, dict(c["hp"], **change)), _ref(c), c["keep"], tol)
    # 5. the last n % 8 elements left untouched
    c = do.build_dense("sgd_momentum", "f32", 2051)
    w, a, _ = _f32_step(c)
    w[2048:], a[2048:] = c["w"][2048:], c["st0"][2048:]
    _rejects(do.check_opt, (w, a, None), _ref(c), c["keep"], tol)
    # 6. the head elements updated twice; 7. one source dropped
    for src in ("f32", "bf16", "onebit"):
        c = do.build_multi(src, 16, 3, do.head_of(3) + 8 * 130 + 5)
        o, n = c["off"], c["n"]
        d = dict(kind=c["kind"], hp=c["hp"], w=c["master"][o:o + n], st0=c["st0"][o:o + n], st1=None,
                 g=c["gsum"].float())
        once = _f32_step(d)
        do.check_opt(once, do.multi_opt64(c), c["keep"], tol)
        w, a = once[0].clone(), once[1].clone()
        d2 = dict(d, w=w[:5], st0=a[:5], g=d["g"][:5])
        w[:5], a[:5], _ = _f32_step(d2)
        _rejects(do.check_opt, (w, a, None), do.multi_opt64(c), c["keep"], tol)
        if src == "onebit":
            less, _ = do.multi_grad64([], o, n, c["words"][:15], c["scales"][:15])
            twice, _ = do.multi_grad64([], o, n, c["words"][[0] + list(range(15))], c["scales"][[0] + list(range(15))])
        else:
            less, _ = do.multi_grad64(c["srcs"][:15], o, n)
            twice, _ = do.multi_grad64([c["srcs"][0]] + c["srcs"][:15], o, n)
        assert not torch.equal(less.float(), c["gsum"].float()) and not torch.equal(twice.float(), c["gsum"].float())
        if src == "onebit":  # a decoded value is never 0: every element notices
            assert int((less != c["gsum"]).sum()) == n
    # 8. the chunk scale indexed by i // 1024; 9. the word bit by i % 64 (segment-relative, not chunk-relative)
    c = do.build_multi("onebit", 2, 1019, 2100)
    o, n = c["off"], c["n"]
    q, i = o + torch.arange(n), torch.arange(n)

    def decode(bit_of, scale_of):  # the word is always that of chunk element off + i
        out = torch.zeros(n)
        for s in range(2):
            sc = c["scales"][s][scale_of // 1024]
            out += torch.where(((c["words"][s][q // 64] >> bit_of) & 1) == 1, sc, -sc)
        return out

    good, bad_scale, bad_bit = decode(q % 64, q), decode(q % 64, i), decode(i % 64, q)
    assert torch.equal(good, c["gsum"].float())
    assert not torch.equal(bad_scale, c["gsum"].float()) and not torch.equal(bad_bit, c["gsum"].float())
    assert torch.equal(bad_scale[:5], good[:5])  # only past the first chunk boundary
    # 10. the short last chunk's scale divided by 1024
    c = do.build_pack(1029, "f32", "f32", False)
    o = do.onebit_pack64(c["g"], c["err"])
    sc = o["scales"].float()
    do.check_pack(c, o["words"], sc, o["err"].float(), None)
    sc_bad = sc.clone()
    sc_bad[1] = sc[1] * 5 / 1024
    es = sc_bad.double().repeat_interleave(1024)[:1029]
    err_bad = (o["c"] - torch.where(o["bits"], es, -es)).float()
    _rejects(do.check_pack, c, o["words"], sc_bad, err_bad, None)
    # ... a pad bit set; a truncated-to-zero bit for c == -0.0
    wbad = o["words"].clone()
    wbad[-1] |= 1 << 40
    _rejects(do.check_pack, c, wbad, sc, o["err"].float(), None)
    wbad = o["words"].clone()
    wbad[0] &= ~4
    _rejects(do.check_pack, c, wbad, sc, o["err"].float(), None)
    # 11. accumulate ignored
    c = do.build_unpack(1029, 3)
    ref = do.onebit_unpack64(c["words"], c["scales"], 1029, 0.5, c["prev"])
    noacc = do.onebit_unpack64(c["words"], c["scales"], 1029, 0.5, None)
    for dt in (torch.float32, torch.bfloat16):
        assert not torch.equal(do.to_dtype(noacc, dt), do.to_dtype(ref, dt))
