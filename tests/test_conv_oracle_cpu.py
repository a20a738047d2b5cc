"""tests/conv_oracle.py against an independent formulation in fp64 (F.conv2d, torch.nn.grad.conv2d_input /
conv2d_weight on NCHW), its prologue / epilogue formulas against bn_oracle's, its bf16 yardstick against
the exact variant on the inputs of every case test_conv_rows_gpu.py runs, its ambiguity caps, its impulse
builders, and its plan replay against the bindings (that part only where the extension imports).  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from . import bn_oracle as bo
from . import conv_oracle as co


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.double().abs().max()))


def _nchw(rows, n, h, w):
    return rows.view(n, h, w, -1).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ------------------------------------------------------------------------------------ vs torch, fp64
@pytest.mark.parametrize("ks,stride,h,w", [(1, 1, 5, 7), (1, 2, 13, 11), (1, 2, 6, 4), (3, 1, 9, 9), (3, 1, 7, 5),
                                           (3, 2, 9, 9), (3, 2, 7, 5), (3, 2, 8, 6), (3, 1, 9, 1), (3, 1, 2, 2)])
def test_gather_matches_conv2d_and_conv2d_weight(ks, stride, h, w):
    n, C, N = 3, 8, 5
    g = torch.Generator().manual_seed(ks + stride + h + w)
    x = torch.randn(n * h * w, C, generator=g, dtype=torch.float64)
    wt = torch.randn(N, C, ks, ks, generator=g, dtype=torch.float64)
    gg = co.geo(h, w, ks, stride, ks // 2)
    A = co.gather_geo(x, gg)
    wm = co.mat3(wt) if ks == 3 else wt.reshape(N, C)
    y = F.conv2d(_nchw(x, n, h, w), wt, None, stride, ks // 2)
    assert y.shape[2:] == (gg[2], gg[3])
    _close(A @ wm.t(), _rows(y))
    dz = torch.randn(n * gg[2] * gg[3], N, generator=g, dtype=torch.float64)
    dw = torch.nn.grad.conv2d_weight(_nchw(x, n, h, w), wt.shape, _nchw(dz, n, gg[2], gg[3]), stride, ks // 2)
    o = co.wgrad_oracle(dz, A)
    _close(o["exact"], co.mat3(dw) if ks == 3 else dw.reshape(N, C))
    _close(o["db"], dz.sum(0))
    assert bool((o["mag"] >= o["exact"].abs() - 1e-12).all())


@pytest.mark.parametrize("h,w", [(9, 9), (7, 5), (2, 2)])
def test_mat3_dgrad_is_conv2d_input(h, w):
    n, C1, C2 = 2, 6, 4
    g = torch.Generator().manual_seed(h + w)
    wt = torch.randn(C2, C1, 3, 3, generator=g, dtype=torch.float64)
    dz = torch.randn(n * h * w, C2, generator=g, dtype=torch.float64)
    ref = torch.nn.grad.conv2d_input((n, C1, h, w), wt, _nchw(dz, n, h, w), padding=1)
    _close(co.gather_geo(dz, co.geo(h, w, 3, 1, 1)) @ co.mat3_dgrad(wt).t(), _rows(ref))


@pytest.mark.parametrize("h,w", [(6, 4), (14, 10), (8, 12)])
def test_stride2_phases_are_conv2d_input(h, w):
    n, C1, C2 = 2, 6, 4
    g = torch.Generator().manual_seed(3 * h + w)
    t = dict(w=torch.randn(C2, C1, 3, 3, generator=g, dtype=torch.float64),
             dz=torch.randn(n * (h // 2) * (w // 2), C2, generator=g, dtype=torch.float64))
    ref = torch.nn.grad.conv2d_input((n, C1, h, w), t["w"], _nchw(t["dz"], n, h // 2, w // 2), stride=2, padding=1)
    o = co.dgrad_s2_oracle(t, n, h, w, 0)
    _close(o["exact"], _rows(ref))
    # every dx row is written by exactly one phase, and its block is that phase's tile
    dsts = torch.cat([co.phase_rows(n, h, w, ph >> 1, ph & 1)[1] for ph in range(4)])
    assert torch.equal(dsts.sort().values, torch.arange(n * h * w))
    assert int(o["block"].max()) < o["G"]


def test_weight_layouts_equal_the_package_helpers():
    from ps_amd.ops.convgemm import _mat3_dgrad, _phase_weights

    wt = torch.randn(8, 6, 3, 3, generator=torch.Generator().manual_seed(1)).bfloat16()
    assert torch.equal(co.mat3_dgrad(wt), _mat3_dgrad(wt))
    for ph, wp in enumerate(_phase_weights(wt)):
        assert torch.equal(co.phase_weight(wt, ph >> 1, ph & 1), wp)


# ------------------------------------------------------------------------------------ formulas
def test_prologues_and_masks_are_bn_oracles():
    g = torch.Generator().manual_seed(5)
    R, C = 50, 16
    x, r = torch.randn(R, C, generator=g).bfloat16(), torch.randn(R, C, generator=g).bfloat16()
    cf, cf2 = co._coef(C, g), co._coef(C, g)
    a, amb, ulp = co.stage_bn_relu(x, cf)
    _close(a, bo.apply(x, cf, None, None, 1, True)[0], 0.0)
    assert amb.shape == a.shape and bool((ulp > 0).all())
    for rc in (None, cf2):
        ye, yy, mag = co.stage_block_out(x, r, cf, rc)
        _close(ye, bo.apply(x, cf, r, rc, 1, False)[0], 0.0)
        _close(yy, co.bf16r(ye), 0.0)
        assert torch.equal(co.mask_bits(yy), co.mask_bits(ye))  # abits: o > 0 before the rounding == aout > 0
    c3 = torch.randn(3 * C, generator=g).float()
    ye, yy, mag = co.stage_bn_bwd(x, r, c3)
    _close(ye, bo.bwd_apply(x, r, c3, False)[0], 0.0)
    _close(yy, bo.bwd_apply(x, r, c3, True)[0], 0.0)
    # epilogue 3's mask is the ReLU of bn_oracle.apply on z; set (a) is bn_oracle.ambiguous
    acc = torch.randn(R, C, generator=g, dtype=torch.float64)
    o = co.epilogue(3, acc, acc.abs(), dict(aux=x, mc=cf))
    on = bo.unpack_bits(bo.mask_bits(bo.apply(x, cf, None, None, 1, False)[0]), (R, C))
    _close(o["exact"], acc * on, 0.0)
    _close(o["yard"], co.bf16r(acc) * on, 0.0)
    assert torch.equal(o["amb"], bo.ambiguous(x, cf))


def test_epilogues_by_hand():
    g = torch.Generator().manual_seed(6)
    n, oh, ow, N = 2, 5, 3, 8
    M = n * oh * ow
    acc = torch.randn(M, N, generator=g, dtype=torch.float64)
    mag = acc.abs() + 1.0
    r = torch.randn(M, N, generator=g).bfloat16()
    keep, keep2 = torch.rand(M, N, generator=g) > 0.5, torch.rand(M, N, generator=g) > 0.4
    t = dict(aux=r, bits=co.mask_bits(keep.double()), bits2=co.mask_bits(keep2.double()), images=n, OH=oh, OW=ow)
    c0 = co.bf16r(acc)
    for epi, res in ((2, r.double()), (5, r.double() * keep), (7, r.double()), (6, r.double() * keep), (9, r.double() * keep)):
        o = co.epilogue(epi, acc, mag, t)
        k2 = keep2.double() if epi >= 6 else 1.0
        _close(o["exact"], (acc + res) * k2, 0.0)
        _close(o["yard"], co.bf16r(c0 + res) * k2, 0.0)  # the second rounding
        _close(o["mag"], mag + res.abs(), 0.0)
    ts = dict(t, aux=torch.randn(n * 3 * 2, N, generator=g).bfloat16())
    for epi in (4, 8):
        o = co.epilogue(epi, acc, mag, ts)
        full = torch.zeros(n, oh, ow, N, dtype=torch.float64)
        full[:, ::2, ::2] = ts["aux"].double().view(n, 3, 2, N)
        _close(o["exact"], (acc + full.view(M, N)) * (keep2.double() if epi == 8 else 1.0), 0.0)
    # sums: terms from a stored c, per block
    tt = dict(kshift=torch.randn(N, generator=g).float())
    d = c0 - tt["kshift"].double()
    terms = co.sum_terms(1, c0, tt)
    _close(terms[0], d, 0.0)
    _close(terms[1], d * d, 0.0)
    blocks = co.fwd_blocks(M, 4, 3)
    assert blocks.tolist()[:13] == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 0]
    s, a = co.block_sums(terms, blocks, 3)
    _close(s.sum(1), torch.stack([d.sum(0), (d * d).sum(0)]), 1e-13)
    assert bool((a >= s.abs() - 1e-12).all())


# ------------------------------------------------------------------------------------ yardstick sanity
def _sane(o, impulse=False):
    """The yardstick is within the elementwise rule of the exact oracle, and (unless exact by construction)
    differs from it."""
    bad, worst = co.elemerr(o["yard"], o["exact"], o["mag"])
    assert bad == 0, (bad, worst)
    if not impulse:
        assert co.rowerr(o["yard"], o["exact"]) > 0.0


def _fwd_oracle(case):
    t = co.fwd_inputs(case)
    assert t["share_a"] <= co.CAP and t["share_b"] <= co.CAP, (t["share_a"], t["share_b"])
    return t, co.epilogue(case["epi"], t["acc"], t["mag"], t)


@pytest.mark.parametrize("case", co.FWD_CASES, ids=co.case_id)
def test_forward_case_yardstick_and_ambiguity_caps(case):
    t, o = _fwd_oracle(case)
    impulse = case.get("kind") == "impulse"
    _sane(o, impulse)
    if case["pro"] in (co.PRO_BLOCK_OUT, co.PRO_BN_BWD):
        _sane(dict(yard=t["aout_yard"], exact=t["aout_exact"], mag=t["aout_mag"]))
    if impulse:  # bit for bit an input element or zero
        want = t["A"][:, t["kn"]]
        assert torch.equal(o["exact"], want) and torch.equal(o["yard"], want)
        assert bool(torch.isin(o["yard"], torch.cat([t["a"].double().unique(), torch.zeros(1, dtype=torch.float64)])).all())


@pytest.mark.parametrize("case", co.BIG_CASES, ids=co.case_id)
def test_conv_big_case_yardstick_and_ambiguity_caps(case):
    """The 65300 x 1024 x 256 shape: the exact GEMM is computed once per operand set and shared."""
    t, o = _fwd_oracle(case)
    _sane(o)
    if case["pro"] in (co.PRO_BLOCK_OUT, co.PRO_BN_BWD):
        _sane(dict(yard=t["aout_yard"], exact=t["aout_exact"], mag=t["aout_mag"]))


@pytest.mark.parametrize("images,H,W,C1,C2", co.DGRAD_S2_CASES)
@pytest.mark.parametrize("epi", [0, 3])
def test_dgrad_s2_case_yardstick(images, H, W, C1, C2, epi):
    t = co.dgrad_s2_inputs(images, H, W, C1, C2, epi, 31 + H + C1 + epi)
    assert t["share_a"] <= co.CAP
    _sane(co.dgrad_s2_oracle(t, images, H, W, epi))


@pytest.mark.parametrize("case", co.WGRAD_CASES, ids=co.wgrad_id)
def test_wgrad_case_yardstick_and_impulse(case):
    t = co.wgrad_inputs(case)
    assert t["share_b"] <= co.CAP, t["share_b"]
    o = co.wgrad_oracle(t["dz"], t["A"], None, t["amb"], t["ulp"])
    impulse = case.get("kind") == "impulse"
    _sane(o, impulse)
    if impulse:
        assert torch.equal(o["yard"], t["A"][t["mn"]]) and torch.equal(o["exact"], o["yard"])


@pytest.mark.parametrize("M,N,K,levels", co.DB_CASES)
def test_linear_wgrad_db_case_yardstick(M, N, K, levels):
    dz, x = co.db_inputs(M, N, K)
    o = co.wgrad_oracle(dz, x.double())
    _sane(o)
    assert bool((o["db_mag"] >= o["db"].abs()).all()) and bool((o["db_mag"] > 0).all())


@pytest.mark.parametrize("M", co.FUSED_MS)
@pytest.mark.parametrize("plain", [False, True])
def test_fused_backward_oracle_is_the_unfused_chain(M, plain):
    """conv11_bwd_fused's oracle == stage_bn_bwd, then the data-gradient GEMM with epilogue 3 and the weight
    gradient over relu(bn2(z2)), assembled from the pieces above; caps and yardstick sanity."""
    t = co.fused_inputs(M, plain, 77 + M)
    o = co.fused_oracle(t, plain)
    assert o["share_a"] <= co.CAP and o["share_b"] <= co.CAP
    _, dz3, _ = co.stage_bn_bwd(t["g"], t["z3"], t["cbwd"])
    _close(o["dz3"], dz3, 0.0)
    acc = dz3 @ t["wt"].double().t()
    a2 = t["z2"].double() if plain else co.stage_bn_relu(t["z2"], t["cf2"])[0]
    if plain:
        _close(o["gy"]["exact"], acc)
    else:
        cd = t["cf2"].double()
        _close(o["gy"]["exact"], acc * (t["z2"].double() * cd[:64] + cd[64:] > 0))
    _close(o["dw"]["exact"], dz3.t() @ a2)
    if M > 1:
        _sane(o["gy"])
    _sane(o["dw"])


# ------------------------------------------------------------------------------------ plan replay
def _native():
    """The extension, or a skip where none is built; one that is built but fails to load is an error."""
    import glob
    import os

    import ps_amd
    from ps_amd.ops import native

    if not glob.glob(os.path.join(os.path.dirname(ps_amd.__file__), "_C*.so")):
        pytest.skip("the HIP extension is not built here")
    return native()  # raises where a built extension does not load


def test_plan_replay_equals_the_bindings():
    nv = _native()
    for c in co.FWD_CASES + co.BIG_CASES:
        g = co.geo(c["H"], c["W"], c["ks"], c["stride"], c["pad"])
        M = c["images"] * g[2] * g[3]
        p = co.plan_fwd(M, c["N"], c["C"], g, c["pro"], c["epi"])
        src2 = {co.PRO_BLOCK_OUT: 1, co.PRO_BN_BWD: 2}.get(c["pro"], 0)
        assert [p["bm"], p["bn"], p["gm"]] == list(nv.conv_gemm_plan(M, c["N"], c["C"], g, c["pro"] != 0, c["epi"], src2)), c
        assert (p["family"], p["tpb"]) == (c["family"], c["tpb"]), (c, p)
        assert nv.conv_gemm_family(M, c["N"], c["C"], g, c["pro"], c["epi"]) == co.FAMILY[p["family"]], (c, p)
    for c in co.WGRAD_CASES:
        g = co.geo(c["H"], c["W"], c["ks"], c["stride"], c["pad"])
        M, K = c["images"] * g[2] * g[3], c["ks"] ** 2 * c["C"]
        p = co.plan_wgrad(M, c["N"], K, c["C"], g, c["pro"])
        assert [p[k] for k in ("kind", "tn", "tk", "tiles", "nsplit", "rows", "groups")] == \
            list(nv.conv_wgrad_plan(M, c["N"], K, c["C"], g, c["pro"])), c
        assert (p["kind"], p["levels"]) == (c["wkind"], c["levels"]), (c, p)
    for M, N, K, levels in co.DB_CASES:
        p = co.plan_wgrad(M, N, K, K, [M, 1, M, 1, 1, 1, 0], False)
        assert 1 <= p["kind"] <= 4 and p["levels"] == levels
        assert [p[k] for k in ("kind", "tn", "tk", "tiles", "nsplit", "rows", "groups")] == \
            list(nv.conv_wgrad_plan(M, N, K, K, [M, 1, M, 1, 1, 1, 0], False))
    for images, H, W, C1, C2 in co.DGRAD_S2_CASES:
        M = images * (H // 2) * (W // 2)
        assert list(nv.conv_dgrad_s2_plan(M, C1)) == [128 if C1 % 128 == 0 else 64, -(-M // 128)]
    assert nv.conv11_bwd_fused_supported(64, 256, False) and nv.conv11_bwd_fused_supported(64, 256, True)


def test_plan_replay_numbers_the_case_table_quotes():
    p = co.plan_fwd(20000, 1024, 64, [20000, 1, 20000, 1, 1, 1, 0], 0, 1)
    assert (p["tiles"], p["gm"], p["tpb"], p["nk"], p["L"]) == (157, 64, 3, 1, 3 * 8 + 2 + 2 + 3)
    p = co.plan_fwd(40001, 512, 128, [40001, 1, 40001, 1, 1, 1, 0], 0, 1)
    assert (p["tiles"], p["gm"], p["tpb"]) == (313, 128, 3)
    p = co.plan_fwd(65300, 256, 1024, [65300, 1, 65300, 1, 1, 1, 0], 0, 1)
    assert (p["family"], p["gm"], p["L"]) == ("big", 256, 28)
    assert co.plan_fused(33000) == dict(gm=256, tiles=258, tpb=2, L=38, groups=16)
    assert co.plan_fused(300)["groups"] == 0
