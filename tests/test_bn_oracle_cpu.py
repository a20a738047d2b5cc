"""tests/bn_oracle.py against torch's own batch_norm / max_pool2d in fp64 with autograd, by hand at
R = 3, its geometry replay against the numbers test_bn_rows_gpu.py's case table quotes, its bf16
yardstick against the exact variant, and its builders' assertions.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from . import bn_oracle as bo


def _close(a, b, tol=1e-11):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.double().abs().max()))


# ------------------------------------------------------------------------------------ vs autograd
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("R,C", [(3, 8), (50, 24)])
def test_bn_matches_batch_norm_autograd_fp64(R, C, with_res, act):
    c = bo.bn_inputs(R, C, 7 + R + C)
    x = c["x"].double().requires_grad_()
    res = c["res"].double().requires_grad_() if with_res else None
    ga, be = c["gamma"].double().requires_grad_(), c["beta"].double().requires_grad_()
    rm, rv = c["rm0"].double().clone(), c["rv0"].double().clone()
    y = F.batch_norm(x, rm, rv, ga, be, True, bo.MOMENTUM, bo.EPS)
    if with_res:
        y = y + res
    if act:
        y = torch.relu(y)
    y.backward(c["dy"].double())

    st = bo.stats(c["x"])
    cf = bo.coef(c["gamma"], c["beta"], st["mean"], st["invstd"])
    yo, mag = bo.apply(c["x"], cf, c["res"] if with_res else None, None, act)
    _close(yo, y.detach())
    assert bool((mag >= yo.abs() - 1e-12).all())
    rmo, rvo = bo.running(c["rm0"], c["rv0"], st["mean"], st["var"], R)
    _close(rmo, rm)
    _close(rvo, rv)
    b = bo.bn_bwd(yo > 0 if act else None, c["dy"], c["x"], c["gamma"], st["mean"], st["invstd"])
    _close(b["dx"], x.grad, 1e-9)
    _close(b["dgamma"], ga.grad, 1e-9)
    _close(b["dbeta"], be.grad, 1e-9)
    if with_res:
        _close(b["dres"], res.grad)
    assert bool((b["mag_dx"] >= b["dx"].abs() - 1e-9).all())
    assert bool((b["abs_dgamma"] >= b["dgamma"].abs() - 1e-9).all() and (b["abs_dbeta"] >= b["dbeta"].abs() - 1e-9).all())
    # the three ways a caller builds the mask agree
    if act and not with_res:
        bits = bo.mask_bits(yo)
        assert torch.equal(bo.unpack_bits(bits, yo.shape), yo > 0)
        assert torch.equal(c["x"].double() * cf[:C] + cf[C:] > 0, yo > 0)


def test_dual_apply_is_two_batch_norms():
    c = bo.bn_inputs(40, 16, 3)
    st, sr = bo.stats(c["x"]), bo.stats(c["res"])
    cf = bo.coef(c["gamma"], c["beta"], st["mean"], st["invstd"])
    g2 = c["beta"] + 1.0
    rc = bo.coef(g2, c["gamma"], sr["mean"], sr["invstd"])
    want = torch.relu(F.batch_norm(c["x"].double(), None, None, c["gamma"].double(), c["beta"].double(), True, 0.1, bo.EPS)
                      + F.batch_norm(c["res"].double(), None, None, g2.double(), c["gamma"].double(), True, 0.1, bo.EPS))
    _close(bo.apply(c["x"], cf, c["res"], rc, 1)[0], want)


@pytest.mark.parametrize("shape", bo.POOL_SHAPES, ids=str)
def test_pool_matches_max_pool2d_with_indices(shape):
    N, C, H, W, k, s, p = shape
    c = bo.pool_inputs(N, C, H, W, k, s, p, 11)
    zt = c["z"].double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    want, ind = F.max_pool2d(zt, k, s, p, return_indices=True)
    y, idx = bo.pool_fwd(c["z"], None, k, s, p)
    assert torch.equal(y.permute(0, 3, 1, 2), want.detach())
    OH, OW = y.shape[1], y.shape[2]
    t = idx.long().permute(0, 3, 1, 2)
    h = torch.arange(OH).view(1, 1, OH, 1) * s - p + t // k
    w = torch.arange(OW).view(1, 1, 1, OW) * s - p + t % k
    assert torch.equal(h * W + w, ind)  # bf16 data has ties: both keep the first tap in (kh, kw) order
    want.backward(c["dy"].double().permute(0, 3, 1, 2))
    dx, mag = bo.pool_bwd(c["dy"], idx, H, W, k, s, p)
    _close(dx.permute(0, 3, 1, 2), zt.grad)
    assert bool((mag >= dx.abs() - 1e-12).all())


def test_fused_pool_and_stem_backward_match_autograd():
    N, C, H, W = 2, 16, 6, 10
    c = bo.pool_inputs(N, C, H, W, 3, 2, 1, 5)
    sc, sh = c["mc"].double()[:C], c["mc"].double()[C:]
    y, idx = bo.pool_fwd(c["z"], c["mc"], 3, 2, 1)
    a = torch.relu(c["z"].double() * sc + sh).float().bfloat16().double().permute(0, 3, 1, 2)
    want, ind = F.max_pool2d(a, 3, 2, 1, return_indices=True)
    assert torch.equal(y.permute(0, 3, 1, 2), want)
    # stem backward: batch statistics of z, gamma = sc / invstd so that mc is the forward's own coefficients
    st = bo.stats(c["z"].view(-1, C))
    gamma = sc / st["invstd"]
    beta = sh + st["mean"] * sc
    zt = c["z"].double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    gt, bt = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    pre = torch.relu(F.batch_norm(zt, None, None, gt, bt, True, 0.1, bo.EPS))
    # route the gradient through the oracle's stored taps (ties between equal bf16 values are the forward's business)
    g, _ = bo.pool_bwd(c["dy"], idx, H, W, 3, 2, 1, rounded=True)
    pre.backward(g.permute(0, 3, 1, 2))
    out = bo.pool_bn_bwd(c["dy"], idx, c["z"], c["mc"], gamma, st["mean"], st["invstd"])
    _close(out["dx"].permute(0, 3, 1, 2), zt.grad, 1e-9)
    _close(out["dgamma"], gt.grad, 1e-9)
    _close(out["dbeta"], bt.grad, 1e-9)


# ------------------------------------------------------------------------------------ by hand
def test_by_hand_three_rows():
    """Channel 0 of a 3 x 8 tensor holds 1, 2, 6: mean 3, biased variance 14 / 3, unbiased 7."""
    x = torch.zeros(3, 8)
    x[:, 0] = torch.tensor([1.0, 2.0, 6.0])
    x[:, 1:] = torch.tensor([0.0, 1.0, 2.0])[:, None]
    x = x.bfloat16()
    st = bo.stats(x, eps=0.0)
    assert abs(st["mean"][0] - 3.0) < 1e-15 and abs(st["var"][0] - 14.0 / 3.0) < 1e-15
    assert abs(st["dm"][0] - 2.0) < 1e-15 and abs(st["absdev"][0] - 2.0) < 1e-15 and abs(st["sq"][0] - 26.0 / 3.0) < 1e-14
    is0 = (14.0 / 3.0) ** -0.5
    assert abs(st["invstd"][0] - is0) < 1e-15
    rm, rv = bo.running(torch.ones(8), torch.ones(8), st["mean"], st["var"], 3, 0.1)
    assert abs(rm[0] - (0.9 + 0.3)) < 1e-15 and abs(rv[0] - (0.9 + 0.7)) < 1e-15  # 14/3 * 3/2 = 7
    gamma, beta = torch.full((8,), 2.0), torch.full((8,), 0.5)
    cf = bo.coef(gamma, beta, st["mean"], st["invstd"])
    assert abs(cf[0] - 2 * is0) < 1e-15 and abs(cf[8] - (0.5 - 6 * is0)) < 1e-15
    y, mag = bo.apply(x, cf, None, None, 1)
    want = [max(0.0, 0.5 + 2 * is0 * (v - 3)) for v in (1.0, 2.0, 6.0)]
    assert max(abs(float(y[i, 0]) - want[i]) for i in range(3)) < 1e-15 and want[0] == 0.0 and want[2] > 0
    assert abs(float(mag[0, 0]) - (2 * is0 + abs(0.5 - 6 * is0))) < 1e-15
    bits = bo.mask_bits(y)
    # row 0 is below every channel's mean by more than beta allows; row 1 only in channel 0 (bit 0 of its byte)
    assert want[1] == 0.0 and bits.dtype == torch.uint8 and bits.tolist() == [0x00, 0xFE, 0xFF]
    # backward with dy = (1, 2, 4) and the mask (0, 1, 1) on channel 0
    dy = torch.zeros(3, 8)
    dy[:, 0] = torch.tensor([1.0, 2.0, 4.0])
    mask = torch.ones(3, 8, dtype=torch.bool)
    mask[0, 0] = False
    b = bo.bn_bwd(mask, dy.bfloat16(), x, gamma, st["mean"].float().double(), torch.full((8,), is0, dtype=torch.float64))
    xh = [(v - 3) * is0 for v in (1.0, 2.0, 6.0)]
    sd, sx = 6.0, 2 * xh[1] + 4 * xh[2]
    assert abs(b["dbeta"][0] - sd) < 1e-14 and abs(b["dgamma"][0] - sx) < 1e-14
    assert abs(b["abs_dgamma"][0] - (2 * abs(xh[1]) + 4 * abs(xh[2]))) < 1e-14 and abs(b["abs_dbeta"][0] - 6.0) < 1e-14
    for i, dz in enumerate((0.0, 2.0, 4.0)):
        want_dx = 2 * is0 * (dz - sd / 3 - xh[i] * sx / 3)
        assert abs(float(b["dx"][i, 0]) - want_dx) < 1e-13
        assert float(b["dres"][i, 0]) == dz
    ca, cb, cc = b["coef"][0], b["coef"][8], b["coef"][16]
    assert abs(ca - 2 * is0) < 1e-15 and abs(cb + 2 * is0 * is0 * sx / 3) < 1e-14
    assert abs(cc - (-2 * is0 * 2.0 + 2 * is0 * is0 * sx / 3 * 3.0)) < 1e-13


# ------------------------------------------------------------------------------------ geometry
GEOM = {  # the numbers quoted in test_bn_rows_gpu.py's case table
    (3, 8): dict(G=1, rows_per_block=3, rows_thread=1, full=False, tail=True, empty=0),
    (392, 136): dict(G=49, rows_per_block=8, rows_it=8, rows_thread=1, fixed_c=False, ctiles=1),
    (999, 192): dict(rows_per_block=8, rows_it=8, fixed_c=False, tail=True, ctiles=1),
    (392, 2048): dict(ctiles=8, fixed_c=True, rows_per_block=8),
    (4096, 64): dict(tail=False, full=True, fixed_c=True),
    (20000, 256): dict(G=2048, rows_per_block=10, rows_it=8, empty=48, pass2=1, pass4=0, rows_thread=2),
    (50000, 256): dict(G=2048, rows_per_block=25, rows_it=8, empty=48, pass4=1, tail4=0, rows_thread=4),
    (70000, 136): dict(G=2048, rows_per_block=35, rows_it=8, pass4=1, tail4=1, fixed_c=False),
    (26001, 264): dict(G=1024, ctiles=2, rows_per_block=26, empty=23, pass4=1, tail4=0, fin_threads=512),
    (270001, 64): dict(G=2048, rows_per_block=132, rows_it=32, empty=2, pass4=1, tail4=1, rows_thread=5),
    (1600003, 8): dict(G=2048, rows_per_block=782, rows_it=256, pass4=1, tail4=0, rows_thread=4, fin_threads=512),
}


@pytest.mark.parametrize("shape", sorted(GEOM), ids=str)
def test_geometry_matches_case_table(shape):
    g = bo.geometry(*shape)
    for key, want in GEOM[shape].items():
        assert g[key] == want, (shape, key, g[key], want)
    want_L = (g["rows_thread"] + g["rows_it"] - 1 + -(-g["G"] // g["fin_threads"]) + 6 + g["fin_threads"] // 64 - 1 + 3)
    assert g["L"] == want_L
    assert set(GEOM) == set(bo.BN_SHAPES + bo.BN_BIG_SHAPES) and bo.BN_SHIFT_SHAPE in GEOM


def test_geometry_against_a_direct_replay_of_the_loops():
    """rows of thread row r0 in a full block, counted by walking the kernel's two loops."""
    for R, C in sorted(GEOM):
        g = bo.geometry(R, C)
        step, rpb = g["rows_it"], g["rows_per_block"]
        for U, pk, tk in ((4, "pass4", "tail4"), (2, "pass2", "tail2")):
            r, n = 0, 0
            while r + (U - 1) * step < rpb:
                r, n = r + U * step, n + 1
            t = 0
            while r < rpb:
                r, t = r + step, t + 1
            assert (n, t) == (g[pk], g[tk]) and U * n + t == g["rows_thread"]
        assert g["empty"] == sum(1 for b in range(g["G"]) if b * rpb >= R)


def test_pool_geometry_matches_case_table():
    want = {(2, 64, 9, 9, 3, 2, 1): ("flat", "row", "s2k3", "k3"), (2, 64, 10, 12, 2, 2, 0): ("flat", "row", "generic", "generic"),
            (1, 128, 9, 8, 3, 1, 1): ("row", "row", "generic", "k3"), (3, 24, 10, 10, 3, 2, 1): ("flat", "flat", "quad", "k3"),
            (2, 8, 6, 4, 3, 2, 1): ("flat", "flat", "quad", "k3"), (2, 64, 10, 16, 2, 2, 0): ("row", "row", "generic", "generic")}
    assert set(want) == set(bo.POOL_SHAPES)
    for shape, w in want.items():
        g = bo.pool_geometry(*shape)
        assert (g["fwd"], g["bwd"], g["bwd_kernel"], g["fwd_bn_kernel"]) == w, (shape, g)


# ------------------------------------------------------------------------------------ yardstick, builders
@pytest.mark.parametrize("kind,R,C", [("randn", 3, 8), ("randn", 392, 136), ("shift", 3000, 64), ("outlier", 3000, 64)])
def test_yardstick_within_elemerr_of_exact(kind, R, C):
    c = bo.bn_inputs(R, C, 21 + R, kind)
    st = bo.stats(c["x"])
    if kind == "outlier":
        assert bool((st["dm"].abs() > 3 * st["var"].sqrt()).all())  # K = x[0] really is a poor shift
    cf = bo.coef(c["gamma"], c["beta"], st["mean"], st["invstd"])
    rc = bo.coef(c["beta"], c["gamma"], st["mean"], st["invstd"])
    for res, rcoef, act in ((None, None, 0), (c["res"], None, 1), (c["res"], rc, 1)):
        y_e, mag = bo.apply(c["x"], cf, res, rcoef, act)
        y_y, _ = bo.apply(c["x"], cf, res, rcoef, act, rounded=True)
        assert bo.elemerr(y_y, y_e, mag)[0] == 0
        assert torch.equal(y_y, bo.bf16r(y_y))
    mean, invstd = st["mean"].float(), st["invstd"].float()
    mask = bo.apply(c["x"], cf, None, None, 1)[0] > 0
    for m in (None, mask):
        e = bo.bn_bwd(m, c["dy"], c["x"], c["gamma"], mean, invstd)
        y = bo.bn_bwd(m, c["dy"], c["x"], c["gamma"], mean, invstd, rounded=True)
        bad, worst = bo.elemerr(y["dx"], e["dx"], e["mag_dx"])
        assert bad == 0 and worst < 0.6  # half a bf16 ulp is 2^-9 <= 2^-7 |ref|... : far inside
        assert torch.equal(y["dgamma"], e["dgamma"]) and torch.equal(y["dres"], e["dres"])
        assert torch.equal(y["dres"], bo.bf16r(y["dres"]))  # the masked dy is a bf16 number


def test_pool_yardstick_within_elemerr_of_exact():
    for N, C, H, W in bo.POOL_BN_SHAPES:
        c = bo.pool_inputs(N, C, H, W, 3, 2, 1, 9)
        _, idx = bo.pool_fwd(c["z"], c["mc"], 3, 2, 1)
        st = bo.stats(c["z"].view(-1, C))
        e = bo.pool_bn_bwd(c["dy"], idx, c["z"], c["mc"], c["gamma"], st["mean"].float(), st["invstd"].float())
        y = bo.pool_bn_bwd(c["dy"], idx, c["z"], c["mc"], c["gamma"], st["mean"].float(), st["invstd"].float(), rounded=True)
        assert bo.elemerr(y["dx"], e["dx"], e["mag_dx"])[0] == 0
        d_e, mag = bo.pool_bwd(c["dy"], idx, H, W, 3, 2, 1)
        d_y, _ = bo.pool_bwd(c["dy"], idx, H, W, 3, 2, 1, rounded=True)
        assert bo.elemerr(d_y, d_e, mag)[0] == 0


def test_ambiguity_assertion_fires_and_settle_moves_the_element():
    x = torch.full((4, 8), 1.5).bfloat16()
    cf = torch.cat([torch.full((8,), 2.0), torch.full((8,), -3.0)])
    x[2, 5] = 3.0  # unambiguous
    assert int(bo.ambiguous(x, cf).sum()) == 31
    with pytest.raises(AssertionError, match="ambiguous"):
        bo.assert_unambiguous(x, cf)
    y = bo.settle(x, cf)
    assert float(y[0, 0]) == 1.5 + 2.0 ** -7 and float(y[2, 5]) == 3.0
    bo.assert_unambiguous(y, cf)
    # a near miss that fp32 could still get wrong: x sc + sh = 2^-23 relative
    cf2 = torch.cat([torch.full((8,), 2.0), torch.full((8,), -3.0 * (1 + 2.0 ** -24))]).double()
    assert bool(bo.ambiguous(x[:1], cf2).all())


def test_builders_assert_their_preconditions():
    with pytest.raises(AssertionError):
        bo.bn_inputs(1, 8, 0)  # one row: zero variance
    with pytest.raises(AssertionError, match="outside"):
        bo.pool_bwd(torch.ones(1, 2, 2, 8).bfloat16(), torch.zeros(1, 2, 2, 8, dtype=torch.uint8), 4, 4, 3, 2, 1)
