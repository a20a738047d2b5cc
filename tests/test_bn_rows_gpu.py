"""The NHWC BatchNorm kernels (csrc/kernels/bn_act.hip) and the max-pool / fused stem-backward kernels
(csrc/kernels/pool.hip) element by element against the fp64 oracles of tests/bn_oracle.py, on every
dispatch path of their launchers.  native() entry points are called directly, and each backward is
given the oracle's mean / invstd / y / bits, so every kernel is judged on its own.

Bounds
  bf16 tensors   (y, dx, dres, dz, pool dx)  no element with |kernel - yardstick| > 2^-6 |yardstick|
                 + 2^-14 mag, and rowerr(kernel, exact) <= 3 rowerr(yardstick, exact).
                 y of bn_act_fwd is judged with the [scale | shift] the kernel returned, which are
                 themselves judged by the rules below.
  fp32 sums      (dgamma, dbeta)  |got - oracle| <= 2^-24 L sum|terms|, L = geometry()["L"]: the
                 roundings on the longest addition chain, ceil(rows_per_block / rows_it) in registers
                 + (rows_it - 1) in the serial LDS fold + ceil(G / fin_threads) in sum_partials8 + 6
                 in wave_sum + (waves - 1) + 3 inside a term.  pool_bn_bwd: 4 pixels per quad and
                 ceil(quads / (256 G)) quads per thread in registers, 256 / (C / 8) - 1 in its LDS
                 fold, then the same finalize.
  mean           within dmean = 2^-24 (L absdev + 2 |mean|): the sum of x - K (K = x[0]) costs
                 2^-24 L mean|x - K|, the division and K + dm one rounding each.
  variance       within dvar = 2^-24 L (sq + dm^2), sq = mean (x - K)^2.  The kernel returns invstd,
                 not the variance, so the rule is applied as
  invstd         relative rho = dvar / (2 (var + eps)) + 2^-22  (d v^-1/2 = -1/2 v^-3/2 dv; 2^-22
                 covers + eps, rsqrtf and the rounding of var itself).
  scale, shift   scale = gamma invstd:  |d scale| <= |scale| (rho + 2^-24)
                 shift = beta - mean scale:  |d shift| <= |scale| dmean + |mean scale| (rho + 3 2^-24)
                                                          + 2^-24 |shift|
                 eval mode: the same with dmean = 0 and rho = 2^-22 (invstd from the running variance).
  ca, cb, cc     (bn_bwd_coef; dsd, dsx the errors of the two sums, 0 when the partials are given)
                 ca = gamma invstd:        |d ca| <= 2^-24 |ca|
                 cb = -ca invstd sx / R:   |d cb| <= |ca invstd| dsx / R + 4 2^-24 |cb|
                 cc = -ca sd / R + ca invstd (sx / R) mean:
                                           |d cc| <= |ca| dsd / R + |ca invstd mean| dsx / R
                                                     + 5 2^-24 (|ca sd / R| + |ca invstd mean sx / R|)
  running stats  within 2^-22 relative of (1 - m) r0 + m (the kernel's own mean | variance R / (R - 1)).
                 The kernel's variance is recovered from what it returns, as invstd^-2 - eps.  The
                 builder gives r0 the sign of the mean, so "relative to the update" and "relative to
                 its terms" coincide.
  exact          mask bits == (y_kernel > 0);  pool forward value and FIRST argmax tap;  dres ==
                 masked dy bit for bit;  dgamma / dbeta of bn_bwd_partials == the partials they were
                 given (G = 1);  every output identical on a second call.

Cases -> path (R x C; numbers from bn_oracle.geometry, re-checked by test_bn_oracle_cpu.py)
  3 x 8          G = 1, one live thread row, R / (R - 1) = 1.5, nvec = 3 < 256: apply takes only the tail
  392 x 136      C / 8 = 17 inside tpr 32 (idle lanes), FIXED_C false
  999 x 192      C / 8 = 24, FIXED_C false, apply tail
  392 x 2048     8 channel tiles, FIXED_C true
  4096 x 64      nvec an exact multiple of 512: apply has no tail
  20000 x 256    G = 2048, rows_per_block 10, 48 empty blocks; the 2-deep loop of bn_bwd_reduce<1>
                 runs and the 4-deep loops do not
  26001 x 264    two channel tiles, the second with one live group; G = 1024, rows_per_block 26, 23
                 empty blocks
  50000 x 256 *  rows_per_block 25: one 4-deep pass for thread row 0, tails of 3 rows elsewhere, 48
                 empty blocks
  70000 x 136 *  the same with idle lanes, rows_per_block 35 (a 4-deep pass plus a tail row)
  270001 x 64 *  G = ceil(R / 128) capped at 2048, rows_per_block 132, rows_it 32: a 4-deep pass for
                 every thread row plus a tail row for thread rows 0 - 3, 2 empty blocks
  1600003 x 8 *  tpr 1, rows_it 256: 255-step LDS fold, rows_per_block 782
  50000 x 256 *  with x = 50 + 0.05 randn ('shift'), and again with x[0] a 6-sigma outlier
                 ('outlier'): the shifted sums where K = x[0] is a good and a poor shift; the bound
                 scales with sq + dm^2, so both are judged by the same rule
  Every case runs bn_act_fwd training {res, no res} x {relu, none} (* relu + res; none without),
  bn_act_fwd eval, bn_stats, bn_apply_coef {no res, res, res + rcoef} x {act 0, 1} x {mask, no
  mask} (* res + rcoef + act 1 + mask), bn_act_bwd with act 0, act 1 from y, act 1 from mask_coef
  (ACT 2), act 3 from bits, each with and without dres where the binding allows, and affine false
  once (* ACT 1 + dres; ACT 2; ACT 3), and bn_bwd_partials / bn_bwd_coef with the oracle's sums.
  The starred cases are the six largest and run the starred variants only.

Pool cases (N, C, H, W, k, s, p); forward with and without coefficients, backward against pool_bwd
  (2, 64, 9, 9, 3, 2, 1)     odd size, W C / 8 = 72: row-mapped bwd_kernel<., true>; forward K3, flat
  (2, 64, 10, 12, 2, 2, 0)   row-mapped generic backward; BN non-K3 forward, flat (OW C / 8 = 48)
  (1, 128, 9, 8, 3, 1, 1)    row-mapped generic backward with up to 9 covering windows; row-mapped K3 forward
  (2, 64, 10, 16, 2, 2, 0)   OW C / 8 = 64: the BN non-K3 forward with the row mapping (added: the
                             two cases above leave that kernel on the flat mapping)
  (3, 24, 10, 10, 3, 2, 1)   C / 8 = 3: flat mapping, quad kernel
  (2, 8, 6, 4, 3, 2, 1)      quad kernel where OH - 1 is clamped
  (2, 64, 16, 16), (3, 32, 6, 10)   pool_bn_bwd against the pool_bn_bwd oracle; (2, 64, 16, 16) again
                             with dy nonzero in only the last output row and column (the clamped windows)

Observed on MI355X (271 tests, 70 s wall for the file), over all cases of an output:
rowerr(kernel) / rowerr(yardstick) (the bound is 3), in brackets the yardstick's own rowerr, and the
worst |kernel - yardstick| as a share of the elementwise tolerance (the bound is 1; no element was
outside it):

    fwd.y        1.00 (0.0016 - 0.0037)  0.49      bwd.dx       1.00 (0.0011 - 0.0037)  0.49
    eval.y       1.00 (0.0016 - 0.0037)  0.00      partials.dx  1.00 (0.0017 - 0.0037)  0.49
    apply.y      1.00 (0.0016 - 0.0037)  0.49      stem.dz      1.00 (0.0024 - 0.0027)  0.29
    pool.dx      1.00 (0 - 0.0034)       0.00

The ratio is 1.00 in every case to the printed digits: the kernels round where the yardstick does.
fp32 outputs, worst share of their bound: mean 0.32, invstd 0.13, scale 0.46, shift 0.34, running
mean 0.56, running variance 0.59, dgamma 0.12, dbeta 0.11, stem dgamma 0.05, stem dbeta 0.01,
ca | cb | cc 0.99 (ca's bound is the one rounding of gamma invstd: a share near 1 is half an ulp).
No bound had to be widened and no kernel finding came out of these cases.
"""
import functools

import pytest
import torch

from ps_amd.ops import native

from . import bn_oracle as bo

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 3.0
U22 = 2.0 ** -22

SMALL = [(R, C, "randn") for R, C in bo.BN_SHAPES]
BIG = [(R, C, "randn") for R, C in bo.BN_BIG_SHAPES] + [bo.BN_SHIFT_SHAPE + ("shift",), bo.BN_SHIFT_SHAPE + ("outlier",)]


def _cid(c):
    return f"{c[0]}x{c[1]}" + ("" if c[2] == "randn" else "-" + c[2])


def _variants(small, starred):
    """(case, variant) for every variant on the small cases and the starred ones on the big cases."""
    return [(c, v) for c in SMALL for v in small] + [(c, v) for c in BIG for v in starred]


def _vid(cv):
    return _cid(cv[0]) + "-" + "-".join(str(v) for v in cv[1])


def _dev(t):
    return t.to(DEV) if t is not None else None


def _bf16_bounds(name, tag, got, exact, yard, mag=None):
    got = got.cpu()
    assert got.shape == yard.shape and got.dtype == torch.bfloat16
    e, y = bo.rowerr(got, exact), bo.rowerr(yard, exact)
    bad, worst = bo.elemerr(got, yard, mag)
    print(f"RATIO {name} {tag}: kernel {e:.5f} yardstick {y:.5f} ratio {e / y if y else float(e > 0):.2f} "
          f"elemerr bad {bad} worst {worst:.2f}")
    assert e <= FACTOR * y, (name, e, y)  # a yardstick without error (one addend per element) leaves none to the kernel
    assert bad == 0, (name, bad, worst)


def _within(name, tag, got, ref, tol):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff = (got - ref).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / tol.clamp_min(1e-300)).max().item()
    print(f"SUM {name} {tag}: worst {ratio:.3f} of the bound")
    assert bool(torch.isfinite(got).all()) and bool((diff <= tol).all()), (name, ratio)


def _same(a, b):
    for u, v in zip(a, b):
        if u is None or not isinstance(u, torch.Tensor) or u.numel() == 0:
            continue
        assert torch.equal(u, v), "a second call gave a different result"


# ------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def _case(R, C, kind):
    """Inputs and forward oracle of one case, computed once and left unchanged."""
    c = bo.bn_inputs(R, C, 100 + R + C, kind)
    st = bo.stats(c["x"])
    c.update(st=st, geo=bo.geometry(R, C), mean32=st["mean"].float(), invstd32=st["invstd"].float())
    return c


@functools.lru_cache(maxsize=None)
def _y_relu(R, C, kind, with_res):
    """The forward's bf16 output relu(bn(x) [+ res]) from the fp32 coefficients mc: what a backward reads."""
    c = _case(R, C, kind)
    return bo.apply(c["x"], c["mc"], c["res"] if with_res else None, None, 1, rounded=True)[0].to(torch.bfloat16)


def _check_stats(tag, c, R, mean, invstd, coef, rm, rv, training=True):
    st, L, C = c["st"], c["geo"]["L"], c["x"].shape[1]
    if training:
        dmean = bo.U24 * (L * st["absdev"] + 2 * st["mean"].abs())
        dvar = bo.U24 * L * (st["sq"] + st["dm"].pow(2))
        rho = dvar / (2 * (st["var"] + bo.EPS)) + U22
        m_o, is_o = st["mean"], st["invstd"]
        _within("fwd.mean", tag, mean, m_o, dmean)
        _within("fwd.invstd", tag, invstd, is_o, rho * is_o)
        # running statistics from the kernel's own mean and (recovered) variance
        mk, isk = mean.cpu().double(), invstd.cpu().double()
        vk = isk.pow(-2) - bo.EPS
        rm_u, rv_u = bo.running(c["rm0"], c["rv0"], mk, vk, R)
        _within("fwd.rmean", tag, rm, rm_u, U22 * rm_u.abs())
        _within("fwd.rvar", tag, rv, rv_u, U22 * rv_u.abs())
    else:
        dmean, rho = torch.zeros(C, dtype=torch.float64), torch.full((C,), U22, dtype=torch.float64)
        m_o, is_o = c["rm0"].double(), (c["rv0"].double() + bo.EPS).rsqrt()
        assert torch.equal(rm.cpu(), c["rm0"]) and torch.equal(rv.cpu(), c["rv0"])  # eval leaves them alone
    cf = bo.coef(c["gamma"], c["beta"], m_o, is_o)
    sc, sh = cf[:C], cf[C:]
    assert coef.shape == (2 * C,) and coef.dtype == torch.float32
    _within("fwd.scale", tag, coef[:C], sc, sc.abs() * (rho + bo.U24))
    _within("fwd.shift", tag, coef[C:], sh, sc.abs() * dmean + (m_o * sc).abs() * (rho + 3 * bo.U24) + bo.U24 * sh.abs())


# ------------------------------------------------------------------------------------ forward
FWD = _variants([(r, a) for r in ("res", "nores") for a in (1, 0)], [("res", 1), ("nores", 0)])


@pytest.mark.parametrize("cv", FWD, ids=_vid)
def test_bn_act_fwd_training(cv):
    (R, C, kind), (rmode, act) = cv
    c, tag = _case(R, C, kind), _vid(cv)
    res = c["res"] if rmode == "res" else None
    x, rs, ga, be = _dev(c["x"]), _dev(res), _dev(c["gamma"]), _dev(c["beta"])

    def run():
        rm, rv = _dev(c["rm0"]).clone(), _dev(c["rv0"]).clone()
        return native().bn_act_fwd(x, rs, ga, be, rm, rv, True, bo.MOMENTUM, bo.EPS, act) + [rm, rv]

    out = run()
    _same(out, run())
    y, mean, invstd, coef, rm, rv = out
    _check_stats(tag, c, R, mean, invstd, coef, rm, rv)
    y_e, mag = bo.apply(c["x"], coef.cpu(), res, None, act)
    y_y, _ = bo.apply(c["x"], coef.cpu(), res, None, act, rounded=True)
    _bf16_bounds("fwd.y", tag, y, y_e, y_y, mag)


@pytest.mark.parametrize("case", SMALL + BIG, ids=_cid)
def test_bn_act_fwd_eval(case):
    R, C, kind = case
    c, tag = _case(*case), _cid(case)
    rm, rv = _dev(c["rm0"]).clone(), _dev(c["rv0"]).clone()
    args = (_dev(c["x"]), None, _dev(c["gamma"]), _dev(c["beta"]), rm, rv, False, bo.MOMENTUM, bo.EPS, 1)
    y, _, _, coef = native().bn_act_fwd(*args)
    y2, _, _, coef2 = native().bn_act_fwd(*args)
    _same([y, coef], [y2, coef2])
    _check_stats(tag, c, R, None, None, coef, rm, rv, training=False)
    y_e, mag = bo.apply(c["x"], coef.cpu(), None, None, 1)
    y_y, _ = bo.apply(c["x"], coef.cpu(), None, None, 1, rounded=True)
    _bf16_bounds("eval.y", tag, y, y_e, y_y, mag)


@pytest.mark.parametrize("case", SMALL + BIG, ids=_cid)
def test_bn_stats(case):
    R, C, kind = case
    c, tag = _case(*case), _cid(case)

    def run():
        rm, rv = _dev(c["rm0"]).clone(), _dev(c["rv0"]).clone()
        return native().bn_stats(_dev(c["x"]), _dev(c["gamma"]), _dev(c["beta"]), rm, rv, True, bo.MOMENTUM, bo.EPS) + [rm, rv]

    out = run()
    _same(out, run())
    mean, invstd, coef, rm, rv = out
    _check_stats(tag, c, R, mean, invstd, coef, rm, rv)


APPLY = _variants([(r, a, m) for r in ("nores", "res", "rcoef") for a in (0, 1) for m in ("mask", "nomask")],
                  [("rcoef", 1, "mask")])


@pytest.mark.parametrize("cv", APPLY, ids=_vid)
def test_bn_apply_coef(cv):
    (R, C, kind), (rmode, act, mmode) = cv
    c, tag = _case(R, C, kind), _vid(cv)
    res = None if rmode == "nores" else c["res"]
    # the identity branch's own coefficients: any per-channel [scale | shift] will do
    rcoef = torch.cat([c["rv0"], c["beta"] - 0.25]).contiguous() if rmode == "rcoef" else None
    args = (_dev(c["x"]), _dev(c["mc"]), _dev(res), _dev(rcoef), act, mmode == "mask")
    y, mb = native().bn_apply_coef(*args)
    _same([y, mb], native().bn_apply_coef(*args))
    y_e, mag = bo.apply(c["x"], c["mc"], res, rcoef, act)
    y_y, _ = bo.apply(c["x"], c["mc"], res, rcoef, act, rounded=True)
    _bf16_bounds("apply.y", tag, y, y_e, y_y, mag)
    if mmode == "mask":
        assert mb.dtype == torch.uint8 and mb.shape == (R * C // 8,)
        assert torch.equal(mb.cpu(), bo.mask_bits(y.cpu()))
    else:
        assert mb is None or mb.numel() == 0


# ------------------------------------------------------------------------------------ backward
# (mask source, dres, affine): act 0 | act 1 from y | act 1 from mask_coef (ACT 2, no residual) | act 3 from bits
BWD = _variants([("none", False, True), ("none", True, True), ("y", False, True), ("y", True, True), ("mc", False, True),
                 ("bits", False, True), ("bits", True, True), ("y", False, False)],
                [("y", True, True), ("mc", False, True), ("bits", False, True)])


def _bwd_inputs(c, R, C, kind, src, dres):
    """-> (bool mask or None, the bn_act_bwd arguments y, act, mask_coef, mbits)."""
    if src == "none":
        return None, None, 0, None, None
    if src == "mc":
        bo.assert_unambiguous(c["x"], c["mc"])
        mc = c["mc"].double()
        return c["x"].double() * mc[:C] + mc[C:] > 0, None, 1, c["mc"], None
    y = _y_relu(R, C, kind, dres)
    if src == "y":
        return y > 0, y, 1, None, None
    return y > 0, None, 3, None, bo.mask_bits(y)


@pytest.mark.parametrize("cv", BWD, ids=_vid)
def test_bn_act_bwd(cv):
    (R, C, kind), (src, dres, affine) = cv
    c, tag = _case(R, C, kind), _vid(cv)
    mask, y, act, mc, bits = _bwd_inputs(c, R, C, kind, src, dres)
    gamma = c["gamma"] if affine else None
    args = (_dev(c["dy"]), _dev(y), _dev(c["x"]), _dev(gamma), _dev(c["mean32"]), _dev(c["invstd32"]), act, dres,
            affine, _dev(mc), _dev(bits))
    out = native().bn_act_bwd(*args)
    _same(out, native().bn_act_bwd(*args))
    dx, dr, dg, db = out
    e = bo.bn_bwd(mask, c["dy"], c["x"], gamma, c["mean32"], c["invstd32"])
    yd, _ = bo.bwd_apply(e["dres"], c["x"], e["coef"], rounded=True)
    _bf16_bounds("bwd.dx", tag, dx, e["dx"], yd, e["mag_dx"])
    if dres:
        assert dr.dtype == torch.bfloat16 and torch.equal(dr.cpu().double(), e["dres"])  # the masked dy, bit for bit
    else:
        assert dr is None or dr.numel() == 0
    if affine:
        L = c["geo"]["L"]
        _within("bwd.dgamma", tag, dg, e["dgamma"], bo.U24 * L * e["abs_dgamma"])
        _within("bwd.dbeta", tag, db, e["dbeta"], bo.U24 * L * e["abs_dbeta"])
    else:
        assert (dg is None or dg.numel() == 0) and (db is None or db.numel() == 0)


def _coef3_bounds(c3, mean, invstd, sd, sx, R, dsd, dsx):
    C = mean.shape[0]
    ca, cb = c3[:C], c3[C:2 * C]
    is_, mu = invstd.double(), mean.double()
    t1, t2 = (ca * sd / R).abs(), (ca * is_ * mu * sx / R).abs()
    return torch.cat([bo.U24 * ca.abs(), (ca * is_).abs() * dsx / R + 4 * bo.U24 * cb.abs(),
                      ca.abs() * dsd / R + (ca * is_ * mu).abs() * dsx / R + 5 * bo.U24 * (t1 + t2)])


@pytest.mark.parametrize("case", SMALL + BIG, ids=_cid)
def test_bn_bwd_partials_and_coef(case):
    """bn_bwd_partials / bn_bwd_coef (the finalize + apply behind the GEMM epilogues' partial sums) given the
    oracle's two sums as one partial row: the sums come back unchanged, the coefficients are a few
    roundings from the oracle's, and dx = ca g + cb x + cc is bn_bwd_apply_kernel<0, false, .>."""
    R, C, kind = case
    c, tag = _case(*case), _cid(case)
    y = _y_relu(R, C, kind, True)
    g = torch.where(y > 0, c["dy"], torch.zeros_like(c["dy"]))  # the masked gradient a producer hands over
    e = bo.bn_bwd(None, g, c["x"], c["gamma"], c["mean32"], c["invstd32"])
    part = torch.stack([e["dbeta"], e["dgamma"]]).float().view(2, 1, C).contiguous()
    sd, sx = part[0, 0].double(), part[1, 0].double()
    c3 = bo.bwd_coef(sd, sx, c["gamma"], c["mean32"], c["invstd32"], R)
    args = (_dev(g), _dev(c["x"]), _dev(part), _dev(c["gamma"]), _dev(c["mean32"]), _dev(c["invstd32"]))
    out = native().bn_bwd_partials(*args)
    _same(out, native().bn_bwd_partials(*args))
    dx, dg, db = out
    assert torch.equal(dg.cpu(), part[1, 0]) and torch.equal(db.cpu(), part[0, 0])
    dg2, db2, coef = native().bn_bwd_coef(_dev(part), _dev(c["gamma"]), _dev(c["mean32"]), _dev(c["invstd32"]), R)
    assert torch.equal(dg2, dg) and torch.equal(db2, db)
    zero = torch.zeros(C, dtype=torch.float64)
    _within("bwd.coef", tag, coef, c3, _coef3_bounds(c3, c["mean32"], c["invstd32"], sd, sx, R, zero, zero))
    d_e, mag = bo.bwd_apply(g, c["x"], c3)
    d_y, _ = bo.bwd_apply(g, c["x"], c3, rounded=True)
    _bf16_bounds("partials.dx", tag, dx, d_e, d_y, mag)


def test_bn_act_bwd_short_gamma_raises():
    c = _case(392, 136, "randn")
    with pytest.raises(RuntimeError, match="gamma size"):
        native().bn_act_bwd(_dev(c["dy"]), None, _dev(c["x"]), _dev(c["gamma"][:128]), _dev(c["mean32"]),
                            _dev(c["invstd32"]), 0, False, True, None, None)


# ------------------------------------------------------------------------------------ pool
@functools.lru_cache(maxsize=None)
def _pool_case(shape):
    N, C, H, W, k, s, p = shape
    c = bo.pool_inputs(N, C, H, W, k, s, p, 300 + H + W + C)
    c["plain"] = bo.pool_fwd(c["z"], None, k, s, p)
    c["bn"] = bo.pool_fwd(c["z"], c["mc"], k, s, p)
    return c


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("shape", bo.POOL_SHAPES, ids=str)
def test_maxpool_fwd_value_and_first_argmax_exact(shape, bn):
    N, C, H, W, k, s, p = shape
    c = _pool_case(shape)
    args = (_dev(c["z"]), _dev(c["mc"]) if bn else None, k, s, p)
    y, idx = native().maxpool_nhwc_fwd(*args)
    _same([y, idx], native().maxpool_nhwc_fwd(*args))
    y_o, idx_o = c["bn" if bn else "plain"]
    assert y.dtype == torch.bfloat16 and torch.equal(y.cpu().double(), y_o)
    assert idx.dtype == torch.uint8 and torch.equal(idx.cpu(), idx_o)


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("shape", bo.POOL_SHAPES, ids=str)
def test_maxpool_bwd(shape, bn):
    """The gather backward against the fp64 scatter by the stored taps; the taps are the oracle's (after the
    ReLU, idx holds long runs of tap 0 where a whole window is zero)."""
    N, C, H, W, k, s, p = shape
    c, tag = _pool_case(shape), f"{shape}-{'bn' if bn else 'plain'}"
    idx = c["bn" if bn else "plain"][1]
    dx = native().maxpool_nhwc_bwd(_dev(c["dy"]), _dev(idx), H, W, k, s, p)
    assert torch.equal(dx, native().maxpool_nhwc_bwd(_dev(c["dy"]), _dev(idx), H, W, k, s, p))
    d_e, mag = bo.pool_bwd(c["dy"], idx, H, W, k, s, p)
    d_y, _ = bo.pool_bwd(c["dy"], idx, H, W, k, s, p, rounded=True)
    _bf16_bounds("pool.dx", tag, dx.view(-1, C), d_e.view(-1, C), d_y.view(-1, C), mag.view(-1, C))


def _pool_L(N, C, H, W):
    cv = C // 8
    quads = N * (H // 2) * (W // 2) * cv
    G = max(1, min(2048, (quads + 255) // 256))
    fin = 1024 if G >= 4096 else 512 if G >= 1024 else 256
    return 4 * -(-quads // (256 * G)) + (256 // cv - 1) + -(-G // fin) + 6 + (fin // 64 - 1) + 3


@pytest.mark.parametrize("shape,edge", [(s, False) for s in bo.POOL_BN_SHAPES] + [(bo.POOL_BN_SHAPES[0], True)],
                         ids=lambda v: str(v))
def test_pool_bn_bwd(shape, edge):
    N, C, H, W = shape
    c, tag = _pool_case((N, C, H, W, 3, 2, 1)), f"{shape}{'-edge' if edge else ''}"
    idx = c["bn"][1]
    dy = c["dy"]
    if edge:  # only the windows that the quad loop clamps contribute
        dy = torch.zeros_like(dy)
        dy[:, -1], dy[:, :, -1] = c["dy"][:, -1], c["dy"][:, :, -1]
    st = bo.stats(c["z"].view(-1, C))
    mean, invstd = st["mean"].float(), st["invstd"].float()
    args = (_dev(dy), _dev(idx), _dev(c["z"]), _dev(c["mc"]), _dev(c["gamma"]), _dev(mean), _dev(invstd))
    out = native().pool_bn_bwd(*args)
    _same(out, native().pool_bn_bwd(*args))
    dz, dg, db = out
    e = bo.pool_bn_bwd(dy, idx, c["z"], c["mc"], c["gamma"], mean, invstd)
    y = bo.pool_bn_bwd(dy, idx, c["z"], c["mc"], c["gamma"], mean, invstd, rounded=True)
    _bf16_bounds("stem.dz", tag, dz.view(-1, C), e["dx"].view(-1, C), y["dx"].view(-1, C), e["mag_dx"].view(-1, C))
    L = _pool_L(N, C, H, W)
    _within("stem.dgamma", tag, dg, e["dgamma"], bo.U24 * L * e["abs_dgamma"])
    _within("stem.dbeta", tag, db, e["dbeta"], bo.U24 * L * e["abs_dbeta"])
