"""The fused transformer row kernels (csrc/kernels/transformer.hip) element by element and row by
row against the fp64 oracles of tests/transformer_oracle.py, on every dispatch path of the
launchers.  native() entry points are called directly: layernorm_fwd / layernorm_bwd with an
explicit seed, and both backwards with the oracle's s / mean / rstd, so each is judged on its own.

Bounds (the same for every kernel)
  bf16 outputs   rowerr(kernel, exact) <= 3 rowerr(yardstick, exact) per row, and no element with
                 |kernel - yardstick| > 2^-6 |yardstick| + 2^-14 mag (transformer_oracle.elemerr).
  bit-exact      v of rope_split, the dv part of dqkv, s without dropout and at p = 0.5 (one bf16
                 + bf16 sum, rounded once; 1 / (1 - 0.5) is exact), do == dx at p = 0.
  s at p = 0.1   1 / (1 - p) is not exact and x + o * m may be contracted into one fma: at most
                 1e-3 of the elements may differ from bf16(fp64 value), and none by more than one
                 bf16 ulp + 2^-22 |o m|.  The second term matters only where x and o m cancel
                 (9 x = -10 o has bf16 solutions, e.g. 2.5 - 2.25 / 0.9: the fp64 sum is 0 or
                 1e-16, the fp32 one 1e-7): the fp32 value before the rounding is off by at most
                 2^-23 |o m| for the scale (0.1f, 1 - p and the division, one rounding each) plus
                 2^-24 |o m| for the product, which is far below an ulp of s everywhere else, so
                 there the rule is one ulp exactly (two bf16 numbers differ by whole ulps).
                 y, mean and rstd are then judged against ln_from_s(the s the kernel wrote).
  fp32 sums      |got - rounded oracle| <= 2^-24 L sum|terms|, L = the roundings on the longest
                 addition chain plus 3 for the roundings inside a term:
      dw, dgamma, dbeta (register path)  L = ceil(R / 4096) + 3 + 14 + 3.  part_grid caps the grid at
            1024 blocks = 4096 waves, a wave adds its ceil(R / 4096) rows in registers;
            block_fold_rows adds the 4 waves in order (3); colsum_kernel twice: a launch sums at
            most 32 entries per output as 8 chains of <= 4 plus a 3-level tree, or <= 7 entries
            in the tail chain (7 roundings each way; _colsum_roundings replays the loop bounds
            for the G at hand and the test asserts <= 14).
      dw (rms_dw_kernel path, D > 2048)  L = per + 14 + 3, per = ceil(R / P) rows in one chain,
            P = min(ceil(R / 4), 512) partitions, then the same two colsum launches.
      mean, rstd   L = 8 VPT + 6 + 4: a lane adds its 8 VPT elements in one chain, wave_sum has
            6 shuffle levels, and 4 covers the division by D, + eps, rsqrt and the squares /
            differences.  rstd = v^-1/2, so its bound is relative to rstd / 2.

Cases -> path ((R, D) for both norms unless noted; VPT = ceil(D / 512) rounded up to 1, 2, 4, 8)
  1 x 8, 5 x 8      VPT 1, one active lane, waves without a row; G = 1 / 2 partial rows (colsum Y = G < 32)
  37 x 520          VPT 2, only lane 0 holds a second vector
  37 x 1536         VPT 4: three full vectors, an empty fourth
  37 x 2048         VPT 4 full; last D of rmsnorm_bwd_kernel (register backward)
  37 x 2056         VPT 8 with nv = 257; first D of rmsnorm_bwd_dx2_kernel + rms_dw_kernel (second
                    column block with one live thread); layernorm_bwd_kernel<8>
  19 x 4096         VPT 8 full (layernorm_bwd_kernel<8>: four [8][8] register arrays)
  1000 x 520        G = 250 partial rows: colsum outputs y < 26 take the unrolled loop, y >= 26 the tail only
  8201 x 64         row_grid capped at 2048 blocks: the forward's PSAMD_ROW_LOOP takes a second
                    pass; part_grid capped at 1024: backward waves own 2 - 3 rows; G = 1024,
                    colsum unrolled 4 times, no tail
  2051 x 2056 (RMS) rms_dw_kernel with P = 512, per = 5: partitions 0 - 409 full, 410 one row, 411 - 511 empty
  RMSNorm runs every shape with and without (residual, ds_in) and with fp32 and bf16 weights;
  LayerNorm every shape at p = 0 with both weight types, and p = 0.1, 0.5 with a seed below and a
  seed above 2^32 at 37 x 1536, 19 x 4096, 8201 x 64.  The keep mask comes from the oracle's own
  Philox (philox_keep), never from the kernel.
  SwiGLU  7 x 8 (one vector per row), 33 x 1032 (fv = 129), 4100 x 1032 (528 900 work items >
          2048 x 256: the grid-stride loop takes a second pass); row 1 ramps g from -120 to 120.
  RoPE    (B, S, H, KV, hd) = (1, 5, 3, 1, 16): hv = 1, KV = 1;  (2, 33, 4, 4, 32): KV = H;
          (2, 7, 8, 2, 128);  (4, 1030, 8, 4, 128): 527 360 work items, second pass.  cs holds a
          random angle per (position, pair); one more case runs rope_table(S, hd, 10.0).

Observed on MI355X, over all cases of an output: rowerr(kernel) / rowerr(yardstick) (the bound is
3), in brackets the yardstick's own rowerr, and the worst |kernel - yardstick| as a share of the
elementwise tolerance (the bound is 1; no element was outside it):

    rms.y       1.00 (0.0019 - 0.0048)  0.55      ln.y       1.00 (0.0031 - 0.0071)  0.48
    rms.dx      1.00 (0.0014 - 0.0023)  0.49      ln.dx      1.00 (0.0015 - 0.0024)  0.49
    swiglu.h    1.00 (0.0013 - 0.0020)  0.44      ln.do      1.00 (0.0011 - 0.0018)  0.49
    swiglu.dgu  1.00 (0.0017 - 0.0025)  0.49      rope.q     1.00 (0.0019 - 0.0022)  0.48
    rope.dqkv   1.00 (0.0019 - 0.0026)  0.49      rope.k     1.00 (0.0019 - 0.0023)  0.45

The ratio is 1.00 in every case to the printed digits: the kernels round where the yardstick does.
fp32 sums, worst share of 2^-24 L sum|terms|: rms.dw 0.06, ln.dgamma 0.13, ln.dbeta 0.01, ln.mean
0.04, rms.rstd 0.23, ln.rstd 0.29.  s at p = 0.1: 8.0e-5 - 1.5e-4 of the elements differ from
bf16(fp64 value) (the bound is 1e-3); 2 - 18 cancelling elements per case differ by more than one
ulp and are inside ulp + 2^-22 |o m|.  RoPE adjoint: |lhs - rhs| 0.003 - 0.73 against summed
tolerances of 5.7 - 126 497 (a weak check by construction: the tolerance grows with the element
count, a random discrepancy with its root; the per-element backward check is the sharp one).
"""
import functools

import pytest
import torch

from ps_amd.ops import native, nn_ops
from ps_amd.ops import transformer as T

from . import transformer_oracle as to

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 3.0
WDT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _dev(t):
    return t.to(DEV) if t is not None else None


def _bf16_bounds(name, tag, got, exact, yard, mag=None):
    got = got.cpu()
    assert got.shape == yard.shape and got.dtype == torch.bfloat16
    e, y = to.rowerr(got, exact), to.rowerr(yard, exact)
    bad, worst = to.elemerr(got, yard, mag)
    print(f"RATIO {name} {tag}: kernel {e:.5f} yardstick {y:.5f} ratio {e / y:.2f} elemerr bad {bad} worst {worst:.2f}")
    assert y > 0
    assert e <= FACTOR * y, (name, e, y)
    assert bad == 0, (name, bad, worst)


def _sum_bound(name, tag, got, ref, mag, L, scale=1.0):
    got = got.cpu().double()
    assert got.shape == ref.shape
    tol = to.U24 * L * mag * scale
    ratio = ((got - ref).abs() / tol.clamp_min(1e-300)).max().item()
    print(f"SUM {name} {tag}: L {L} worst {ratio:.3f} of the bound")
    assert bool(((got - ref).abs() <= tol).all()), (name, L, ratio)


def _vpt(D):
    v = (D // 8 + 63) // 64
    return 1 if v <= 1 else 2 if v <= 2 else 4 if v <= 4 else 8


def _colsum_roundings(G):
    """Roundings on the longest chain of colsum2's two launches over G partial rows, replayed from
    colsum_kernel's loop bounds (an addition to 0 or of 0 is exact)."""
    def launch(G, Y):
        worst = 0
        for y in range(Y):
            b, k = y, 0
            while b + 7 * Y < G:
                b, k = b + 8 * Y, k + 1
            tail = len(range(b, G, Y))
            worst = max(worst, max(k + tail - 1, 0) + (3 if k else 0))
        return worst
    Y = min(G, 32)
    return launch(G, Y) + launch(Y, 1)


def _L_regs(R):
    G = min((R + 3) // 4, 1024)
    assert _colsum_roundings(G) <= 14
    return -(-R // 4096) + 3 + 14 + 3


def _L_rms_dw(R):
    P = min((R + 3) // 4, 512)
    assert _colsum_roundings(P) <= 14
    return -(-R // P) + 14 + 3


def _L_stat(D):
    return 8 * _vpt(D) + 6 + 4


# ------------------------------------------------------------------------------------ RMSNorm
RMS_CASES = [(R, D, res, wd) for (R, D) in to.NORM_SHAPES + to.RMS_ONLY_SHAPES for res in (False, True)
             for wd in ("f32", "bf16")]


def _rms_id(c):
    R, D, res, wd = c
    return f"{R}x{D}-{'res' if res else 'plain'}-{wd}"


@functools.lru_cache(maxsize=None)
def _rms_inputs(R, D):
    return to.norm_inputs(R, D, 1000 + R + D)


@functools.lru_cache(maxsize=None)
def _rms_case(R, D, res, wd):
    """Inputs, fp64 oracle and yardstick of one case, computed once and left unchanged."""
    c = _rms_inputs(R, D)
    w = c["w"].to(WDT[wd])
    r, ds = (c["r"], c["ds"]) if res else (None, None)
    _, y_e, _ = to.rms_fwd(c["x"], r, w, to.RMS_EPS)
    s_y, y_y, rstd_y = to.rms_fwd(c["x"], r, w, to.RMS_EPS, rounded=True)
    s_in, rstd_in = s_y.to(torch.bfloat16), rstd_y.float()  # what rmsnorm_bwd is given
    dx_e, _, _, _ = to.rms_bwd(c["dy"], s_in, w, rstd_in, ds)
    dx_y, dw_y, mag_dx, mag_dw = to.rms_bwd(c["dy"], s_in, w, rstd_in, ds, rounded=True)
    return dict(x=c["x"], r=r, ds=ds, dy=c["dy"], w=w, y_e=y_e, s_y=s_y, y_y=y_y, rstd_y=rstd_y, s_in=s_in,
                rstd_in=rstd_in, dx_e=dx_e, dx_y=dx_y, dw_y=dw_y, mag_dx=mag_dx, mag_dw=mag_dw)


@pytest.mark.parametrize("case", RMS_CASES, ids=_rms_id)
def test_rmsnorm_forward(case):
    R, D, res, wd = case
    c, tag = _rms_case(*case), _rms_id(case)
    s, y, rstd = native().rmsnorm_fwd(_dev(c["x"]), _dev(c["r"]), _dev(c["w"]), to.RMS_EPS)
    if res:
        assert torch.equal(s.cpu().double(), c["s_y"])  # one bf16 + bf16 sum, rounded once
    _bf16_bounds("rms.y", tag, y, c["y_e"], c["y_y"])
    _sum_bound("rms.rstd", tag, rstd, c["rstd_y"], c["rstd_y"], _L_stat(D), 0.5)


@pytest.mark.parametrize("case", RMS_CASES, ids=_rms_id)
def test_rmsnorm_backward(case):
    R, D, res, wd = case
    c, tag = _rms_case(*case), _rms_id(case)
    dx, dw = native().rmsnorm_bwd(_dev(c["dy"]), _dev(c["s_in"]), _dev(c["w"]), _dev(c["rstd_in"]), _dev(c["ds"]))
    _bf16_bounds("rms.dx", tag, dx, c["dx_e"], c["dx_y"], c["mag_dx"])
    assert dw.dtype == torch.float32
    _sum_bound("rms.dw", tag, dw, c["dw_y"], c["mag_dw"], _L_rms_dw(R) if D > 2048 else _L_regs(R))


# ------------------------------------------------------------------------------------ LayerNorm
LN_CASES = [(R, D, 0.0, 0, wd) for (R, D) in to.NORM_SHAPES for wd in ("f32", "bf16")]
LN_CASES += [(R, D, p, seed, ("f32", "bf16")[(i + j) % 2]) for (R, D) in to.DROP_SHAPES
             for i, p in enumerate((0.1, 0.5)) for j, seed in enumerate(to.SEEDS)]


def _ln_id(c):
    R, D, p, seed, wd = c
    return f"{R}x{D}-p{p}-{'hi' if seed >> 32 else 'lo'}-{wd}"


@functools.lru_cache(maxsize=None)
def _ln_inputs(R, D):
    return to.norm_inputs(R, D, 2000 + R + D, shift=3.0)


@functools.lru_cache(maxsize=None)
def _keep(seed, R, D, p):
    return to.philox_keep(seed, R * D, p).view(R, D) if p > 0 else None


@functools.lru_cache(maxsize=None)
def _ln_case(R, D, p, seed, wd):
    c = _ln_inputs(R, D)
    gamma, beta = c["w"].to(WDT[wd]), c["b"].to(WDT[wd])
    keep = _keep(seed, R, D, p)
    s_e = to.ln_fwd(c["x"], c["r"], keep, p)
    s_y = to.ln_fwd(c["x"], c["r"], keep, p, rounded=True)
    y_e, _, _, _ = to.ln_from_s(s_e, gamma, beta, to.LN_EPS)
    _, mean_y, rstd_y, _ = to.ln_from_s(s_y, gamma, beta, to.LN_EPS, rounded=True)
    s_in, mean_in, rstd_in = s_y.to(torch.bfloat16), mean_y.float(), rstd_y.float()  # what layernorm_bwd is given
    dx_e, do_e, _, _, _ = to.ln_bwd(c["dy"], s_in, gamma, mean_in, rstd_in, keep, p)
    dx_y, do_y, dg_y, db_y, mags = to.ln_bwd(c["dy"], s_in, gamma, mean_in, rstd_in, keep, p, rounded=True)
    return dict(x=c["x"], o=c["r"], dy=c["dy"], gamma=gamma, beta=beta, keep=keep, s_y=s_y, y_e=y_e, s_in=s_in,
                mean_in=mean_in, rstd_in=rstd_in, dx_e=dx_e, do_e=do_e, dx_y=dx_y, do_y=do_y, dg_y=dg_y, db_y=db_y,
                mags=mags)


@pytest.mark.parametrize("case", LN_CASES, ids=_ln_id)
def test_layernorm_forward(case):
    R, D, p, seed, wd = case
    c, tag = _ln_case(*case), _ln_id(case)
    s, y, mean, rstd = native().layernorm_fwd(_dev(c["x"]), _dev(c["o"]), _dev(c["gamma"]), _dev(c["beta"]),
                                              to.LN_EPS, p, seed)
    s = s.cpu()
    sk = s.double()
    if p == 0.1:
        diff = (sk - c["s_y"]).abs()
        share = (diff > 0).double().mean().item()
        ulp = to.bf16_ulp(torch.maximum(sk.abs(), c["s_y"].abs()))
        delta = 2.0 ** -22 * (c["o"].double() * c["keep"].double() / (1.0 - p)).abs()
        print(f"FLIP ln.s {tag}: share {share:.2e}, {int((diff > ulp).sum())} cancelling elements beyond one ulp")
        assert share <= 1e-3, share
        assert bool((diff <= ulp + delta).all())
    else:
        assert torch.equal(sk, c["s_y"])
    y_y, mean_y, rstd_y, mag_y = to.ln_from_s(s, c["gamma"], c["beta"], to.LN_EPS, rounded=True)
    _bf16_bounds("ln.y", tag, y, c["y_e"], y_y, mag_y)
    L = _L_stat(D)
    _sum_bound("ln.mean", tag, mean, mean_y, sk.abs().mean(-1), L)
    _sum_bound("ln.rstd", tag, rstd, rstd_y, rstd_y, L, 0.5)


@pytest.mark.parametrize("case", LN_CASES, ids=_ln_id)
def test_layernorm_backward(case):
    R, D, p, seed, wd = case
    c, tag = _ln_case(*case), _ln_id(case)
    dx, do, dg, db = native().layernorm_bwd(_dev(c["dy"]), _dev(c["s_in"]), _dev(c["gamma"]), _dev(c["mean_in"]),
                                            _dev(c["rstd_in"]), p, seed)
    _bf16_bounds("ln.dx", tag, dx, c["dx_e"], c["dx_y"], c["mags"]["dx"])
    if p > 0:
        _bf16_bounds("ln.do", tag, do, c["do_e"], c["do_y"], c["mags"]["do"])
        live = (dx != 0).cpu()
        assert torch.equal((do != 0).cpu()[live], c["keep"][live])  # zero on exactly the dropped elements
    else:
        assert torch.equal(do, dx)
    L = _L_regs(R)
    _sum_bound("ln.dgamma", tag, dg, c["dg_y"], c["mags"]["dgamma"], L)
    _sum_bound("ln.dbeta", tag, db, c["db_y"], c["mags"]["dbeta"], L)


MASK_CASES = [(R, D, p, seed) for (R, D) in to.DROP_SHAPES for p in (0.1, 0.5) for seed in to.SEEDS]


@pytest.mark.parametrize("case", MASK_CASES, ids=lambda c: f"{c[0]}x{c[1]}-p{c[2]}-{'hi' if c[3] >> 32 else 'lo'}")
def test_layernorm_mask_is_philox(case):
    """x = 0, o = 1: s is the scaled keep mask.  It is philox_keep's (counter i // 4, word i % 4, both
    seed halves as the key), and nn_ops.dropout draws the same stream, as transformer.hip promises."""
    R, D, p, seed = case
    keep = _keep(seed, R, D, p)
    x = torch.zeros(R, D, device=DEV, dtype=torch.bfloat16)
    one = torch.ones(D, device=DEV)
    s, _, _, _ = native().layernorm_fwd(x, x + 1, one, one - 1, to.LN_EPS, p, seed)
    assert torch.equal((s != 0).cpu(), keep)
    kept = torch.tensor(1.0 / (1.0 - p)).to(torch.bfloat16).item()
    assert bool(((s == kept) | (s == 0)).all())
    d = nn_ops.dropout(x + 1, p, seed, 0)
    assert torch.equal((d != 0).cpu(), keep)


# ------------------------------------------------------------------------------------ SwiGLU
@functools.lru_cache(maxsize=None)
def _swiglu_case(R, F):
    gu, dh = to.swiglu_inputs(R, F, 3000 + R)
    h_e, _ = to.swiglu_fwd(gu)
    h_y, mag_h = to.swiglu_fwd(gu, rounded=True)
    d_e, _ = to.swiglu_bwd(dh, gu)
    d_y, mag_d = to.swiglu_bwd(dh, gu, rounded=True)
    return dict(gu=gu, dh=dh, h_e=h_e, h_y=h_y, mag_h=mag_h, d_e=d_e, d_y=d_y, mag_d=mag_d)


@pytest.mark.parametrize("R,F", to.SWIGLU_SHAPES)
def test_swiglu_forward(R, F):
    c = _swiglu_case(R, F)
    h = native().swiglu_fwd(_dev(c["gu"]))
    assert bool(torch.isfinite(h.float()).all())
    _bf16_bounds("swiglu.h", f"{R}x{F}", h, c["h_e"], c["h_y"], c["mag_h"])


@pytest.mark.parametrize("R,F", to.SWIGLU_SHAPES)
def test_swiglu_backward(R, F):
    c = _swiglu_case(R, F)
    dgu = native().swiglu_bwd(_dev(c["dh"]), _dev(c["gu"]))
    assert bool(torch.isfinite(dgu.float()).all())
    _bf16_bounds("swiglu.dgu", f"{R}x{F}", dgu, c["d_e"], c["d_y"], c["mag_d"])


# ------------------------------------------------------------------------------------ RoPE + split
ROPE_CASES = list(range(len(to.ROPE_SHAPES) + 1))  # the last one: rope_table(S, hd, 10.0)


def _rope_id(i):
    shape = (to.ROPE_SHAPES + [to.ROPE_TABLE_SHAPE])[i]
    return "x".join(map(str, shape)) + ("-table" if i == len(to.ROPE_SHAPES) else "")


@functools.lru_cache(maxsize=None)
def _rope_case(i):
    shape = (to.ROPE_SHAPES + [to.ROPE_TABLE_SHAPE])[i]
    B, S, H, KV, hd = shape
    qkv, gq, gk, gv, cs = to.rope_inputs(*shape, 4000 + i)
    if i == len(to.ROPE_SHAPES):
        cs = T.rope_table(S, hd, to.ROPE_TABLE_THETA, DEV).cpu()
    q_e, k_e, v_e, _, _ = to.rope_fwd(qkv, cs, H, KV)
    q_y, k_y, _, mq, mk = to.rope_fwd(qkv, cs, H, KV, rounded=True)
    d_e, _ = to.rope_bwd(gq, gk, gv, cs)
    d_y, mag_d = to.rope_bwd(gq, gk, gv, cs, rounded=True)
    return dict(shape=shape, qkv=qkv, gq=gq, gk=gk, gv=gv, cs=cs, q_e=q_e, k_e=k_e, v_e=v_e, q_y=q_y, k_y=k_y, mq=mq,
                mk=mk, d_e=d_e, d_y=d_y, mag_d=mag_d)


def test_rope_table_is_the_fp64_table():
    """cos / sin of s * theta^(-2 i / hd): the fp32 inverse frequency is within 2^-21 relative (the
    exponent's rounding times ln theta, pow, the division), the angle f = s * inv one rounding more,
    cos / sin a few ulps of 1: |error| <= 2^-20 f + 2^-21."""
    _, S, _, _, hd = to.ROPE_TABLE_SHAPE
    cs = T.rope_table(S, hd, to.ROPE_TABLE_THETA, DEV).cpu().double()
    cs64, f = to.rope_table64(S, hd, to.ROPE_TABLE_THETA)
    assert cs.shape == cs64.shape == (S, hd // 2, 2)
    assert bool(((cs - cs64).abs() <= (2.0 ** -20 * f + 2.0 ** -21)[..., None]).all())


@pytest.mark.parametrize("i", ROPE_CASES, ids=_rope_id)
def test_rope_split_forward(i):
    c, tag = _rope_case(i), _rope_id(i)
    B, S, H, KV, hd = c["shape"]
    q, k, v = native().rope_split_fwd(_dev(c["qkv"]), _dev(c["cs"]), H, KV)
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    _bf16_bounds("rope.q", tag, q, c["q_e"], c["q_y"], c["mq"])
    _bf16_bounds("rope.k", tag, k, c["k_e"], c["k_y"], c["mk"])
    assert torch.equal(v.cpu().double(), c["v_e"])


@pytest.mark.parametrize("i", ROPE_CASES, ids=_rope_id)
def test_rope_split_backward_and_adjoint(i):
    c, tag = _rope_case(i), _rope_id(i)
    B, S, H, KV, hd = c["shape"]
    n = H + KV
    dqkv = native().rope_split_bwd(_dev(c["gq"]), _dev(c["gk"]), _dev(c["gv"]), _dev(c["cs"])).cpu()
    _bf16_bounds("rope.dqkv", tag, dqkv[:, :, :n], c["d_e"][:, :, :n], c["d_y"][:, :, :n], c["mag_d"][:, :, :n])
    assert torch.equal(dqkv[:, :, n:].double(), c["d_e"][:, :, n:])
    # <rope(x), g> == <x, rope^T(g)> from the kernels' own outputs, to the summed elementwise tolerance
    q, k, v = (t.cpu().double() for t in native().rope_split_fwd(_dev(c["qkv"]), _dev(c["cs"]), H, KV))
    lhs = (q * c["gq"].double()).sum() + (k * c["gk"].double()).sum() + (v * c["gv"].double()).sum()
    rhs = (c["qkv"].double() * dqkv.double()).sum()
    tol = (to.elemtol_sum(c["gq"], c["q_y"], c["mq"]) + to.elemtol_sum(c["gk"], c["k_y"], c["mk"])
           + to.elemtol_sum(c["qkv"][:, :, :n], c["d_y"][:, :, :n], c["mag_d"][:, :, :n]))
    print(f"ADJOINT rope {tag}: |lhs - rhs| {abs(float(lhs - rhs)):.4f} tolerance {tol:.4f}")
    assert abs(float(lhs - rhs)) <= tol
