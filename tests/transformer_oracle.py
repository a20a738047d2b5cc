"""fp64 oracles, a bf16 rounding yardstick, per-element and per-row error metrics, a Philox keep
mask and input builders for the fused transformer row kernels (csrc/kernels/transformer.hip:
RMSNorm, residual LayerNorm with dropout, SwiGLU, RoPE + split).  Plain torch / numpy on the CPU;
imported by test_transformer_oracle_cpu.py and test_transformer_rows_gpu.py.

Every function takes the bf16 and fp32 tensors the kernel receives and computes in fp64.  With
rounded=True the same formulas round to bf16 exactly where the kernel does and nowhere else:

    rms_fwd    s = bf16(x + r), xhat = bf16(s rstd), y = bf16(xhat w)
    rms_bwd    xhat = bf16(fp32(s rstd)) from the s and the fp32 rstd that are passed in, dx
    ln_fwd     s;  ln_from_s: y;  ln_bwd: dx and do (mean and rstd are passed in)
    swiglu, rope    the outputs

That variant is the yardstick (as in attn_oracle): its row error against the exact variant is what
the bf16 roundings alone cost on the inputs at hand, and the kernel is compared with it element by
element.  fp32 reductions (dw, dgamma, dbeta, mean, rstd) are never rounded.

A `mag` tensor is the sum of the absolute values of the terms that the last expression of an
output combines: the scale of its cancellation error.  elemerr allows 2^-6 |ref| + 2^-14 mag.
For SwiGLU the last expression is a product, not a sum; there mag carries the one absolute error
the fp32 format forces: sigmoid(g) below fp32's smallest normal number 2^-126 (g < -87.3) has no
relative precision left (exp(-g) overflows for g < -88.7 and the quotient is 0), so sigmoid is
allowed an absolute error of 2^-126, scaled by what multiplies it: mag = 2^-112 |g u| and so on,
which 2^-14 turns into 2^-126.  Everywhere else that term is far below the bf16 denormals.
"""
import numpy as np
import torch

from .attn_oracle import bf16r, rowerr  # noqa: F401  (rowerr is re-exported)

U24 = 2.0 ** -24  # one fp32 rounding, relative
REL, MAGREL = 2.0 ** -6, 2.0 ** -14
SIG_FLOOR = 2.0 ** -112  # times MAGREL: 2^-126, fp32's smallest normal number


def _r(x, rounded):
    return bf16r(x) if rounded else x


def elemerr(got, ref, mag=None):
    """(number of elements with |got - ref| > 2^-6 |ref| + 2^-14 mag, worst |got - ref| / that
    tolerance).  Elements where both sides are equal count as ratio 0 (so an exact zero passes)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    tol = REL * ref.abs()
    if mag is not None:
        tol = tol + MAGREL * mag.double()
    diff = (got - ref).abs()
    bad = diff > tol  # NaN compares false: counted separately
    nan = torch.isnan(got) | torch.isinf(got)
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / tol.clamp_min(1e-300))
    return int(bad.sum()) + int(nan.sum()), float(ratio.max()) if ratio.numel() else 0.0


def elemtol_sum(weight, ref, mag=None):
    """sum |weight| * (2^-6 |ref| + 2^-14 mag): the elementwise tolerance carried into an inner product."""
    tol = REL * ref.double().abs()
    if mag is not None:
        tol = tol + MAGREL * mag.double()
    return float((weight.double().abs() * tol).sum())


def bf16_ulp(ref):
    """The spacing of bf16 numbers at |ref| (fp64 tensor), normal range."""
    _, e = torch.frexp(ref.abs().clamp(min=2.0 ** -120))
    return torch.ldexp(torch.ones_like(ref), e - 8)


# ------------------------------------------------------------------------------------ Philox
_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10: counter words c0..c3 (numpy arrays or ints, each < 2^32) and key (k0, k1)
    -> the four output words as uint64 arrays holding 32-bit values."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _LO
        hi1, lo1 = p1 >> np.uint64(32), p1 & _LO
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def philox_keep(seed, n, p):
    """bool [n]: element i is kept when word i % 4 of Philox(key = seed, counter = i // 4), taken
    as (word >> 8) * 2^-24 in fp32, is >= fp32(p)."""
    seed = int(seed)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32(q & _LO, q >> np.uint64(32), 0, 0, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=1).reshape(-1)[:n]
    u = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return torch.from_numpy(u >= np.float32(p))


# ------------------------------------------------------------------------------------ RMSNorm
def rms_fwd(x, r, w, eps, rounded=False):
    """x, r (or None) [R, D] bf16, w [D] -> s [R, D] (x + r, or x), y [R, D], rstd [R]."""
    s = x.double()
    if r is not None:
        s = _r(s + r.double(), rounded)
    rstd = torch.rsqrt(s.pow(2).mean(-1) + eps)
    xh = _r(s * rstd[:, None], rounded)
    return s, _r(xh * w.double(), rounded), rstd


def rms_bwd(dy, s, w, rstd, ds_in, rounded=False):
    """From the s [R, D] and rstd [R] that are passed in -> dx [R, D], dw [D] (never rounded),
    mag_dx, mag_dw."""
    d, sd, rs = dy.double(), s.double(), rstd.double()[:, None]
    xh = sd * rs
    if rounded:
        xh = bf16r(xh.float().double())  # the kernel's fp32 product, then bf16
    g = d * w.double()
    c = (g * xh).mean(-1, keepdim=True)
    dx = rs * g - rs * xh * c
    mag = (rs * g).abs() + (rs * xh * c).abs()
    if ds_in is not None:
        dx, mag = dx + ds_in.double(), mag + ds_in.double().abs()
    return _r(dx, rounded), (d * xh).sum(0), mag, (d * xh).abs().sum(0)


# ------------------------------------------------------------------------------------ LayerNorm
def ln_fwd(x, o, keep, p, rounded=False):
    """s = x + o * keep / (1 - p)  (keep None or p == 0: s = x + o)."""
    od = o.double()
    if keep is not None and p > 0:
        od = od * keep.double() / (1.0 - p)
    return _r(x.double() + od, rounded)


def ln_from_s(s, gamma, beta, eps, rounded=False):
    """-> y [R, D], mean [R], rstd [R], mag_y."""
    sd = s.double()
    mean = sd.mean(-1)
    c = sd - mean[:, None]
    rstd = torch.rsqrt(c.pow(2).mean(-1) + eps)
    t = c * rstd[:, None] * gamma.double()
    return _r(t + beta.double(), rounded), mean, rstd, t.abs() + beta.double().abs()


def ln_bwd(dy, s, gamma, mean, rstd, keep, p, rounded=False):
    """From the s, mean and rstd that are passed in -> dx, do [R, D], dgamma, dbeta [D] (never
    rounded) and dict(dx, do, dgamma, dbeta) of magnitudes."""
    d, rs = dy.double(), rstd.double()[:, None]
    xh = (s.double() - mean.double()[:, None]) * rs
    g = d * gamma.double()
    m1 = g.mean(-1, keepdim=True)
    m2 = (g * xh).mean(-1, keepdim=True)
    ds = rs * g - rs * m1 - rs * xh * m2
    mag = (rs * g).abs() + (rs * m1).abs() + (rs * xh * m2).abs()
    scale = 1.0
    if keep is not None and p > 0:
        scale = keep.double() / (1.0 - p)
    mags = dict(dx=mag, do=mag * scale, dgamma=(d * xh).abs().sum(0), dbeta=d.abs().sum(0))
    return _r(ds, rounded), _r(ds * scale, rounded), (d * xh).sum(0), d.sum(0), mags


# ------------------------------------------------------------------------------------ SwiGLU
def swiglu_fwd(gu, rounded=False):
    """gu [R, 2F] = [g | u] -> h [R, F] = silu(g) u, mag_h."""
    g, u = gu.double().chunk(2, dim=-1)
    return _r(g * torch.sigmoid(g) * u, rounded), SIG_FLOOR * (g * u).abs()


def swiglu_bwd(dh, gu, rounded=False):
    """-> dgu [R, 2F] = [dh u silu'(g) | dh silu(g)], mag_dgu.  silu'(g) = sig (1 + g (1 - sig))
    cancels near g = -1.28; both sides also carry the sigmoid floor of the module docstring."""
    g, u = gu.double().chunk(2, dim=-1)
    d = dh.double()
    sg = torch.sigmoid(g)
    t = g * (1.0 - sg)
    dg = d * u * sg * (1.0 + t)
    du = d * g * sg
    mag_dg = (d * u).abs() * (sg * (1.0 + t.abs()) + SIG_FLOOR * (1.0 + g.abs()))
    mag_du = SIG_FLOOR * (d * g).abs()
    return _r(torch.cat([dg, du], -1), rounded), torch.cat([mag_dg, mag_du], -1)


# ------------------------------------------------------------------------------------ RoPE
def _rot(x, cs, sign):
    half = x.shape[-1] // 2
    c, s = cs.double()[..., 0], sign * cs.double()[..., 1]  # [S, half], broadcast over [B, heads]
    x1, x2 = x[..., :half], x[..., half:]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    return out, mag


def rope_fwd(qkv, cs, H, KV, rounded=False):
    """qkv [B, S, H + 2 KV, hd], cs [S, hd/2, 2] -> q [B, H, S, hd], k, v [B, KV, S, hd] (rotate
    halves: (x1, x2) -> (x1 c - x2 s, x2 c + x1 s); v copied), mag_q, mag_k."""
    x = qkv.double().transpose(1, 2)
    q, mq = _rot(x[:, :H], cs, 1.0)
    k, mk = _rot(x[:, H:H + KV], cs, 1.0)
    return _r(q, rounded), _r(k, rounded), x[:, H + KV:].contiguous(), mq, mk


def rope_bwd(dq, dk, dv, cs, rounded=False):
    """The adjoint (rotation by -angle on dq, dk; dv copied) -> dqkv [B, S, H + 2 KV, hd], mag."""
    gq, mq = _rot(dq.double(), cs, -1.0)
    gk, mk = _rot(dk.double(), cs, -1.0)
    gv = dv.double()
    out = torch.cat([_r(gq, rounded), _r(gk, rounded), gv], 1).transpose(1, 2).contiguous()
    return out, torch.cat([mq, mk, torch.zeros_like(gv)], 1).transpose(1, 2).contiguous()


def rope_table64(S, hd, theta):
    """[S, hd/2, 2] (cos, sin) of angle s * theta^(-2 i / hd), fp64."""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    f = torch.outer(torch.arange(S, dtype=torch.float64), inv)
    return torch.stack([torch.cos(f), torch.sin(f)], -1), f


# ------------------------------------------------------------------------------------ builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows(R, D, g, shift=0.0):
    """randn + shift; with R >= 4: row 0 times 30, row 1 times 0.01, last row zero.  The shift is
    scaled with its row: 3 + 0.01 randn would be, in bf16, a row of three distinct values around
    its mean, the nearly constant non-zero row whose s - mean is ill-conditioned at eps = 1e-12."""
    t = torch.randn(R, D, generator=g, dtype=torch.float64) + shift
    if R >= 4:
        t[0] *= 30.0
        t[1] *= 0.01
        t[-1] = 0.0
    return t.to(torch.bfloat16)


def norm_inputs(R, D, seed, shift=0.0):
    """dict(x, r, dy, ds) bf16 [R, D] and fp32 w = 1 + randn / 4, b = randn / 4 [D] (per column, so
    that row / column mix-ups show).  x carries `shift` (3 for LayerNorm: a nonzero row mean); r is
    the residual / the dropout branch."""
    g = _gen(seed)
    x, r = _rows(R, D, g, shift), _rows(R, D, g)
    dy = torch.randn(R, D, generator=g, dtype=torch.float64).to(torch.bfloat16)
    ds = torch.randn(R, D, generator=g, dtype=torch.float64).to(torch.bfloat16)
    w = (1.0 + 0.25 * torch.randn(D, generator=g)).float()
    b = (0.25 * torch.randn(D, generator=g)).float()
    return dict(x=x, r=r, dy=dy, ds=ds, w=w, b=b)


RAMP = 120.0


def swiglu_inputs(R, F, seed):
    """gu [R, 2F] and dh [R, F] randn bf16; the g half of row 1 is a ramp from -120 to 120."""
    g = _gen(seed)
    gu = torch.randn(R, 2 * F, generator=g, dtype=torch.float64)
    gu[1, :F] = torch.linspace(-RAMP, RAMP, F, dtype=torch.float64)
    dh = torch.randn(R, F, generator=g, dtype=torch.float64)
    return gu.to(torch.bfloat16), dh.to(torch.bfloat16)


def rope_inputs(B, S, H, KV, hd, seed):
    """qkv and the three output gradients randn bf16; cs [S, hd/2, 2] fp32 from angles uniform in
    [0, 2 pi), one per (position, pair): every entry distinct and far from the identity."""
    g = _gen(seed)
    qkv = torch.randn(B, S, H + 2 * KV, hd, generator=g, dtype=torch.float64).to(torch.bfloat16)
    gq = torch.randn(B, H, S, hd, generator=g, dtype=torch.float64).to(torch.bfloat16)
    gk = torch.randn(B, KV, S, hd, generator=g, dtype=torch.float64).to(torch.bfloat16)
    gv = torch.randn(B, KV, S, hd, generator=g, dtype=torch.float64).to(torch.bfloat16)
    ang = torch.rand(S, hd // 2, generator=g, dtype=torch.float64) * (2.0 * torch.pi)
    cs = torch.stack([torch.cos(ang), torch.sin(ang)], -1).float().contiguous()
    return qkv, gq, gk, gv, cs


# (R, D) of the row kernels, the smallest that reach each path (test_transformer_rows_gpu.py maps them)
NORM_SHAPES = [(1, 8), (5, 8), (37, 520), (37, 1536), (37, 2048), (37, 2056), (19, 4096), (1000, 520), (8201, 64)]
RMS_ONLY_SHAPES = [(2051, 2056)]
DROP_SHAPES = [(37, 1536), (19, 4096), (8201, 64)]
SEEDS = [12345, 12345 + (7 << 40)]
SWIGLU_SHAPES = [(7, 8), (33, 1032), (4100, 1032)]
ROPE_SHAPES = [(1, 5, 3, 1, 16), (2, 33, 4, 4, 32), (2, 7, 8, 2, 128), (4, 1030, 8, 4, 128)]
ROPE_TABLE_SHAPE, ROPE_TABLE_THETA = (2, 33, 4, 4, 32), 10.0
RMS_EPS, LN_EPS = 1e-5, 1e-12
