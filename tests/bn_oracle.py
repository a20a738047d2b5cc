"""fp64 oracles, a bf16 yardstick, a replay of the launch geometry and input builders for the
NHWC BatchNorm kernels (csrc/kernels/bn_act.hip) and the max-pool / fused stem kernels
(csrc/kernels/pool.hip).  Plain torch on the CPU; imported by test_bn_oracle_cpu.py and
test_bn_rows_gpu.py.  bf16r, rowerr, elemerr, U24, REL and MAGREL are transformer_oracle's.

Every function takes the bf16 and fp32 tensors the kernel receives and computes in fp64.  With
rounded=True the same formulas round to bf16 exactly where the kernel stores bf16 and nowhere else:

    apply        y
    bn_bwd       dx (dres is the masked dy, a bf16 number already)
    pool_bwd     dx
    pool_bn_bwd  the pooled gradient (always: the unfused path stores it) and dz

That variant is the yardstick: its row error against the exact variant is what the bf16 stores
alone cost, and the kernel is compared with it element by element.  fp32 outputs (mean, invstd,
coefficients, dgamma, dbeta) are never rounded.  A `mag` tensor is the sum of the absolute values
of the terms the last expression of an output adds: elemerr allows 2^-6 |ref| + 2^-14 mag.

Layout: activations are [R, C] rows (R = N H W of an NHWC tensor), pool tensors [N, H, W, C].
"""
import torch
import torch.nn.functional as F

from .transformer_oracle import MAGREL, REL, U24, bf16r, elemerr, rowerr  # noqa: F401  (re-exported)

EPS, MOMENTUM = 1e-5, 0.1
AMBIG = 2.0 ** -22  # relative distance from zero below which fp32 may get the sign of x sc + sh wrong


def _r(x, rounded):
    return bf16r(x) if rounded else x


# ------------------------------------------------------------------------------------ forward
def stats(x, eps=EPS):
    """x [R, C] -> dict(mean, var (biased), invstd, and about the kernel's shift K = x[0]:
    dm = mean - K, absdev = mean |x - K|, sq = mean (x - K)^2), each [C] fp64."""
    xd = x.double()
    mean = xd.mean(0)
    var = (xd - mean).pow(2).mean(0)
    d = xd - xd[0]
    return dict(mean=mean, var=var, invstd=(var + eps).rsqrt(), dm=d.mean(0), absdev=d.abs().mean(0),
                sq=d.pow(2).mean(0))


def running(rm0, rv0, mean, var, R, momentum=MOMENTUM):
    """The running-statistics update with the unbiased variance var R / (R - 1)."""
    unb = var.double() * (R / (R - 1.0)) if R > 1 else var.double()
    return ((1.0 - momentum) * rm0.double() + momentum * mean.double(),
            (1.0 - momentum) * rv0.double() + momentum * unb)


def coef(gamma, beta, mean, invstd):
    """[scale | shift] = [gamma invstd | beta - mean gamma invstd], [2C] fp64 (gamma / beta None: 1 / 0)."""
    is_ = invstd.double()
    ga = gamma.double() if gamma is not None else torch.ones_like(is_)
    be = beta.double() if beta is not None else torch.zeros_like(is_)
    return torch.cat([ga * is_, be - mean.double() * ga * is_])


def apply(x, cf, res=None, rcoef=None, act=0, rounded=False):
    """y = act(x sc + sh [+ res | + res rs + rh]) -> (y, mag)."""
    C = x.shape[1]
    cf = cf.double()
    t = x.double() * cf[:C]
    o, mag = t + cf[C:], t.abs() + cf[C:].abs()
    if res is not None and rcoef is not None:
        rc = rcoef.double()
        tr = res.double() * rc[:C]
        o, mag = o + (tr + rc[C:]), mag + tr.abs() + rc[C:].abs()
    elif res is not None:
        o, mag = o + res.double(), mag + res.double().abs()
    if act == 1:
        o = o.clamp_min(0.0)
    return _r(o, rounded), mag


def mask_bits(y):
    """uint8 [numel / 8]: bit j of byte v is y.flatten()[8 v + j] > 0."""
    b = (y.reshape(-1, 8) > 0).to(torch.int32)
    w = 2 ** torch.arange(8, dtype=torch.int32)
    return (b * w).sum(1).to(torch.uint8)


def unpack_bits(bits, shape):
    """The inverse of mask_bits: a bool tensor of `shape`."""
    w = 2 ** torch.arange(8, dtype=torch.int32)
    return ((bits.to(torch.int32)[:, None] & w) != 0).reshape(shape)


# ------------------------------------------------------------------------------------ backward
def bwd_coef(sd, sx, gamma, mean, invstd, R):
    """From sd = sum dz and sx = sum dz xhat: [ca | cb | cc] of dx = ca dz + cb x + cc, [3C] fp64."""
    is_, mu = invstd.double(), mean.double()
    k = (gamma.double() if gamma is not None else torch.ones_like(is_)) * is_
    md, mx = sd.double() / R, sx.double() / R
    return torch.cat([k, -k * is_ * mx, -k * md + k * is_ * mx * mu])


def bwd_apply(dz, x, c3, rounded=False):
    """dx = ca dz + cb x + cc -> (dx, mag_dx)."""
    C = x.shape[1]
    c3 = c3.double()
    t1, t2, cc = c3[:C] * dz.double(), c3[C:2 * C] * x.double(), c3[2 * C:]
    return _r(t1 + t2 + cc, rounded), t1.abs() + t2.abs() + cc.abs()


def bn_bwd(mask, dy, x, gamma, mean, invstd, rounded=False):
    """mask: bool [R, C] built by the caller (from y, from the bits, or from x sc + sh > 0 in fp64),
    or None for the identity.  mean / invstd are the fp32 vectors the kernel is given.
    -> dict(dx, dres (= dz, the masked dy), dgamma, dbeta, coef = ca | cb | cc, mag_dx, and
    abs_dgamma / abs_dbeta = sum |terms| of the two sums)."""
    R = x.shape[0]
    dz = dy.double()
    if mask is not None:
        dz = dz * mask.double()
    tx = dz * ((x.double() - mean.double()) * invstd.double())
    sd, sx = dz.sum(0), tx.sum(0)
    c3 = bwd_coef(sd, sx, gamma, mean, invstd, R)
    dx, mag = bwd_apply(dz, x, c3, rounded)
    return dict(dx=dx, dres=dz, dgamma=sx, dbeta=sd, coef=c3, mag_dx=mag, abs_dgamma=tx.abs().sum(0),
                abs_dbeta=dz.abs().sum(0))


# ------------------------------------------------------------------------------------ pool
def _osize(H, k, s, p):
    return (H + 2 * p - k) // s + 1


def pool_fwd(z, cf, k, s, p):
    """z [N, H, W, C] bf16.  With cf = [scale | shift]: the window max of bf16(relu(z sc + sh)) (the
    exact product-sum rounded once to fp32, as the kernel's fma, then to bf16); with cf None the
    plain window max.  -> (y [N, OH, OW, C] fp64, idx uint8: the FIRST tap kh k + kw attaining it)."""
    N, H, W, C = z.shape
    a = z.double().permute(0, 3, 1, 2)
    if cf is not None:
        cf = cf.double()
        a = torch.relu(a * cf[:C].view(1, C, 1, 1) + cf[C:].view(1, C, 1, 1)).float().bfloat16().double()
    pad = -1.0 if cf is not None else float("-inf")  # padding never wins
    cols = F.unfold(F.pad(a, (p, p, p, p), value=pad), k, stride=s)  # [N, C k k, L], tap-major within a channel
    OH, OW = _osize(H, k, s, p), _osize(W, k, s, p)
    cols = cols.view(N, C, k * k, OH, OW)
    y = cols.max(dim=2).values
    first = (cols == y.unsqueeze(2)).to(torch.uint8).argmax(dim=2)
    return y.permute(0, 2, 3, 1).contiguous(), first.permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def pool_bwd(dy, idx, H, W, k, s, p, rounded=False):
    """Scatter dy [N, OH, OW, C] to the stored taps -> (dx [N, H, W, C], mag = sum |dy| per element)."""
    N, OH, OW, C = dy.shape
    t = idx.long()
    h = torch.arange(OH).view(1, OH, 1, 1) * s - p + t // k
    w = torch.arange(OW).view(1, 1, OW, 1) * s - p + t % k
    assert bool(((h >= 0) & (h < H) & (w >= 0) & (w < W)).all()), "a stored tap points outside the input"
    n = torch.arange(N).view(N, 1, 1, 1)
    c = torch.arange(C).view(1, 1, 1, C)
    flat = (((n * H + h) * W + w) * C + c).reshape(-1)
    g = dy.double().reshape(-1)
    dx = torch.zeros(N * H * W * C, dtype=torch.float64).index_add_(0, flat, g)
    mag = torch.zeros(N * H * W * C, dtype=torch.float64).index_add_(0, flat, g.abs())
    return _r(dx.view(N, H, W, C), rounded), mag.view(N, H, W, C)


def pool_bn_bwd(dy, idx, z, mc, gamma, mean, invstd, rounded=False):
    """The stem backward z -> BN -> ReLU -> pool 3x3/2/1: pool_bwd (its result rounded to bf16, where
    the unfused path stores it), the ReLU mask z sc + sh > 0 in fp64, then bn_bwd.  -> bn_bwd's dict
    with [N, H, W, C] dx / mag_dx."""
    N, H, W, C = z.shape
    g, _ = pool_bwd(dy, idx, H, W, 3, 2, 1, rounded=True)
    z2 = z.reshape(-1, C)
    mask = z2.double() * mc.double()[:C] + mc.double()[C:] > 0
    out = bn_bwd(mask, g.view(-1, C), z2, gamma, mean, invstd, rounded)
    for key in ("dx", "mag_dx", "dres"):
        out[key] = out[key].view(N, H, W, C)
    return out


# ------------------------------------------------------------------------------------ geometry
def geometry(R, C):
    """Replay of red_geom, bn_red_blocks, fin_threads and apply_grid (bn_act.hip) for an [R, C] tensor:
    G blocks per channel tile, rows_per_block, rows_it (rows a block covers per step), rows_thread
    (steps of one thread), pass4 / pass2 (iterations of the 4-deep / 2-deep unrolled loop for thread
    row 0 of a full block), tail4 / tail2 (thread row 0's rows left to the tail loop after them),
    empty (blocks with no row), fixed_c (the apply kernels' FIXED_C), tail (the apply kernels' tail
    `if` is taken by some thread), full (their 2-vector loop runs at all) and L, the roundings on
    the longest addition chain of a channel sum: ceil(rows_per_block / rows_it) in registers,
    rows_it - 1 in the serial LDS fold, ceil(G / fin_threads) in sum_partials8, 6 in wave_sum,
    waves - 1 across the waves, 3 inside a term."""
    cv = C // 8
    tpr = 1
    while tpr < min(cv, 32):
        tpr <<= 1
    rows_it = 256 // tpr
    ctiles = (cv + 31) // 32
    g = (R + 127) // 128
    want = (2048 + ctiles - 1) // ctiles
    if g < want:
        g = min(want, (R + 7) // 8)
    g = max(1, min(g, 2048))
    rpb = -(-R // g)
    rows_thread = -(-rpb // rows_it)

    def unrolled(U):
        r, n = 0, 0
        while r + (U - 1) * rows_it < rpb:
            r, n = r + U * rows_it, n + 1
        return n, len(range(r, rpb, rows_it))

    (pass4, tail4), (pass2, tail2) = unrolled(4), unrolled(2)
    fin = 1024 if g >= 4096 else 512 if g >= 1024 else 256
    nvec = R * cv
    grid = max(1, min((nvec + 511) // 512, 1 << 22))
    stride = grid * 256
    L = rows_thread + (rows_it - 1) + -(-g // fin) + 6 + (fin // 64 - 1) + 3
    return dict(G=g, ctiles=ctiles, rows_per_block=rpb, rows_it=rows_it, rows_thread=rows_thread, pass4=pass4,
                tail4=tail4, pass2=pass2, tail2=tail2, empty=g - -(-R // rpb), fixed_c=stride % cv == 0,
                tail=nvec % (2 * stride) != 0, full=nvec > stride, fin_threads=fin, L=L)


def pool_geometry(N, C, H, W, k, s, p):
    """Replay of pool.hip's launchers: the forward / backward mapping ('row' or 'flat'), the backward
    kernel ('quad', 's2k3' or 'generic') and the forward kernel with coefficients ('k3' or 'generic')."""
    cv = C // 8
    OH, OW = _osize(H, k, s, p), _osize(W, k, s, p)

    def mapping(width):
        return "row" if cv & (cv - 1) == 0 and width * cv >= 64 else "flat"

    quad = k == 3 and s == 2 and p == 1 and H % 2 == 0 and W % 2 == 0
    return dict(fwd=mapping(OW), bwd="flat" if quad else mapping(W),
                bwd_kernel="quad" if quad else "s2k3" if (k, s) == (3, 2) else "generic",
                fwd_bn_kernel="k3" if k == 3 else "generic", OH=OH, OW=OW)


# ------------------------------------------------------------------------------------ builders
def ambiguous(x, cf):
    """bool like x: |x sc + sh| <= 2^-22 (|x sc| + |sh|) in fp64 -- where a ReLU mask recomputed in
    fp32 (fused multiply-add or not) may differ from the fp64 one."""
    C = x.shape[-1]
    cf = cf.double()
    t = x.double() * cf[:C]
    return (t + cf[C:]).abs() <= AMBIG * (t.abs() + cf[C:].abs())


def settle(x, cf):
    """x with every ambiguous element moved one bf16 step away from zero; asserts none remain."""
    a = ambiguous(x, cf)
    if bool(a.any()):
        x = torch.where(a, (x.view(torch.int16) + 1).view(torch.bfloat16), x)
    assert_unambiguous(x, cf)
    return x


def assert_unambiguous(x, cf):
    n = int(ambiguous(x, cf).sum())
    assert n == 0, f"{n} elements have an ambiguous ReLU mask"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def bn_inputs(R, C, seed, kind="randn"):
    """dict(x, res, dy bf16 [R, C]; gamma, beta, rm0, rv0 fp32 [C]).
    kind 'randn': x = std_c randn + mean_c with std_c in [0.5, 2.5], mean_c ~ N(0, 1);
    'shift': x = 50 + 0.05 randn (|mean| >> std; in bf16 a handful of values 0.25 apart);
    'outlier': the same with row 0 at 50 + 6 * 0.05, so the kernel's shift K = x[0] is a poor one.
    x is settled against its own fp32 [scale | shift] (`mc`, what ACT 2 is given), so its recomputed
    ReLU mask is unambiguous.  dy = 0.5 randn + a_c + b_c xhat with |a_c|, |b_c| in [1, 2]: both
    projection terms of dx are of order 1.  Asserts var > 0, |mean dy| >= 0.25 and
    |mean dy xhat| >= 0.25 per channel, and that rm0 has the sign of the mean (no cancellation in
    the running-mean update)."""
    g = _gen(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    if kind == "randn":
        x = rn(R, C) * (0.5 + 2.0 * ru(C)) + rn(C)
    else:
        x = 50.0 + 0.05 * rn(R, C)
        if kind == "outlier":
            x[0] = 50.0 + 6 * 0.05
    x = x.bfloat16()
    gamma, beta = (ru(C) + 0.5).float(), (0.3 * rn(C)).float()
    st = stats(x)
    mc = coef(gamma, beta, st["mean"], st["invstd"]).float()
    x = settle(x, mc)
    st = stats(x)
    assert bool((st["var"] > 0).all())
    sign = lambda t: torch.where(t < 0.5, -1.0, 1.0)  # noqa: E731
    a, b = sign(ru(C)) * (1.0 + ru(C)), sign(ru(C)) * (1.0 + ru(C))
    xh = ((x.double() - st["mean"]) * st["invstd"]).float()
    dy = (0.5 * rn(R, C) + a + b * xh).bfloat16()
    assert bool((dy.double().mean(0).abs() >= 0.25).all()), "dy lost its per-channel mean"
    assert bool(((dy.double() * xh.double()).mean(0).abs() >= 0.25).all()), "dy lost its xhat component"
    res = rn(R, C).bfloat16()
    rm0 = (torch.where(st["mean"] < 0, -1.0, 1.0) * (0.5 + ru(C).double())).float()
    rv0 = (ru(C) + 0.5).float()
    assert bool((rm0.double() * st["mean"] >= 0).all())
    return dict(x=x, res=res, dy=dy, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, mc=mc)


def pool_inputs(N, C, H, W, k, s, p, seed):
    """dict(z bf16 [N, H, W, C], mc = [scale | shift] fp32 with scale in [0.5, 1.5] and shift ~ 0.3 N(0, 1)
    (z settled against it), gamma, and dy bf16 [N, OH, OW, C] = 0.5 randn + a_c)."""
    g = _gen(seed)
    z = torch.randn(N, H, W, C, generator=g).bfloat16()
    mc = torch.cat([torch.rand(C, generator=g) + 0.5, 0.3 * torch.randn(C, generator=g)]).float()
    z = settle(z, mc)
    gamma = (torch.rand(C, generator=g) + 0.5).float()
    a = 1.0 + torch.rand(C, generator=g)
    dy = (0.5 * torch.randn(N, _osize(H, k, s, p), _osize(W, k, s, p), C, generator=g) + a).bfloat16()
    return dict(z=z, mc=mc, gamma=gamma, dy=dy)


# (R, C) -> the path it reaches (test_bn_rows_gpu.py's header maps them; test_bn_oracle_cpu.py re-checks
# the numbers against geometry())
BN_SHAPES = [(3, 8), (392, 136), (999, 192), (392, 2048), (4096, 64), (20000, 256), (26001, 264)]
BN_BIG_SHAPES = [(50000, 256), (70000, 136), (270001, 64), (1600003, 8)]  # starred variants only
BN_SHIFT_SHAPE = (50000, 256)  # kinds 'shift' and 'outlier'
# (N, C, H, W, k, s, p)
POOL_SHAPES = [(2, 64, 9, 9, 3, 2, 1), (2, 64, 10, 12, 2, 2, 0), (1, 128, 9, 8, 3, 1, 1), (3, 24, 10, 10, 3, 2, 1),
               (2, 8, 6, 4, 3, 2, 1), (2, 64, 10, 16, 2, 2, 0)]
POOL_BN_SHAPES = [(2, 64, 16, 16), (3, 32, 6, 10)]
