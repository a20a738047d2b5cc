"""fp64 oracles and input builders for the dense side of the parameter server: fused_opt_kernel,
fused_opt_multi_kernel and reduce_multi_kernel (csrc/kernels/optim.hip), the 1-bit kernels
(csrc/kernels/compress.hip) and the bucket kernels (csrc/kernels/reduce.hip).  Plain torch on the
CPU; imported by test_dense_oracle_cpu.py and test_dense_gpu.py.

The oracles are written from the kernels' comments and opt_apply<KIND> (through rows_oracle._apply64),
not from ops/optim.py::_apply_ref or the CPU branches of ops/compress.py and ops/reduce.py.

Every builder asserts its conditions before anything can be launched: the share of FTRL elements on
either side of the |z| <= l1 branch, the number of elements too close to that threshold (left out of
the comparison), that the exact gradient grid sums exactly, that every source differs from every
other, that the sentinels are in place outside a segment, and that a segment lies inside every buffer
it indexes (the kernels do not bounds-check).

Scalars the kernels receive as `float` (gscale, beta1, scale, a, sc, mult) enter the oracles rounded
to fp32, and 1 - beta1 / 1 - sc as the fp32 difference the kernels form: the oracles describe the
operation on the values the kernel is given, in exact arithmetic from there on.
"""
import torch

from .rows_oracle import (ADAGRAD, ADAM, DENSE_HP, FTRL, GDTYPES, HP_SETS, SGD, U8, U24, _HP_DEFAULT, _apply64, _gen,
                          bf16_ulp)

__all__ = ["SGD", "ADAM", "ADAGRAD", "FTRL", "DENSE_HP", "HP_SETS", "GDTYPES", "U8", "U24", "bf16_ulp"]

CHUNK = 1024     # kOnebitChunk: elements per 1-bit scale
MAX_SRC = 16     # kPlaneMaxSrc
SENTINEL = -77.0  # fills whole-chunk buffers outside a segment (bf16-representable)
OPT_TOL = 2e-5   # |got - ref| <= OPT_TOL (1 + |ref|): the project's optimizer bound against fp64
TIE_EPS = 1e-5   # an FTRL element this close to l1 may take either branch in fp32
MAX_TIES = 2
GRID_WRAP_VEC = 8 * 2048 * 256 + 8 * 300 + 5   # fused_opt_kernel<VEC>: 2048 blocks x 256 lanes x 8 < n / 8 * 8
GRID_WRAP_SCALAR = 2048 * 256 + 777            # fused_opt_kernel<!VEC>: 2048 blocks x 256 lanes < n
GRID_WRAP_MULTI = 8 * 2048 * 256 + 8 * 300 + 13


def f32(x):
    """The python number x as the kernel receives it: rounded to fp32."""
    return float(torch.tensor(x, dtype=torch.float32))


def one_minus_f32(x):
    """1.f - x as the kernels form it (fp32 subtraction of the fp32 x)."""
    return float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(x, dtype=torch.float32))


def head_of(off):
    """Elements before the first 8-aligned chunk element of a segment that starts at chunk element off."""
    return (8 - (off & 7)) & 7


def _hp(hp):
    h = dict(_HP_DEFAULT)
    assert not set(hp) - set(h), sorted(set(hp) - set(h))
    h.update(hp)
    return h


# ------------------------------------------------------------------------------ dense optimizer
def dense_opt64(kind, w, st0, st1, g, gscale_t=None, **hp):
    """(w, st0, st1, wout) in fp64 after one dense step of opt_apply<KIND>; inputs are left
    unchanged.  g is the gradient as pushed (fp32 or bf16, or an fp64 sum of sources), multiplied by
    gscale and, when given, by the device scale gscale_t; a missing state reads as 0 and is returned
    as None.  wout is what the copy-out holds before it is rounded to the pull buffer's dtype: w."""
    h = _hp(hp)
    scale = f32(h["gscale"]) * (float(gscale_t) if gscale_t is not None else 1.0)
    W, G = w.double(), g.double().reshape(w.shape) * scale
    zero = torch.zeros_like(W)
    nw, a, b = _apply64(kind, W, st0.double() if st0 is not None else zero, st1.double() if st1 is not None else zero,
                        G, h)
    return nw, (a if st0 is not None else None), (b if st1 is not None else None), nw.clone()


def ftrl_margin(w, st0, st1, g, gscale_t=None, **hp):
    """(zero, tie) bool masks of one FTRL step in fp64: zero = the element takes the |z| <= l1 branch
    (z of mode 1, the new z of mode 0); tie = its distance from l1 is under TIE_EPS."""
    h = _hp(hp)
    scale = f32(h["gscale"]) * (float(gscale_t) if gscale_t is not None else 1.0)
    z, n, G = st0.double(), st1.double(), g.double().reshape(w.shape) * scale
    if h["ftrl_mode"] == 0:
        z = z + G - (torch.sqrt(n + G * G) - torch.sqrt(n)) / h["lr"] * w.double()
    return z.abs() <= h["l1"], (z.abs() - h["l1"]).abs() < TIE_EPS


def _dense_states(kind, n, gen, momentum):
    pos = lambda: torch.rand(n, generator=gen) + 0.1  # noqa: E731
    if kind == SGD:
        return (torch.randn(n, generator=gen) if momentum else None), None
    if kind == ADAM:
        return 0.1 * torch.randn(n, generator=gen), pos()
    if kind == ADAGRAD:
        return pos(), None
    return torch.randn(n, generator=gen), pos()  # FTRL: z, n


def _keep_mask(kind, hp, w, st0, st1, g, gscale_t=None):
    """The elements a comparison covers (all but FTRL threshold ties); asserts the FTRL conditions."""
    n = w.numel()
    if kind != FTRL:
        return torch.ones(n, dtype=torch.bool)
    assert hp["l1"] == 0.5, "the dense FTRL sets use l1 = 0.5"
    zero, tie = ftrl_margin(w, st0, st1, g, gscale_t, **hp)
    assert int(tie.sum()) <= MAX_TIES, f"{int(tie.sum())} elements within {TIE_EPS} of l1"
    share = float(zero.double().mean())
    if n >= 64:
        assert 0.1 <= share <= 0.9, f"{share:.2f} of the elements take the |z| <= l1 branch"
    elif n >= 4:
        assert 0 < int(zero.sum()) < n, "a short FTRL case must still take both branches"
    return ~tie


ADAM_COLD = 3  # the element of every dense Adam case with g = 0, m = 1e-7, v = 0
DENSE_NS = (7, 8, 275, 2051)  # below one vector; one vector; the CTR width; a body and a 3-element tail


def build_dense(hpname, gdt, n, seed=0, gscale_t=None):
    """One fused_opt case: dict(kind, hp, w, st0, st1, g, gscale_t, keep)."""
    kind, _, _, hp = HP_SETS[hpname]
    assert hpname in DENSE_HP
    gen = _gen(seed + 101 * DENSE_HP.index(hpname) + n)
    w = torch.randn(n, generator=gen)
    st0, st1 = _dense_states(kind, n, gen, hp.get("momentum", 0.0))
    g = torch.randn(n, generator=gen).to(GDTYPES[gdt])
    if kind == ADAM:  # a weight that never saw a gradient: v = 0, where only eps keeps the step finite
        g[ADAM_COLD], st0[ADAM_COLD], st1[ADAM_COLD] = 0.0, 1e-7, 0.0
    hp = dict(hp)
    return dict(kind=kind, hp=hp, w=w, st0=st0, st1=st1, g=g, gscale_t=gscale_t,
                keep=_keep_mask(kind, hp, w, st0, st1, g, gscale_t))


def build_dense_wrap(aligned):
    """The two large fused_opt cases: SGD with momentum past the 2048-block grid cap."""
    return build_dense("sgd_momentum", "f32", GRID_WRAP_VEC if aligned else GRID_WRAP_SCALAR, seed=9)


# ------------------------------------------------------------------------- multi-source gradient
def multi_grad64(srcs, off, n, words=None, scales=None):
    """(sum, sumabs) in fp64 of the multi-source gradient of segment [off, off + n): element i is the
    sum over the sources, in order, of source s at chunk element off + i.  The 1-bit form (words int64
    [nsrc, nw], scales [nsrc, ns]) decodes +-scales[s][(off + i) // 1024], the sign from bit
    (off + i) % 64 of word (off + i) // 64 (1 = plus)."""
    q = off + torch.arange(n, dtype=torch.int64)
    tot, sumabs = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    if words is not None:
        assert not srcs and 1 <= words.shape[0] == scales.shape[0] <= MAX_SRC
        assert off >= 0 and off + n <= 64 * words.shape[1] and off + n <= CHUNK * scales.shape[1]
        for s in range(words.shape[0]):
            bit = (words[s][q // 64] >> (q % 64)) & 1
            sc = scales[s].double()[q // CHUNK]
            tot = tot + torch.where(bit == 1, sc, -sc)
            sumabs = sumabs + sc.abs()
        return tot, sumabs
    assert 1 <= len(srcs) <= MAX_SRC
    for s in srcs:
        assert off >= 0 and off + n <= s.numel()
        v = s.double().reshape(-1)[q]
        tot, sumabs = tot + v, sumabs + v.abs()
    return tot, sumabs


def multi_bound(nsrc, sumabs):
    """Rounded fp32 sums of nsrc sources: (nsrc + 1) 2^-24 sum|g_s| (rows_oracle.segment_bound's rule)."""
    return (nsrc + 1.0) * U24 * sumabs


def exact_grid(n, gen):
    """k 2^-7 with integer |k| <= 128: bf16-representable, and any 16 of them sum exactly in fp32."""
    return torch.randint(-128, 129, (n,), generator=gen).float() * 2.0 ** -7


def segments(src):
    """(off, n) of every small segment: every phase 0..7 with exactly one vector after the head and
    with head + body + tail; a segment shorter than its own head; for 1-bit a head that crosses a
    64-bit word and a segment from chunk 0 over chunks 1 and 2 into chunk 3."""
    out = [(3, 2)]
    out += [(off, head_of(off) + 8) for off in range(8)]
    out += [(off, head_of(off) + 8 * 130 + 5) for off in range(8)]
    if src == "onebit":
        out += [(61, head_of(61) + 8 * 130 + 5), (1019, 2100)]
    return out


def build_sources(src, nsrc, L, gen, exact=True):
    """dict(srcs, words, scales): nsrc whole-chunk sources of L elements, pairwise different."""
    assert 1 <= nsrc <= MAX_SRC and L % CHUNK == 0
    if src == "onebit":
        words = torch.randint(-2 ** 63, 2 ** 63 - 1, (nsrc, L // 64), generator=gen, dtype=torch.int64)
        scales = torch.randint(1, 257, (nsrc, L // CHUNK), generator=gen).float() * 2.0 ** -8
        for a in range(nsrc):
            for b in range(a):
                assert not torch.equal(words[a], words[b])
        return dict(srcs=[], words=words, scales=scales)
    srcs = [(exact_grid(L, gen) if exact else torch.randn(L, generator=gen)).to(GDTYPES[src]) for _ in range(nsrc)]
    for a in range(nsrc):
        for b in range(a):
            assert not torch.equal(srcs[a], srcs[b])
        if exact:
            assert torch.equal(srcs[a].double(), srcs[a].to(torch.bfloat16).double())
    return dict(srcs=srcs, words=None, scales=None)


def build_multi(src, nsrc, off, n, hpname="sgd_momentum", wout=None, exact=True, seed=0):
    """One fused_opt_multi / reduce_multi case.  master, st0, st1 and pull (wout's dtype, or None) are
    whole chunks: the segment [off, off + n) holds the values, everything else SENTINEL.  keep marks
    the segment elements a comparison covers."""
    kind, _, _, hp = HP_SETS[hpname]
    hp = dict(hp)
    L = (off + n + CHUNK - 1) // CHUNK * CHUNK
    assert 0 <= off and 0 < n and off + n <= L
    gen = _gen(seed + 7919 * off + 31 * n + nsrc)
    S = build_sources(src, nsrc, L, gen, exact)
    w = torch.randn(n, generator=gen)
    a, b = _dense_states(kind, n, gen, hp.get("momentum", 0.0))

    def whole(x, dtype=torch.float32):
        if x is None:
            return None
        buf = torch.full((L,), SENTINEL, dtype=dtype)
        buf[off:off + n] = x.to(dtype)
        return buf

    master, st0, st1 = whole(w), whole(a), whole(b)
    pull = None if wout is None else torch.full((L,), SENTINEL, dtype=GDTYPES[wout])
    inside = torch.zeros(L, dtype=torch.bool)
    inside[off:off + n] = True
    for buf in (master, st0, st1, pull):
        if buf is not None:
            assert bool((buf[~inside] == SENTINEL).all()) and buf.numel() == L
    gsum, sumabs = multi_grad64(S["srcs"], off, n, S["words"], S["scales"])
    if exact:  # the sum is an fp32 number, whatever the order of the additions
        assert torch.equal(gsum, gsum.float().double()) and float(gsum.abs().max()) <= MAX_SRC
    keep = _keep_mask(kind, hp, w, a, b, gsum)
    return dict(kind=kind, hp=hp, off=off, n=n, L=L, nsrc=nsrc, src=src, master=master, st0=st0, st1=st1, pull=pull,
                inside=inside, gsum=gsum, sumabs=sumabs, keep=keep, **S)


def multi_opt64(c):
    """(w, st0, st1) of the segment in fp64 after the fused reduce + step of case c."""
    o, n = c["off"], c["n"]
    seg = lambda x: None if x is None else x[o:o + n]  # noqa: E731
    w, a, b, _ = dense_opt64(c["kind"], seg(c["master"]), seg(c["st0"]), seg(c["st1"]), c["gsum"], **c["hp"])
    return w, a, b


# ----------------------------------------------------------------------------------- 1-bit pack
PACK_NS = (5, 64, 1000, 1024, 1029, 2048, 3001)


def pack_words(bits):
    """int64 words of a bool vector: element i at word i // 64, bit i % 64 (= byte i // 8, bit i % 8 of
    the little-endian words); the pad bits of the last word are 0."""
    n = bits.numel()
    nw = (n + 63) // 64
    b = torch.zeros(nw * 64, dtype=torch.int64)
    b[:n] = bits.to(torch.int64)
    return (b.reshape(nw, 64) << torch.arange(64, dtype=torch.int64)).sum(1)  # disjoint bits: sum = or


def unpack_bits(words, n):
    q = torch.arange(n, dtype=torch.int64)
    return ((words[q // 64] >> (q % 64)) & 1) == 1


def onebit_pack64(g, err, mom=None, beta1=0.0, bits=None):
    """dict(c, m, scales, bits, words, err) in fp64: with mom, m = beta1 mom + (1 - beta1) g first and
    c = m + e, else c = g + e; scales[k] = mean |c| over the valid elements of chunk k; bit = c >= 0
    (so +0 and -0 give 1); err = c - (bit ? scale : -scale).  `bits` (bool [n]) replaces the sign
    decision in the new error: the error that belongs to bits stored by someone else."""
    n = g.numel()
    x, m = g.double().reshape(-1), None
    if mom is not None:
        m = f32(beta1) * mom.double().reshape(-1) + one_minus_f32(beta1) * x
        x = m
    c = x + err.double().reshape(-1)
    ns = (n + CHUNK - 1) // CHUNK
    cp = torch.zeros(ns * CHUNK, dtype=torch.float64)
    cp[:n] = c.abs()
    valid = torch.full((ns,), float(CHUNK), dtype=torch.float64)
    valid[-1] = n - (ns - 1) * CHUNK
    scales = cp.reshape(ns, CHUNK).sum(1) / valid
    own = c >= 0
    use = own if bits is None else bits
    es = scales.repeat_interleave(CHUNK)[:n]
    return dict(c=c, m=m, scales=scales, bits=own, words=pack_words(own), err=c - torch.where(use, es, -es),
                elem_scale=es)


def pack_margin(o, g, err, mom):
    """bool [n]: the elements whose sign the fp32 rounding of m cannot change:
    |c| > 2^-21 (|m| + |g| + |e|)."""
    return o["c"].abs() > 2.0 ** -21 * (o["m"].abs() + g.double().abs() + err.double().abs())


def build_pack(n, gdt, edt, with_mom, seed=0):
    """dict(g, err, mom, beta1): randn inputs with c == +0 at element 1, c == -0.0 at element 2, and an
    all-zero chunk 1 when there are at least two whole chunks."""
    gen = _gen(seed + n)
    g = torch.randn(n, generator=gen)
    err = 0.1 * torch.randn(n, generator=gen)
    mom = torch.randn(n, generator=gen) if with_mom else None
    bufs = [x for x in (g, err, mom) if x is not None]
    if n >= 5:
        for x in bufs:
            x[1], x[2] = 0.0, -0.0
    if n >= 2 * CHUNK:
        for x in bufs:
            x[CHUNK:2 * CHUNK] = 0.0
    g, err = g.to(GDTYPES[gdt]), err.to(GDTYPES[edt])
    mom = mom.to(GDTYPES[edt]) if with_mom else None
    c = dict(g=g, err=err, mom=mom, beta1=0.9 if with_mom else 0.0, n=n)
    o = onebit_pack64(g, err, mom, c["beta1"])
    if n >= 5:
        assert float(o["c"][1]) == 0.0 and float(o["c"][2]) == 0.0 and bool(o["bits"][1]) and bool(o["bits"][2])
        assert torch.signbit(o["c"][2]) and not torch.signbit(o["c"][1])
    if n >= 2 * CHUNK:
        assert float(o["scales"][1]) == 0.0
    if with_mom:
        assert int((~pack_margin(o, g, err, mom)).sum()) - (3 if n >= 5 else 0) - (CHUNK if n >= 2 * CHUNK else 0) <= 4
    return c


def pack_bounds(o, edt_bf16):
    """(scale bound [ns], error bound [n]): a 1024-term fp32 tree sum and the divide,
    1030 2^-24 mean|c|; the error 2^-23 (|c| + scale) plus the scale's bound, and one bf16 ulp of the
    reference for a bf16 buffer."""
    sb = 1030.0 * U24 * o["scales"]
    eb = 2.0 ** -23 * (o["c"].abs() + o["elem_scale"]) + sb.repeat_interleave(CHUNK)[:o["c"].numel()]
    if edt_bf16:
        eb = eb + bf16_ulp(o["err"])
    return sb, eb


def mom_bound(o, g, mom, beta1, bf16):
    """|m - ref|: two products, the sum and the fp32 1 - beta1: 4 2^-24 (|beta1 m| + |(1 - beta1) g|),
    plus one bf16 ulp for a bf16 buffer."""
    b = 4.0 * U24 * (f32(beta1) * mom.double().abs() + one_minus_f32(beta1) * g.double().abs())
    return b + (bf16_ulp(o["m"]) if bf16 else 0.0)


# --------------------------------------------------------------------------------- 1-bit unpack
UNPACK_NS = (5, 1029, 3001)


def onebit_unpack64(words, scales, n, mult=1.0, prev=None):
    """out = (prev if accumulate else 0) + mult * sum over workers, in order, of the decoded values."""
    tot, _ = multi_grad64([], 0, n, words, scales)
    tot = tot * f32(mult)
    return tot + prev.double().reshape(-1) if prev is not None else tot


def build_unpack(n, nworkers, seed=0):
    """dict(words, scales, prev): exact scales (multiples of 2^-8 in [2^-8, 1]) and a previous output
    on the exact grid, so mult = 0.5 gives an fp32-exact result with and without accumulate."""
    gen = _gen(seed + 13 * n + nworkers)
    L = (n + CHUNK - 1) // CHUNK * CHUNK
    S = build_sources("onebit", nworkers, L, gen)
    prev = exact_grid(n, gen)
    assert bool((prev != 0).any())
    ref = onebit_unpack64(S["words"], S["scales"], n, 0.5, prev)
    assert torch.equal(ref, ref.float().double())
    return dict(words=S["words"][:, :(n + 63) // 64].contiguous(), scales=S["scales"], prev=prev, n=n)


# ------------------------------------------------------------------------------- reduce.hip
ELEM_NS = (5, 8, 2051)


def sumsq64(x):
    return x.double().pow(2).sum()


def clip64(sumsq, max_norm):
    """min(1, max_norm / (sqrt(sumsq) + 1e-6))."""
    return min(1.0, f32(max_norm) / (float(sumsq) ** 0.5 + f32(1e-6)))


def cast64(x, scale):
    """scale * x: the exact product of two fp32 numbers (48 bits: exact in fp64)."""
    return x.double() * f32(scale)


def axpy64(a, x, y):
    """(y + a x, |y| + |a x|)."""
    ax = f32(a) * x.double()
    return y.double() + ax, y.double().abs() + ax.abs()


def reduce_n64(x, scale):
    """scale * sum_k x[k] for x [k, n], in order."""
    acc = torch.zeros(x.shape[1], dtype=torch.float64)
    for k in range(x.shape[0]):
        acc = acc + x[k].double()
    return acc * f32(scale)


def lerp64(w0, w, sc):
    """(sc w0 + (1 - sc) w, |sc w0| + |(1 - sc) w|)."""
    a, b = f32(sc) * w0.double(), one_minus_f32(sc) * w.double()
    return a + b, a.abs() + b.abs()


def fma_bound(mag, ref, out_bf16):
    """axpy / lerp: 2 2^-24 of the summed magnitudes (a product and the sum, or two fused
    multiply-adds), plus one bf16 ulp of the reference for a bf16 output."""
    return 2.0 * U24 * mag + (bf16_ulp(ref) if out_bf16 else 0.0)


def to_dtype(ref64, dtype):
    """An fp64 value that is exact in fp48 -> fp32 (one rounding to nearest even) -> dtype (another)."""
    return ref64.float().to(dtype)


def build_elem(n, xdt, ydt, seed=0, k=3):
    """dict(x, y, xs [k, n] on the exact grid) for cast / axpy / reduce_n."""
    gen = _gen(seed + n)
    x = torch.randn(n, generator=gen).to(GDTYPES[xdt])
    y = torch.randn(n, generator=gen).to(GDTYPES[ydt])
    xs = torch.stack([exact_grid(n, gen) for _ in range(k)]).to(GDTYPES[xdt])
    for a in range(k):
        for b in range(a):
            assert not torch.equal(xs[a], xs[b]) or n < 3
    return dict(x=x, y=y, xs=xs)


# ---------------------------------------------------------------------------------- checkers
# What test_dense_gpu.py asserts of the kernels' results; test_dense_oracle_cpu.py runs the same
# checkers on the fp32 CPU paths (which must pass) and on wrong variants (which must not).
def opt_err(got, ref, keep=None):
    """max |got - ref| / (1 + |ref|) over the compared elements."""
    e = (got.double().reshape(-1) - ref.reshape(-1)).abs() / (1.0 + ref.reshape(-1).abs())
    assert not torch.isnan(e).any(), "NaN in the result"
    if keep is not None:
        e = e[keep]
    return float(e.max()) if e.numel() else 0.0


def check_opt(got, ref, keep, tol):
    """got / ref: (w, st0, st1), a state that does not exist None in both."""
    for name, x, r in zip(("w", "st0", "st1"), got, ref):
        assert (x is None) == (r is None), name
        if r is not None:
            e = opt_err(x, r, keep)
            assert e <= tol, f"{name}: {e:.3g} > {tol}"


def check_copy_out(w, wout):
    """The pull buffer is the kernel's own fp32 w, rounded to nearest even for bf16: bit for bit."""
    assert torch.equal(wout, w.to(wout.dtype)), "copy-out differs from w"


def check_outside(got, before, inside):
    """Everything outside the segment is bit-identical to what it was."""
    assert torch.equal(got[~inside], before[~inside]), "an element outside the segment changed"


def cpu_coef_slack(g, beta1):
    """The fp32 CPU paths form 1 - beta1 in double and round it (0.1f for beta1 = 0.9), the kernels
    subtract in fp32 (1.f - 0.9f = 0.1f - 3.7e-8): what that puts between a CPU path's momentum and the
    oracle's.  Never part of a GPU bound."""
    return abs(f32(1.0 - beta1) - one_minus_f32(beta1)) * g.double().abs().reshape(-1)


def check_pack(c, words, scales, err, mom, mom_slack=0.0):
    """onebit_pack's results on build_pack case c (the buffers as the op left them)."""
    n, g = c["n"], c["g"]
    o = onebit_pack64(g, c["err"], c["mom"], c["beta1"])
    bits = unpack_bits(words, n)
    assert words.numel() == (n + 63) // 64 and torch.equal(words, pack_words(bits)), "pad bits of the last word"
    if c["mom"] is None:
        assert torch.equal(words, o["words"]), f"{int((bits != o['bits']).sum())} sign bits differ"
    else:
        safe = pack_margin(o, g, c["err"], c["mom"])
        assert torch.equal(bits[safe], o["bits"][safe]), "a sign bit outside the rounding margin differs"
        mb = mom_bound(o, g, c["mom"], c["beta1"], mom.dtype == torch.bfloat16)
        over = (mom.double() - o["m"]).abs() - mb - mom_slack
        assert float(over.max()) <= 0.0, f"momentum {float(over.max()):.3g} over its bound"
        o = onebit_pack64(g, c["err"], c["mom"], c["beta1"], bits=bits)
    sb, eb = pack_bounds(o, err.dtype == torch.bfloat16)
    over = (scales.double() - o["scales"]).abs() - sb
    assert float(over.max()) <= 0.0, f"scale {float(over.max()):.3g} over its bound, chunk {int(over.argmax())}"
    over = (err.double() - o["err"]).abs() - eb
    assert float(over.max()) <= 0.0, f"error {float(over.max()):.3g} over its bound, element {int(over.argmax())}"


def check_bounded(got, ref, bound, what):
    over = (got.double().reshape(-1) - ref.reshape(-1)).abs() - bound.reshape(-1)
    assert not torch.isnan(over).any(), "NaN in the result"
    assert float(over.max()) <= 0.0, f"{what}: {float(over.max()):.3g} over the bound, element {int(over.argmax())}"
