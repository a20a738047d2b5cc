"""The dense shard kernels against the fp64 oracles of tests/dense_oracle.py: the dense half of
csrc/kernels/optim.hip, csrc/kernels/compress.hip and csrc/kernels/reduce.hip, every instantiation
the launchers can select.

    test                                 cases                                    kernel
    test_fused_opt                       8 sets x fp32 / bf16 g x n 7 / 8 / 275 / 2051
                                           aligned, wout none / bf16 / fp32       fused_opt_kernel<KIND, float | uint16_t, OUT 0 / 1 / 2, VEC true>
                                                                                  (n 7: tail loop only; 8: one vector; 2051: body + 3-element tail)
                                           every base 4 bytes in                  fused_opt_kernel<KIND, G, OUT, VEC false>
                                           gscale_t given (the fp32-wout runs)    the device-scale read of both
                                         sets: sgd (st0 == nullptr), sgd_momentum (dampening), sgd_nesterov, adam, adamw,
                                         adagrad, ftrl0_dense (mode 0), ftrl1_dense (mode 1)
    test_fused_opt_one_misaligned        only wout / only a bf16 g 4 bytes in     fused_opt_kernel<kSGD, G, OUT, false> by the launcher's test;
                                                                                  16 2^-24 (1 + |w|) from the aligned run
    test_fused_opt_grid_wrap             aligned, 4 196 709 elements              fused_opt_kernel<kSGD, float, 0, true>: 2048 x 256 lanes < n / 8
                                         4 bytes in, 525 065 elements             fused_opt_kernel<kSGD, float, 0, false>: 2048 x 256 lanes < n
    test_reduce_multi                    fp32 / bf16 / 1-bit x nsrc 1 / 2 / 16    reduce_multi_kernel<0, float>, <0, uint16_t>, <1, float>
                                         every phase off 0..7 at n = head + 8 and head + 8 * 130 + 5, off 3 n 2 (all head);
                                         1-bit also off 61 (first vector opens a new word) and off 1019 n 2100 (four chunks)
    test_reduce_multi_rounded            randn, 16 fp32 / bf16 sources            the same two, against (nsrc + 1) 2^-24 sum|g_s|
    test_fused_opt_multi_segments        the same segments, SGD with momentum,    fused_opt_multi_kernel<kSGD, 0 | 1, float | uint16_t, OUT 0 / 1 / 2>
                                         wout none / bf16 / fp32 by off % 3
    test_fused_opt_multi_sets            8 sets x 3 source forms x 3 wout         fused_opt_multi_kernel<KIND, ONEBIT, G, OUT>, every KIND
                                         off 5, n = 3 + 8 * 130 + 5, nsrc 2
    test_fused_opt_multi_grid_wrap       off 5, 4 196 717 elements, 2 bf16 srcs   fused_opt_multi_kernel<kSGD, 0, uint16_t, 0>, second turn of the loop
    test_multi_bindings_refuse           host-side checks only                    (nothing is launched)
    test_opt_bindings_refuse_kind_and_hyper  kind 4 / -1, a 15-element hyper vector   fused_opt, fused_opt_multi, sparse_opt (nothing is launched)
    test_onebit_pack                     n 5 / 64 / 1000 / 1024 / 1029 / 2048 /   onebit_pack_kernel<float | uint16_t, float | uint16_t, MOM false | true>
                                         3001 x g dtype x err dtype x momentum    (full-vector and ragged paths, a block's second chunk absent / present)
    test_onebit_momentum                 g dtype x momentum dtype, n 3001         onebit_momentum_kernel<G, E>
    test_onebit_unpack                   n 5 / 1029 / 3001 x 1 / 3 workers x      onebit_unpack_reduce_kernel<float | uint16_t>, vec = 1 (aligned)
                                         fp32 / bf16 out x accumulate 0 / 1       and vec = 0 (destination one element in)
    test_elementwise                     n 5 / 8 / 2051 / 2056 x dtype pairs,     cast_kernel<X, Y>, axpy_kernel<X, Y>, reduce_n_kernel<X, Y> (vec needs
                                         aligned and 4 bytes in                   n % 8 == 0: 8 and 2056), lerp_kernel<float | uint16_t>
    test_sumsq_and_clip                  fp32 / bf16, aligned and 4 bytes in,     sumsq_partial_kernel<T>, sumsq_partial_scalar_kernel<T>,
                                         n 2051 / 70 001, accumulate              sumsq_finish_kernel, clip_factor_kernel

sparse_opt_kernel and sparse_opt_vec_kernel (the other half of optim.hip) belong to test_rows_gpu.py.

Bounds.  Optimizer: |got - ref| <= 2e-5 (1 + |ref|) for w, st0, st1 against fp64 at every set: on the same
inputs the fp32 CPU path stays under 4e-6 (test_dense_oracle_cpu.py), FTRL mode 1 included.  FTRL elements
within 1e-5 of the l1 threshold (at most 2 per case, asserted by the builder) are not compared.  Copy-out: the
kernel's own w rounded to the pull dtype, bit for bit.  reduce_multi, reduce_n, cast and 1-bit unpack on the
exact grid: bit-exact.  1-bit pack: words bit-exact without momentum (pad bits 0); with momentum wherever
|c| > 2^-21 (|m| + |g| + |e|); scales within 1030 2^-24 mean|c|; errors within 2^-23 (|c| + scale) plus that,
for the bit actually stored; one bf16 ulp more for a bf16 buffer.  axpy / lerp: 2 2^-24 of the summed
magnitudes, plus one bf16 ulp for a bf16 output.  sumsq: 1e-4 relative.  clip factor: 4 2^-23 relative (sqrt,
add, divide, each within an ulp).

Everything outside a segment is a sentinel before the launch and bit-identical after it; the sources are
unchanged.  Every segment was checked on the CPU to lie inside every buffer it indexes.
"""
import pytest
import torch

from ps_amd import ops
from ps_amd.ops import compress as C
from ps_amd.ops import native
from ps_amd.ops import reduce as R

from . import dense_oracle as do

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = do.GDTYPES
WOUTS = (None, "bf16", "f32")


def _at(x, nbytes=0):
    """x on the GPU in a buffer of its own, its base nbytes past a 16-byte boundary (contiguous)."""
    if x is None:
        return None
    k, rem = divmod(nbytes, x.element_size())
    assert rem == 0
    buf = torch.empty(x.numel() + k, dtype=x.dtype, device=DEV)
    v = buf[k:]
    v.copy_(x.reshape(-1))
    assert v.data_ptr() % 16 == nbytes and v.is_contiguous()
    return v


def _cpu(x):
    return None if x is None else x.cpu()


# ------------------------------------------------------------------------------------ fused_opt
def _run_dense(c, wdt=None, mis=0, mis_wout=None, mis_g=None, gscale_t=None):
    """Launch ops.fused_opt on the case; compare with dense_opt64; -> (w, st0, st1, wout) on the CPU."""
    n = c["w"].numel()
    w, a, b = _at(c["w"], mis), _at(c["st0"], mis), _at(c["st1"], mis)
    g = _at(c["g"], mis if mis_g is None else mis_g)
    wout = None if wdt is None else _at(torch.full((n,), 9.0, dtype=DT[wdt]), mis if mis_wout is None else mis_wout)
    gs = None if gscale_t is None else gscale_t.to(DEV)
    ops.fused_opt(c["kind"], w, a, b, g, wout=wout, gscale_t=gs, **c["hp"])
    ref = do.dense_opt64(c["kind"], c["w"], c["st0"], c["st1"], c["g"], gscale_t, **c["hp"])
    got = (_cpu(w), _cpu(a), _cpu(b))
    do.check_opt(got, ref[:3], c["keep"], do.OPT_TOL)
    if wout is not None:
        do.check_copy_out(got[0], wout.cpu())
    assert torch.equal(g.cpu(), c["g"])
    return got + (_cpu(wout),)


@pytest.mark.parametrize("gdt", ["f32", "bf16"])
@pytest.mark.parametrize("n", do.DENSE_NS)
@pytest.mark.parametrize("hpname", do.DENSE_HP)
def test_fused_opt(hpname, n, gdt):
    for mis in (0, 4):
        for wdt in WOUTS:
            gs = torch.tensor([0.75]) if wdt == "f32" else None
            _run_dense(do.build_dense(hpname, gdt, n, gscale_t=gs), wdt, mis, gscale_t=gs)


@pytest.mark.parametrize("which", ["wout_bf16", "wout_f32", "g_bf16"])
def test_fused_opt_one_misaligned(which):
    c = do.build_dense("sgd_momentum", "bf16", 2051)
    wdt = "f32" if which == "wout_f32" else "bf16"
    base = _run_dense(c, wdt)
    one = _run_dense(c, wdt, mis_wout=4) if which.startswith("wout") else _run_dense(c, wdt, mis_g=4)
    # the vector and the scalar kernel contract their multiply-adds differently, so the two runs are not
    # bit-identical; each evaluates the same ~8 fp32 operations on the same inputs: 16 2^-24 (1 + |w|) apart
    # at the most.  (Each run's copy-out equals its own w bit for bit: checked in _run_dense.)
    for x, y in zip(base[:2], one[:2]):
        do.check_bounded(y, x.double(), 16 * do.U24 * (1.0 + x.double().abs()), which)


@pytest.mark.parametrize("aligned", [True, False])
def test_fused_opt_grid_wrap(aligned):
    _run_dense(do.build_dense_wrap(aligned), None, 0 if aligned else 4)


# ------------------------------------------------------------------ reduce_multi, fused_opt_multi
def _sources(c):
    srcs = [s.to(DEV) for s in c["srcs"]]
    words = None if c["words"] is None else c["words"].to(DEV)
    scales = None if c["scales"] is None else c["scales"].to(DEV)
    return srcs, words, scales


def _sources_unchanged(c, srcs, words, scales):
    for s, r in zip(srcs, c["srcs"]):
        assert torch.equal(s.cpu(), r), "a source changed"
    if words is not None:
        assert torch.equal(words.cpu(), c["words"]) and torch.equal(scales.cpu(), c["scales"])


def _run_reduce(c):
    o, n = c["off"], c["n"]
    srcs, words, scales = _sources(c)
    before = torch.full((c["L"],), do.SENTINEL)
    out = before.to(DEV)
    native().reduce_multi(srcs, o, n, out[o:o + n], words, scales)
    got = out.cpu()
    do.check_outside(got, before, c["inside"])
    _sources_unchanged(c, srcs, words, scales)
    return got[o:o + n]


@pytest.mark.parametrize("nsrc", [1, 2, 16])
@pytest.mark.parametrize("src", ["f32", "bf16", "onebit"])
def test_reduce_multi(src, nsrc):
    for off, n in do.segments(src):
        c = do.build_multi(src, nsrc, off, n)
        got = _run_reduce(c)
        ndiff = int((got.double() != c["gsum"]).sum())
        assert torch.equal(got.double(), c["gsum"]), f"off {off}, n {n}: {ndiff} elements differ"


@pytest.mark.parametrize("src", ["f32", "bf16"])
def test_reduce_multi_rounded(src):
    c = do.build_multi(src, 16, 3, do.head_of(3) + 8 * 130 + 5, exact=False)
    do.check_bounded(_run_reduce(c), c["gsum"], do.multi_bound(16, c["sumabs"]), "reduce_multi")


def _run_multi(c):
    o, n = c["off"], c["n"]
    seg = lambda x: None if x is None else x[o:o + n]  # noqa: E731
    bufs = [None if x is None else x.to(DEV) for x in (c["master"], c["st0"], c["st1"], c["pull"])]
    srcs, words, scales = _sources(c)
    native().fused_opt_multi(c["kind"], seg(bufs[0]), seg(bufs[1]), seg(bufs[2]), srcs, o, seg(bufs[3]),
                             ops.hyper_vec(c["hp"]), None, words, scales)
    got = [_cpu(x) for x in bufs]
    do.check_opt(tuple(seg(x) for x in got[:3]), do.multi_opt64(c), c["keep"], do.OPT_TOL)
    if got[3] is not None:
        do.check_copy_out(seg(got[0]), seg(got[3]))
    for x, before in zip(got, (c["master"], c["st0"], c["st1"], c["pull"])):
        if x is not None:
            do.check_outside(x, before, c["inside"])
    assert not torch.equal(seg(got[0]), seg(c["master"]))
    _sources_unchanged(c, srcs, words, scales)


@pytest.mark.parametrize("nsrc", [1, 2, 16])
@pytest.mark.parametrize("src", ["f32", "bf16", "onebit"])
def test_fused_opt_multi_segments(src, nsrc):
    for off, n in do.segments(src):
        _run_multi(do.build_multi(src, nsrc, off, n, "sgd_momentum", wout=WOUTS[off % 3]))


@pytest.mark.parametrize("src", ["f32", "bf16", "onebit"])
@pytest.mark.parametrize("hpname", do.DENSE_HP)
def test_fused_opt_multi_sets(hpname, src):
    for wdt in WOUTS:
        _run_multi(do.build_multi(src, 2, 5, do.head_of(5) + 8 * 130 + 5, hpname, wout=wdt))


def test_fused_opt_multi_grid_wrap():
    _run_multi(do.build_multi("bf16", 2, 5, do.GRID_WRAP_MULTI, "sgd"))


def test_multi_bindings_refuse():
    """Each refusal is a host-side TORCH_CHECK: a Python exception, and nothing is launched."""
    m = native()
    hp = ops.hyper_vec(do.HP_SETS["sgd"][3])
    chunk = torch.ones(1024, device=DEV)
    srcs = [torch.ones(1024, device=DEV) for _ in range(17)]
    words = torch.zeros(1, 32, dtype=torch.int64, device=DEV)
    scales = torch.ones(1, 1, device=DEV)

    def opt(w, s, off, wout=None, words=None, scales=None):
        m.fused_opt_multi(do.SGD, w, None, None, s, off, wout, hp, None, words, scales)

    good = torch.ones(1024, device=DEV)
    opt(good[8:24], srcs[:1], 8)  # the well-formed call passes and steps
    assert float(good[8]) != 1.0 and float(good[7]) == 1.0 and float(good[24]) == 1.0
    bad = [
        lambda: opt(chunk[1000:1024], srcs[:1], 1008),                          # off + n past a source
        lambda: m.reduce_multi(srcs[:1], 1016, 16, chunk[8:24], None, None),    # the same for reduce_multi
        lambda: opt(chunk[8:24], srcs, 8),                                      # 17 sources
        lambda: m.reduce_multi(srcs, 8, 16, chunk[8:24], None, None),
        lambda: opt(chunk[9:25], srcs[:1], 8),                                  # w out of phase with off
        lambda: opt(chunk[8:24], srcs[:1], 8, wout=chunk[9:25]),                # wout out of phase
        lambda: m.reduce_multi(srcs[:1], 3, 16, chunk[8:24], None, None),       # out out of phase
        lambda: opt(chunk[8:24], srcs[:1], -8),                                 # off < 0
        lambda: opt(chunk[8:24], [srcs[0], srcs[1].bfloat16()], 8),             # mixed dtypes
        lambda: opt(chunk[8:24], [srcs[0], srcs[1].cpu()], 8),                  # mixed devices
        lambda: opt(chunk[8:24], [srcs[0][1:]], 8),                             # a misaligned source base
        lambda: opt(chunk[8:24], [], 2040, words=words, scales=torch.ones(1, 2, device=DEV)),  # past 64 nw = 2048
        lambda: opt(chunk[0:16], [], 1024, words=words, scales=scales),         # past 1024 ns = 1024
        lambda: opt(chunk[8:24], srcs[:1], 8, words=words, scales=scales),      # srcs and the 1-bit form together
        lambda: opt(chunk[8:24], [], 8, words=words),                           # words without scales
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert bool((chunk == 1.0).all())  # nothing ran


def test_opt_bindings_refuse_kind_and_hyper():
    """An optimizer kind outside 0..3 and a hyper-parameter vector of the wrong length are refused on the
    host by all three bindings; the extension unpacks the vector in the order ops.hyper_vec packs it."""
    m = native()
    assert tuple(m.OPT_HYPER_FIELDS) == ops.HYPER_FIELDS
    hp = ops.hyper_vec(do.HP_SETS["sgd"][3])
    w, a, b, g = (torch.full((16,), v, device=DEV) for v in (1.0, 2.0, 3.0, 4.0))
    table, ta, tb, tg = (x.reshape(4, 4) for x in (w, a, b, g))
    rows = torch.arange(4, device=DEV)

    def calls(kind, h):
        return [lambda: m.fused_opt(kind, w, a, b, g, None, h, None),
                lambda: m.fused_opt_multi(kind, w, a, b, [g], 0, None, h, None, None, None),
                lambda: m.sparse_opt(kind, table, ta, tb, rows, tg, False, False, h)]

    for kind in (4, -1):
        for call in calls(kind, hp):
            with pytest.raises(RuntimeError):
                call()
    for call in calls(do.SGD, hp[:15]):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    for x, v in ((w, 1.0), (a, 2.0), (b, 3.0), (g, 4.0)):
        assert bool((x == v).all())  # nothing ran


# --------------------------------------------------------------------------------------- 1-bit
@pytest.mark.parametrize("with_mom", [False, True])
@pytest.mark.parametrize("edt", ["f32", "bf16"])
@pytest.mark.parametrize("gdt", ["f32", "bf16"])
@pytest.mark.parametrize("n", do.PACK_NS)
def test_onebit_pack(n, gdt, edt, with_mom):
    c = do.build_pack(n, gdt, edt, with_mom)
    nw, ns = C.packed_sizes(n)
    words = torch.full((nw,), -1, dtype=torch.int64, device=DEV)
    scales = torch.full((ns,), -1.0, device=DEV)
    g, err, mom = c["g"].to(DEV), c["err"].to(DEV), _at(c["mom"])
    C.onebit_pack(g, err, words, scales, mom, c["beta1"])
    do.check_pack(c, words.cpu(), scales.cpu(), err.cpu(), _cpu(mom))
    assert torch.equal(g.cpu(), c["g"])


@pytest.mark.parametrize("mdt", ["f32", "bf16"])
@pytest.mark.parametrize("gdt", ["f32", "bf16"])
def test_onebit_momentum(gdt, mdt):
    c = do.build_pack(3001, gdt, mdt, True)
    m = c["mom"].to(DEV)
    C.onebit_momentum(c["g"].to(DEV), m, 0.9)
    o = do.onebit_pack64(c["g"], c["err"], c["mom"], 0.9)
    do.check_bounded(m.cpu(), o["m"], do.mom_bound(o, c["g"], c["mom"], 0.9, mdt == "bf16"), "momentum")


@pytest.mark.parametrize("odt", ["f32", "bf16"])
@pytest.mark.parametrize("nworkers", [1, 3])
@pytest.mark.parametrize("n", do.UNPACK_NS)
def test_onebit_unpack(n, nworkers, odt):
    c = do.build_unpack(n, nworkers)
    words, scales = c["words"].to(DEV), c["scales"].to(DEV)
    for mis in (0, DT[odt].itemsize):  # aligned: 8-element vector stores; one element in: element stores
        for acc in (False, True):
            buf = torch.full((n + 17,), do.SENTINEL, dtype=DT[odt])
            k = mis // DT[odt].itemsize
            buf[k:k + n] = c["prev"].to(DT[odt])
            dev = _at(buf)
            out = dev[k:k + n]
            assert out.data_ptr() % 16 == mis
            C.onebit_unpack_reduce(words, scales, out, 0.5, acc)
            ref = do.onebit_unpack64(c["words"], c["scales"], n, 0.5, c["prev"] if acc else None)
            got = dev.cpu()
            assert torch.equal(got[k:k + n], do.to_dtype(ref, DT[odt])), f"mis {mis}, accumulate {acc}"
            assert bool((got[:k] == do.SENTINEL).all()) and bool((got[k + n:] == do.SENTINEL).all())
    assert torch.equal(words.cpu(), c["words"])


# ---------------------------------------------------------------------------------- reduce.hip
@pytest.mark.parametrize("ydt", ["f32", "bf16"])
@pytest.mark.parametrize("xdt", ["f32", "bf16"])
@pytest.mark.parametrize("n", do.ELEM_NS + (2056,))
def test_elementwise(n, xdt, ydt):
    c = do.build_elem(n, xdt, ydt)
    for mis in (0, 4):
        x = _at(c["x"], mis)
        y = _at(torch.full((n,), 9.0, dtype=DT[ydt]), mis)
        R.cast_(x, y, 0.3)
        assert torch.equal(y.cpu(), do.to_dtype(do.cast64(c["x"], 0.3), DT[ydt])), f"cast, base + {mis}"
        y = _at(c["y"], mis)
        R.axpy_(0.3, x, y)
        ref, mag = do.axpy64(0.3, c["x"], c["y"])
        do.check_bounded(y.cpu(), ref, do.fma_bound(mag, ref, ydt == "bf16"), f"axpy, base + {mis}")
        assert torch.equal(x.cpu(), c["x"])
        xs = _at(c["xs"], mis).view(c["xs"].shape)
        y = _at(torch.full((n,), 9.0, dtype=DT[ydt]), mis)
        R.reduce_n(xs, y, 0.25)
        assert torch.equal(y.cpu(), do.to_dtype(do.reduce_n64(c["xs"], 0.25), DT[ydt])), f"reduce_n, base + {mis}"
        if xdt == "f32":
            w0, w = c["x"], c["y"].float()
            out = _at(torch.full((n,), 9.0, dtype=DT[ydt]), mis)
            R.lerp(_at(w0, mis), _at(w, mis), 0.3, out)
            ref, mag = do.lerp64(w0, w, 0.3)
            do.check_bounded(out.cpu(), ref, do.fma_bound(mag, ref, ydt == "bf16"), f"lerp, base + {mis}")


@pytest.mark.parametrize("n", [2051, 70001])
@pytest.mark.parametrize("xdt", ["f32", "bf16"])
def test_sumsq_and_clip(xdt, n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DT[xdt])
    ref = float(do.sumsq64(x))
    for mis in (0, 4):  # 4 bytes in: sumsq_partial_scalar_kernel
        out = torch.full((1,), 5.0, device=DEV)
        R.sumsq(_at(x, mis), out)
        assert abs(float(out) - ref) <= 1e-4 * ref, f"base + {mis}"
        R.sumsq(_at(x, mis), out, accumulate=True)
        assert abs(float(out) - 2 * ref) <= 1e-4 * 2 * ref, f"accumulate, base + {mis}"
    sq = out.clone()
    for max_norm in (1.5, 1e6):  # clipped; not clipped (exactly 1)
        f = float(R.clip_factor(sq, max_norm))
        want = do.clip64(float(sq), max_norm)
        assert abs(f - want) <= 4 * 2.0 ** -23 * want
    assert float(R.clip_factor(sq, 1e6)) == 1.0
