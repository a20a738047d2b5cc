"""The sparse-row HIP kernels against the fp64 oracles of tests/rows_oracle.py, on their vectorised
paths, at DLRM width (dim = 128) and past the 2048-block grid cap.

Which kernel each case reaches (lg = log2(dim / 4); see also the table in rows_oracle.py):

    test                              cases                         kernel
    test_sparse_opt                   dim 4 / 16 / 128 / 256        sparse_opt_vec_kernel<KIND, float | uint16_t>, lg 0 / 2 / 5 / 6
                                      dim 12 / 10 / 260             sparse_opt_kernel<KIND, float | uint16_t>
    test_sparse_opt_misaligned_base   dim 128, table + 4 bytes      sparse_opt_kernel (the alignment test of the launcher;
                                      3 optimizers x 3 forms        each form reads rows / perm / ncount its own way)
    test_sparse_opt_grid_wrap         dim 128, 20 000 entries       sparse_opt_vec_kernel, 2048 blocks x 8 rows < 20 000
                                      dim 10, 10 000 entries        sparse_opt_kernel, 2048 blocks x 4 rows < 10 000
    test_segment_reduce               dim 4 / 16 / 128 / 256        segment_reduce_rows_vec_kernel<S, O>, S, O in {float, uint16_t}
                                      dim 10 / 260                  segment_reduce_rows_kernel<S, O>
    test_segment_reduce_grid_wrap     dim 128, 20 000 segments      segment_reduce_rows_vec_kernel<float, float>
    test_gather_rows                  fp32 table, off 0 / 8:
                                        dim 4 / 16 / 128 / 256      gather_rows_lg_kernel<float | uint16_t>
                                        dim 12 / 260, fp32 out      gather_rows_vec4_kernel
                                        dim 12 / 260, bf16 out      gather_rows_kernel<float, uint16_t>
                                        dim 10                      gather_rows_kernel<float, O>
                                      off 2, any dim                gather_rows_kernel<float, O>
                                      bf16 table, any dim / off     gather_rows_kernel<uint16_t, O>
    test_gather_rows_grid_wrap        dim 128, 20 000 rows          gather_rows_lg_kernel<float>
    test_lazy_init_rows               dim 4 / 8 / 64 / 128 / 256    lazy_init_rows_kernel, L = 1 / 2 / 16 / 32 / 64 lanes per row
                                      dim 12 / 6                    lazy_init_rows_kernel, one row per wave, scalar tail stores
    test_lazy_init_rows_grid_wrap     dim 4, 600 000 entries        lazy_init_rows_kernel, 2048 blocks x 256 entries < 600 000
    test_scatter_add_rows             fp32 / bf16 source            scatter_add_rows_kernel<float | uint16_t>
    test_embedding_bag_fwd            fp32 / bf16 out, off 0 / 5    embedding_bag_fwd_kernel<float | uint16_t>
    test_row_plane                    dim 128 / 12 / 260            row_plane_recv_kernel, row_plane_send_kernel<4>, row_plane_accum_kernel<4>
                                      (cap 2048: two accumulate blocks per worker; cap 512: one)
                                      dim 10                        row_plane_recv_kernel, row_plane_send_kernel<1>, row_plane_accum_kernel<1>
                                      then the apply                sparse_opt_vec_kernel (128) / sparse_opt_kernel (12, 10, 260)
    test_row_plane_send_block_stride  dim 256, 131 200 blocks       row_plane_send_kernel<4>, block-stride loop past 65 536 blocks

The other kernels of that stretch of sparse.hip are outside this file: sparse_lr_fwd_kernel is
covered by test_kernels_gpu.py::test_embedding_bag_and_lr, hash_slots_kernel by the test_hash_slots_*
tests of test_sparse_gpu.py, and unique_runs_kernel runs in every GPU SparseTable lookup
(test_sparse_gpu.py::test_sparse_table_gpu_matches_cpu, ..._world1_is_host_sync_free).

Bounds.  sparse_opt: 2e-5 (1 + |ref|) for the table and both states against fp64; the fp32 CPU path
stays within 1e-5 of the same oracle on the same inputs (test_rows_oracle_cpu.py).  segment_reduce:
(n + 1) 2^-24 sum|x| for a segment of n rows, plus 2^-8 |ref| for a bf16 output.  gather: bit-exact
for ACT_NONE and ACT_RELU, assert_close defaults (fp32) or one bf16 ulp (bf16) for leaky and sigmoid.
lazy_init: bit-exact against the Philox oracle S.init_values, at a span (hi - lo) that is a power of
two and at one that is not.  Row plane: exact copies; the
accumulator within 3 * 2^-24 sum|g| of the rank-order fp64 sum.

Every index handed to a kernel was checked on the CPU by the builder that made it.
"""
import pytest
import torch

from ps_amd import ops
from ps_amd.ops import native
from ps_amd.ops import sparse as S

from . import rows_oracle as ro

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPT_TOL = 2e-5
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _dev(x):
    return x.to(DEV) if x is not None else None


# ------------------------------------------------------------------------------------ sparse_opt
def _run_opt(c, misalign=False):
    """Launch ops.sparse_opt on the case and compare table, st0, st1 with sparse_opt64."""
    if misalign:  # a view 4 bytes into its storage: contiguous, not 16-byte aligned
        buf = torch.empty(c["table"].numel() + 1, device=DEV)
        t = buf[1:].view(c["table"].shape)
        t.copy_(c["table"])
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    else:
        t = _dev(c["table"]).clone()
    a, b = _dev(c["st0"]), _dev(c["st1"])
    rows = _dev(c["rows"])
    perm = rows if c["perm"] is c["rows"] else _dev(c["perm"])
    nc = None if c["ncount"] is None else torch.tensor([c["ncount"]], dtype=torch.int32, device=DEV)
    ops.sparse_opt(c["kind"], t, a, b, rows, _dev(c["grad"]), rowwise=c["rowwise"], skip_zero=c["skip_zero"],
                   perm=perm, ncount=nc, **c["hp"])
    rt, ra, rb = ro.sparse_opt64(c["kind"], c["table"], c["st0"], c["st1"], c["rows"], c["grad"], perm=c["perm"],
                                 rowwise=c["rowwise"], skip_zero=c["skip_zero"], ncount=c["ncount"], **c["hp"])
    for name, got, ref, src in (("table", t, rt, c["table"]), ("st0", a, ra, c["st0"]), ("st1", b, rb, c["st1"])):
        if ref is None:
            continue
        got = got.cpu()
        err = ((got.double() - ref).abs() / (1.0 + ref.abs())).max().item()
        assert err <= OPT_TOL, f"{name}: {err:.3g} > {OPT_TOL}"
        # rows never named: bit-identical to the input
        assert torch.equal(got[~c["named"]], src[~c["named"]]), f"{name}: an unnamed row changed"
    assert not torch.equal(t.cpu()[c["named"]], c["table"][c["named"]])
    assert torch.equal(rows.cpu(), c["rows"])  # the index lists are read-only


@pytest.mark.parametrize("dim,gdt,hp,form", ro.opt_cases(), ids=lambda v: str(v))
def test_sparse_opt(dim, gdt, hp, form):
    _run_opt(ro.build_opt(dim, gdt, hp, form))


@pytest.mark.parametrize("hp", ro.HP_SHORT)
@pytest.mark.parametrize("form", ro.FORMS)
def test_sparse_opt_misaligned_base(hp, form):
    _run_opt(ro.build_opt(128, "f32", hp, form), misalign=True)


@pytest.mark.parametrize("dim,n", [(128, 20000), (10, 10000)])
def test_sparse_opt_grid_wrap(dim, n):
    _run_opt(ro.build_opt_wrap(dim, n))


# ---------------------------------------------------------------------------- segment_reduce_rows
def _run_segment(dim, sdt, odt, mean, nseg, seed, lens=ro.SEG_LENS):
    n = ro.seg_rows(nseg, lens)
    perm, seg_off = ro.build_segments(nseg, n, seed, lens)
    src = torch.randn(n, dim, generator=torch.Generator().manual_seed(seed + 1)).to(sdt)
    out = torch.full((nseg, dim), 9.0, dtype=odt, device=DEV)
    S.segment_reduce_rows(src.to(DEV), perm.to(DEV), seg_off.to(DEV), out, mean)
    ref, sumabs, cnt = ro.segment_reduce64(src, perm, seg_off, mean)
    bound = ro.segment_bound(ref, sumabs, cnt, mean, odt == torch.bfloat16)
    over = (out.cpu().double() - ref).abs() - bound
    assert not torch.isnan(over).any(), "NaN in the output"
    worst = int(over.max(1).values.argmax())
    assert over.max().item() <= 0.0, f"{over.max().item():.3g} over the bound, segment {worst}"


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("odt", ["f32", "bf16"])
@pytest.mark.parametrize("sdt", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [4, 16, 128, 256, 10, 260])
def test_segment_reduce(dim, sdt, odt, mean):
    # 75 segments: each length of SEG_LENS ten times; at dim 4 a wave step holds 64 segments
    _run_segment(dim, DT[sdt], DT[odt], mean, 75, 31 + dim)


@pytest.mark.parametrize("mean", [False, True])
def test_segment_reduce_grid_wrap(mean):
    # 2048 blocks x 4 waves x 2 segments = 16 384 < 20 000; short segments keep the source near 12 MB
    _run_segment(128, torch.float32, torch.float32, mean, 20000, 5, lens=(0, 1, 2, 1, 0, 3, 1))


# ------------------------------------------------------------------------------------ gather_rows
def _check_gather(table, rows, odt, out_off, act, pad=16):
    dim = table.shape[1]
    ro.check_rows(rows, table.shape[0])
    out = torch.full((rows.numel(), dim + pad), 5.0, dtype=odt, device=DEV)
    assert out_off + dim <= out.shape[1]
    S.gather_rows(table.to(DEV), rows.to(DEV), out, out_off, act)
    out = out.cpu()
    keep = torch.ones(dim + pad, dtype=torch.bool)
    keep[out_off:out_off + dim] = False
    assert bool((out[:, keep] == 5.0).all()), "a column outside the slice was written"
    got = out[:, out_off:out_off + dim]
    ref = ro.gather64(table, rows, act)
    assert bool((got[rows < 0] == 0).all())
    if act in (ro.ACT_NONE, ro.ACT_RELU):
        assert torch.equal(got, ref.float().to(odt)), "not bit-exact"  # fp64 -> fp32 is exact here, -> bf16 is RNE
    elif odt == torch.float32:
        torch.testing.assert_close(got, ref.float())
    else:
        over = (got.double() - ref).abs() - ro.bf16_ulp(ref)
        assert over.max().item() <= 0.0, f"{over.max().item():.3g} over one bf16 ulp"


@pytest.mark.parametrize("out_off", [0, 8, 2])
@pytest.mark.parametrize("odt", ["f32", "bf16"])
@pytest.mark.parametrize("tdt", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [4, 16, 128, 256, 12, 260, 10])
def test_gather_rows(dim, tdt, odt, out_off):
    g = torch.Generator().manual_seed(100 + dim)
    table = torch.randn(500, dim, generator=g).to(DT[tdt])
    rows = torch.randint(0, 500, (333,), generator=g)  # 333: two blocks at dim 4, an odd tail everywhere
    rows[::13] = -1
    for act in (ro.ACT_NONE, ro.ACT_RELU, ro.ACT_LEAKY, ro.ACT_SIGMOID):
        _check_gather(table, rows, DT[odt], out_off, act)


@pytest.mark.parametrize("odt", ["f32", "bf16"])
def test_gather_rows_grid_wrap(odt):
    # 2048 blocks x 4 waves x 2 rows = 16 384 < 20 000
    g = torch.Generator().manual_seed(9)
    table = torch.randn(6000, 128, generator=g)
    rows = torch.randint(0, 6000, (20000,), generator=g)
    rows[::101] = -1
    _check_gather(table, rows, DT[odt], 0, ro.ACT_RELU, pad=0)


# --------------------------------------------------------------------------------- lazy_init_rows
SENT = 7.0


def _lazy_case(n, table_rows, seed):
    """(rows, flagged): n entries with -1 pads and duplicates; `flagged` rows exist already."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, table_rows, (n,), generator=g)
    rows[::17] = -1
    rows[5::23] = rows[4::23][:rows[5::23].numel()]  # adjacent duplicates inside one 64-entry step
    rows[-3:] = rows[:3]                             # and duplicates far apart
    live = rows[rows >= 0].unique()
    flagged = live[torch.randperm(live.numel(), generator=g)[:live.numel() // 5]]
    return ro.check_rows(rows, table_rows), flagged


def _run_lazy(dim, n, table_rows, use_keys, lo, hi, seed=1234, row_base=1000):
    rows, flagged = _lazy_case(n, table_rows, seed + dim)
    # one key per row (duplicates of a row must agree); field bits above bit 44 as in map mode
    keys = (rows * 7919 + (3 << 44)) if use_keys else None
    table = torch.full((table_rows, dim), SENT, device=DEV)
    flags = torch.zeros(table_rows, dtype=torch.uint8)
    flags[flagged] = 1
    flags = flags.to(DEV)
    S.lazy_init_rows(table, rows.to(DEV), flags, seed, row_base, lo, hi, keys=_dev(keys))
    table, flags = table.cpu(), flags.cpu()
    named = torch.zeros(table_rows, dtype=torch.bool)
    named[rows[rows >= 0]] = True
    want_flags = named.clone()
    want_flags[flagged] = True
    assert torch.equal(flags.bool(), want_flags) and int(flags.max()) == 1
    new = named.clone()
    new[flagged] = False
    idx = torch.nonzero(new).reshape(-1)
    gkeys = idx * 7919 + (3 << 44) if use_keys else idx + row_base
    ref = S.init_values(seed, gkeys, dim, lo, hi)
    assert bool((table[~new] == SENT).all()), "a flagged or unnamed row was written"
    return table[idx], ref, idx.numel()


@pytest.mark.parametrize("lo,hi", [(-0.1, 0.1), (-0.25, 0.25)], ids=["span0.2", "span0.5"])
@pytest.mark.parametrize("use_keys", [True, False], ids=["keys", "row_base"])
@pytest.mark.parametrize("dim", [4, 8, 64, 128, 256, 12, 6])
def test_lazy_init_rows(dim, use_keys, lo, hi):
    # 200 entries -> four 64-entry wave steps, each with far more new rows than P = 64 / L for dim >= 8.
    # span 0.2 is not a power of two: lo + span * u must be a rounded product and a rounded sum, as in
    # the host oracles, for the bits to agree (one fused multiply-add differs in the last place)
    got, ref, nnew = _run_lazy(dim, 200, 400, use_keys, lo, hi)
    assert nnew > 100
    assert torch.equal(got, ref)


def test_lazy_init_rows_grid_wrap():
    # 2048 blocks x 4 waves x 64 entries = 524 288 < 600 000
    got, ref, nnew = _run_lazy(4, 600000, 100000, False, -0.5, 0.5)
    assert nnew > 70000
    assert torch.equal(got, ref)


# --------------------------------------------------------------- scatter_add_rows, embedding_bag
@pytest.mark.parametrize("sdt", ["f32", "bf16"])
def test_scatter_add_rows(sdt):
    g = torch.Generator().manual_seed(21)
    table = torch.randn(300, 10, generator=g)
    rows = ro.check_rows(torch.randperm(300, generator=g)[:130], 300)  # unique rows: no conflicts
    src = torch.randn(130, 10, generator=g).to(DT[sdt])
    t = table.to(DEV)
    S.scatter_add_rows(src.to(DEV), rows.to(DEV), t)
    ref = table.double()
    ref[rows] += src.double()
    bound = torch.zeros_like(ref)
    bound[rows] = 3 * ro.U24 * (table.double()[rows].abs() + src.double().abs())  # two terms: (n + 1) 2^-24 sum|x|
    assert ((t.cpu().double() - ref).abs() - bound).max().item() <= 0.0
    untouched = torch.ones(300, dtype=torch.bool)
    untouched[rows] = False
    assert torch.equal(t.cpu()[untouched], table[untouched])


@pytest.mark.parametrize("out_off", [0, 5])
@pytest.mark.parametrize("odt", ["f32", "bf16"])
def test_embedding_bag_fwd(odt, out_off):
    g = torch.Generator().manual_seed(22)
    table = torch.randn(200, 10, generator=g)
    ids = ro.check_rows(torch.randint(0, 200, (37, 7), generator=g), 200)
    for act in (ro.ACT_RELU, ro.ACT_SIGMOID):
        out = torch.full((37, 7 * 10 + 9), 5.0, dtype=DT[odt], device=DEV)
        S.embedding_bag_fwd(table.to(DEV), ids.to(DEV), out, out_off, act)
        out = out.cpu()
        got = out[:, out_off:out_off + 70]
        assert bool((out[:, :out_off] == 5.0).all()) and bool((out[:, out_off + 70:] == 5.0).all())
        ref = ro.gather64(table, ids.reshape(-1), act).reshape(37, 70)
        if act == ro.ACT_RELU:
            assert torch.equal(got, ref.float().to(DT[odt]))
        elif odt == "f32":
            torch.testing.assert_close(got, ref.float())
        else:
            assert ((got.double() - ref).abs() - ro.bf16_ulp(ref)).max().item() <= 0.0


# ------------------------------------------------------------------- row plane, single process
def _ptrs(ts):
    return [int(t.data_ptr()) for t in ts]


@pytest.mark.parametrize("dim,counts,cap,table_rows", ro.PLANE_CASES, ids=str)
def test_row_plane(dim, counts, cap, table_rows):
    """recv -> send -> accum (two rounds) -> apply, with W = 3 local arenas passed as peer pointers."""
    p = ro.build_plane_case(dim, counts, cap, table_rows)
    W, cap, me = p["W"], p["cap"], p["me"]
    nat = native()
    # recv: keys and (offset, count) pairs, exactly
    skeys, meta = [_dev(x) for x in p["skeys"]], [_dev(x) for x in p["meta"]]
    rkeys = torch.full((W * cap,), -5, dtype=torch.int64, device=DEV)
    pmeta = torch.full((2 * W,), -5, dtype=torch.int64, device=DEV)
    nat.row_plane_recv(_ptrs(skeys), _ptrs(meta), me, cap, rkeys, pmeta)
    rkeys_ref, pmeta_ref = ro.row_plane_recv_ref(p["skeys"], p["meta"], me, cap)
    assert torch.equal(rkeys.cpu(), rkeys_ref) and torch.equal(pmeta.cpu(), pmeta_ref)

    # send: the rows of the resolved slots, zero rows for unresolved ones, nothing outside [off, off + cnt)
    rslots = ro.check_rows(ro.plane_slots(rkeys_ref, 7), table_rows)
    for w in range(W):  # what the kernels will index in each arena stays inside it
        assert p["offs"][w] + counts[w] <= p["arenas"][w].shape[0] == p["grads"][w].shape[0]
    arenas = [_dev(a).clone() for a in p["arenas"]]
    table = _dev(p["table"])
    nat.row_plane_send(table, _dev(rslots), pmeta, _ptrs(arenas), cap)
    for got, ref in zip(arenas, ro.row_plane_send_ref(p["table"], rslots, pmeta_ref, p["arenas"], cap)):
        assert torch.equal(got.cpu(), ref)

    # accum, round 1: overwrite on first touch (acc starts at a sentinel), rank-order sums after
    acc = torch.full((table_rows, dim), 100.0, device=DEV)
    tflag = torch.zeros(table_rows, dtype=torch.int32, device=DEV)
    touched = torch.full((table_rows,), -1, dtype=torch.int64, device=DEV)
    tcount = torch.zeros(1, dtype=torch.int32, device=DEV)
    sent = torch.full((table_rows, dim), 100.0)
    flags0 = torch.zeros(table_rows, dtype=torch.int32)

    def accum_round(grads_cpu, slots, tag, acc_before, flags_before):
        grads = [_dev(x) for x in grads_cpu]
        touched.fill_(-1)
        tcount.zero_()
        nat.row_plane_accum(_ptrs(grads), _dev(slots), pmeta, acc, tflag, tag, touched, tcount, cap)
        ref, flags_ref, tset = ro.row_plane_accum_ref(grads_cpu, slots, pmeta_ref, acc_before, flags_before, tag, cap)
        sumabs = torch.zeros(table_rows, dim, dtype=torch.float64)
        for w in range(W):
            s = slots[w * cap:w * cap + counts[w]]
            gw = grads_cpu[w].double()[p["offs"][w]:p["offs"][w] + counts[w]]
            sumabs.index_add_(0, s[s >= 0], gw[s >= 0].abs())
        got = acc.cpu()
        over = (got.double() - ref).abs() - 3 * ro.U24 * sumabs  # untouched rows: bound 0, so exact
        assert over.max().item() <= 0.0, f"acc {over.max().item():.3g} over the bound"
        nt = int(tcount.item())
        tl = touched.cpu()
        assert nt == len(tset) and set(tl[:nt].tolist()) == tset and bool((tl[nt:] == -1).all())
        assert torch.equal(tflag.cpu(), flags_ref)
        return got, flags_ref, tset

    acc1, flags1, t1 = accum_round(p["grads"], rslots, 1, sent, flags0)
    shared = torch.zeros(table_rows, dtype=torch.int64)
    for w in range(W):
        s = rslots[w * cap:w * cap + counts[w]]
        shared[s[s >= 0]] += 1
    assert int((shared == 2).sum()) >= 1 and (not all(counts) or int((shared == 3).sum()) >= 1)
    assert t1 == set(torch.nonzero(shared).reshape(-1).tolist())

    # round 2, new tag, reset count, fewer slots: overwrites round 1's rows, keeps the rest
    rslots2 = ro.check_rows(ro.plane_slots(rslots, 5), table_rows)
    acc2, _, t2 = accum_round(p["grads2"], rslots2, 2, acc1, flags1)
    assert t2 <= t1 and len(t2) >= 1

    # the production apply: rows = perm = touched, live length on the device
    kind, rowwise, skip_zero, hp = ro.HP_SETS[ro.plane_apply_set(dim)]
    st0, st1 = ro.build_states(kind, rowwise, table_rows, dim, 3)
    tl = ro.check_rows(touched.cpu(), table_rows)
    t, a, b = table.clone(), _dev(st0), _dev(st1)
    ops.sparse_opt(kind, t, a, b, touched, acc, rowwise=rowwise, skip_zero=skip_zero, perm=touched, ncount=tcount, **hp)
    rt, ra, rb = ro.sparse_opt64(kind, p["table"], st0, st1, tl, acc2, perm=tl, rowwise=rowwise, skip_zero=skip_zero,
                                 ncount=int(tcount.item()), **hp)
    un = torch.ones(table_rows, dtype=torch.bool)
    un[list(t2)] = False
    for got, ref, src in ((t, rt, p["table"]), (a, ra, st0), (b, rb, st1)):
        if ref is not None:
            got = got.cpu()
            assert ((got.double() - ref).abs() / (1.0 + ref.abs())).max().item() <= OPT_TOL
            assert torch.equal(got[un], src[un])
    assert not torch.equal(t.cpu()[~un], p["table"][~un])


def test_row_plane_send_block_stride():
    """W = 2, dim 256 (4 entries per block), cap 262 400: worker 1's entries begin at block 65 600,
    past the 65 536-block grid, so only the block-stride step reaches them."""
    W, cap, dim, counts = 2, 262400, 256, (300, 1000)
    g = torch.Generator().manual_seed(8)
    table = torch.randn(2048, dim, generator=g)
    rslots = torch.full((W * cap,), -1, dtype=torch.int64)
    for w in range(W):
        rslots[w * cap:w * cap + counts[w]] = torch.randint(0, 2048, (counts[w],), generator=g)
    rslots[3], rslots[cap + 998] = -1, -1
    # stale slots past a worker's count must not be sent anywhere
    rslots[cap + 1000:cap + 1040] = 5
    ro.check_rows(rslots, 2048)
    pmeta = torch.tensor([0, counts[0], 0, counts[1]], dtype=torch.int64)
    arenas_cpu = [torch.full((c, dim), -3.0) for c in counts]  # the arenas hold only cnt rows each
    arenas = [a.to(DEV) for a in arenas_cpu]
    native().row_plane_send(table.to(DEV), rslots.to(DEV), pmeta.to(DEV), _ptrs(arenas), cap)
    for got, ref in zip(arenas, ro.row_plane_send_ref(table, rslots, pmeta, arenas_cpu, cap)):
        assert torch.equal(got.cpu(), ref)
