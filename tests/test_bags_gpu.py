"""The multi-hot bag kernels (csrc/kernels/bags.hip) per element against the fp64 oracles of
tests/bags_oracle.py, on the path each case was written for (the launcher's return code is
asserted); the ``bag_pool`` route's composition against the same bounds; ``lookup_bags`` on the GPU
against the CPU table, sync-free, through a growth, bitwise against the one-hot lookup, and with
two processes on cuda:0."""
import functools

import pytest
import torch

from ps_amd.ops import sparse as S

from . import bags_oracle as bo
from . import dist_util
from .test_bags_oracle_cpu import _one_hot_pair

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# (dim, misaligned base, path the launcher must report)
DIMS = [(4, False, 1), (16, False, 1), (128, False, 1), (256, False, 1), (10, False, 0), (12, False, 0),
        (260, False, 0), (128, True, 0)]
DTYPES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _case(dim, weights):
    return bo.make_case(dim, seed=100 + dim, weights=weights)


@functools.lru_cache(maxsize=None)
def _refs(dim, weights, mean, dout_dtype):
    c = _case(dim, weights)
    dout = c.dout.to(dout_dtype)
    return (bo.oracle_fwd(c.rows, c.inv, c.bag_off, c.bag_of, c.weights, mean),
            bo.oracle_bwd(dout, c.perm, c.seg_off, c.bag_of, c.bag_off, c.weights, mean), dout)


def _off4(t: torch.Tensor) -> torch.Tensor:
    """A GPU copy of ``t`` whose base is 4 bytes past a 16-byte boundary."""
    k = 4 // t.element_size()
    buf = torch.empty(t.numel() + k, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _dev(c):
    idx = {k: getattr(c, k).to(DEV) for k in ("inv", "bag_off", "bag_of", "perm", "seg_off")}
    return idx, (None if c.weights is None else c.weights.to(DEV))


def _unchanged(idx, c):
    for k, v in idx.items():
        assert torch.equal(v.cpu(), getattr(c, k)), f"{k} was written"


@pytest.mark.parametrize("dim,misaligned,path", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("mean", [False, True])
def test_bag_pool_fwd_per_element(dim, misaligned, path, dtype, weights, mean):
    c = _case(dim, weights)
    idx, w = _dev(c)
    rows = _off4(c.rows) if misaligned else c.rows.to(DEV)
    out = torch.full((c.nbags, dim), float("nan"), dtype=dtype, device=DEV)
    _, got = S.bag_pool_fwd(rows, idx["inv"], idx["bag_off"], out, w, mean, return_path=True)
    assert got == path
    bo.assert_within(out, *_refs(dim, weights, mean, dtype)[0], mean, f"fwd dim {dim}")
    _unchanged(idx, c)


@pytest.mark.parametrize("dim,misaligned,path", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("mean", [False, True])
def test_bag_pool_bwd_per_element(dim, misaligned, path, dtype, weights, mean):
    c = _case(dim, weights)
    idx, w = _dev(c)
    _, ref, dout = _refs(dim, weights, mean, dtype)
    dout = _off4(dout) if misaligned else dout.to(DEV)
    drows = torch.full((c.nseg, dim), float("nan"), device=DEV)  # nseg = nnz: empty pad segments included
    _, got = S.bag_pool_bwd(dout, idx["perm"], idx["seg_off"], idx["bag_of"], idx["bag_off"], drows, w, mean,
                            return_path=True)
    assert got == path
    bo.assert_within(drows, *ref, mean, f"bwd dim {dim}")
    _unchanged(idx, c)


def test_bag_pool_grid_wraps_at_20000_bags_and_segments():
    """dim 128: 8 bags (segments) per block, at most 2048 blocks -> the grid-stride loop wraps."""
    c = bo.make_case(128, nbags=20000, nu=20000, seed=7, weights=True, pad_segments=False)
    assert c.nbags == 20000 and c.nseg == 20000 and 2048 * 8 < 20000
    idx, w = _dev(c)
    out = torch.empty(c.nbags, 128, device=DEV)
    _, p = S.bag_pool_fwd(c.rows.to(DEV), idx["inv"], idx["bag_off"], out, w, True, return_path=True)
    assert p == 1
    bo.assert_within(out, *bo.oracle_fwd(c.rows, c.inv, c.bag_off, c.bag_of, c.weights, True), True, "fwd wrap")
    drows = torch.empty(c.nseg, 128, device=DEV)
    _, p = S.bag_pool_bwd(c.dout.to(DEV), idx["perm"], idx["seg_off"], idx["bag_of"], idx["bag_off"], drows, w, True,
                          return_path=True)
    assert p == 1
    bo.assert_within(drows, *bo.oracle_bwd(c.dout, c.perm, c.seg_off, c.bag_of, c.bag_off, c.weights, True), True,
                     "bwd wrap")


@pytest.mark.parametrize("dim", [128, 10])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("mean", [False, True])
def test_bag_pool_route_disabled_composition_meets_the_same_bounds(monkeypatch, dim, dtype, weights, mean):
    monkeypatch.setenv("PS_AMD_DISABLE", "bag_pool")
    c = _case(dim, weights)
    idx, w = _dev(c)
    fref, bref, dout = _refs(dim, weights, mean, dtype)
    out = torch.empty(c.nbags, dim, dtype=dtype, device=DEV)
    _, p = S.bag_pool_fwd(c.rows.to(DEV), idx["inv"], idx["bag_off"], out, w, mean, return_path=True)
    assert p == -1  # the one-hot kernels, not a bag kernel
    bo.assert_within(out, *fref, mean, "composed fwd")
    drows = torch.empty(c.nseg, dim, device=DEV)
    _, p = S.bag_pool_bwd(dout.to(DEV), idx["perm"], idx["seg_off"], idx["bag_of"], idx["bag_off"], drows, w, mean,
                          return_path=True)
    assert p == -1
    bo.assert_within(drows, *bref, mean, "composed bwd")
    _unchanged(idx, c)


def test_pool_unique_autograd_matches_the_composition(monkeypatch):
    c = _case(128, True)
    idx, w = _dev(c)
    nu = c.rows.shape[0]
    seg_off = idx["seg_off"][:nu + 1].contiguous()  # one segment per leaf row: without the empty pads

    def run():
        leaf = c.rows.to(DEV).requires_grad_(True)
        out = S.pool_unique(leaf, idx["inv"], idx["perm"], seg_off, idx["bag_off"], idx["bag_of"], w, True,
                            torch.bfloat16)
        out.backward(c.dout.to(DEV).bfloat16())
        return out.detach().float().cpu(), leaf.grad.cpu()

    fused = run()
    monkeypatch.setenv("PS_AMD_DISABLE", "bag_pool")
    comp = run()
    fref, bref, _ = _refs(128, True, True, torch.bfloat16)
    bref = tuple(t[:nu] for t in bref)
    for o, g in (fused, comp):
        bo.assert_within(o.bfloat16(), *fref, True, "pool_unique out")
        bo.assert_within(g, *bref, True, "pool_unique grad")


# ------------------------------------------------------------------------------------- table
def _table_run(dev, mode, grow=False, rows=3000, steps=4):
    from ps_amd.parallel.sparse_table import SparseTable
    from ps_amd.parallel.updaters import AdagradUpdater

    t = SparseTable("t", 16, [rows] * 4, AdagradUpdater(0.05, 1e-8, rowwise=True), init=(-0.2, 0.2), id_mode=mode,
                    seed=3, device=dev, fields=4, grow=grow)
    outs = []
    for step in range(steps):
        v, o, w = bo.make_bags(32, 4, 400, seed=50 + step, weights=True)
        if mode == "map":
            v = v * 7919 + (1 << 35)
        out = t.lookup_bags(v.to(dev), o.to(dev), weights=w.to(dev), mode="mean" if step % 2 else "sum")
        (out.float().pow(2).sum() * 0.01).backward()
        t.push_pending()
        outs.append(out.detach().cpu())
    syncs = t.stats["host_syncs"]
    t.synchronize()
    return outs, syncs, dict(t.stats)


@pytest.mark.parametrize("mode", ["map", "direct"])
def test_lookup_bags_gpu_matches_cpu(mode):
    a, _, _ = _table_run("cpu", mode)
    b, _, _ = _table_run(DEV, mode)
    for x, y in zip(a, b):
        torch.testing.assert_close(y, x, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mode", ["map", "direct"])
def test_lookup_bags_gpu_world1_is_host_sync_free(mode):
    _, syncs, _ = _table_run(DEV, mode, steps=5)
    assert syncs == 0


def test_lookup_bags_growable_table_matches_a_table_built_large():
    small, _, st = _table_run(DEV, "map", grow=True, rows=16)
    large, _, _ = _table_run(DEV, "map", grow=False, rows=3000)
    assert st["grows"] >= 1, st
    for x, y in zip(small, large):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", DTYPES)
def test_length_one_bags_are_bitwise_the_one_hot_lookup_on_gpu(dtype):
    _one_hot_pair(DEV, dtype)


def _w2_body(tp, samples, steps):
    from ps_amd.parallel.sparse_table import ShardedSparseTable
    from ps_amd.parallel.updaters import AdagradUpdater

    torch.cuda.set_device(0)
    t = ShardedSparseTable("emb", 16, [300] * 4, tp, AdagradUpdater(0.05, 1e-8, rowwise=True), init=(-0.1, 0.1),
                           seed=4, device=DEV, fields=4, average=False, exchange="auto")
    W, r = tp.world, tp.rank
    outs = []
    for s in range(steps):
        v, o, w = bo.make_bags(samples, 4, 300, seed=70 + s, weights=True)
        v, o, w = bo.slice_bags(v, o, 4, r * samples // W, (r + 1) * samples // W, w)
        out = t.lookup_bags(v.to(DEV), o.to(DEV), weights=w.to(DEV), mode="mean")
        (out.pow(2).sum() * 0.05).backward()
        t.push_pending()
        outs.append(out.detach().cpu())
    t.synchronize()
    rows = t.pull(torch.arange(300, device=DEV).repeat(4, 1).t().contiguous()).cpu()
    torch.cuda.synchronize()
    info = {"exchange": t.exchange, "info": {k: str(v) for k, v in t.exchange_info.items()}}
    t.close()
    return outs, rows, info


def test_lookup_bags_two_processes_on_one_gpu_equal_one_rank(record_property):
    w2 = dist_util.run(_w2_body, 2, (32, 3), timeout=120.0)
    w1 = dist_util.run(_w2_body, 1, (32, 3), timeout=120.0)[0]
    record_property("exchange_info", str(w2[0][2]))
    print("exchange_info:", w2[0][2])
    assert w2[0][2]["exchange"] == w2[1][2]["exchange"] in ("plane", "collective")
    for s in range(3):
        torch.testing.assert_close(torch.cat([w2[0][0][s], w2[1][0][s]]), w1[0][s], rtol=1e-5, atol=1e-5)
    for r in range(2):
        torch.testing.assert_close(w2[r][1], w1[1], rtol=1e-5, atol=1e-5)
