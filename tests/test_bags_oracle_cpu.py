"""Multi-hot embedding bags without a GPU: the CPU paths of ``bag_pool_fwd`` / ``bag_pool_bwd`` /
``pool_unique`` against the fp64 oracles of tests/bags_oracle.py and against torch's own
``embedding_bag``; ``SparseTable.lookup_bags`` against a dense ``nn.EmbeddingBag`` model built from
the same Philox rows; length-1 bags against the one-hot ``lookup`` bit for bit; W = 2 (gloo
processes) and W = 3 (loopback threads) against the single-process run; the layers and the DLRM."""
import pytest
import torch
import torch.nn.functional as F

from ps_amd.ops import sparse as S
from ps_amd.parallel.sparse_table import ShardedSparseTable, SparseTable
from ps_amd.parallel.transport import run_loopback
from ps_amd.parallel.updaters import AdagradUpdater

from . import bags_oracle as bo
from . import dist_util

MODES = [("sum", False), ("sum", True), ("mean", False), ("mean", True)]  # (mode, weights)


@pytest.mark.parametrize("dim", [4, 10, 128])
@pytest.mark.parametrize("mode,weights", MODES)
def test_cpu_ops_meet_the_oracle_bounds(dim, mode, weights):
    c = bo.make_case(dim, seed=dim, weights=weights)
    mean = mode == "mean"
    idx = [t.clone() for t in (c.inv, c.bag_off, c.bag_of, c.perm, c.seg_off)]
    out, path = S.bag_pool_fwd(c.rows, c.inv, c.bag_off, torch.empty(c.nbags, dim), c.weights, mean, return_path=True)
    assert path == -1  # no kernel on CPU tensors
    bo.assert_within(out, *bo.oracle_fwd(c.rows, c.inv, c.bag_off, c.bag_of, c.weights, mean), mean, "fwd")
    drows = S.bag_pool_bwd(c.dout, c.perm, c.seg_off, c.bag_of, c.bag_off, torch.empty(c.nseg, dim), c.weights, mean)
    bo.assert_within(drows, *bo.oracle_bwd(c.dout, c.perm, c.seg_off, c.bag_of, c.bag_off, c.weights, mean), mean,
                     "bwd")
    for a, b in zip(idx, (c.inv, c.bag_off, c.bag_of, c.perm, c.seg_off)):
        assert torch.equal(a, b)


def test_cpu_ops_bf16_out_and_bf16_dout():
    c = bo.make_case(16, seed=5, weights=True)
    out = S.bag_pool_fwd(c.rows, c.inv, c.bag_off, torch.empty(c.nbags, 16, dtype=torch.bfloat16), c.weights, True)
    bo.assert_within(out, *bo.oracle_fwd(c.rows, c.inv, c.bag_off, c.bag_of, c.weights, True), True, "fwd bf16")
    dout = c.dout.bfloat16()
    drows = S.bag_pool_bwd(dout, c.perm, c.seg_off, c.bag_of, c.bag_off, torch.empty(c.nseg, 16), c.weights, True)
    bo.assert_within(drows, *bo.oracle_bwd(dout, c.perm, c.seg_off, c.bag_of, c.bag_off, c.weights, True), True,
                     "bwd bf16")


@pytest.mark.parametrize("mode,weights", [("sum", False), ("mean", False), ("sum", True)])
def test_cpu_ops_match_torch_embedding_bag(mode, weights):
    """forward = F.embedding_bag on the unique rows; backward = its autograd gradient of the rows."""
    c = bo.make_case(12, seed=9, weights=weights, pad_segments=False)
    w = c.rows.clone().requires_grad_(True)
    ref = F.embedding_bag(c.inv, w, c.bag_off[:-1], mode=mode, per_sample_weights=c.weights,
                          include_last_offset=False)
    ref.backward(c.dout)
    out = S.bag_pool_fwd(c.rows, c.inv, c.bag_off, torch.empty(c.nbags, 12), c.weights, mode == "mean")
    torch.testing.assert_close(out, ref.detach(), rtol=1e-5, atol=1e-5)
    drows = S.bag_pool_bwd(c.dout, c.perm, c.seg_off, c.bag_of, c.bag_off, torch.empty(c.nseg, 12), c.weights,
                           mode == "mean")
    torch.testing.assert_close(drows, w.grad, rtol=1e-5, atol=1e-5)
    # pool_unique: the same through autograd
    leaf = c.rows.clone().requires_grad_(True)
    o2 = S.pool_unique(leaf, c.inv, c.perm, c.seg_off, c.bag_off, c.bag_of, c.weights, mode == "mean")
    o2.backward(c.dout)
    torch.testing.assert_close(o2.detach(), ref.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(leaf.grad, w.grad, rtol=1e-5, atol=1e-5)


def test_pool_unique_refuses_weights_that_require_grad():
    c = bo.make_case(4, seed=1, weights=True)
    with pytest.raises(ValueError):
        S.pool_unique(c.rows, c.inv, c.perm, c.seg_off, c.bag_off, c.bag_of, c.weights.requires_grad_(True))


def test_bag_pool_is_a_route():
    from ps_amd import knobs

    assert "bag_pool" in knobs.ROUTES and knobs.enabled("bag_pool")


# ------------------------------------------------------------------------------------- table
ROWS, FIELDS, DIM, SEED, INIT = [60, 40], 2, 8, 3, (-0.2, 0.2)


def _dense_model(mode):
    """nn.EmbeddingBag over the table's key space (direct mode: key = field offset + id), rows from
    the table's own first-touch init."""
    w = S.init_values(SEED, torch.arange(sum(ROWS)), DIM, *INIT)
    return torch.nn.EmbeddingBag.from_pretrained(w.clone(), freeze=False, mode=mode, include_last_offset=True)


def _flat_keys(values, offsets):
    G = offsets.numel() - 1
    f = torch.repeat_interleave(torch.arange(G) % FIELDS, offsets[1:] - offsets[:-1])
    return values + torch.tensor([0, ROWS[0]])[f]


@pytest.mark.parametrize("mode,weights", [("sum", False), ("mean", False), ("sum", True)])
def test_table_lookup_bags_equals_dense_embedding_bag_and_trains_like_it(mode, weights):
    t = SparseTable("t", DIM, ROWS, AdagradUpdater(0.05, 1e-8), init=INIT, seed=SEED, fields=FIELDS)
    emb = _dense_model(mode)
    opt = torch.optim.Adagrad(emb.parameters(), lr=0.05, eps=1e-8)
    for step in range(3):
        b = bo.make_bags(24, FIELDS, 40, seed=20 + step, weights=weights)
        values, offsets = b[0], b[1]
        w = b[2] if weights else None
        out = t.lookup_bags(values, offsets, weights=w, mode=mode)
        assert out.shape == (24, FIELDS, DIM)
        ref = emb(_flat_keys(values, offsets), offsets, per_sample_weights=w).view(24, FIELDS, DIM)
        torch.testing.assert_close(out.detach(), ref.detach(), rtol=1e-5, atol=1e-6)
        plan = t._pending[-1]
        opt.zero_grad()
        (out.pow(2).sum() * 0.05).backward()
        (ref.pow(2).sum() * 0.05).backward()
        torch.testing.assert_close(plan.leaf.grad, emb.weight.grad[plan.rslots], rtol=1e-5, atol=1e-6)
        t.push_pending()
        opt.step()
    t.synchronize()
    got, want = t.pull_keys(torch.arange(sum(ROWS))), emb.weight.detach()
    assert bool(((got - want).abs() <= 1e-5 * (1 + want.abs())).all())


def _one_hot_pair(device="cpu", out_dtype=None):
    mk = lambda: SparseTable("t", DIM, ROWS, AdagradUpdater(0.05, 1e-8, rowwise=True), init=INIT, seed=SEED,  # noqa: E731
                             fields=FIELDS, device=device)
    a, b = mk(), mk()
    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        ids = torch.randint(0, 12, (32, FIELDS), generator=g).to(device)  # duplicates within the batch
        ra = a.lookup(ids, out_dtype)
        rb = b.lookup_bags(ids.reshape(-1), torch.arange(ids.numel() + 1, device=device), out_dtype=out_dtype)
        assert torch.equal(ra, rb)
        pa, pb = a._pending[-1], b._pending[-1]
        (ra.float().pow(2).sum() * 0.05).backward()
        (rb.float().pow(2).sum() * 0.05).backward()
        assert torch.equal(pa.leaf.grad, pb.leaf.grad)
        a.push_pending()
        b.push_pending()
    a.synchronize()
    b.synchronize()
    assert torch.equal(a.table, b.table)


def test_length_one_bags_are_bitwise_the_one_hot_lookup():
    _one_hot_pair()


def test_lookup_bags_shapes_checks_and_empty_input():
    t = SparseTable("t", DIM, ROWS, AdagradUpdater(0.05, 1e-8), init=INIT, seed=SEED, fields=FIELDS)
    z = t.lookup_bags(torch.zeros(0, dtype=torch.int64), torch.zeros(5, dtype=torch.int64))
    assert z.shape == (2, FIELDS, DIM) and not bool(z.any())
    with pytest.raises(ValueError):
        t.lookup_bags(torch.zeros(3, dtype=torch.int64), torch.tensor([0, 1, 2, 3]))  # 3 bags, 2 fields
    with pytest.raises(ValueError):
        t.lookup_bags(torch.zeros(2, dtype=torch.int64), torch.tensor([0, 1, 2]), mode="max")
    with pytest.raises(ValueError):
        t.lookup_bags(torch.zeros(2, dtype=torch.int64), torch.tensor([0, 1, 2]),
                      weights=torch.ones(2, requires_grad=True))
    one = SparseTable("o", DIM, 50, AdagradUpdater(0.05, 1e-8), init=INIT, seed=SEED)
    assert one.lookup_bags(torch.tensor([1, 2, 3]), torch.tensor([0, 0, 3, 3])).shape == (3, DIM)
    # keys_of is what it was: the factored helper sees the same flat ids / fields
    ids = torch.tensor([[3, 7], [59, 39]])
    keys, nbad = t.keys_of(ids)
    assert keys.tolist() == [3, 67, 59, 99] and int(nbad) == 0


def _sharded_body(tp, use_prefetch, steps=3, samples=24):
    t = ShardedSparseTable("emb", DIM, [300] * 3, tp, AdagradUpdater(0.05, 1e-8, rowwise=True), init=(-0.1, 0.1),
                           seed=4, fields=3, average=False)
    W, r = tp.world, tp.rank
    batches = []
    for s in range(steps):
        v, o, w = bo.make_bags(samples, 3, 300, seed=30 + s, weights=True)
        batches.append(bo.slice_bags(v, o, 3, r * samples // W, (r + 1) * samples // W, w))
    outs = []
    if use_prefetch:
        t.prefetch_bags(batches[0][0], batches[0][1])
    for i, (v, o, w) in enumerate(batches):
        if use_prefetch and i + 1 < steps:
            t.prefetch_bags(batches[i + 1][0], batches[i + 1][1])
        out = t.lookup_bags(v, o, weights=w, mode="mean")
        (out.pow(2).sum() * 0.05).backward()
        t.push_pending()
        outs.append(out.detach().clone())
    t.synchronize()
    return outs, t.pull(torch.arange(300).repeat(3, 1).t().contiguous()), len(t._pf)


def _assert_sharded_equals_single(per_rank, single):
    outs1, rows1, _ = single
    for s in range(len(outs1)):
        torch.testing.assert_close(torch.cat([p[0][s] for p in per_rank]), outs1[s], rtol=1e-5, atol=1e-5)
    for p in per_rank:
        torch.testing.assert_close(p[1], rows1, rtol=1e-5, atol=1e-5)


def test_sharded_lookup_bags_gloo_world2_equals_single_process():
    _assert_sharded_equals_single(dist_util.run(_sharded_body, 2, (False,)), run_loopback(_sharded_body, 1, False)[0])


def test_sharded_lookup_bags_loopback_world3_equals_single_process():
    _assert_sharded_equals_single(run_loopback(_sharded_body, 3, False), run_loopback(_sharded_body, 1, False)[0])


@pytest.mark.parametrize("world", [1, 2])
def test_prefetch_bags_then_lookup_bags_equals_inline_routing(world):
    a = run_loopback(_sharded_body, world, False)
    b = run_loopback(_sharded_body, world, True)
    for (oa, ta, _), (ob, tb, left) in zip(a, b):
        assert left == 0  # every prefetched route was consumed by its lookup
        for x, y in zip(oa, ob):
            assert torch.equal(x, y)
        assert torch.equal(ta, tb)


# ----------------------------------------------------------------------------- layers / model
def test_embedding_bag_layer_pushes_like_embedding_layer():
    from ps_amd.models.layers import EmbeddingBagLayer, EmbeddingLayer

    mk = lambda: SparseTable("t", DIM, ROWS, AdagradUpdater(0.05, 1e-8), init=INIT, seed=SEED, fields=FIELDS)  # noqa: E731
    ta, tb = mk(), mk()
    la, lb = EmbeddingLayer("em", FIELDS, DIM, ta, activation="relu"), EmbeddingBagLayer("em", FIELDS, DIM, tb,
                                                                                        activation="relu")
    ids = torch.randint(0, 30, (16, FIELDS), generator=torch.Generator().manual_seed(2))
    oa = la(ids)
    ob = lb(ids.reshape(-1), torch.arange(ids.numel() + 1))
    assert ob.shape == (16, FIELDS * DIM) and torch.equal(oa, ob)
    oa.sum().backward()
    ob.sum().backward()
    assert la.push_sparse() == lb.push_sparse() > 0
    assert torch.equal(ta.table, tb.table)
    v, o, w = bo.make_bags(16, FIELDS, 30, seed=3, weights=True)
    assert EmbeddingBagLayer("em", FIELDS, DIM, tb, mode="mean")(v, o, w).shape == (16, FIELDS * DIM)
    lb.clear()
    assert not tb._pending


def test_dlrm_length_one_bags_equal_the_one_hot_model_bitwise():
    from ps_amd.models.dlrm import DLRM, dlrm_batch, dlrm_batch_multihot

    rows = [50, 70, 30]

    def run(multihot):
        torch.manual_seed(0)
        m = DLRM(dense_in=13, table_rows=rows, dim=8, bottom=(16,), top=(16, 8), overlap=False)
        dense, sparse, y = dlrm_batch(32, rows, seed=5)
        sp = (sparse.reshape(-1), torch.arange(sparse.numel() + 1)) if multihot else sparse
        m.prefetch(sp)
        logit = m(dense, sp)
        F.binary_cross_entropy_with_logits(logit, y).backward()
        m.push_sparse()
        m.emb.table.synchronize()
        return logit.detach(), [p.grad.clone() for p in m.parameters()], m.emb.table.table.clone()

    (la, ga, ta), (lb, gb, tb) = run(False), run(True)
    assert torch.equal(la, lb) and torch.equal(ta, tb)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
    dense, (values, offsets), y = dlrm_batch_multihot(16, rows, 5, seed=1)
    ln = offsets[1:] - offsets[:-1]
    assert offsets.numel() == 16 * 3 + 1 and int(offsets[-1]) == values.numel() and int(ln.max()) <= 5
    assert int(ln.min()) == 0 and bool((values < torch.tensor(rows)[torch.arange(48) % 3].repeat_interleave(ln)).all())
    torch.manual_seed(0)
    m = DLRM(dense_in=13, table_rows=rows, dim=8, bottom=(16,), top=(16, 8), overlap=False)
    assert m(dense, (values, offsets)).shape == (16,)
