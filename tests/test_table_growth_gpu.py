"""Growable sparse tables on cuda:0.

* rehash_rows (HIP) vs the composition oracle (hash_slots insert + masked index copies): moved
  rows are copies, so every comparison is bit-exact.  The probe position of a key under
  collisions depends on the insertion order, which neither side fixes, so rows are compared per
  key, and the map itself through its own lookups.
* SparseTable built with rows=8 and grow=True against the same table sized generously: growth
  while a plan is pending, while micro-batches are queued, and with the push on the side stream.
* The growth policy on the device: no host wait while growing or afterwards.
* W = 2 thread-ranks, the checkpoint of a grown table, and a reference model on growable tables.
"""
import pytest
import torch

from ps_amd.ops import sparse as S
from ps_amd.parallel.transport import run_loopback

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


# ------------------------------------------------------------------------------ kernel
def _keys(kind, n):
    if kind == "seq":
        return torch.arange(n) + 1000
    g = torch.Generator().manual_seed(n)
    ids = torch.randperm(1 << 20, generator=g)[:n] * 1048573 + (1 << 39)  # distinct, below 2^44
    return ((torch.arange(n) % 4) << 44) | ids  # keys carrying field bits


def _fresh(cap, dim, states):
    hk = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    table = torch.zeros(cap, dim, device=DEV)
    flags = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    st = {"none": [], "rowwise": [torch.zeros(cap, device=DEV)],
          "full2": [torch.zeros(cap, dim, device=DEV) for _ in range(2)]}[states]
    return hk, table, flags, st


def _check_rehash(old_cap, new_cap, dim, states, keys):
    g = torch.Generator().manual_seed(old_cap + dim)
    hk, table, flags, st = _fresh(old_cap, dim, states)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    old_slots = S.hash_slots(hk, keys.to(DEV), True, status) if keys.numel() else keys.to(DEV)
    # every old position holds data, live or not: only the live ones may arrive
    table.copy_(torch.randn(old_cap, dim, generator=g))
    flags.copy_(torch.randint(0, 2, (old_cap,), generator=g).to(torch.uint8))
    for s in st:
        s.copy_(torch.rand(s.shape, generator=g) + 0.5)
    new = _fresh(new_cap, dim, states)
    ref = _fresh(new_cap, dim, states)
    remap = S.rehash_rows(hk, new[0], table, new[1], flags, new[2], st, new[3])
    rref = S.rehash_rows_ref(hk, ref[0], table, ref[1], flags, ref[2], st, ref[3])
    assert int(status.item()) == 0
    live = hk >= 0
    assert int(live.sum()) == keys.numel()
    assert torch.equal(remap < 0, ~live) and torch.equal(rref < 0, ~live)  # -1 exactly at the empty positions
    q, qr = remap[live], rref[live]
    assert q.unique().numel() == q.numel() and int(q.min() if q.numel() else 0) >= 0
    assert int(q.max() if q.numel() else 0) < new_cap
    assert torch.equal(new[0][q], hk[live])
    assert torch.equal(torch.sort(new[0]).values, torch.sort(ref[0]).values)  # same keys in both maps
    if keys.numel():  # the new map finds every key where the rows went
        found = S.hash_slots(new[0], keys.to(DEV), False, status)
        assert torch.equal(found, remap[old_slots]) and int(status.item()) == 0
    # payload at the new slots == the old rows == what the oracle moved, bit for bit
    for got, want, old in [(new[1], ref[1], table), (new[2], ref[2], flags)] + list(zip(new[3], ref[3], st)):
        assert torch.equal(got[q], old[live]) and torch.equal(got[q], want[qr])
        rest = torch.ones(new_cap, dtype=torch.bool, device=DEV)
        rest[q] = False
        assert not got[rest].any()  # every other row is still zero
    rest = torch.ones(new_cap, dtype=torch.bool, device=DEV)
    rest[q] = False
    assert (new[0][rest] == -1).all()


@pytest.mark.parametrize("caps", [(64, 128), (64, 1024)])
@pytest.mark.parametrize("states", ["none", "rowwise", "full2"])
@pytest.mark.parametrize("dim", [1, 6, 8, 64])
def test_rehash_rows_matches_oracle(dim, states, caps):
    for kind in ("seq", "fields"):
        _check_rehash(caps[0], caps[1], dim, states, _keys(kind, caps[0] // 2 - 1))  # load just under 1/2


@pytest.mark.parametrize("states", ["none", "rowwise", "full2"])
def test_rehash_rows_grid_stride_wraps(states):
    """32768 positions at dim 8: more lane groups than the launch has, so every group walks
    several positions."""
    _check_rehash(32768, 65536, 8, states, _keys("fields", 32768 // 2 - 1))


@pytest.mark.parametrize("dim", [1, 6, 8, 64])
def test_rehash_rows_empty_map(dim):
    _check_rehash(64, 128, dim, "rowwise", torch.zeros(0, dtype=torch.int64))


def test_rehash_rows_rejects_small_target():
    hk, table, flags, _ = _fresh(64, 4, "none")
    nk, nt, nf, _ = _fresh(64, 4, "none")
    with pytest.raises(ValueError):
        S.rehash_rows(hk, nk, table, nt, flags, nf)
    with pytest.raises(RuntimeError):  # the binding checks on its own
        S.native().rehash_rows(hk, nk, table, nt, flags, nf, [], [], torch.empty_like(hk))


# ------------------------------------------------------------------------------ W = 1 table
def _table(grow, dev=DEV, **kw):
    from ps_amd.parallel.sparse_table import SparseTable
    from ps_amd.parallel.updaters import AdamUpdater

    return SparseTable("t", 8, 8 if grow else [1000, 500], AdamUpdater(0.05), init=(-0.2, 0.2), id_mode="map",
                       seed=3, device=dev, fields=2, grow=grow, **kw)


def _ids(steps=4, batch=64, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 400, (batch, 2), generator=g) * 7919 + (1 << 35)).to(DEV) for _ in range(steps)]


def _step(t, ids):
    rows = t.lookup(ids)
    (rows.float().pow(2).sum() * 0.01).backward()
    t.push_pending()
    return rows.detach()


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def _grown_ok(t, at_least=2):
    t.synchronize()  # raises if the map ever overflowed
    assert t.stats["grows"] >= at_least and t.stats["capacity"] == t.shard.capacity == t.shard.hkeys.numel()
    assert t.table.shape[0] == t.flags.shape[0] == t.shard.capacity
    assert int(t.shard.status.item()) == 0


@pytest.mark.parametrize("overlap", [False, True])
def test_growable_table_equals_fixed(overlap):
    a, b = _table(True, overlap=overlap), _table(False, overlap=overlap)
    assert a.stats["capacity"] == 64
    for ids in _ids():
        _close(_step(a, ids), _step(b, ids))
    _grown_ok(a)
    probe = torch.cat(_ids())
    _close(a.pull(probe), b.pull(probe))
    assert int((a.shard.hkeys >= 0).sum()) == int((b.shard.hkeys >= 0).sum())


def test_growth_while_a_plan_is_pending():
    """Two lookups before one backward: the second one grows the shard while the first one's
    plan still holds owner-local slots, which must follow the rows."""
    a, b = _table(True), _table(False)
    grew_pending = 0
    for small, big in zip(_ids(3, 32, seed=5), _ids(3, 64, seed=6)):
        outs = []
        for t in (a, b):
            r1 = t.lookup(small)
            g0 = t.stats["grows"]
            r2 = t.lookup(big)
            if t is a and t.stats["grows"] > g0:
                grew_pending += 1
            (r1.float().pow(2).sum() * 0.01 + r2.float().pow(2).sum() * 0.02).backward()
            t.push_pending()
            outs.append((r1.detach(), r2.detach()))
        _close(outs[0][0], outs[1][0])
        _close(outs[0][1], outs[1][1])
    assert grew_pending >= 1
    _grown_ok(a)
    probe = torch.cat(_ids(3, 32, seed=5) + _ids(3, 64, seed=6))
    _close(a.pull(probe), b.pull(probe))


def test_growth_while_micro_batches_are_queued():
    """accumulating=True over two micro-batches: the second lookup grows the shard while the
    first micro-batch's (slot, gradient) pairs wait for the round's single update."""
    a, b = _table(True), _table(False)
    grew_queued = 0
    for small, big in zip(_ids(3, 32, seed=7), _ids(3, 64, seed=8)):
        outs = []
        for t in (a, b):
            t.accumulating = True
            r1 = t.lookup(small)
            (r1.float().pow(2).sum() * 0.01).backward()
            t.push_pending()
            assert len(t._acc) == 1
            g0 = t.stats["grows"]
            r2 = t.lookup(big)
            if t is a and t.stats["grows"] > g0:
                grew_queued += 1
            (r2.float().pow(2).sum() * 0.01).backward()
            t.accumulating = False
            t.push_pending()
            assert not t._acc
            outs.append((r1.detach(), r2.detach()))
        _close(outs[0][0], outs[1][0])
        _close(outs[0][1], outs[1][1])
    assert grew_queued >= 1
    _grown_ok(a)
    probe = torch.cat(_ids(3, 32, seed=7) + _ids(3, 64, seed=8))
    _close(a.pull(probe), b.pull(probe))


def test_growth_takes_no_host_sync():
    """The device work of a step done before the next one starts (the synchronize stands in
    for the model's compute): growth is decided from landed snapshots and the bound alone, and
    lookups of keys that exist neither wait nor grow."""
    a = _table(True)
    batches = _ids()
    for ids in batches:
        _step(a, ids)
        torch.cuda.synchronize()
    assert a.stats["host_syncs"] == 0
    grows = a.stats["grows"]
    assert grows >= 2
    for i in range(10):
        _step(a, batches[i % 4])
        torch.cuda.synchronize()
        assert a.stats["grows"] == grows
    assert a.stats["host_syncs"] == 0
    _grown_ok(a)


def test_checkpoint_of_grown_table_loads_into_small_one():
    a = _table(True)
    for ids in _ids():
        _step(a, ids)
    sd = a.state_dict()
    b = _table(True)
    b.load_state_dict(sd)
    assert b.stats["capacity"] == a.stats["capacity"] == b.shard.hkeys.numel()
    assert b.shard._pol.live_snap == int((a.shard.hkeys >= 0).sum()) and b.shard._pol.since == 0
    probe = torch.cat(_ids())
    assert torch.equal(b.pull(probe), a.pull(probe))
    for ids in _ids(6)[4:]:  # both go on training, and growing on their own, alike
        _close(_step(b, ids), _step(a, ids))
    _grown_ok(b, at_least=0)


# ------------------------------------------------------------------------------ W = 2
def _sparse_body(tp, rows, grow, dev):
    from ps_amd.parallel.sparse_table import ShardedSparseTable
    from ps_amd.parallel.updaters import AdagradUpdater

    t = ShardedSparseTable("emb", 16, rows, tp, AdagradUpdater(0.1, 1e-8, rowwise=True), init=(-0.1, 0.1),
                           id_mode="map", seed=3, device=dev, fields=2, grow=grow)
    g = torch.Generator().manual_seed(100 + tp.rank)
    for _ in range(3):
        ids = torch.randint(0, 1500, (128, 2), generator=g)
        out = t.lookup(ids.to(dev))
        (out.float() * torch.linspace(-1, 1, 16, device=dev)).sum().backward()
        t.push_pending()
    probe = torch.arange(1500).repeat(2, 1).t().contiguous()
    out = t.pull(probe.to(dev)).cpu()
    t.synchronize()
    return out, dict(t.stats), t.exchange


def test_growable_world2_gpu_equals_fixed_cpu():
    res = run_loopback(_sparse_body, 2, [8, 8], True, DEV)
    ref = run_loopback(_sparse_body, 2, [3000, 2000], False, torch.device("cpu"))
    for r in range(2):
        torch.testing.assert_close(res[r][0], res[0][0], rtol=0, atol=0)
        torch.testing.assert_close(res[r][0], ref[0][0], rtol=1e-5, atol=1e-6)
        assert res[r][1]["grows"] >= 1 and res[r][1]["capacity"] > 256 and res[r][2] == "collective"


# ------------------------------------------------------------------------------ model
def _dnn_body(tp, emb_rows, grow):
    from ps_amd.context import ctx
    from ps_amd.data.dataset import synthetic_ctr
    from ps_amd.models.reference import DNN, local_table_factory
    from ps_amd.train.trainer import CollectiveEngine, Trainer

    ctx.init()
    tf = local_table_factory("cuda", seed=7, grow=True) if grow else local_table_factory("cuda", seed=7)
    m = DNN.build_model(4, 8, 6, [32, 8, 1], gen=torch.Generator().manual_seed(0), emb_rows=emb_rows,
                        table_factory=tf, init_scale=0.2).to(DEV)
    tr = Trainer(m, CollectiveEngine(m, tp, bucket_mb=0.002, overlap=False), device=DEV)
    for i in range(3):
        tr.train([synthetic_ctr(64, fields=4, numeric=6, ids_per_field=40, wide_k=0, wide_size=500, seed=i)])
    tr.engine.synchronize()
    ids = torch.arange(40).repeat(4, 1).t().contiguous().to(DEV)
    tab = m.tables()["emF"]
    return ({k: v.detach().cpu() for k, v in m.named_parameters()}, tab.pull(ids).cpu(), dict(tab.stats))


def test_reference_model_on_growable_tables():
    grown = run_loopback(_dnn_body, 1, 8, True)[0]
    fixed = run_loopback(_dnn_body, 1, 256, False)[0]
    for k, v in fixed[0].items():
        torch.testing.assert_close(grown[0][k], v, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(grown[1], fixed[1], rtol=1e-4, atol=1e-4)
    assert grown[2]["grows"] >= 1 and fixed[2]["grows"] == 0
