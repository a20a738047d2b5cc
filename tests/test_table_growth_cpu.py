"""Growable sparse tables on the CPU: the growth policy (pure bookkeeping, driven with scripted
call sizes and snapshots), CPU tables that grow vs tables sized generously from the start,
the checkpoint of a grown table, W = 2 over the loopback transport, and the argument errors.
"""
import random

import pytest
import torch

from ps_amd.ops import sparse as S
from ps_amd.parallel.sparse_table import (GROW_HARD_LOAD, GROW_SOFT_LOAD, GrowthPolicy, RowShard, ShardedSparseTable,
                                          SparseTable)
from ps_amd.parallel.transport import run_loopback
from ps_amd.parallel.updaters import AdagradUpdater, AdamUpdater


# ------------------------------------------------------------------------------ policy
class _Map:
    """What the policy's owner would do, minus the device: a set of live keys, and snapshots that
    have landed at the next call when ``delay`` is 0, ``delay`` calls later than that otherwise
    (None: never on their own)."""

    def __init__(self, cap, delay):
        self.pol = GrowthPolicy(cap)
        self.live = set()
        self.delay = delay
        self.snap = None  # [count, calls until landed]
        self.waits = 0
        self.grows = []

    def _poll(self):
        assert self.pol.in_flight and self.snap is not None
        if self.snap[1] is not None and self.snap[1] < 0:
            v, self.snap = self.snap[0], None
            return v
        return None

    def _wait(self):
        # a wait is asked for only when a snapshot is in flight and has not landed
        assert self.pol.in_flight and self.snap is not None
        assert self.snap[1] is None or self.snap[1] >= 0
        self.waits += 1
        v, self.snap = self.snap[0], None
        return v

    def call(self, keys):
        n = len(keys)
        if self.snap is not None and self.snap[1] is not None:
            self.snap[1] -= 1
        new = self.pol.admit(n, self._poll, self._wait)
        if new is not None:
            assert new >= 2 * (self.grows[-1] if self.grows else 0)
            self.grows.append(new)
        # admitted: even if every key were new, the map stays at or below the hard load
        assert (self.pol.bound + n) * GROW_HARD_LOAD[1] <= self.pol.cap * GROW_HARD_LOAD[0]
        assert len(self.live | set(keys)) <= self.pol.bound + n  # the bound never underestimates
        self.live |= set(keys)
        if self.pol.launched(n):
            assert self.snap is None  # at most one in flight
            self.snap = [len(self.live), self.delay]
        return new


@pytest.mark.parametrize("delay", [0, 1, 3, None])
def test_policy_never_admits_above_hard_load(delay):
    rng = random.Random(7)
    m = _Map(64, delay)
    for _ in range(300):
        n = rng.choice([1, 5, 40, 128, 700])
        m.call([rng.randrange(5000) for _ in range(n)])  # the assertions are in _Map.call
    assert m.pol.cap & (m.pol.cap - 1) == 0 and len(m.live) * 2 <= m.pol.cap
    assert m.pol.waits == m.waits
    if delay == 0:  # a snapshot that has always landed is never waited for
        assert m.waits == 0


def test_policy_steady_table_no_waits_no_growth():
    """Lookups of keys that already exist: the count stays put, snapshots land one call late,
    and the policy neither waits nor grows however long that goes on."""
    m = _Map(4096, 1)
    keys = list(range(1000))
    m.call(keys)
    cap = m.pol.cap
    for i in range(2000):
        m.call(keys[(i * 128) % 872:][:128])
    assert m.waits == 0 and m.grows == [] and m.pol.cap == cap == 4096
    assert m.pol.live_snap == 1000


def test_policy_first_call_far_above_capacity_grows_without_wait():
    m = _Map(64, None)
    new = m.call(list(range(100000)))
    assert new == 1 << 19 and m.waits == 0  # smallest power of two with 100000 at load <= 1/4
    assert m.pol.cap == new and m.pol.grows == 1


def test_policy_snapshot_decides_instead_of_growing():
    """The bound (duplicates counted) passes the hard load, but the snapshot says otherwise:
    landed -> no wait and no growth; not landed -> one wait, then no growth."""
    for delay, waits in ((0, 0), (None, 1)):
        m = _Map(1024, delay)
        keys = list(range(200))
        m.call(keys)            # bound 200
        m.call(keys)            # bound 400 > 3/8 * 1024: snapshot enqueued (true count 200)
        assert m.snap is not None and m.pol.bound * GROW_SOFT_LOAD[1] > m.pol.cap * GROW_SOFT_LOAD[0]
        m.call(keys)            # 400 + 200 > 512 on the bound; 200 + 200 with the snapshot
        assert m.grows == [] and m.waits == waits and m.pol.live_snap == 200


# ------------------------------------------------------------------------------ CPU oracle of the kernel
def test_rehash_rows_cpu_model():
    old = torch.full((16,), -1, dtype=torch.int64)
    keys = torch.tensor([5, (3 << 44) | 9, 21, 1 << 40, 37, 53, 69])
    slots = S._probe_insert_cpu(old, keys)
    assert sorted(old[slots].tolist()) == sorted(keys.tolist()) and len(set(slots.tolist())) == 7
    table = torch.randn(16, 3)
    flags = torch.randint(0, 2, (16,), dtype=torch.uint8)
    st = torch.rand(16)
    new = torch.full((32,), -1, dtype=torch.int64)
    nt, nf, ns = torch.zeros(32, 3), torch.zeros(32, dtype=torch.uint8), torch.zeros(32)
    remap = S.rehash_rows(old, new, table, nt, flags, nf, [st], [ns])
    assert torch.equal(remap < 0, old < 0)
    live = old >= 0
    assert torch.equal(new[remap[live]], old[live])
    assert torch.equal(nt[remap[live]], table[live]) and torch.equal(ns[remap[live]], st[live])
    assert torch.equal(nf[remap[live]], flags[live])
    rest = torch.ones(32, dtype=torch.bool)
    rest[remap[live]] = False
    assert not nt[rest].any() and not ns[rest].any() and not nf[rest].any() and (new[rest] == -1).all()
    with pytest.raises(ValueError):
        S.rehash_rows(old, torch.full((16,), -1, dtype=torch.int64), table, nt, flags, nf)


# ------------------------------------------------------------------------------ tables
def _table(grow, **kw):
    rows = 8 if grow else [1000, 500]
    return SparseTable("t", 8, rows, AdamUpdater(0.05), init=(-0.2, 0.2), id_mode="map", fields=2, grow=grow, **kw)


def _ids(steps=4):
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, 400, (64, 2), generator=g) * 7919 + (1 << 35) for _ in range(steps)]


def _step(t, ids):
    rows = t.lookup(ids)
    (rows.float().pow(2).sum() * 0.01).backward()
    t.push_pending()
    return rows.detach()


def test_growable_cpu_table_equals_fixed():
    a, b = _table(True), _table(False)
    assert a.stats["capacity"] == 16
    for ids in _ids():
        assert torch.equal(_step(a, ids), _step(b, ids))  # insertion-ordered slots: identical
    a.synchronize()
    assert a.stats["grows"] >= 2 and a.stats["capacity"] == a.shard.capacity >= len(a.shard.idmap)
    assert a.table.shape[0] == a.flags.shape[0] == a.states[0].shape[0] == a.shard.capacity
    assert b.stats["grows"] == 0 and b.stats["capacity"] == 1500
    n = len(a.shard.idmap)
    assert torch.equal(a.table[:n], b.table[:n]) and torch.equal(a.states[1][:n], b.states[1][:n])


def test_small_table_without_grow_still_fails():
    t = SparseTable("t", 8, 8, AdamUpdater(0.05), init=(-0.2, 0.2), id_mode="map", fields=2)
    with pytest.raises(RuntimeError, match="shard full"):
        t.lookup(_ids(1)[0])


def test_row_shard_grow_cpu_keeps_rows():
    sh = RowShard(4, 8, "map", 0, 1, (-1.0, 1.0), torch.device("cpu"), AdagradUpdater(0.1, 1e-8, rowwise=True),
                  grow=True)
    keys = torch.tensor([11, 7, (1 << 44) | 7])
    rows = sh.read(sh.slots(keys), keys).clone()
    sh.states[0][:3] = torch.tensor([1.0, 2.0, 3.0])
    assert sh.grow(32) is None and sh.capacity == 32
    assert torch.equal(sh.slots(keys, insert=False), torch.arange(3))
    assert torch.equal(sh.table[:3], rows) and sh.states[0][:4].tolist() == [1.0, 2.0, 3.0, 0.0]
    assert sh.table.shape == (32, 4) and not sh.table[3:].any() and not sh.flags[3:].any()


def test_checkpoint_of_grown_table_loads_into_small_one():
    a = _table(True)
    for ids in _ids():
        _step(a, ids)
    sd = a.state_dict()
    b = _table(True)
    assert b.stats["capacity"] == 16
    b.load_state_dict(sd)
    assert b.stats["capacity"] == a.stats["capacity"] == b.shard.capacity and b.round == a.round
    probe = torch.cat(_ids())
    assert torch.equal(b.pull(probe), a.pull(probe))
    more = _ids(6)[4:]  # the resumed table keeps training, and growing, like the original
    for ids in more:
        assert torch.equal(_step(b, ids), _step(a, ids))
    c = _table(False)  # non-growable tables load as before: shapes must match
    with pytest.raises(RuntimeError):
        c.load_state_dict(sd)


def _sparse_body(tp, rows, grow, dev):
    t = ShardedSparseTable("emb", 16, rows, tp, AdagradUpdater(0.1, 1e-8, rowwise=True), init=(-0.1, 0.1),
                           id_mode="map", seed=3, device=dev, fields=2, grow=grow)
    g = torch.Generator().manual_seed(100 + tp.rank)
    for _ in range(3):
        ids = torch.randint(0, 1500, (128, 2), generator=g)
        rows_ = t.lookup(ids.to(dev))
        (rows_.float() * torch.linspace(-1, 1, 16, device=dev)).sum().backward()
        t.push_pending()
    probe = torch.arange(1500).repeat(2, 1).t().contiguous()
    out = t.pull(probe.to(dev)).cpu()
    t.synchronize()
    return out, dict(t.stats), t.exchange, dict(t.exchange_info)


def test_growable_world2_cpu_equals_fixed():
    cpu = torch.device("cpu")
    grown = run_loopback(_sparse_body, 2, [8, 8], True, cpu)
    fixed = run_loopback(_sparse_body, 2, [3000, 2000], False, cpu)
    for r in range(2):
        assert torch.equal(grown[r][0], fixed[r][0])
        assert grown[r][1]["grows"] >= 1 and grown[r][1]["capacity"] > 74
        assert grown[r][2] == "collective" and "growable" in grown[r][3]["fallback"]
    assert torch.equal(grown[0][0], grown[1][0])


# ------------------------------------------------------------------------------ arguments
@pytest.mark.parametrize("mode", ["direct", "hash"])
def test_grow_needs_map_mode(mode):
    with pytest.raises(ValueError, match="map"):
        SparseTable("t", 4, 16, id_mode=mode, grow=True)
    with pytest.raises(ValueError, match="map"):
        ShardedSparseTable("t", 4, 16, id_mode=mode, grow=True)


def test_grow_rejects_row_plane():
    with pytest.raises(ValueError, match="plane"):
        ShardedSparseTable("t", 4, 16, id_mode="map", grow=True, exchange="plane")


def test_async_row_table_rejects_grow():
    from ps_amd.parallel.async_rows import AsyncRowTable

    with pytest.raises(ValueError, match="grow"):
        AsyncRowTable("t", 4, 16, None, grow=True)


def test_grow_keyword_on_factories_and_config():
    from ps_amd.config import Config
    from ps_amd.models.reference import local_table_factory, sharded_table_factory

    t = local_table_factory(seed=1, grow=True)("emb", 4, 8, (-0.1, 0.1), None, 2)
    assert t.growable and t.shard.growable
    t = local_table_factory(seed=1, grow=True)("wide", 1, 8, (0.0, 0.0), "hash", 1)
    assert not t.growable  # tables of another mode stay fixed-size
    t = sharded_table_factory(None, seed=1, grow=True)("emb", 4, 8, (-0.1, 0.1))
    assert t.growable
    assert not local_table_factory(seed=1)("emb", 4, 8, (-0.1, 0.1)).growable
    assert Config().grow_rows is False
    assert Config.from_args(["-Dgrow_rows=1"], base=Config()).grow_rows is True
    assert Config.from_env({"PS_AMD_GROW_ROWS": "1"}).grow_rows is True
