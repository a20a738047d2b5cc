"""Expiring rows of growable sparse tables on the CPU: the oracle of ``compact_rows`` against a
dict, the growth policy in expiring mode (pure bookkeeping, driven with scripted rounds and
snapshots), a CPU table against a Python model of "a row untouched for more than N rounds is a new
row", the argument errors, the factories / Config, and the checkpoint with and without stamps.
"""
import random

import pytest
import torch

from ps_amd.ops import sparse as S
from ps_amd.parallel.sparse_table import (GROW_HARD_LOAD, GrowthPolicy, RowShard, ShardedSparseTable, SparseTable,
                                          TcpSparseTable)
from ps_amd.parallel.updaters import AdagradUpdater


# ------------------------------------------------------------------------------ oracle of the kernel
def _old_map(cap, dim, keys, stamps, seed):
    g = torch.Generator().manual_seed(seed)
    hk = torch.full((cap,), -1, dtype=torch.int64)
    slots = S._probe_insert_cpu(hk, keys)
    table = torch.randn(cap, dim, generator=g)  # every position holds data, live or not
    flags = torch.randint(0, 2, (cap,), generator=g).to(torch.uint8)
    st = [torch.rand(cap, generator=g) + 0.5, torch.rand(cap, dim, generator=g) + 0.5]
    stamp = torch.randint(-50, 50, (cap,), generator=g).to(torch.int32)
    stamp[slots] = stamps.to(torch.int32)
    return hk, table, flags, st, stamp, slots


def _new_map(cap, dim):
    return (torch.full((cap,), -1, dtype=torch.int64), torch.zeros(cap, dim), torch.zeros(cap, dtype=torch.uint8),
            [torch.zeros(cap), torch.zeros(cap, dim)], torch.zeros(cap, dtype=torch.int32))


@pytest.mark.parametrize("dim", [1, 8])
@pytest.mark.parametrize("caps", [(64, 64), (256, 64), (64, 128)])
def test_compact_rows_ref_matches_dict_model(caps, dim):
    old_cap, new_cap = caps
    cutoff = 7
    g = torch.Generator().manual_seed(old_cap + dim)
    keys = ((torch.arange(30) % 3) << 44) | (torch.randperm(1 << 16, generator=g)[:30] * 7919 + (1 << 33))
    stamps = torch.randint(cutoff - 2, cutoff + 3, (30,), generator=g)
    stamps[:4] = torch.tensor([cutoff, cutoff - 1, cutoff, cutoff - 1])  # both sides of the boundary
    hk, table, flags, st, stamp, slots = _old_map(old_cap, dim, keys, stamps, seed=dim)
    model = {int(k): (table[s].clone(), int(flags[s]), float(st[0][s]), st[1][s].clone(), int(t))
             for k, s, t in zip(keys.tolist(), slots.tolist(), stamps.tolist()) if t >= cutoff}
    nk, nt, nf, ns, nstamp = _new_map(new_cap, dim)
    counters = torch.tensor([5, 11])  # added to, not overwritten
    status = torch.zeros(1, dtype=torch.int32)
    remap = S.compact_rows(hk, nk, table, nt, flags, nf, stamp, nstamp, cutoff, counters, status, st, ns)
    assert int(status) == 0 and counters.tolist() == [5 + len(model), 11 + 30 - len(model)]
    assert 0 < len(model) < 30 and 2 * len(model) <= new_cap
    gone = torch.ones(old_cap, dtype=torch.bool)
    for k, s in zip(keys.tolist(), slots.tolist()):
        q = int(remap[s])
        if k not in model:
            assert q == -1 and k not in nk.tolist()
            continue
        gone[s] = False
        row, flag, h, full, t = model[k]
        assert int(nk[q]) == k and torch.equal(nt[q], row) and int(nf[q]) == flag and float(ns[0][q]) == h
        assert torch.equal(ns[1][q], full) and int(nstamp[q]) == t
    assert (remap[gone] == -1).all() and (remap[~gone] >= 0).all()
    rest = torch.ones(new_cap, dtype=torch.bool)
    rest[remap[~gone]] = False
    assert int((~rest).sum()) == len(model)  # distinct new slots
    assert (nk[rest] == -1).all() and not nt[rest].any() and not nf[rest].any() and not nstamp[rest].any()
    assert not ns[0][rest].any() and not ns[1][rest].any()


def test_compact_rows_ref_overfull_target():
    """100 fresh keys into 64 slots: exactly 64 are placed, the rest get remap -1, status is set."""
    keys = torch.arange(100) * 104729 + 5
    hk, table, flags, st, stamp, slots = _old_map(256, 2, keys, torch.full((100,), 9), seed=3)
    nk, nt, nf, ns, nstamp = _new_map(64, 2)
    counters = torch.zeros(2, dtype=torch.int64)
    status = torch.zeros(1, dtype=torch.int32)
    remap = S.compact_rows(hk, nk, table, nt, flags, nf, stamp, nstamp, 9, counters, status, st, ns)
    placed = remap[slots] >= 0
    assert int(placed.sum()) == 64 and int((remap >= 0).sum()) == 64 and int(status) == 1
    assert counters.tolist() == [64, 0] and (nk >= 0).all()
    assert torch.equal(nk[remap[slots[placed]]], keys[placed])
    assert torch.equal(nt[remap[slots[placed]]], table[slots[placed]])


@pytest.mark.parametrize("cap", [32, 96, 0])
def test_compact_rows_rejects_bad_capacity(cap):
    hk, table, flags, st, stamp, _ = _old_map(64, 2, torch.arange(5), torch.zeros(5), seed=1)
    nk, nt, nf, ns, nstamp = _new_map(cap, 2)
    with pytest.raises(ValueError, match="power-of-two"):
        S.compact_rows(hk, nk, table, nt, flags, nf, stamp, nstamp, 0, torch.zeros(2, dtype=torch.int64),
                       torch.zeros(1, dtype=torch.int32), st, ns)


# ------------------------------------------------------------------------------ policy
class _ExpMap:
    """The policy's owner minus the device: key -> stamp, compaction when the policy says so, and
    (live, fresh) snapshots that land ``delay`` calls after the next one (None: only when waited
    for).  One call per round."""

    def __init__(self, cap, n_exp, delay):
        self.pol = GrowthPolicy(cap, expiring=True)
        self.n_exp, self.delay = n_exp, delay
        self.stamp = {}
        self.snap = None
        self.round = 0
        self.waits = 0
        self.decisions = []  # (round, old cap, new cap, survivors)

    def _poll(self):
        assert self.pol.in_flight and self.snap is not None
        if self.snap[1] is not None and self.snap[1] < 0:
            v, self.snap = self.snap[0], None
            return v
        return None

    def _wait(self):
        assert self.pol.in_flight and self.snap is not None
        assert self.snap[1] is None or self.snap[1] >= 0
        self.waits += 1
        v, self.snap = self.snap[0], None
        return v

    def call(self, keys):
        n, cutoff = len(keys), self.round - self.n_exp
        if self.snap is not None and self.snap[1] is not None:
            self.snap[1] -= 1
        old = self.pol.cap
        new = self.pol.admit(n, self._poll, self._wait)
        if new is not None:
            assert new >= 64 and new & (new - 1) == 0
            self.stamp = {k: t for k, t in self.stamp.items() if t >= cutoff}
            self.snap = None  # the owner forgets the snapshot of the old map
            assert not self.pol.in_flight
            assert 2 * len(self.stamp) <= new  # the survivors fill at most half of the target
            self.decisions.append((self.round, old, new, len(self.stamp)))
        # after the decision: never above the hard load, and the bound holds for the live keys
        assert (self.pol.bound + n) * GROW_HARD_LOAD[1] <= self.pol.cap * GROW_HARD_LOAD[0]
        assert len(set(self.stamp) | set(keys)) <= self.pol.bound + n
        for k in keys:
            self.stamp[k] = self.round
        if self.pol.launched(n):
            assert self.snap is None
            self.snap = [(len(self.stamp), sum(t >= cutoff for t in self.stamp.values())), self.delay]
        assert new is None or self.pol.in_flight  # a compaction asks for a new snapshot at once
        self.round += 1
        return new


@pytest.mark.parametrize("delay", [0, 1, 3, None])
def test_expiring_policy_never_above_hard_load(delay):
    rng = random.Random(11)
    m = _ExpMap(64, 2, delay)
    fresh = iter(range(10 ** 6, 10 ** 7))
    for _ in range(300):
        n = rng.choice([1, 5, 40, 128, 700])
        m.call([rng.randrange(3000) if rng.random() < 0.5 else next(fresh) for _ in range(n)])
    assert m.pol.compactions == len(m.decisions) > 3 and m.pol.waits == m.waits
    assert any(new < old for _, old, new, _ in m.decisions)  # it shrinks, too
    if delay == 0:
        assert m.waits == 0


def test_expiring_policy_same_size_when_fresh_bound_fits():
    """32 new ids a round, N = 2, snapshots landed by the next call: the map holds the last three
    rounds after each compaction, so 4 * (96 + 32) = 512 slots do, again and again."""
    m = _ExpMap(64, 2, 0)
    for r in range(200):
        m.call(list(range(32 * r, 32 * r + 32)))
    caps = [new for _, _, new, _ in m.decisions]
    assert m.waits == 0 and len(caps) > 20 and caps[:2] == [256, 512] and set(caps[2:]) == {512}
    assert all(old == new for _, old, new, _ in m.decisions[2:])
    assert len(m.stamp) <= 256 and m.pol.grows == 2


def test_expiring_policy_grows_when_fresh_bound_does_not_fit():
    m = _ExpMap(64, 2, 0)
    new = m.call(list(range(1000)))
    assert new == 4096 and m.pol.grows == 1 and m.pol.compactions == 1
    for r in range(1, 4):  # the same keys every round: all fresh, nothing to evict, no room to give back
        m.call(list(range(1000)))
    assert m.pol.cap == 4096 and len(m.stamp) == 1000
    new = m.call(list(range(5000, 9000)))  # 1000 fresh + 4000 new do not fit 4096 at load 1/2
    assert new == 32768 and m.decisions[-1][3] == 1000


def test_plain_policy_is_untouched():
    p = GrowthPolicy(64)
    assert p.admit(40) == 256 and (p.live_snap, p.since, p.grows, p.compactions) == (0, 0, 1, 0)
    assert p.launched(40) is False and p.since == 40 and not p.expiring


# ------------------------------------------------------------------------------ table against a model
N_EXP, DIM, SEED, LR, EPS = 2, 8, 3, 0.1, 1e-8
INIT = (-0.2, 0.2)


def _table(dev=None, **kw):
    return SparseTable("t", DIM, 8, AdagradUpdater(LR, EPS, rowwise=True), init=INIT, id_mode="map", seed=SEED,
                       device=dev, grow=True, expire_after=N_EXP, **kw)


def _stream(rounds=14):
    """Per round: 4 ids in every round, 6 that return after 2 rounds (inside the window), 5 that
    return after 3 and 5 rounds (expired), 20 that never return, and duplicates."""
    out = []
    for r in range(rounds):
        ids = [1, 2, 3, 4, 2]
        if r % 2 == 0:
            ids += list(range(100, 106))
        if r % 3 == 0:
            ids += list(range(200, 205)) + [200]
        if r % 5 == 0:
            ids += list(range(300, 305))
        ids += [1000 + 20 * r + i for i in range(20)]
        out.append(torch.tensor(ids) * 7919 + (1 << 35))
    return out


def _step(t, ids):
    rows = t.lookup(ids)
    (rows.float().pow(2).sum() * 0.01).backward()
    t.push_pending()
    return rows.detach()


class _Model:
    """key -> [row, row-wise Adagrad state, round of the last lookup]; a row whose gap exceeds N is
    reset to the deterministic init of its key and zero state."""

    def __init__(self):
        self.rows = {}
        self.round = 0
        self.reborn = 0

    def step(self, ids):
        out = []
        uniq, cnt = torch.unique(ids, return_counts=True)
        for k in uniq.tolist():
            e = self.rows.get(k)
            if e is None or self.round - e[2] > N_EXP:
                self.reborn += e is not None
                e = self.rows[k] = [S.init_values(SEED, torch.tensor([k]), DIM, *INIT)[0], 0.0, self.round]
            e[2] = self.round
        for k in ids.tolist():
            out.append(self.rows[k][0].clone())
        for k, c in zip(uniq.tolist(), cnt.tolist()):
            e = self.rows[k]
            g = 0.02 * c * e[0]
            e[1] = e[1] + float((g * g).mean())
            e[0] = e[0] - LR * g / (torch.sqrt(torch.tensor(e[1])) + EPS)
        self.round += 1
        return torch.stack(out)


def test_cpu_table_matches_expiry_model():
    t, m = _table(), _Model()
    fresh = S.init_values(SEED, _stream(1)[0][5:11], DIM, *INIT)
    for r, ids in enumerate(_stream()):
        got, want = _step(t, ids), m.step(ids)
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
        if r in (6, 10):  # ids 200..204: seen at rounds 0, 3, 6 -- expired each time, a new row again
            assert torch.equal(got[11:16], S.init_values(SEED, ids[11:16], DIM, *INIT))
            assert torch.equal(got[11:16], SparseTable("t", DIM, 8, init=INIT, id_mode="map", seed=SEED).pull(ids[11:16]))
        if r == 2:  # ids 100..105 return inside the window: trained rows, not the init
            assert not torch.equal(got[5:11], fresh)
    assert m.reborn > 10 and t.stats["compactions"] >= 2
    st = t.row_stats()
    assert st["evicted"] + len(t.shard.idmap) + m.reborn >= len(m.rows)
    # state of every live row of the model, through the shard's own map
    keys = torch.tensor([k for k, e in m.rows.items() if m.round - 1 - e[2] <= N_EXP])
    slots = t.shard.slots(keys, insert=False)
    assert (slots >= 0).all()
    torch.testing.assert_close(t.states[0][slots], torch.tensor([m.rows[int(k)][1] for k in keys]), rtol=1e-5,
                               atol=1e-6)
    torch.testing.assert_close(t.table[slots], torch.stack([m.rows[int(k)][0] for k in keys]), rtol=1e-5, atol=1e-6)


def test_cpu_evict_shrinks_and_keeps_the_fresh_rows():
    t = _table()
    for ids in _stream(6):
        _step(t, ids)
    before = t.pull(_stream(6)[5])  # round 6 lookups: these rows are fresh
    n = t.evict()
    assert n == int((t.shard.stamp[:len(t.shard.idmap)] >= t.round - N_EXP).sum()) == len(t.shard.idmap)
    assert t.stats["capacity"] == t.shard.capacity == max(64, 1 << (4 * n - 1).bit_length()) == 256
    assert torch.equal(t.pull(_stream(6)[5]), before)
    for _ in range(3):  # three rounds on four ids: everything else expires, the table shrinks
        _step(t, torch.tensor([1, 2, 3, 4]) * 7919 + (1 << 35))
    done = t.stats["compactions"]
    assert t.evict() == 4 and t.stats["capacity"] == 64 and t.stats["compactions"] == done + 1
    assert t.row_stats()["evicted"] >= n - 4
    with pytest.raises(ValueError, match="max_age"):
        t.evict(0)
    with pytest.raises(ValueError, match="expire_after"):
        SparseTable("t", 4, 8, id_mode="map", grow=True).evict()


def test_row_shard_compact_cpu_returns_remap():
    sh = RowShard(4, 8, "map", 0, 1, (-1.0, 1.0), torch.device("cpu"), AdagradUpdater(0.1, 1e-8, rowwise=True),
                  grow=True, expire_after=1)
    keys = torch.tensor([11, 7, (1 << 44) | 7, 5])
    rows = sh.read(sh.slots(keys, now=0), keys).clone()
    sh.slots(keys[[1, 3]], now=1)
    sh.states[0][:4] = torch.tensor([1.0, 2.0, 3.0, 4.0])
    remap = sh.compact(64, 1)
    assert remap[:4].tolist() == [-1, 0, -1, 1] and (remap[4:] == -1).all() and sh.capacity == 64
    assert sh.slots(keys, insert=False).tolist() == [-1, 0, -1, 1]
    assert torch.equal(sh.table[:2], rows[[1, 3]]) and sh.states[0][:3].tolist() == [2.0, 4.0, 0.0]
    assert sh.stamp[:3].tolist() == [1, 1, 0] and sh.counters.tolist() == [2, 2] and not sh.table[2:].any()


# ------------------------------------------------------------------------------ arguments
def test_expire_after_needs_grow_and_a_positive_age():
    for cls in (SparseTable, ShardedSparseTable):
        with pytest.raises(ValueError, match="grow"):
            cls("t", 4, 16, id_mode="map", expire_after=2)
        with pytest.raises(ValueError, match=">= 1"):
            cls("t", 4, 16, id_mode="map", grow=True, expire_after=0)
        with pytest.raises(ValueError, match="map"):
            cls("t", 4, 16, id_mode="hash", grow=True, expire_after=2)
    with pytest.raises(ValueError, match="grow"):
        RowShard(4, 8, "map", 0, 1, (0.0, 0.0), torch.device("cpu"), None, expire_after=2)


def test_expire_after_rejects_row_plane():
    with pytest.raises(ValueError, match="plane"):
        ShardedSparseTable("t", 4, 16, id_mode="map", grow=True, expire_after=2, exchange="plane")


def test_async_and_tcp_tables_treat_expire_after_like_grow():
    from ps_amd.parallel.async_rows import AsyncRowTable

    with pytest.raises(ValueError, match="expire_after"):
        AsyncRowTable("t", 4, 16, None, expire_after=2)
    for kw in ({"grow": True}, {"expire_after": 2}):  # the TCP table has neither argument
        with pytest.raises(TypeError):
            TcpSparseTable("t", 4, 16, None, **kw)


def test_expire_keyword_on_factories_and_config(monkeypatch):
    from ps_amd.apps import common
    from ps_amd.config import Config
    from ps_amd.models.reference import local_table_factory, sharded_table_factory

    t = local_table_factory(seed=1, grow=True, expire_after=3)("emb", 4, 8, (-0.1, 0.1), None, 2)
    assert t.expire_after == 3 and t.shard.expire_after == 3 and t.shard.stamp.dtype == torch.int32
    t = local_table_factory(seed=1, grow=True, expire_after=3)("wide", 1, 8, (0.0, 0.0), "hash", 1)
    assert not t.expire_after and t.shard.stamp is None  # tables of another mode stay as they are
    t = sharded_table_factory(None, seed=1, grow=True, expire_after=3)("emb", 4, 8, (-0.1, 0.1))
    assert t.expire_after == 3
    t = local_table_factory(seed=1, grow=True)("emb", 4, 8, (-0.1, 0.1))
    assert not t.expire_after and t.shard.stamp is None and "compactions" not in t.stats
    for f in (local_table_factory, lambda **kw: sharded_table_factory(None, **kw)):
        with pytest.raises(ValueError, match="grow"):
            f(expire_after=3)
    assert Config().expire_rows == 0
    assert Config.from_args(["-Dexpire_rows=3"], base=Config()).expire_rows == 3
    assert Config.from_env({"PS_AMD_EXPIRE_ROWS": "4"}).expire_rows == 4
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cfg = Config.from_args(["-Dexpire_rows=3", "-Dgrow_rows=1"], base=Config())
    _, make = common.connect(cfg)
    assert make("emb", 4, 8, (-0.1, 0.1)).expire_after == 3
    with pytest.raises(ValueError, match="grow_rows"):
        common.connect(Config.from_args(["-Dexpire_rows=3"], base=Config()))


# ------------------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip_with_stamps():
    a = _table()
    for ids in _stream(5):
        _step(a, ids)
    sd = a.state_dict()
    assert sd["stamp"].dtype == torch.int32 and sd["stamp"].shape[0] == a.shard.capacity
    b = _table()
    b.load_state_dict(sd)
    assert b.round == a.round and torch.equal(b.shard.stamp, a.shard.stamp) and b.stats["capacity"] == a.shard.capacity
    for ids in _stream(10)[5:]:  # both go on expiring, compacting and training alike
        assert torch.equal(_step(b, ids), _step(a, ids))
    assert b.stats["compactions"] >= 1


def test_checkpoint_without_stamps_and_into_plain_table():
    plain = SparseTable("t", DIM, 8, AdagradUpdater(LR, EPS, rowwise=True), init=INIT, id_mode="map", seed=SEED,
                        grow=True)
    for ids in _stream(5):
        _step(plain, ids)
    sd = plain.state_dict()
    assert "stamp" not in sd
    b = _table()
    b.load_state_dict(sd)  # every row counts as touched at the loaded round
    n = len(b.shard.idmap)
    assert n == len(plain.shard.idmap) and (b.shard.stamp[:n] == plain.round).all()
    probe = _stream(1)[0]  # last seen at round 0: expired by round 5, but touched at the load
    assert torch.equal(b.pull(probe), plain.pull(probe))
    d = SparseTable("t", DIM, 8, AdagradUpdater(LR, EPS, rowwise=True), init=INIT, id_mode="map", seed=SEED, grow=True)
    a = _table()
    for ids in _stream(3):
        _step(a, ids)
    d.load_state_dict(a.state_dict())  # a table without expiry ignores the saved stamps
    probe = _stream(3)[2]  # (rows inside the window: the expiring table does not reset them)
    assert d.shard.stamp is None and torch.equal(d.pull(probe), a.pull(probe))
