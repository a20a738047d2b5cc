"""Expiring rows of growable sparse tables on cuda:0.

* compact_rows (HIP) vs the composition oracle (mask the expired keys, hash_slots insert, masked
  index copies): moved rows are copies, so every comparison is bit-exact.  Probe positions depend
  on the insertion order, which neither side fixes, so rows are compared per key and the map through
  its own lookups (as the rehash_rows tests do).
* The stamping lookup against hash_slots on a twin map.
* SparseTable(rows=8, grow=True, expire_after=2) against the CPU table of the same arguments on a
  scripted stream: with the push on the side stream, with a plan pending across a compaction, with
  micro-batches queued.
* Bounded memory on a stream of ids that never return, evict(), W = 2 thread-ranks, bags.
"""
import pytest
import torch

from ps_amd.ops import sparse as S
from ps_amd.parallel.transport import run_loopback

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CUT = 7


# ------------------------------------------------------------------------------ compact_rows
def _keys(n, seed=0):
    g = torch.Generator().manual_seed(n + seed)
    ids = torch.randperm(1 << 20, generator=g)[:n] * 1048573 + (1 << 39)  # distinct, below 2^44
    return ((torch.arange(n) % 4) << 44) | ids  # keys carrying field bits


def _fresh(cap, dim, states):
    hk = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    table = torch.zeros(cap, dim, device=DEV)
    flags = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    st = {"none": [], "rowwise": [torch.zeros(cap, device=DEV)],
          "full2": [torch.zeros(cap, dim, device=DEV) for _ in range(2)]}[states]
    stamp = torch.zeros(cap, dtype=torch.int32, device=DEV)
    return hk, table, flags, st, stamp


def _stamps(filt, n, g):
    if filt == "none":
        return torch.randint(CUT, CUT + 3, (n,), generator=g)
    if filt == "all":
        return torch.randint(CUT - 3, CUT, (n,), generator=g)
    s = torch.randint(CUT - 2, CUT + 3, (n,), generator=g)
    s[:4] = torch.tensor([CUT, CUT - 1, CUT, CUT - 1])[:n]  # both sides of the boundary, always
    return s


def _check_compact(old_cap, new_cap, dim, states, filt, nkeys, keep_every=0):
    g = torch.Generator().manual_seed(old_cap + 3 * dim + new_cap)
    keys = _keys(nkeys, seed=dim)
    hk, table, flags, st, stamp = _fresh(old_cap, dim, states)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    old_slots = S.hash_slots(hk, keys.to(DEV), True, status)
    # every old position holds data, live or not: only the survivors may arrive
    table.copy_(torch.randn(old_cap, dim, generator=g))
    flags.copy_(torch.randint(0, 2, (old_cap,), generator=g).to(torch.uint8))
    for s in st:
        s.copy_(torch.rand(s.shape, generator=g) + 0.5)
    stamp.copy_(torch.randint(-9, 99, (old_cap,), generator=g).to(torch.int32))
    if keep_every:
        kst = torch.where(torch.arange(nkeys) % keep_every == 0, CUT, CUT - 1)
    else:
        kst = _stamps(filt, nkeys, g)
    stamp[old_slots] = kst.to(DEV, torch.int32)
    keep_k = kst >= CUT
    n_keep = int(keep_k.sum())
    assert 2 * n_keep <= new_cap  # (on the CPU) the survivors fill at most half of the target
    live = hk >= 0
    keep = live & (stamp >= CUT)
    assert int(live.sum()) == nkeys and int(keep.sum()) == n_keep

    runs = []
    for fn in (S.compact_rows, S.compact_rows, S.compact_rows_ref):
        new = _fresh(new_cap, dim, states)
        counters = torch.tensor([3, 4], device=DEV)
        remap = fn(hk, new[0], table, new[1], flags, new[2], stamp, new[4], CUT, counters, status, st, new[3])
        assert (counters - torch.tensor([3, 4], device=DEV)).tolist() == [n_keep, nkeys - n_keep]
        assert torch.equal(remap < 0, ~keep)  # -1 exactly at the empty and the evicted positions
        runs.append((new, remap))
    assert int(status.item()) == 0
    (new, remap), (new2, remap2), (ref, rref) = runs
    q, q2, qr = remap[keep], remap2[keep], rref[keep]
    if n_keep:
        assert q.unique().numel() == n_keep and int(q.min()) >= 0 and int(q.max()) < new_cap
    assert torch.equal(new[0][q], hk[keep]) and torch.equal(ref[0][qr], hk[keep])
    assert torch.equal(torch.sort(new[0]).values, torch.sort(ref[0]).values)  # same keys in both maps
    found = S.hash_slots(new[0], keys.to(DEV), False, status)  # survivors where the rows went, evicted keys absent
    want = torch.where(keep_k.to(DEV), remap[old_slots], torch.full_like(old_slots, -1))
    assert torch.equal(found, want)
    rest = torch.ones(new_cap, dtype=torch.bool, device=DEV)
    rest[q] = False
    assert (new[0][rest] == -1).all()
    pay = lambda m: [m[1], m[2], m[4]] + list(m[3])  # noqa: E731
    for got, got2, want, old in zip(pay(new), pay(new2), pay(ref), [table, flags, stamp] + st):
        assert torch.equal(got[q], old[keep]) and torch.equal(got[q], want[qr])  # bit for bit
        assert torch.equal(got2[q2], got[q])  # two runs give equal results
        assert not got[rest].any()  # every other destination row is zero


@pytest.mark.parametrize("filt", ["none", "all", "random"])
@pytest.mark.parametrize("states", ["none", "rowwise", "full2"])
@pytest.mark.parametrize("dim", [1, 6, 8, 64, 80, 128])
def test_compact_rows_matches_oracle(dim, states, filt):
    for old_cap, new_cap in ((64, 64), (128, 64), (64, 128), (1024, 64)):
        _check_compact(old_cap, new_cap, dim, states, filt, 30)


@pytest.mark.parametrize("states", ["none", "rowwise", "full2"])
def test_compact_rows_grid_stride_wraps(states):
    """32768 -> 16384 positions at dim 8 with a quarter of 16000 keys surviving: more lane groups
    than the launch has, so every group walks several positions."""
    _check_compact(32768, 16384, 8, states, None, 16000, keep_every=4)


def test_compact_rows_rejects_bad_target():
    old, new = _fresh(64, 4, "none"), _fresh(32, 4, "none")
    cnt, status = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        S.compact_rows(old[0], new[0], old[1], new[1], old[2], new[2], old[4], new[4], 0, cnt, status)
    with pytest.raises(RuntimeError):  # the binding checks on its own
        S.native().compact_rows(old[0], new[0], old[1], new[1], old[2], new[2], old[4], new[4], 0, cnt, status, [], [],
                                torch.empty_like(old[0]))


# ------------------------------------------------------------------------------ stamping lookup
def test_hash_slots_stamp_equals_hash_slots_and_stamps():
    cap = 256
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    b = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    first = _keys(40).to(DEV)
    stamp = torch.full((cap,), 5, dtype=torch.int32, device=DEV)

    def twin_agrees(ids, got):
        # which of two colliding new keys gets the nearer position is decided by a race, so the
        # twin is the map after the launch: plain hash_slots must resolve every id to the same slot
        twin = b.clone()
        assert torch.equal(S.hash_slots(twin, ids, True, status), got) and torch.equal(twin, b)
        assert torch.equal(got < 0, ids < 0) and torch.equal(b[got[ids >= 0]], ids[ids >= 0])

    twin_agrees(first, S.hash_slots_stamp(b, first, stamp, 6, status))
    assert int((stamp == 6).sum()) == 40 and int((stamp == 5).sum()) == cap - 40
    # known keys, new keys, duplicates of both kinds and pad keys in one launch
    ids = torch.cat([first[:10], _keys(30, seed=9).to(DEV), first[:10], torch.full((7,), -1, device=DEV)])
    ids = torch.cat([ids, ids[10:25]])[torch.randperm(72, generator=torch.Generator().manual_seed(1)).to(DEV)]
    before = stamp.clone()
    got = S.hash_slots_stamp(b, ids, stamp, 9, status)
    twin_agrees(ids, got)
    assert int(status.item()) == 0 and int((b >= 0).sum()) == 70
    hit = torch.zeros(cap, dtype=torch.bool, device=DEV)
    hit[got[got >= 0]] = True
    assert int(hit.sum()) == 40 and (stamp[hit] == 9).all() and torch.equal(stamp[~hit], before[~hit])
    assert int((stamp == 6).sum()) == 30  # the keys of the first launch this one did not ask for


@pytest.mark.parametrize("states", ["rowwise", "full2"])
@pytest.mark.parametrize("dim", [1, 6, 128])
def test_hash_slots_stamp_resets_expired_rows(dim, states):
    """A key found with stamp < cutoff gets the state of a slot never used; stamp == cutoff stays."""
    cap = 128
    hk, table, flags, st, stamp = _fresh(cap, dim, states)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    keys = _keys(40).to(DEV)
    slots = S.hash_slots(hk, keys, True, status)
    g = torch.Generator().manual_seed(dim)
    table.copy_(torch.randn(cap, dim, generator=g))
    flags.fill_(1)
    for s in st:
        s.copy_(torch.rand(s.shape, generator=g) + 0.5)
    kst = torch.randint(CUT - 2, CUT + 2, (40,), generator=g)
    kst[:2] = torch.tensor([CUT, CUT - 1])
    stamp[slots] = kst.to(DEV, torch.int32)
    want = [t.clone() for t in [table, flags] + st]
    ask = torch.cat([keys[:20], keys[:5], _keys(8, seed=4).to(DEV), torch.full((3,), -1, device=DEV)])
    old = (kst[:20] < CUT).to(DEV)
    for t in want:
        t[slots[:20][old]] = 0
    got = S.hash_slots_stamp(hk, ask, stamp, CUT + 2, status, cutoff=CUT, table=table, flags=flags, states=st)
    assert torch.equal(got[:20], slots[:20]) and torch.equal(got[20:25], slots[:5]) and int(status.item()) == 0
    assert 0 < int(old.sum()) < 20
    for t, w in zip([table, flags] + st, want):
        assert torch.equal(t, w)
    assert (stamp[got[:33]] == CUT + 2).all() and torch.equal(stamp[slots[20:]].cpu(), kst[20:].to(torch.int32))


# ------------------------------------------------------------------------------ W = 1 table
from .test_table_expiry_cpu import DIM, INIT, N_EXP, SEED, _stream, _table  # noqa: E402 -- the scripted stream


def _step(t, ids):
    rows = t.lookup(ids.to(t.device))
    (rows.float().pow(2).sum() * 0.01).backward()
    t.push_pending()
    return rows.detach().cpu()


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def _new_ids(i, n=400):
    return (torch.arange(n) + n * i + 10 ** 6) * 7919 + (1 << 35)


def _compacted_ok(t, at_least=2):
    t.synchronize()  # raises if the map ever overflowed
    assert t.stats["compactions"] >= at_least and t.stats["capacity"] == t.shard.capacity == t.shard.hkeys.numel()
    assert t.table.shape[0] == t.flags.shape[0] == t.shard.stamp.shape[0] == t.shard.capacity
    assert int(t.shard.status.item()) == 0


def _same_live_rows(a, b):
    """The GPU table's unexpired rows == the CPU table's, optimizer state included."""
    sh = a.shard
    keys = sh.hkeys[(sh.hkeys >= 0) & (sh.stamp >= a.round - N_EXP)].cpu()
    sa, sb = sh.slots(keys.to(DEV), insert=False).cpu(), b.shard.slots(keys, insert=False)
    assert keys.numel() and (sb >= 0).all() and a.round == b.round
    _close(a.table.cpu()[sa], b.table[sb])
    _close(a.states[0].cpu()[sa], b.states[0][sb])


@pytest.mark.parametrize("overlap", [False, True])
def test_expiring_gpu_table_equals_cpu_table(overlap):
    a, b = _table(DEV, overlap=overlap), _table()
    for r, ids in enumerate(_stream()):
        got = _step(a, ids)
        _close(got, _step(b, ids))
        if r in (6, 9):  # ids 200..204 come back expired: the init of a fresh table, bit for bit
            assert torch.equal(got[11:16], S.init_values(SEED, ids[11:16], DIM, *INIT))
    _compacted_ok(a)
    _same_live_rows(a, b)


def test_compaction_while_a_plan_is_pending():
    """Two lookups before one backward: the second one compacts the shard while the first one's
    plan still holds owner-local slots, which must follow the rows."""
    a, b = _table(DEV), _table()
    hit = 0
    for i, small in enumerate(_stream(8)):
        big = torch.cat([small[:9], _new_ids(i)])
        outs = []
        for t in (a, b):
            r1 = t.lookup(small.to(t.device))
            c0 = t.stats["compactions"]
            r2 = t.lookup(big.to(t.device))
            hit += t is a and t.stats["compactions"] > c0
            (r1.float().pow(2).sum() * 0.01 + r2.float().pow(2).sum() * 0.02).backward()
            t.push_pending()
            outs.append((r1.detach().cpu(), r2.detach().cpu()))
        _close(outs[0][0], outs[1][0])
        _close(outs[0][1], outs[1][1])
    assert hit >= 2
    _compacted_ok(a)
    _same_live_rows(a, b)


def test_compaction_while_micro_batches_are_queued():
    """accumulating=True over two micro-batches: the second lookup compacts the shard while the
    first micro-batch's (slot, gradient) pairs wait for the round's single update."""
    a, b = _table(DEV), _table()
    hit = 0
    for i, small in enumerate(_stream(8)):
        outs = []
        for t in (a, b):
            t.accumulating = True
            r1 = t.lookup(small.to(t.device))
            (r1.float().pow(2).sum() * 0.01).backward()
            t.push_pending()
            assert len(t._acc) == 1
            c0 = t.stats["compactions"]
            r2 = t.lookup(_new_ids(i).to(t.device))
            hit += t is a and t.stats["compactions"] > c0
            (r2.float().pow(2).sum() * 0.01).backward()
            t.accumulating = False
            t.push_pending()
            assert not t._acc
            outs.append((r1.detach().cpu(), r2.detach().cpu()))
        _close(outs[0][0], outs[1][0])
        _close(outs[0][1], outs[1][1])
    assert hit >= 2
    _compacted_ok(a)
    _same_live_rows(a, b)


def test_bounded_memory_on_a_stream_of_new_ids():
    """200 rounds of 32 ids that never return, N = 2, each step's device work done before the next
    (the synchronize stands in for the model's compute, as in test_growth_takes_no_host_sync).

    Capacity bound.  A snapshot counts as fresh the rows of at most three rounds (the stamps r - 2,
    r - 1, r of the round r that enqueued it): 96.  It is enqueued right after a compaction or
    above the soft load, and has landed by the next call, so at a decision ``since`` is 0 and
    fresh_bound + n = 96 + 32: the policy asks for pow2(4 * 128) = 512 slots, every time, once
    three rounds have passed."""
    from ps_amd.parallel.sparse_table import SparseTable
    from ps_amd.parallel.updaters import AdagradUpdater

    def make(**kw):
        return SparseTable("t", 8, 8, AdagradUpdater(0.1, 1e-8, rowwise=True), init=(-0.2, 0.2), id_mode="map", seed=3,
                           device=DEV, grow=True, **kw)

    a, plain = make(expire_after=2), make()
    caps, comps = [], []
    for r in range(200):
        ids = (torch.arange(32) + 32 * r) * 7919 + (1 << 35)
        _step(a, ids)
        _step(plain, ids)
        torch.cuda.synchronize()
        caps.append(a.stats["capacity"])
        comps.append(a.stats["compactions"])
    assert a.stats["host_syncs"] == 0
    assert comps[49] < comps[99] < comps[149] < comps[199]  # keeps rising
    assert caps[199] == caps[99] and max(caps) <= 512
    assert 4 * caps[199] <= plain.stats["capacity"]
    live = int((a.shard.hkeys >= 0).sum())
    assert a.row_stats()["evicted"] + live == 6400 and 2 * live <= caps[199]
    assert a.stats["grows"] == 2  # 64 -> 256 -> 512: "grows" counts the capacity increases only
    _compacted_ok(a)


def test_evict_shrinks_to_64_slots_with_one_host_sync():
    a = _table(DEV)
    for ids in _stream(3) + [_new_ids(0, 200)]:
        _step(a, ids)
    a.round += N_EXP + 1  # rounds pass without a lookup: every row expires
    torch.cuda.synchronize()
    syncs, comps, live = a.stats["host_syncs"], a.stats["compactions"], int((a.shard.hkeys >= 0).sum())
    assert a.stats["capacity"] > 64 and live > 64
    assert a.evict() == 0
    assert a.stats["capacity"] == a.shard.hkeys.numel() == 64 and not (a.shard.hkeys >= 0).any()
    assert a.stats["host_syncs"] == syncs + 1 and a.stats["compactions"] == comps + 1
    assert a.row_stats()["evicted"] >= live and a.shard._pol.bound == 0
    ids = _stream(1)[0]
    assert torch.equal(a.pull(ids.to(DEV)).cpu(), _table().pull(ids))  # every key is a new row again
    _compacted_ok(a, at_least=1)


# ------------------------------------------------------------------------------ W = 2
def _sparse_body(tp, dev):
    from ps_amd.parallel.sparse_table import ShardedSparseTable
    from ps_amd.parallel.updaters import AdagradUpdater

    t = ShardedSparseTable("t", DIM, 8, tp, AdagradUpdater(0.1, 1e-8, rowwise=True), init=INIT, id_mode="map",
                           seed=SEED, device=dev, grow=True, expire_after=N_EXP)
    outs = []
    for ids in _stream():  # every rank looks up the whole batch: summed and averaged, the W = 1 update
        rows = t.lookup(ids.to(dev))
        (rows.float().pow(2).sum() * 0.01).backward()
        t.push_pending()
        outs.append(rows.detach().cpu())
    t.synchronize()
    return outs, t.row_stats(), t.exchange, dict(t.exchange_info)


def test_expiring_world2_gpu_equals_world1_cpu():
    res = run_loopback(_sparse_body, 2, DEV)
    b = _table()
    for i, ids in enumerate(_stream()):
        want = _step(b, ids)
        for r in range(2):
            _close(res[r][0][i], want)
    for r in range(2):
        assert res[r][2] == "collective" and "expiring" in res[r][3]["fallback"]
    assert res[0][1]["compactions"] + res[1][1]["compactions"] >= 2
    assert res[0][1]["evicted"] + res[1][1]["evicted"] > 0


# ------------------------------------------------------------------------------ bags
def test_lookup_bags_id_returns_after_eviction():
    """Bag 0 holds ``keep`` in every round and ``gone`` in rounds 0 and 5: at round 5 ``gone`` is a
    new row, so the bag is the trained row of ``keep`` plus the init of ``gone``."""
    a, b = _table(DEV), _table()
    keep, gone = 7919 * 3 + 5, 7919 * 11 + 5
    init = S.init_values(SEED, torch.tensor([gone]), DIM, *INIT)[0]
    for r in range(8):
        vals = ([keep, gone] if r in (0, 5) else [keep]) + _new_ids(r, 40).tolist()  # new ids: the map compacts
        values = torch.tensor(vals)
        offsets = torch.tensor([0, len(vals) - 40, len(vals) - 20, len(vals)])
        krow = b.table[b.shard.slots(torch.tensor([keep]), insert=False)][0].clone() if r else None
        outs = []
        for t in (a, b):
            out = t.lookup_bags(values.to(t.device), offsets.to(t.device), mode="sum")
            (out.float().pow(2).sum() * 0.01).backward()
            t.push_pending()
            outs.append(out.detach().cpu())
        _close(outs[0], outs[1])
        if r == 1:
            assert not torch.equal(b.table[b.shard.slots(torch.tensor([gone]), insert=False)][0], init)  # trained
        if r == 5:
            _close(outs[0][0], krow + init)
    _compacted_ok(a, at_least=1)


