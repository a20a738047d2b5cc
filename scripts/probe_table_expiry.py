"""Cost of expiring rows: compact_rows vs rehash_rows, the stamping lookup vs hash_slots, and the
capacity of an expiring table on a stream of ids that never return.

1. A 2^21-slot map with 1M live rows of dim 128 moves into 2^22 slots: ``rehash_rows`` (every row)
   against ``compact_rows`` with 1.0, 0.5 and 0.1 of the rows surviving, into the same 2^22 slots
   and into the map the policy would pick (max(64, pow2(4 * survivors))).  With a row-wise Adagrad
   state and with two full Adam states.
2. 1.7M keys that are all in a 2^22-slot map: ``hash_slots`` with insert, ``hash_slots_stamp``, and
   ``hash_slots_stamp`` with the rebirth check (no row is old enough to be reset).
3. SparseTable(grow=True, expire_after=2), 200 rounds of 4096 new ids: capacity and the device
   counter ``evicted`` after every round, next to the capacity of a plain growable table.

Everything is timed with device events in one process, the variants alternating inside every
round after three warm-up rounds; medians, with min .. max as the run-to-run spread.

usage: python scripts/probe_table_expiry.py [--out profiles/table_expiry_probe.txt] [--iters 10]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ps_amd.ops import sparse as S  # noqa: E402


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _alternate(runs, iters, before=None):
    times = {k: [] for k in runs}
    for it in range(iters + 3):
        for name, fn in runs.items():
            if before is not None:
                before(name)
            torch.cuda.synchronize()
            t = _timed(fn)
            if it >= 3:
                times[name].append(t)
    return times


def _row(name, ts, extra=""):
    return f"  {name:34s} {statistics.median(ts):9.3f} ms  [{min(ts):.3f} .. {max(ts):.3f}]{extra}"


def _pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def migration(dev, states, iters, lines):
    old_cap, big, dim, live = 1 << 21, 1 << 22, 128, 1_000_000
    g = torch.Generator().manual_seed(0)
    ids = torch.randperm(1 << 23, generator=g)[:live] * 1048573 + (1 << 39)
    keys = (((torch.arange(live) % 4) << 44) | ids).to(dev)
    hk = torch.full((old_cap,), -1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    slots = S.hash_slots(hk, keys, True, status)
    table = torch.randn(old_cap, dim, device=dev)
    flags = torch.ones(old_cap, dtype=torch.uint8, device=dev)
    mk = (lambda cap: [torch.empty(cap, device=dev)]) if states == "rowwise" else \
        (lambda cap: [torch.empty(cap, dim, device=dev) for _ in range(2)])
    st = mk(old_cap)
    for s in st:
        s.uniform_()
    stamp = torch.zeros(old_cap, dtype=torch.int32, device=dev)
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    lines.append(f"{old_cap} slots, {live} live rows, dim {dim}, states: {states}")
    for share in (1.0, 0.5, 0.1):
        surv = int(live * share)
        stamp.zero_()
        stamp[slots[torch.randperm(live, generator=g)[:surv].to(dev)]] = 1
        small = max(64, _pow2(4 * surv))
        new = {cap: (torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dim, device=dev),
                     torch.empty(cap, dtype=torch.uint8, device=dev), mk(cap),
                     torch.empty(cap, dtype=torch.int32, device=dev)) for cap in {big, small}}

        def reset(name):
            n = new[small if name.endswith("policy") else big]
            n[0].fill_(-1)
            for t in (n[1], n[2], n[4], *n[3]):
                t.zero_()

        def compact(cap):
            n = new[cap]
            return S.compact_rows(hk, n[0], table, n[1], flags, n[2], stamp, n[4], 1, counters, status, st, n[3])

        b = new[big]
        runs = {"rehash_rows -> 2^22": lambda: S.rehash_rows(hk, b[0], table, b[1], flags, b[2], st, b[3]),
                "compact_rows -> 2^22": lambda: compact(big),
                "compact_rows -> policy": lambda: compact(small)}
        times = _alternate(runs, iters, reset)
        reset("policy")
        counters.zero_()
        remap = compact(small)
        found = S.hash_slots(new[small][0], keys, False, status)
        assert counters.tolist() == [surv, live - surv] and int((found >= 0).sum()) == surv
        assert torch.equal(found, remap[slots]) and int(status.item()) == 0
        ok = found >= 0
        assert torch.equal(new[small][1][found[ok]], table[slots[ok]])
        moved = 2 * surv * dim * 4 * (1 if states == "rowwise" else 3)
        lines.append(f" survivors {share:.1f} ({surv} rows, policy target {small} slots)")
        for k, v in times.items():
            extra = "" if k.startswith("rehash") else f"  {moved / statistics.median(v) / 1e6:7.1f} GB/s of rows + full states moved"
            lines.append(_row(k, v, extra))
        del new


def lookup(dev, iters, lines):
    cap, n, dim = 1 << 22, 1_700_000, 128
    g = torch.Generator().manual_seed(1)
    ids = torch.randperm(1 << 23, generator=g)[:n] * 1048573 + (1 << 39)
    keys = (((torch.arange(n) % 4) << 44) | ids).to(dev)
    hk = torch.full((cap,), -1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stamp = torch.zeros(cap, dtype=torch.int32, device=dev)
    S.hash_slots_stamp(hk, keys, stamp, 5, status)
    table = torch.zeros(cap, dim, device=dev)
    flags = torch.ones(cap, dtype=torch.uint8, device=dev)
    state = torch.zeros(cap, device=dev)
    runs = {"hash_slots (insert)": lambda: S.hash_slots(hk, keys, True, status),
            "hash_slots_stamp": lambda: S.hash_slots_stamp(hk, keys, stamp, 6, status),
            "hash_slots_stamp + rebirth check": lambda: S.hash_slots_stamp(hk, keys, stamp, 6, status, cutoff=4,
                                                                           table=table, flags=flags, states=[state])}
    times = _alternate(runs, iters * 2)
    assert int(status.item()) == 0 and flags.all()
    lines.append(f"lookup of {n} keys, all present, in a {cap}-slot map")
    for k, v in times.items():
        lines.append(_row(k, v))


def stream(dev, lines):
    from ps_amd.parallel.sparse_table import SparseTable
    from ps_amd.parallel.updaters import AdagradUpdater

    def make(**kw):
        return SparseTable("t", 16, 8, AdagradUpdater(0.1, 1e-8, rowwise=True), init=(-0.1, 0.1), id_mode="map",
                           device=dev, grow=True, **kw)

    a, plain = make(expire_after=2), make()
    rec = []
    for r in range(200):
        ids = (torch.arange(4096) + 4096 * r) * 7919 + (1 << 35)
        for t in (a, plain):
            rows = t.lookup(ids.to(dev))
            (rows.float().pow(2).sum() * 0.01).backward()
            t.push_pending()
        torch.cuda.synchronize()
        rec.append((a.stats["capacity"], int(a.shard.counters[1].item()), plain.stats["capacity"]))
    a.synchronize()
    st = a.row_stats()
    lines.append("200 rounds of 4096 new ids, expire_after=2: round: capacity / evicted so far (plain growable capacity)")
    for r0 in range(0, 200, 4):
        lines.append("  " + "   ".join(f"{r:3d}: {c:6d} / {e:7d} ({p:8d})" for r, (c, e, p) in
                                       zip(range(r0, r0 + 4), rec[r0:r0 + 4])))
    lines.append(f"  compactions {st['compactions']}, grows {st['grows']}, host_syncs {st['host_syncs']}, evicted "
                 f"{st['evicted']}, live {int((a.shard.hkeys >= 0).sum())}, ids seen {200 * 4096}")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/table_expiry_probe.txt")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("probe_table_expiry needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    lines = [f"expiring sparse tables on {torch.cuda.get_device_name(0)}: device events, median of {a.iters} "
             "alternating rounds (min .. max in brackets)"]
    for states in ("rowwise", "full2"):
        migration(dev, states, a.iters, lines)
    lookup(dev, a.iters, lines)
    stream(dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
