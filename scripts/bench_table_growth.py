"""Migration rate of a growing sparse shard: rehash_rows vs a device copy vs the composition oracle.

A 2^20-slot map at load just under 1/2, dim 64 rows with a row-wise Adagrad state, moves into
2^21 slots.  All three are timed with device events in one run, alternating, after a warm-up:

  rehash_rows   GB/s of rows read plus written (2 * live * dim * 4 bytes), and of everything the
                pass touches (keys, remap, flags, state on top);
  d2d copy      a contiguous copy of as many bytes as the live rows (same read + write count);
  oracle        hash_slots insert + nonzero + masked index copies (ops.sparse.rehash_rows_ref).

usage: python scripts/bench_table_growth.py [--out profiles/table_growth_migration.txt] [--iters 20]
"""
import argparse
import statistics
import sys

import torch

from ps_amd.ops import sparse as S


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/table_growth_migration.txt")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lg", type=int, default=20, help="log2 of the old capacity")
    ap.add_argument("--dim", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_table_growth needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    old_cap, new_cap, dim = 1 << a.lg, 2 << a.lg, a.dim
    live = old_cap // 2 - 1
    g = torch.Generator().manual_seed(0)
    ids = torch.randperm(1 << (a.lg + 2), generator=g)[:live] * 1048573 + (1 << 39)
    keys = (((torch.arange(live) % 4) << 44) | ids).to(dev)
    hk = torch.full((old_cap,), -1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    S.hash_slots(hk, keys, True, status)
    table = torch.randn(old_cap, dim, device=dev)
    flags = torch.ones(old_cap, dtype=torch.uint8, device=dev)
    state = torch.rand(old_cap, device=dev)
    nk = torch.empty(new_cap, dtype=torch.int64, device=dev)
    nt = torch.empty(new_cap, dim, device=dev)
    nf = torch.empty(new_cap, dtype=torch.uint8, device=dev)
    ns = torch.empty(new_cap, device=dev)
    src = torch.randn(live, dim, device=dev)
    dst = torch.empty_like(src)

    def reset():
        nk.fill_(-1)
        nt.zero_()
        nf.zero_()
        ns.zero_()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    runs = {
        "rehash_rows": lambda: S.rehash_rows(hk, nk, table, nt, flags, nf, [state], [ns]),
        "d2d_copy": lambda: dst.copy_(src),
        "oracle": lambda: S.rehash_rows_ref(hk, nk, table, nt, flags, nf, [state], [ns]),
    }
    times = {k: [] for k in runs}
    for it in range(a.iters + 3):  # 3 warm-up rounds; the three alternate inside every round
        for name, fn in runs.items():
            reset()
            torch.cuda.synchronize()
            t = timed(fn)
            if it >= 3:
                times[name].append(t)
    # the result of the last rehash_rows round is checked against the map's own lookups
    reset()
    remap = S.rehash_rows(hk, nk, table, nt, flags, nf, [state], [ns])
    found = S.hash_slots(nk, keys, False, status)
    old_slots = S.hash_slots(hk, keys, False, status)
    assert torch.equal(found, remap[old_slots]) and torch.equal(nt[found], table[old_slots])
    assert int(status.item()) == 0

    row_bytes = 2 * live * dim * 4
    all_bytes = row_bytes + 2 * live * (4 + 1) + old_cap * 8 * 2 + live * 8 * 2
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [
        f"table growth migration: {old_cap} -> {new_cap} slots, dim {dim}, row-wise state, {live} live rows",
        f"device: {torch.cuda.get_device_name(0)}; device events, median of {a.iters} alternating rounds "
        "(min .. max in brackets)",
    ]
    for k in runs:
        lines.append(f"  {k:12s} {med[k] * 1e3:9.3f} ms  [{min(times[k]) * 1e3:.3f} .. {max(times[k]) * 1e3:.3f}]")
    lines += [
        f"rehash_rows rows read + written: {row_bytes / med['rehash_rows'] / 1e9:8.1f} GB/s "
        f"({row_bytes / 1e6:.1f} MB); with keys, remap, flags, state: {all_bytes / med['rehash_rows'] / 1e9:.1f} GB/s",
        f"d2d copy of the same row bytes:  {row_bytes / med['d2d_copy'] / 1e9:8.1f} GB/s",
        f"composition oracle:              {med['oracle'] * 1e3:8.3f} ms = {med['oracle'] / med['rehash_rows']:.2f} x "
        "rehash_rows",
        f"rehash_rows / d2d copy time:     {med['rehash_rows'] / med['d2d_copy']:8.2f} x",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
