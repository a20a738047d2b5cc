"""Causal GQA flash attention over packed documents (csrc/kernels/flash_attn.hip, DOCS instantiations)
on the Llama-3-8B bench shape (4 x 4096 tokens, 32 q / 8 kv heads x 128): forward and backward times
of (a) the plain kernels, (b) the document kernels with one document per row, (c) eight documents
of 512 per row, (d) eight documents per row with lengths drawn once from a fixed seed (mean 512).
The variants alternate inside one process, round after round; each line reports the median and the
min - max over the rounds, so a difference can be held against the spread.  Also prints, by formula
from the bounds, the key tiles the forward / dQ kernels visit and the query stages of dK / dV.

    python scripts/probe_flash_docs.py [rounds] [--counts] [--only=a_plain,b_one_doc]
    (--counts: the formulas only, no GPU; --only: these variants, e.g. under a kernel trace, where the
    instantiations are told apart by name and the variants of one instantiation are not)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ps_amd.ops import native  # noqa: E402
from ps_amd.ops.transformer import doc_bounds  # noqa: E402

B, H, KV, S, D = 4, 32, 8, 4096, 128


def layouts():
    g = torch.Generator().manual_seed(0)
    drawn = []
    for _ in range(B):
        cuts = (torch.randperm(S - 1, generator=g)[:7] + 1).sort().values.tolist()
        drawn.append([b - a for a, b in zip([0] + cuts, cuts + [S])])
    return {"a_plain": None, "b_one_doc": [[S]] * B, "c_8x512": [[512] * 8] * B, "d_drawn_mean512": drawn}


def ids_of(rows):
    return torch.stack([torch.repeat_interleave(torch.arange(len(r)), torch.tensor(r)) for r in rows])


def tile_counts(rows):
    """Per (batch row, head), averaged over the rows: 64-key tiles a 256-query block loads in the
    forward / dQ kernels (from the tile of its first query's bound to its diagonal), and 64-query
    stages a 128-key block loads per q head in dK / dV (from its first key to the end of its last
    key's document)."""
    if rows is None:
        rows = [[S]] * B
    start, end = doc_bounds(ids_of(rows))
    fwd = sum((qb * 256 + 255) // 64 + 1 - int(start[b, qb * 256]) // 64 for b in range(B) for qb in range(S // 256))
    dkv = sum((int(end[b, kb * 128 + 127]) + 63) // 64 - kb * 2 for b in range(B) for kb in range(S // 128))
    return fwd / B, dkv / B


def bench(fn, it=50):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 7
    lay = layouts()
    only = [a.split("=", 1)[1].split(",") for a in sys.argv[1:] if a.startswith("--only=")]
    if only:
        lay = {name: lay[name] for name in only[0]}
    for name, rows in lay.items():
        f, d = tile_counts(rows)
        print(json.dumps({"variant": name, "fwd_dq_key_tiles_per_batch_head": f, "dkdv_query_stages_per_batch_kvhead_qhead": d,
                          "doc_lengths_row0": rows[0] if rows else None}), flush=True)
    if "--counts" in sys.argv:
        return
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(B, h, S, D, generator=g).bfloat16().cuda() for h in (H, KV, KV))
    dout = torch.randn(B, S, H * D, generator=g).bfloat16().cuda()
    nat = native()
    runs = {}
    for name, rows in lay.items():
        bounds = () if rows is None else doc_bounds(ids_of(rows).cuda())
        out, lse = nat.fa_fwd(q, k, v, *bounds[:1])
        runs[name] = (lambda bounds=bounds: nat.fa_fwd(q, k, v, *bounds[:1]),
                      lambda bounds=bounds, out=out, lse=lse: nat.fa_bwd(q, k, v, out, dout, lse, *bounds))
    for fwd, bwd in runs.values():  # warm-up: every kernel instantiation, every shape
        for _ in range(3):
            fwd()
            bwd()
    torch.cuda.synchronize()
    times = {name: ([], []) for name in runs}
    for _ in range(rounds):
        for name, (fwd, bwd) in runs.items():
            times[name][0].append(bench(fwd))
            times[name][1].append(bench(bwd))
    for name, (tf, tb) in times.items():
        print(json.dumps({"variant": name, "shape": f"B{B} H{H} KV{KV} S{S} D{D}", "rounds": rounds,
                          "fwd_us_median": round(statistics.median(tf), 1), "fwd_us_min_max": [round(min(tf), 1), round(max(tf), 1)],
                          "bwd_us_median": round(statistics.median(tb), 1), "bwd_us_min_max": [round(min(tb), 1), round(max(tb), 1)]}),
              flush=True)


if __name__ == "__main__":
    main()
