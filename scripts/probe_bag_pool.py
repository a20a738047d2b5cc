"""Fused multi-hot pooling (csrc/kernels/bags.hip) against the composition of the one-hot kernels
it replaces, forward + backward, at DLRM width: dim 128, 26 fields, batch 16384, bag lengths
1..15, ``dlrm_batch`` ids.

The fused path runs with the ``bag_pool`` route on, the composition (gather_rows -> [nnz, dim] ->
segment_reduce_rows forward; gather of the output gradient -> [nnz, dim] -> segment_reduce_rows
backward) with ``PS_AMD_DISABLE=bag_pool`` in the same process, alternating per round.  Prints
times, the bytes each path moves by count (every access counted once, index vectors included) and
the achieved rate against the device-to-device copy rate of profiles/r3_server_kernels_roofline.json.

    python scripts/probe_bag_pool.py [--batch 16384] [--rounds 10] [--iters 20] [--roofline PATH]

The parent process never touches the GPU: every GPU phase (check, time) is a child process under
its own time limit, and a failed phase ends the probe."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS, DIM, ROWS_PER_TABLE, MIN_HOT, MAX_HOT = 26, 128, 100000, 1, 15
PHASES = (("check", 240), ("time", 420))


def _inputs(batch, dev):
    import torch

    from ps_amd.models.dlrm import dlrm_batch_multihot
    from ps_amd.ops import sparse as S

    rows = [ROWS_PER_TABLE] * FIELDS
    _, (values, offsets), _ = dlrm_batch_multihot(batch, rows, MAX_HOT, seed=0, min_hot=MIN_HOT)
    values, offsets = values.to(dev), offsets.to(dev)
    bag_of = S._bag_of(offsets, values.numel())
    keys = (bag_of % FIELDS) * ROWS_PER_TABLE + values
    uniq, inv, _, perm, seg_off = S.unique_with_segments(keys)
    g = torch.Generator(device=dev).manual_seed(1)
    leaf = torch.randn(uniq.numel(), DIM, device=dev, generator=g)
    return leaf, inv.contiguous(), perm.contiguous(), seg_off, offsets, bag_of.contiguous()


def _step(leaf, idx, dout, out_dtype):
    from ps_amd.ops import sparse as S

    leaf.grad = None
    out = S.pool_unique(leaf, *idx, None, False, out_dtype)
    out.backward(dout)
    return out, leaf.grad


def _set_route(fused: bool) -> None:
    if fused:
        os.environ.pop("PS_AMD_DISABLE", None)
    else:
        os.environ["PS_AMD_DISABLE"] = "bag_pool"


def _bytes(nnz, nu, G, osz):
    """(fused, composed) bytes of forward + backward, every access counted once."""
    row, idx = DIM * 4, 8
    fused = (nnz * (row + idx) + (G + 1) * idx + G * DIM * osz  # fwd: rows through inv -> out
             + nnz * (DIM * osz + 2 * idx) + (nu + 1) * idx + nu * row)  # bwd: dout through perm, bag_of -> drows
    comp = (nnz * (row + idx) + nnz * row  # gather_rows: rows through inv -> [nnz, dim]
            + nnz * (row + idx) + (G + 1) * idx + G * DIM * osz  # segment_reduce_rows over the bags
            + nnz * (DIM * osz + idx) + nnz * row  # gather of dout through bag_of -> [nnz, dim]
            + nnz * (row + idx) + (nu + 1) * idx + nu * row)  # segment_reduce_rows over the unique rows
    return fused, comp


def phase_check(args) -> None:
    import torch

    dev = torch.device("cuda", 0)
    leaf, *idx = _inputs(args.batch, dev)
    leaf.requires_grad_(True)
    G = idx[3].numel() - 1
    for dt in (torch.float32, torch.bfloat16):
        dout = torch.randn(G, DIM, device=dev).to(dt)
        _set_route(True)
        o1, g1 = _step(leaf, idx, dout, dt)
        _set_route(False)
        o2, g2 = _step(leaf, idx, dout, dt)
        o1, o2 = o1.detach(), o2.detach()
        torch.cuda.synchronize()
        # both sum each bag / segment in j order with the same grouping: equal bit for bit
        print(f"check {str(dt):15s} out equal: {torch.equal(o1, o2)}  grad equal: {torch.equal(g1, g2)}  "
              f"max |d out| {float((o1.float() - o2.float()).abs().max()):.3e}  "
              f"max |d grad| {float((g1 - g2).abs().max()):.3e}")
        assert torch.allclose(o1.float(), o2.float(), rtol=1e-2 if dt == torch.bfloat16 else 1e-5, atol=1e-5)
        assert torch.allclose(g1, g2, rtol=1e-5, atol=1e-5)


def phase_time(args) -> None:
    import statistics

    import torch

    dev = torch.device("cuda", 0)
    leaf, *idx = _inputs(args.batch, dev)
    leaf.requires_grad_(True)
    nnz, nu, G = idx[0].numel(), leaf.shape[0], idx[3].numel() - 1
    copy_tbps = None
    if os.path.exists(args.roofline):
        copy_tbps = float(json.load(open(args.roofline))["copy_roofline_TBps"])
    print(f"shape: batch {args.batch}, fields {FIELDS}, dim {DIM}, bag lengths {MIN_HOT}..{MAX_HOT}: "
          f"G {G}, nnz {nnz}, unique rows {nu}, [nnz, dim] fp32 = {nnz * DIM * 4 / 1e9:.2f} GB")
    print(f"d2d copy rate: {copy_tbps} TB/s ({os.path.basename(args.roofline)})" if copy_tbps else
          f"d2d copy rate: {args.roofline} not found, fractions not printed")
    for dt in (torch.float32, torch.bfloat16):
        dout = torch.randn(G, DIM, device=dev).to(dt)
        times = {True: [], False: []}
        for fused in (True, False):  # warm up both paths at this shape
            _set_route(fused)
            for _ in range(3):
                _step(leaf, idx, dout, dt)
        torch.cuda.synchronize()
        for _ in range(args.rounds):  # alternate the two paths round by round
            for fused in (True, False):
                _set_route(fused)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    _step(leaf, idx, dout, dt)
                b.record()
                b.synchronize()
                times[fused].append(a.elapsed_time(b) / args.iters)
        bf, bc = _bytes(nnz, nu, G, 2 if dt == torch.bfloat16 else 4)
        for fused, nbytes in ((True, bf), (False, bc)):
            t = times[fused]
            med = statistics.median(t)
            line = (f"{str(dt):15s} {'fused' if fused else 'composed':9s} fwd+bwd  median {med:8.3f} ms  "
                    f"min {min(t):8.3f}  max {max(t):8.3f}  ({args.rounds} rounds x {args.iters})  "
                    f"bytes {nbytes / 1e9:6.2f} GB  {nbytes / med / 1e6:7.1f} GB/s")
            if copy_tbps:
                line += f"  = {nbytes / med / 1e9 / copy_tbps:5.1%} of d2d copy"
            print(line)
        mf, mc = statistics.median(times[True]), statistics.median(times[False])
        print(f"{str(dt):15s} composed / fused time: {mc / mf:.2f}x   bytes: {bc / bf:.2f}x")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--roofline", default=os.path.join(ROOT, "profiles", "r3_server_kernels_roofline.json"))
    ap.add_argument("--phase", choices=[p for p, _ in PHASES])
    args = ap.parse_args()
    if args.phase:
        import torch

        assert torch.cuda.is_available(), "the probe measures on a GPU; there is none"
        {"check": phase_check, "time": phase_time}[args.phase](args)
        return 0
    for name, limit in PHASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--phase", name, "--batch", str(args.batch), "--rounds",
               str(args.rounds), "--iters", str(args.iters), "--roofline", args.roofline]
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f"phase {name}: no result within {limit} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"phase {name}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
