"""Time and size the fused LM-head loss (ops/lm_head.py, route ``fused_head``) against the composition
``cross_entropy(ps_linear(h, w), labels)``.

Alternated pairs in one process after a warm-up of both, device events around each call.  Per shape: forward and
forward + backward time of every pair, the peak of ``torch.cuda.max_memory_allocated`` over the inputs (h, w, labels)
for each path, and the achieved TF/s of the two in-house GEMM kernels timed alone (2 T V D FLOPs each: ``lm_head_fwd``
with its finishing kernel, ``lm_head_dz`` over all chunks of the default chunking).  The register figures are the
compiler's (-Rpass-analysis=kernel-resource-usage), repeated here so that the record is in one file.  Needs a GPU.

    python scripts/probe_lm_head.py [--tokens 16384] [--pairs 5] [--out profiles/lm_head_probe.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ps_amd import knobs  # noqa: E402
from ps_amd.ops import lm_head as L  # noqa: E402
from ps_amd.ops._ext import native  # noqa: E402

SHAPES = [(4096, 128256), (4096, 151936), (2048, 128256)]  # D, V
REGISTERS = ("registers (gfx950, hipcc -O3): lm_head_fwd 208 VGPR 0 AGPR 64 KB LDS 2 waves/SIMD; "
             "lm_head_dz 107 VGPR 64 AGPR 64.25 KB LDS 2 waves/SIMD; lm_head_finish 12 VGPR; no scratch, no spills")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def probe(T, D, V, pairs, emit):
    g = torch.Generator().manual_seed(0)
    h = torch.randn(T, D, generator=g).bfloat16().cuda().requires_grad_()
    w = (0.02 * torch.randn(V, D, generator=g)).bfloat16().cuda().requires_grad_()
    y = torch.randint(0, V, (T,), generator=g).cuda()
    tag = f"T={T} D={D} V={V}"

    def fwd(off):
        os.environ[knobs.ENV] = "fused_head" if off else ""
        with torch.no_grad():
            L.linear_cross_entropy(h, w, y)

    def both(off):
        os.environ[knobs.ENV] = "fused_head" if off else ""
        h.grad = w.grad = None
        L.linear_cross_entropy(h, w, y).backward()

    for run in (fwd, both):
        name = "fwd" if run is fwd else "fwd+bwd"
        peak = {}
        for off in (False, True, False, True):  # warm-up of both; the second round measures the peaks
            h.grad = w.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            run(off)
            torch.cuda.synchronize()
            peak[off] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        emit(f"{tag} {name} peak memory over the inputs: fused {peak[False]:.0f} MiB composition {peak[True]:.0f} MiB "
             f"saved {peak[True] - peak[False]:.0f} MiB (bf16 logits {T * V * 2 / 2 ** 20:.0f} MiB)")
        for i in range(pairs):
            tf, tc = timed(lambda: run(False)), timed(lambda: run(True))
            emit(f"{tag} {name} pair {i}: fused {tf:.2f} ms composition {tc:.2f} ms ratio {tf / tc:.3f}")
    os.environ[knobs.ENV] = ""
    h.grad = w.grad = None

    n, hd, wd = native(), h.detach(), w.detach()
    lse, _ = n.lm_head_fwd(hd, wd, y, -100, 0)
    chunk = L.default_chunk_cols(T, V)
    dz = torch.empty(T * chunk, dtype=torch.bfloat16, device="cuda")
    one = torch.ones(1, device="cuda")

    def dz_all():
        for v0 in range(0, V, chunk):
            c = min(V, v0 + chunk) - v0
            n.lm_head_dz(hd, wd, y, lse, one, one, -100, v0, dz[:T * c].view(T, c))

    flops = 2.0 * T * V * D
    for kname, fn in (("lm_head_fwd", lambda: n.lm_head_fwd(hd, wd, y, -100, 0)), ("lm_head_dz", dz_all)):
        fn()
        for i in range(pairs):
            t = timed(fn)
            emit(f"{tag} {kname} alone, run {i}: {t:.2f} ms {flops / t / 1e9:.0f} TF/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_lm_head needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(REGISTERS)
    for D, V in SHAPES:
        probe(a.tokens, D, V, a.pairs, emit)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
