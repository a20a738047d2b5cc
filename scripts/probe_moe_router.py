"""Time the fused MoE router (ops/moe.py ``router``, route ``moe_router``) against the torch composition ``_router_ref``
on the same bf16 inputs and coefficients, and measure both against fp64.

Alternated pairs in one process after a warm-up of both, device events around ``--reps`` calls each.  Per shape:
  * every row-tile candidate of ``moe_router_fwd`` beside a plain device copy of h's bytes (the kernel's floor: it has
    to stream h once), alternated;
  * ``moe_router_finish`` and ``moe_router_bwd`` beside ``moe_router_fwd`` at the default row tile;
  * forward and forward + backward of ``router`` against ``_router_ref``;
  * the error of both against ``_router_ref`` in fp64 on wts, aux, dh and dWr (the selection of the fused route given
    to all three), and the share of tokens whose top-k set from bf16 logits differs from the fp64 one.
Needs a GPU.

    python scripts/probe_moe_router.py [--tokens 16384] [--pairs 5] [--reps 20] [--out profiles/moe_router_probe.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ps_amd.ops import moe as M  # noqa: E402
from ps_amd.ops._ext import native  # noqa: E402

SHAPES = {"fine": (64, 8, 2048), "mixtral": (8, 2, 4096), "wide": (128, 8, 4096)}  # E, k, D
AUX, ZC = 0.01, 0.001


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us per call


def pairs(label, names, fns, n, reps, emit):
    for fn in fns * 2:  # warm-up of all
        fn()
    torch.cuda.synchronize()
    for i in range(n):
        ts = [timed(fn, reps) for fn in fns]
        emit(f"{label} pair {i}: " + " ".join(f"{nm} {t:.1f} us" for nm, t in zip(names, ts))
             + f" ratio {ts[0] / ts[-1]:.3f}")


def grads(fn, h, w, dwts):
    h, w = h.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    idx, wts, aux = fn(h, w)
    ((wts * dwts.to(wts.dtype)).sum() + aux).backward()
    return idx, (wts.detach(), aux.detach(), h.grad, w.grad)


def probe(name, T, n, reps, emit):
    E, k, D = SHAPES[name]
    g = torch.Generator().manual_seed(0)
    h = torch.randn(T, D, generator=g).bfloat16().cuda()
    w = (torch.randn(E, D, generator=g) / D ** 0.5).bfloat16().cuda()
    dwts = torch.randn(T, k, generator=g).cuda()
    tag = f"{name} T={T} E={E} k={k} D={D}"

    # accuracy: both routes against fp64, the fused selection given to all
    idx, fused = grads(lambda a, b: M.router(a, b, k, True, AUX, ZC), h, w, dwts)
    _, comp = grads(lambda a, b: M._router_ref(a, b, k, True, AUX, ZC, idx=idx), h, w, dwts)
    _, ref = grads(lambda a, b: M._router_ref(a, b, k, True, AUX, ZC, idx=idx), h.double(), w.double(), dwts)
    for what, f, c, r in zip(("wts", "aux", "dh", "dWr"), fused, comp, ref):
        ef, ec = (((t.double() - r).abs().max() / r.abs().max()).item() for t in (f, c))
        emit(f"{tag} error vs fp64 {what}: fused {ef:.3e} composition {ec:.3e} ratio {ef / max(ec, 1e-300):.3f}")
    top64 = M._router_ref(h.double(), w.double(), k)[0].sort(1).values
    for what, got in (("bf16-logit", M._router_ref(h, w, k)[0]), ("fused", idx)):
        diff = (got.sort(1).values != top64).any(1).float().mean().item()
        emit(f"{tag} tokens whose {what} top-k set differs from the fp64 one: {100 * diff:.3f} %")
    del ref, comp, fused, top64

    # row-tile candidates beside the copy of h
    dst, nat = torch.empty_like(h), native()
    for tm in (32, 64):
        pairs(f"{tag} moe_router_fwd row tile {tm} ({(T + tm - 1) // tm} blocks) vs copy of h ({h.numel() * 2 >> 20} MiB)",
              ("kernel", "copy"), [lambda: nat.moe_router_fwd(h, w, k, True, tm), lambda: dst.copy_(h)], n, reps, emit)

    # the two small launches, each beside the forward kernel at the default row tile
    idx, wts, lse, logits, part = nat.moe_router_fwd(h, w, k, True)
    counts = nat.moe_router_finish(part, T, k, AUX, ZC)[0]
    one = torch.ones(1, device="cuda")
    pairs(f"{tag} moe_router_finish ({part.shape[0]} partial rows) / moe_router_bwd / moe_router_fwd",
          ("finish", "bwd", "fwd"), [lambda: nat.moe_router_finish(part, T, k, AUX, ZC),
                                     lambda: nat.moe_router_bwd(logits, lse, idx, wts, dwts, one, counts, True, AUX, ZC),
                                     lambda: nat.moe_router_fwd(h, w, k, True)], n, reps, emit)

    # the op against the composition
    def fwd(fn):
        with torch.no_grad():
            fn(h, w, k, True, AUX, ZC)

    hg, wg = h.clone().requires_grad_(), w.clone().requires_grad_()

    def both(fn):
        hg.grad = wg.grad = None
        _, wts, aux = fn(hg, wg, k, True, AUX, ZC)
        ((wts * dwts).sum() + aux).backward()

    for what, run in (("fwd", fwd), ("fwd+bwd", both)):
        pairs(f"{tag} {what}", ("fused", "composition"), [lambda: run(M.router), lambda: run(M._router_ref)], n, reps, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_moe_router needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for name in SHAPES:
        probe(name, a.tokens, a.pairs, a.reps, emit)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
