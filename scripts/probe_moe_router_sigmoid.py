"""Time the sigmoid / bias / group-limited form of the fused MoE router (ops/moe.py ``router(score="sigmoid")``) against
the torch composition ``_router_ref`` on the same bf16 inputs, bias and coefficients, and measure both against fp64.

The method of scripts/probe_moe_router.py (its helpers are imported): alternated pairs in one process after a warm-up
of all, device events around ``--reps`` calls each.  Per shape:
  * the sigmoid forward kernel, the softmax forward kernel on the same operands and a plain device copy of h's bytes
    (the floor: h is streamed once), alternated -- what the sigmoid epilogue and its group step cost;
  * the sigmoid and softmax backward kernels, alternated;
  * forward and forward + backward of ``router`` against ``_router_ref``;
  * the error of both against ``_router_ref`` in fp64 on wts, aux, dh and dWr (the fused selection given to all
    three), and the share of tokens whose chosen set from bf16 logits differs from the fp64 one.
Needs a GPU.

    python scripts/probe_moe_router_sigmoid.py [--tokens 16384] [--pairs 5] [--reps 20] [--out profiles/moe_router_sigmoid_probe.txt]
"""
import argparse

import torch
from probe_moe_router import grads, pairs  # puts the repository root on sys.path

from ps_amd.ops import moe as M  # noqa: E402
from ps_amd.ops._ext import native  # noqa: E402

SHAPES = {"fine": (64, 6, 2048, 1, 1), "wide-grouped": (128, 8, 4096, 8, 4)}  # E, k, D, n_group, topk_group
AUX, ZC, SCALE = 0.01, 0.001, 2.5


def probe(name, T, n, reps, emit):
    E, k, D, ng, tg = SHAPES[name]
    g = torch.Generator().manual_seed(0)
    h = torch.randn(T, D, generator=g).bfloat16().cuda()
    w = (torch.randn(E, D, generator=g) / D ** 0.5).bfloat16().cuda()
    dwts = torch.randn(T, k, generator=g).cuda()
    bias = (torch.rand(E, generator=g) * 0.2 - 0.1).cuda()
    kw = dict(score="sigmoid", bias=bias, n_group=ng, topk_group=tg, scale=SCALE)
    tag = f"{name} T={T} E={E} k={k} D={D} groups {ng}/{tg}"

    idx, fused = grads(lambda a, b: M.router(a, b, k, True, AUX, ZC, **kw), h, w, dwts)
    _, comp = grads(lambda a, b: M._router_ref(a, b, k, True, AUX, ZC, idx, **kw), h, w, dwts)
    _, ref = grads(lambda a, b: M._router_ref(a, b, k, True, AUX, ZC, idx, **kw), h.double(), w.double(), dwts)
    for what, f, c, r in zip(("wts", "aux", "dh", "dWr"), fused, comp, ref):
        ef, ec = (((t.double() - r).abs().max() / r.abs().max()).item() for t in (f, c))
        emit(f"{tag} error vs fp64 {what}: fused {ef:.3e} composition {ec:.3e} ratio {ef / max(ec, 1e-300):.3f}")
    top64 = M._router_ref(h.double(), w.double(), k, **kw)[0].sort(1).values
    for what, got in (("bf16-logit", M._router_ref(h, w, k, **kw)[0]), ("fused", idx)):
        diff = (got.sort(1).values != top64).any(1).float().mean().item()
        emit(f"{tag} tokens whose {what} chosen set differs from the fp64 one: {100 * diff:.3f} %")
    del ref, comp, fused, top64

    dst, nat = torch.empty_like(h), native()
    sig = lambda: nat.moe_router_fwd(h, w, k, True, 0, True, bias, ng, tg, SCALE)  # noqa: E731
    pairs(f"{tag} moe_router_fwd sigmoid / softmax / copy of h ({h.numel() * 2 >> 20} MiB)", ("sigmoid", "softmax", "copy"),
          [sig, lambda: nat.moe_router_fwd(h, w, k, True), lambda: dst.copy_(h)], n, reps, emit)
    idx, wts, lse, logits, part = sig()
    counts = nat.moe_router_finish(part, T, k, AUX, ZC)[0]
    one = torch.ones(1, device="cuda")
    pairs(f"{tag} moe_router_bwd sigmoid / softmax", ("sigmoid", "softmax"),
          [lambda: nat.moe_router_bwd(logits, lse, idx, wts, dwts, one, counts, True, AUX, ZC, True, SCALE),
           lambda: nat.moe_router_bwd(logits, lse, idx, wts, dwts, one, counts, True, AUX, ZC)], n, reps, emit)

    def fwd(fn):
        with torch.no_grad():
            fn(h, w, k, True, AUX, ZC, **kw)

    hg, wg = h.clone().requires_grad_(), w.clone().requires_grad_()

    def both(fn):
        hg.grad = wg.grad = None
        _, wts, aux = fn(hg, wg, k, True, AUX, ZC, **kw)
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
    assert torch.cuda.is_available(), "probe_moe_router_sigmoid needs a GPU"
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
