"""Time the fused mixture-of-experts FFN (ops/moe.py, route ``moe_ffn``) against the torch composition ``_moe_ref``.

Alternated pairs in one process after a warm-up of both, device events around each call.  Per shape and routing:
forward and forward + backward times of every pair, the achieved TF/s of the fused route over the useful FLOPs
(6 T k D F forward, three times that with the backward; pad rows not counted) and the pad-row fraction of the
row tiles the GEMMs run.  ``--model`` adds one LlamaForCausalLM forward + backward on a 2-layer Mixtral-width
model, route on against off.  Needs a GPU.

    python scripts/probe_moe.py [--tokens 16384] [--pairs 5] [--model] [--out profiles/moe_probe.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ps_amd import knobs  # noqa: E402
from ps_amd.models.transformer import LlamaConfig, LlamaForCausalLM  # noqa: E402
from ps_amd.ops import moe as M  # noqa: E402

SHAPES = {"mixtral": (8, 2, 4096, 14336), "fine": (64, 8, 2048, 1024)}  # E, k, D, F


def routing(kind, T, E, k, g):
    """uniform: k distinct experts per token at random.  skewed: expert e drawn with weight 1 / (e + 1)."""
    p = torch.ones(E) if kind == "uniform" else 1.0 / torch.arange(1, E + 1)
    return torch.multinomial(p.expand(T, E), k, replacement=False, generator=g)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def probe(name, kind, T, pairs, emit):
    E, k, D, F = SHAPES[name]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(T, D, generator=g).bfloat16().cuda().requires_grad_()
    w13 = (torch.randn(E, 2 * F, D, generator=g) / D ** 0.5).bfloat16().cuda().requires_grad_()
    w2 = (torch.randn(E, D, F, generator=g) / F ** 0.5).bfloat16().cuda().requires_grad_()
    wts = torch.rand(T, k, generator=g).cuda().requires_grad_()
    dout = torch.randn(T, D, generator=g).bfloat16().cuda()
    idx = routing(kind, T, E, k, g).cuda()
    counts = M.moe_plan(idx, E)[4].cpu()
    pad = 1.0 - counts.sum().item() / (((counts + 127) // 128).sum().item() * 128)

    def fwd(fn):
        with torch.no_grad():
            fn(x, idx, wts, w13, w2)

    def both(fn):
        for t in (x, w13, w2, wts):
            t.grad = None
        fn(x, idx, wts, w13, w2).backward(dout)

    for run in (fwd, both):
        for fn in (M._MoeFFN.apply, M._moe_ref):  # warm-up of both
            run(fn), run(fn)
        torch.cuda.synchronize()
        flops = 6.0 * T * k * D * F * (1 if run is fwd else 3)
        for i in range(pairs):
            tf, tr = timed(lambda: run(M._MoeFFN.apply)), timed(lambda: run(M._moe_ref))
            emit(f"{name} {kind} T={T} E={E} k={k} D={D} F={F} {'fwd' if run is fwd else 'fwd+bwd'} pair {i}: "
                 f"fused {tf:.3f} ms ({flops / tf / 1e9:.1f} TF/s useful) composition {tr:.3f} ms "
                 f"ratio {tf / tr:.3f} pad rows {pad:.4f}")


def model_probe(T, pairs, emit):
    c = LlamaConfig.mixtral_8x7b()
    c.layers = 2
    M.ROUTE_MAX_ROWS_PER_EXPERT = 1 << 30  # "route on" is the fused kernels at this width too
    torch.manual_seed(0)
    m = LlamaForCausalLM(c).cuda().bfloat16()
    ids = torch.randint(0, c.vocab, (T // 2048, 2048), device="cuda")

    def step(off):
        os.environ[knobs.ENV] = "moe_ffn" if off else ""
        m.zero_grad(set_to_none=True)
        m(ids, labels=ids).backward()

    for off in (False, True, False, True):
        step(off)
    torch.cuda.synchronize()
    for i in range(pairs):
        on, off = timed(lambda: step(False)), timed(lambda: step(True))
        emit(f"llama 2-layer mixtral width, {ids.shape[0]} x 2048 tokens, fwd+bwd pair {i}: route on {on:.2f} ms "
             f"off {off:.2f} ms ratio {on / off:.3f}")
    os.environ[knobs.ENV] = ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "probe_moe needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for name in SHAPES:
        for kind in ("uniform", "skewed"):
            probe(name, kind, a.tokens, a.pairs, emit)
    if a.model:
        model_probe(a.tokens, a.pairs, emit)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
