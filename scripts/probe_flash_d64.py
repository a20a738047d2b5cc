"""Causal GQA flash attention at head dim 64 (csrc/kernels/flash_attn_d64.hip) against the SDPA route on
the Llama-3.2-1B attention shape (32 q / 8 kv heads x 64, S 4096) at B 4 and B 8, and on packed rows of
eight 512-token documents at B 4: forward and backward of attention_causal_gqa on each route.  The two
routes alternate inside one process, pair after pair; each line reports every pair, the median, the
min - max spread and the achieved TF/s (causal FLOPs: forward 2 B H S^2 D, backward 2.5 x), so a
difference can be held against the spread.  --e2e adds LlamaForCausalLM(LlamaConfig.llama32_1b())
forward + backward at 4 x 4096 with the route on and off (a single-box number).

    python scripts/probe_flash_d64.py [pairs] [--e2e]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ps_amd.ops.transformer import attention_causal_gqa, doc_bounds  # noqa: E402

H, KV, S, D = 32, 8, 4096, 64
CASES = {"b4": (4, None), "b8": (8, None), "b4_docs_8x512": (4, [512] * 8)}
ROUTES = {"flash": "", "sdpa": "flash_attn"}  # PS_AMD_DISABLE


def bench(fn, it=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3


def op_runs(B, docs):
    """{route: (forward, backward)} on one set of inputs; the backward replays a retained graph."""
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(B, h, S, D, generator=g).bfloat16().cuda().requires_grad_() for h in (H, KV, KV))
    dout = torch.randn(B, S, H * D, generator=g).bfloat16().cuda()
    bounds = None if docs is None else doc_bounds(torch.repeat_interleave(torch.arange(len(docs)), torch.tensor(docs)).expand(B, S).cuda())
    runs = {}
    for route, off in ROUTES.items():
        def fwd(off=off):
            os.environ["PS_AMD_DISABLE"] = off
            with torch.no_grad():
                return attention_causal_gqa(q, k, v, doc_bounds=bounds)
        os.environ["PS_AMD_DISABLE"] = off
        out = attention_causal_gqa(q, k, v, doc_bounds=bounds)
        runs[route] = (fwd, lambda out=out: torch.autograd.grad(out, (q, k, v), dout, retain_graph=True))
    return runs


def report(name, what, times, flops=None):
    for route, ts in times.items():
        rec = {"case": name, "what": what, "route": route, "us_pairs": [round(t, 1) for t in ts],
               "us_median": round(statistics.median(ts), 1), "us_min_max": [round(min(ts), 1), round(max(ts), 1)]}
        if flops:
            rec["tflops_median"] = round(flops / statistics.median(ts) / 1e6, 1)
        print(json.dumps(rec), flush=True)
    print(json.dumps({"case": name, "what": what, "flash_at_or_below_sdpa_in_every_pair":
                      all(a <= b for a, b in zip(times["flash"], times["sdpa"]))}), flush=True)


def e2e(pairs):
    from ps_amd.models.transformer import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig.llama32_1b()).cuda().to(torch.bfloat16)
    ids = torch.randint(0, 128256, (4, S), device="cuda")

    def step(off):
        os.environ["PS_AMD_DISABLE"] = off
        m(ids, ids.roll(-1, 1)).backward()
        m.zero_grad(set_to_none=True)

    for off in ROUTES.values():
        step(off)
        step(off)
    times = {r: [] for r in ROUTES}
    for _ in range(pairs):
        for route, off in ROUTES.items():
            times[route].append(bench(lambda: step(off), it=3))
    report("llama32_1b fwd+bwd 4x4096, single box", "step", times)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    pairs = int(args[0]) if args else 7
    for name, (B, docs) in CASES.items():
        runs = op_runs(B, docs)
        for fwd, bwd in runs.values():  # warm-up: every kernel, every shape
            for _ in range(3):
                fwd()
                bwd()
        torch.cuda.synchronize()
        tf, tb = {r: [] for r in runs}, {r: [] for r in runs}
        for _ in range(pairs):
            for route, (fwd, bwd) in runs.items():
                tf[route].append(bench(fwd))
                tb[route].append(bench(bwd))
        n = S * S if docs is None else sum(d * d for d in docs)
        flops = 2.0 * B * H * n * D
        report(name, "fwd", tf, flops)
        report(name, "bwd", tb, 2.5 * flops)
    if "--e2e" in sys.argv:
        e2e(pairs)


if __name__ == "__main__":
    main()
