"""Per-head QK RMSNorm + RoPE + split: the fused kernels (csrc/kernels/rope_norm.hip) against the torch
composition (ops.transformer._rope_norm_ref) at 4 x 4096 tokens, 32 query / 8 KV heads, head dim 128 and 64,
fp32 weights: forward (no grad) and backward (autograd.grad on a retained graph) of each.  The two routes
alternate inside one process, pair after pair; each line reports every pair, the median and the min - max
spread, and the achieved GB/s of the fused kernels over the bytes they must move (forward: qkv read, q / k / v
written; backward: the three gradients and qkv read, dqkv written).  The lines, a summary and the kernels'
register / LDS / scratch figures (a device-only compile of the source with the build's flags and
-Rpass-analysis=kernel-resource-usage) are written to --out as sections 1 and 2; a section 3 already in that file
(the error figures, pasted from the GPU test's output) is kept.

    python scripts/probe_qk_norm.py [pairs] [--out profiles/qk_norm_probe.txt]
"""
import json
import os
import re
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ps_amd.ops import transformer as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, H, KV, EPS = 4, 4096, 32, 8, 1e-6
LINES = []


def emit(rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def bench(fn, it=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3


def runs(hd):
    """{route: (forward, backward)} on one set of inputs."""
    g = torch.Generator().manual_seed(hd)
    qkv = torch.randn(B, S, H + 2 * KV, hd, generator=g).bfloat16().cuda().requires_grad_()
    wq, wk = ((0.5 + torch.rand(hd, generator=g)).cuda().requires_grad_() for _ in range(2))
    cs = T.rope_table(S, hd, 1e6, "cuda")
    grads = [torch.randn(B, h, S, hd, generator=g).bfloat16().cuda() for h in (H, KV, KV)]
    out = {}
    for route, fn in (("fused", T.rope_split), ("composition", T._rope_norm_ref)):
        def fwd(fn=fn):
            with torch.no_grad():
                return fn(qkv, cs, H, KV, wq, wk, EPS)
        res = fn(qkv, cs, H, KV, wq, wk, EPS)
        if route == "fused" and "RopeNormSplit" not in res[0].grad_fn.name():
            raise RuntimeError("the fused route did not take the HIP kernels")
        out[route] = (fwd, lambda res=res: torch.autograd.grad(res, (qkv, wq, wk), grads, retain_graph=True))
    return out


def report(hd, what, times, nbytes):
    for route, ts in times.items():
        rec = {"hd": hd, "what": what, "route": route, "us_pairs": [round(t, 1) for t in ts],
               "us_median": round(statistics.median(ts), 1), "us_min_max": [round(min(ts), 1), round(max(ts), 1)]}
        if route == "fused":
            rec["gbps_median"] = round(nbytes / statistics.median(ts) / 1e3, 1)
        emit(rec)
    emit({"hd": hd, "what": what, "fused_below_composition_in_every_pair":
          all(a < b for a, b in zip(times["fused"], times["composition"]))})
    return {r: statistics.median(ts) for r, ts in times.items()}


def resource_table():
    """One line per instantiation of the two kernels, from the compiler's remarks."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/csrc/include", "-ffp-contract=fast",
           "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", f"{ROOT}/csrc/kernels/rope_norm.hip", "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    keys = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    rows = ["# kernel <head dim, weight type>           VGPR  AGPR  SGPR  scratch    LDS  waves/SIMD"]
    for blk in err.split("Function Name: ")[1:]:
        m = re.match(r"_ZN5psamd\d+(rope_norm_split_(?:fwd|bwd)_kernel)ILi(\d+)E([tf])", blk)
        if m:
            v = [re.search(re.escape(k) + r": (\d+)", blk).group(1) for k in keys]
            name = f"{m.group(1)}<{m.group(2)}, {'bf16' if m.group(3) == 't' else 'float'}>"
            rows.append(f"{name:<40}{v[0]:>7}{v[1]:>6}{v[2]:>6}{v[3]:>9}{v[4]:>7}{v[5]:>5}")
    return rows


def write_profile(path, pairs, med):
    keep = ""
    if os.path.exists(path):
        old = open(path).read()
        keep = old[old.index("## 3."):] if "## 3." in old else ""
    txt = ["# Per-head QK RMSNorm fused into RoPE + head split (csrc/kernels/rope_norm.hip) against the torch composition",
           f"# {torch.cuda.get_device_name(0)}, bf16 qkv, fp32 norm weights, {B} x {S} tokens, {H} query / {KV} KV heads",
           "# Sections 1 and 2 are written by scripts/probe_qk_norm.py; section 3 is pasted from the GPU test's output.",
           "", f"## 1. python scripts/probe_qk_norm.py {pairs}",
           "# rope_split(qkv, cs, H, KV, q_norm, k_norm) forward (no grad) and backward (autograd.grad on a retained graph):",
           "# 'fused' is _RopeNormSplit (one kernel forward; one kernel and the two colsum launches backward), 'composition'",
           "# is ops.transformer._rope_norm_ref.  The routes alternate, pair after pair, in one process; 20 calls per timing,",
           "# device events, after warm-up.  us_pairs lists every pair: the run-to-run spread is the list itself.",
           "# gbps_median: the bytes the fused kernels must move over the median; qkv is 201 MB at hd 128 and 101 MB at",
           "# hd 64, so a last-level cache can serve part of each pass -- not an HBM rate."]
    txt += LINES + ["", "# Summary (medians, us):     fused   composition"]
    txt += [f"#   hd {hd:>3}  {what:<8} {m['fused']:>10.1f} {m['composition']:>13.1f}" for (hd, what), m in med.items()]
    txt += ["", "## 2. Compiler resource figures (-Rpass-analysis=kernel-resource-usage, gfx950, the build's flags)"]
    txt += resource_table() + ["", keep.rstrip()]
    with open(path, "w") as f:
        f.write("\n".join(txt).rstrip() + "\n")


def main():
    args = sys.argv[1:]
    out = args.pop(args.index("--out") + 1) if "--out" in args else os.path.join(ROOT, "profiles", "qk_norm_probe.txt")
    args = [a for a in args if a != "--out"]
    pairs = int(args[0]) if args else 7
    med = {}
    for hd in (128, 64):
        rs = runs(hd)
        for fwd, bwd in rs.values():  # warm-up: every kernel, every shape
            for _ in range(3):
                fwd()
                bwd()
        torch.cuda.synchronize()
        tf, tb = {r: [] for r in rs}, {r: [] for r in rs}
        for _ in range(pairs):
            for route, (fwd, bwd) in rs.items():
                tf[route].append(bench(fwd))
                tb[route].append(bench(bwd))
        n = 2 * B * S * (H + 2 * KV) * hd  # bytes of qkv
        med[hd, "forward"] = report(hd, "fwd", tf, 2 * n)
        med[hd, "backward"] = report(hd, "bwd", tb, 3 * n)
    write_profile(out, pairs, med)


if __name__ == "__main__":
    main()
