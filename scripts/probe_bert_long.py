"""The chunked BERT attention kernels (csrc/kernels/attention_long.hip, 128 < S <= 512) against the SDPA
route (PS_AMD_DISABLE=fused_attn) they replace, at B * S = 32768 tokens, H 12, d 64, dropout 0.1:

  attention alone   forward and forward + backward at S in {256, 384, 512}: dense, key_lengths and packed
                    (seqs=), lengths uniform in [64, S] from a seed; the SDPA route of the packed call is
                    repad / SDPA with the key mask / unpad
  BertForMLM        BERT-base, forward + backward at S = 512 (B 64), both routes
  resources         VGPR / AGPR / LDS / scratch of every kernel, from the compiler's
                    -Rpass-analysis=kernel-resource-usage remarks on the source that was built

Both routes of a group alternate in one process; each figure is the median of ``--rounds`` windows of calls
between device events (after warm-up), with the min - max of the windows beside it.  A pair's verdict allows
the larger of the two spreads.  The outputs of the two routes are compared at the timed size (p = 0).  The
table goes to ``--out``; ops/transformer.py's LONG_ROUTE_MAX_S follows the verdicts."""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ps_amd.models.transformer import BertConfig, BertForMLM, mlm_batch  # noqa: E402
from ps_amd.ops.transformer import attention_qkv, pack_seqs, unpad  # noqa: E402

DEV = "cuda"
H, D, P = 12, 64, 0.1


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(variants, rounds, reps):
    for fn in variants.values():  # warm-up: every variant, more than once
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):  # one window of every variant per round
        for k, fn in variants.items():
            ms[k].append(window(fn, reps))
    return ms


def on_route(route, fn):
    """fn with PS_AMD_DISABLE set for the call (the variable is read on every query)."""
    def run():
        os.environ["PS_AMD_DISABLE"] = "" if route == "long" else "fused_attn"
        try:
            return fn()
        finally:
            os.environ["PS_AMD_DISABLE"] = ""
    return run


def table(ms, lines):
    lines.append(f"{'variant':40s} {'median':>9s} {'min':>9s} {'max':>9s} {'spread':>7s}")
    for k, v in ms.items():
        m = statistics.median(v)
        lines.append(f"{k:40s} {m:9.4f} {min(v):9.4f} {max(v):9.4f} {(max(v) - min(v)) / m * 100:6.1f}%")
    lines.append("")


def verdict(ms, what, lines):
    """long against sdpa for one (layout, kind): the difference of the medians beside the larger spread."""
    lo, sd = ms[f"{what}, long"], ms[f"{what}, sdpa"]
    ml, msd = statistics.median(lo), statistics.median(sd)
    spread = max(max(lo) - min(lo), max(sd) - min(sd))
    word = "AT OR BELOW" if ml <= msd + spread else "ABOVE"
    lines.append(f"{what}: long {ml:.4f} ms, sdpa {msd:.4f} ms, long / sdpa {ml / msd:.3f}; spread {spread:.4f} ms: "
                 f"long is {word} the SDPA time.")
    return ml <= msd + spread


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def attention(args, S, lines):
    B = args.tokens // S
    gen = torch.Generator().manual_seed(args.seed + S)
    lens = torch.randint(64, S + 1, (B,), generator=gen)
    seqs = pack_seqs(lens, S, DEV)
    klen = lens.to(DEV, torch.int32)
    pq = (torch.randn(B, S, 3 * H * D, generator=gen) * 0.5).to(DEV).bfloat16()
    pg = torch.randn(B, S, H * D, generator=gen).to(DEV).bfloat16()
    q = {"dense": pq.clone().requires_grad_(True), "key_lengths": pq.clone().requires_grad_(True),
         "packed": unpad(pq, seqs).contiguous().requires_grad_(True)}
    g = {"dense": pg, "key_lengths": pg, "packed": unpad(pg, seqs).contiguous()}
    kw = {"dense": {}, "key_lengths": dict(key_lengths=klen), "packed": dict(seqs=seqs)}
    variants = {}
    for layout in q:
        for route in ("long", "sdpa"):
            f = (lambda layout: lambda: attention_qkv(q[layout], H, P, **kw[layout]))(layout)
            fb = (lambda f, layout: lambda: torch.autograd.grad(f(), q[layout], g[layout]))(f, layout)
            variants[f"{layout}, fwd, {route}"] = on_route(route, f)
            variants[f"{layout}, fwd+bwd, {route}"] = on_route(route, fb)
    lines += [f"## Attention alone, S {S}, B {B} ({B * S} tokens; lengths uniform in [64, {S}]: mean "
              f"{lens.float().mean().item():.1f}, T = {seqs.total}, max_len {seqs.max_len}); ms per call", ""]
    # the two routes' results at this size, without dropout (their masks are different draws)
    for layout in q:
        res = []
        for route in ("long", "sdpa"):
            def once():
                y = attention_qkv(q[layout], H, 0.0, **kw[layout])
                return y.detach(), torch.autograd.grad(y, q[layout], g[layout])[0]
            res.append(on_route(route, once)())
        lines.append(f"{layout}: long against sdpa at p = 0: rel. Frobenius error out {rel(res[0][0], res[1][0]):.2e}, "
                     f"dqkv {rel(res[0][1], res[1][1]):.2e}")
    lines.append("")
    ms = alternate(variants, args.rounds, args.reps)
    table(ms, lines)
    ok = all([verdict(ms, f"{layout}, {kind}", lines) for layout in q for kind in ("fwd", "fwd+bwd")])
    lines.append("")
    return ok


def model(args, lines):
    S = 512
    B = args.tokens // S
    torch.manual_seed(0)
    ids, labels, positions = mlm_batch(B, S, seed=args.seed, with_positions=True, device=DEV)
    m = BertForMLM(BertConfig()).to(DEV).bfloat16().train()

    def step():
        m.zero_grad(set_to_none=True)
        m(ids, labels, positions).backward()

    ms = alternate({"BertForMLM, long": on_route("long", step), "BertForMLM, sdpa": on_route("sdpa", step)},
                   args.rounds, args.model_reps)
    lines += [f"## BertForMLM (BERT-base, dropout 0.1), forward + backward, B {B}, S {S}; ms per step", ""]
    table(ms, lines)
    verdict(ms, "BertForMLM", lines)
    lines.append("")


def resources(lines):
    """The compiler's own figures for the kernels of attention_long.hip (needs hipcc, no GPU)."""
    lines += ["## Kernel resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)", ""]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "csrc", "kernels", "attention_long.hip")
    with tempfile.TemporaryDirectory() as tmp:
        try:
            r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "csrc", "include"),
                                "-c", src, "-o", os.path.join(tmp, "a.o"), "-Rpass-analysis=kernel-resource-usage"],
                               capture_output=True, text=True, timeout=300)
        except (OSError, subprocess.TimeoutExpired) as e:
            lines += [f"not measured: {e}", ""]
            return
    name, row = None, {}
    keys = {"VGPRs": "VGPR", "AGPRs": "AGPR", "ScratchSize [bytes/lane]": "scratch B/lane",
            "Occupancy [waves/SIMD]": "waves/SIMD", "LDS Size [bytes/block]": "LDS B/block"}
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", ln)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            name, row = v, {}
        elif k in keys:
            row[keys[k]] = v
            if k == "LDS Size [bytes/block]" and name:
                short = re.search(r"attn_long_(fwd|dq|dkv)_kernelILb([01])E", name)
                tag = f"attn_long_{short.group(1)}_kernel<DROP={short.group(2)}>" if short else name
                lines.append(f"{tag:34s} " + ", ".join(f"{a} {b}" for a, b in row.items()))
    if r.returncode != 0:
        lines.append(f"hipcc exit {r.returncode}: not measured")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model-reps", type=int, default=2)
    ap.add_argument("--resources-only", action="store_true", help="the compiler's figures alone (no GPU needed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bert_attn_long_probe.txt"))
    args = ap.parse_args()
    lines = []
    if args.resources_only:
        resources(lines)
        print("\n".join(lines))
        return
    if not torch.cuda.is_available():
        sys.exit("probe_bert_long: needs a GPU")
    lines += [f"Chunked BERT attention (attention_long.hip) against the SDPA route, H {H}, d {D}, dropout {P}; "
              f"{torch.cuda.get_device_name(0)}.",
              f"median of {args.rounds} alternated windows between device events (after warm-up) of {args.reps} calls "
              f"(attention), {args.model_reps} (model); min - max of the windows.", ""]
    ok = {S: attention(args, S, lines) for S in (256, 384, 512)}
    model(args, lines)
    lines += ["## Route", "",
              "S at which every attention pair (3 layouts x fwd, fwd+bwd) is at or below the SDPA time within the spread: "
              + (", ".join(str(S) for S, v in ok.items() if v) or "none") + ".", ""]
    resources(lines)
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
