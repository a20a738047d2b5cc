"""BERT-base attention (B 1024, S 128, H 12, d 64; dropout 0.1) alone: fwd / bwd ms and the HBM rate
over qkv + out (+ dout, dqkv) -- to tell kernel headroom from in-step contention.

``--padded``: the same shape as a right-padded batch (lengths uniform in [16, 128] from a seed).
The fused kernels with key_lengths against attention_qkv with the equivalent mask (SDPA: all there
was for such a batch before key_lengths), and -- the cost of the masking code -- the unpadded fused
call against the fused call with every length = S.  All variants alternate in one process; each
figure is the median of ``--rounds`` windows of ``--reps`` calls between device events, with the
min - max of the windows beside it.  The table goes to ``--out``."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ps_amd.ops import native  # noqa: E402
from ps_amd.ops.transformer import attention_qkv  # noqa: E402


def t(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    B, S, H, D = 1024, 128, 12, 64
    for p in (0.1, 0.0):
        qkv = (torch.randn(B, S, 3 * H * D, device="cuda") * 0.5).bfloat16().requires_grad_(True)
        out = attention_qkv(qkv, H, p, None)
        g = torch.randn_like(out)
        tf = t(lambda: attention_qkv(qkv, H, p, None))
        tfb = t(lambda: torch.autograd.grad(attention_qkv(qkv, H, p, None), qkv, g))
        nb = qkv.numel() * 2
        print(json.dumps({"dropout": p, "fwd_ms": round(tf, 4), "fwd_TBs": round((nb + out.numel() * 2) / tf / 1e9, 2),
                          "fwd_bwd_ms": round(tfb, 4), "bwd_ms": round(tfb - tf, 4),
                          "bwd_TBs": round((2 * nb + 2 * out.numel() * 2) / (tfb - tf) / 1e9, 2)}), flush=True)


def padded(args):
    B, S, H, D, p = args.batch, 128, 12, 64, 0.1
    gen = torch.Generator().manual_seed(args.seed)
    lens = torch.randint(16, S + 1, (B,), generator=gen)
    qkv = (torch.randn(B, S, 3 * H * D, generator=gen) * 0.5).to("cuda").bfloat16().requires_grad_(True)
    g = torch.randn(B, S, H * D, generator=gen).to("cuda").bfloat16()
    klen = lens.to("cuda", torch.int32)
    full = torch.full_like(klen, S)
    mask = (torch.arange(S, device="cuda")[None, :] < klen[:, None])[:, None, None, :]

    calls = {
        "fused, key_lengths": lambda: attention_qkv(qkv, H, p, key_lengths=klen),
        "SDPA, key mask": lambda: attention_qkv(qkv, H, p, mask=mask),
        "fused, unpadded": lambda: attention_qkv(qkv, H, p),
        "fused, lengths = S": lambda: attention_qkv(qkv, H, p, key_lengths=full),
    }
    variants = {}
    for name, fn in calls.items():
        variants[(name, "fwd")] = fn
        variants[(name, "fwd+bwd")] = (lambda f: lambda: torch.autograd.grad(f(), qkv, g))(fn)

    # the outputs at the timed size, before any timing: p = 0 so the two paths draw no masks
    with torch.no_grad():
        a = attention_qkv(qkv, H, 0.0, key_lengths=klen).float()
        b = attention_qkv(qkv, H, 0.0, mask=mask).float()
        rel = ((a - b).norm() / b.norm()).item()
        o0, l0 = native().attn_fwd(qkv.detach(), H, p, 99)
        o1, l1 = native().attn_fwd(qkv.detach(), H, p, 99, full)
        d0 = native().attn_bwd(qkv.detach(), o0, g, l0, H, p, 99)
        d1 = native().attn_bwd(qkv.detach(), o1, g, l1, H, p, 99, full)
        same = torch.equal(o0, o1) and torch.equal(l0, l1) and torch.equal(d0, d1)
        del a, b, o0, o1, l0, l1, d0, d1

    for fn in variants.values():  # warm-up: every variant, more than once
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):  # alternated: one window of every variant per round
        for k, fn in variants.items():
            ms[k].append(t(fn, args.reps))

    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [f"BERT-base attention on a right-padded batch: B {B}, S {S}, H {H}, d {D}, dropout {p}; lengths uniform in",
             f"[16, {S}] (seed {args.seed}: mean {lens.float().mean().item():.1f}, {int((lens == S).sum())} full); "
             f"{torch.cuda.get_device_name(0)}.",
             f"ms per call: median of {args.rounds} alternated windows of {args.reps} calls between device events "
             f"(after warm-up), min - max of the windows.", "",
             f"{'variant':22s} {'pass':8s} {'median':>8s} {'min':>8s} {'max':>8s} {'spread':>7s}"]
    for (name, kind), v in ms.items():
        lines.append(f"{name:22s} {kind:8s} {med[(name, kind)]:8.4f} {min(v):8.4f} {max(v):8.4f} "
                     f"{(max(v) - min(v)) / med[(name, kind)] * 100:6.1f}%")
    lines.append("")
    for kind in ("fwd", "fwd+bwd"):
        fl, sd, un = (med[(n, kind)] for n in ("fused, key_lengths", "SDPA, key mask", "fused, unpadded"))
        lines.append(f"{kind}: SDPA with the key mask takes {sd / fl:.2f}x the time of the fused call with key_lengths, "
                     f"which takes {fl / un:.2f} of the unpadded fused call's (it skips the padded key blocks).")
    lines.append("")
    for kind in ("fwd", "fwd+bwd"):  # the cost of the masking code: lengths = S against no lengths
        u, f = ms[("fused, unpadded", kind)], ms[("fused, lengths = S", kind)]
        diff = statistics.median(f) - statistics.median(u)
        spread = max(max(u) - min(u), max(f) - min(f))
        verdict = "COSTS MORE than" if diff > spread else "is FASTER by more than" if diff < -spread else "is within"
        pct = diff / statistics.median(u) * 100
        lines.append(f"{kind}: lengths = S minus the unpadded call: {diff:+.4f} ms ({pct:+.1f}%); "
                     f"it {verdict} the run-to-run spread of {spread:.4f} ms (the larger min - max of the two).")
    lines += ["", f"outputs at this size: fused key_lengths vs SDPA key mask (p = 0), relative Frobenius error {rel:.2e};",
              f"lengths = S vs no lengths (p = {p}, one seed): out, lse, dqkv bitwise equal: {same}."]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--padded", action="store_true")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "bert_attn_padded_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_bert_attn: needs a GPU")
    padded(a) if a.padded else main()
