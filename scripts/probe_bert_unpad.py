"""Unpadded BERT (BertForMLM.forward(..., seqs=)) against the right-padded path (lengths=) on one batch:
B 1024, S 128, BERT-base, dropout 0.1, lengths uniform in [16, 128] from a seed -- the batch of
probe_bert_attn.py --padded.

  attention alone   the packed call against the key_lengths call on the same sequences, and with every
                    length = S (the same work either way: the cost of the packed addressing)
  one BertLayer     forward + backward, seqs= against key_lengths=
  BertForMLM        12 layers, and 0 layers (embeddings + MLM head at the masked positions alone),
                    forward + backward, seqs= against lengths=

All variants of a group alternate in one process; each figure is the median of ``--rounds`` windows of
calls between device events, with the min - max of the windows beside it.  The table goes to ``--out``."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ps_amd.models.transformer import BertConfig, BertForMLM, BertLayer, mlm_batch  # noqa: E402
from ps_amd.ops import native  # noqa: E402
from ps_amd.ops.transformer import attention_qkv, pack_seqs, repad, unpad  # noqa: E402

DEV = "cuda"


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


def table(ms, lines):
    lines.append(f"{'variant':34s} {'median':>9s} {'min':>9s} {'max':>9s} {'spread':>7s}")
    for k, v in ms.items():
        m = statistics.median(v)
        lines.append(f"{k:34s} {m:9.4f} {min(v):9.4f} {max(v):9.4f} {(max(v) - min(v)) / m * 100:6.1f}%")
    lines.append("")


def ratio(ms, a, b, what, lines, tokens=None):
    ma, mb = statistics.median(ms[a]), statistics.median(ms[b])
    tail = "" if tokens is None else f"; the token ratio T / (B * S) is {tokens:.3f}"
    lines.append(f"{what}: {a} takes {ma / mb:.3f} of {b}{tail}.")


def same_work(ms, a, b, what, lines):
    u, f = ms[b], ms[a]
    diff = statistics.median(f) - statistics.median(u)
    spread = max(max(u) - min(u), max(f) - min(f))
    verdict = "COSTS MORE than" if diff > spread else "is FASTER by more than" if diff < -spread else "is within"
    lines.append(f"{what}: {a} minus {b}: {diff:+.4f} ms ({diff / statistics.median(u) * 100:+.1f}%); it {verdict} the "
                 f"run-to-run spread of {spread:.4f} ms (the larger min - max of the two).")


def attention(args, lens, lines):
    B, S, H, D, p = args.batch, 128, 12, 64, 0.1
    gen = torch.Generator().manual_seed(args.seed + 1)
    pq = (torch.randn(B, S, 3 * H * D, generator=gen) * 0.5).to(DEV).bfloat16()
    pg = torch.randn(B, S, H * D, generator=gen).to(DEV).bfloat16()
    variants, check = {}, []
    for tag, ln in (("", lens), (", lengths = S", torch.full_like(lens, S))):
        seqs = pack_seqs(ln, S, DEV)
        klen = ln.to(DEV, torch.int32)
        q = unpad(pq, seqs).contiguous().requires_grad_(True)
        g = unpad(pg, seqs).contiguous()
        qp = repad(q.detach(), seqs).contiguous().requires_grad_(True)  # zero pad rows
        gp = repad(g, seqs).contiguous()
        fp = (lambda q, seqs: lambda: attention_qkv(q, H, p, seqs=seqs))(q, seqs)
        fk = (lambda qp, klen: lambda: attention_qkv(qp, H, p, key_lengths=klen))(qp, klen)
        variants[f"packed{tag}, fwd"] = fp
        variants[f"key_lengths{tag}, fwd"] = fk
        variants[f"packed{tag}, fwd+bwd"] = (lambda f, q, g: lambda: torch.autograd.grad(f(), q, g))(fp, q, g)
        variants[f"key_lengths{tag}, fwd+bwd"] = (lambda f, q, g: lambda: torch.autograd.grad(f(), q, g))(fk, qp, gp)
        with torch.no_grad():  # the outputs at the timed size: bitwise the key_lengths call's valid rows
            o0, l0 = native().attn_fwd(q.detach(), H, p, 99, None, seqs.cu, seqs.max_len)
            d0 = native().attn_bwd(q.detach(), o0, g, l0, H, p, 99, None, seqs.cu, seqs.max_len)
            o1, l1 = native().attn_fwd(qp.detach(), H, p, 99, klen)
            d1 = native().attn_bwd(qp.detach(), o1, gp, l1, H, p, 99, klen)
            check.append(torch.equal(o0, unpad(o1, seqs)) and torch.equal(d0, unpad(d1, seqs))
                         and torch.equal(l0, unpad(l1.transpose(1, 2), seqs).t()))
            del o0, l0, d0, o1, l1, d1
    ms = alternate(variants, args.rounds, args.reps)
    lines += ["## 2. Attention alone (H 12, d 64, dropout 0.1); ms per call", ""]
    table(ms, lines)
    for kind in ("fwd", "fwd+bwd"):
        ratio(ms, f"packed, {kind}", f"key_lengths, {kind}", kind, lines)
    for kind in ("fwd", "fwd+bwd"):
        same_work(ms, f"packed, lengths = S, {kind}", f"key_lengths, lengths = S, {kind}", kind, lines)
    lines += [f"packed out, lse, dqkv bitwise the key_lengths call's valid rows at this size (p = {p}, one seed): "
              f"probe lengths {check[0]}, lengths = S {check[1]}.", ""]


def layer_and_model(args, lens, lines):
    B, S = args.batch, 128
    torch.manual_seed(0)
    ids, labels, positions, lengths, seqs = mlm_batch(B, S, seed=args.seed, with_positions=True, lengths=lens,
                                                      device=DEV, packed=True)
    klen = lengths.to(torch.int32)
    tokens = seqs.total / (B * S)
    c = BertConfig()
    layer = BertLayer(c).to(DEV).bfloat16().train()
    xp = torch.randn(B, S, c.hidden, device=DEV).bfloat16().requires_grad_(True)
    xu = unpad(xp.detach(), seqs).contiguous().requires_grad_(True)
    gp, gu = torch.randn_like(xp), torch.randn_like(xu)

    def run_layer(x, g, **kw):
        layer.zero_grad(set_to_none=True)
        layer(x, **kw).backward(g)

    ms = alternate({"BertLayer, key_lengths=": lambda: run_layer(xp, gp, key_lengths=klen),
                    "BertLayer, seqs=": lambda: run_layer(xu, gu, seqs=seqs)}, args.rounds, args.layer_reps)
    lines += ["## 3. One BertLayer and the whole BertForMLM, forward + backward; ms per call", ""]
    table(ms, lines)
    ratio(ms, "BertLayer, seqs=", "BertLayer, key_lengths=", "layer", lines, tokens)
    lines.append("")
    del layer, xp, xu, gp, gu
    res = {}
    for nl in (12, 0):
        m = BertForMLM(BertConfig(layers=nl)).to(DEV).bfloat16().train()

        def run_model(**kw):
            m.zero_grad(set_to_none=True)
            m(ids, labels, positions, **kw).backward()

        res.update(alternate({f"BertForMLM {nl:2d} layers, lengths=": lambda: run_model(lengths=klen),
                              f"BertForMLM {nl:2d} layers, seqs=": lambda: run_model(seqs=seqs)},
                             args.rounds, args.model_reps))
        del m
    table(res, lines)
    ratio(res, "BertForMLM 12 layers, seqs=", "BertForMLM 12 layers, lengths=", "model", lines, tokens)
    ratio(res, "BertForMLM  0 layers, seqs=", "BertForMLM  0 layers, lengths=", "embeddings + head alone", lines, tokens)
    med = {k: statistics.median(v) for k, v in res.items()}
    lp = med["BertForMLM 12 layers, lengths="] - med["BertForMLM  0 layers, lengths="]
    ls = med["BertForMLM 12 layers, seqs="] - med["BertForMLM  0 layers, seqs="]
    lines += [f"the 12 layers alone (12 layers minus 0 layers): lengths= {lp:.3f} ms, seqs= {ls:.3f} ms, ratio {ls / lp:.3f}.", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--layer-reps", type=int, default=20)
    ap.add_argument("--model-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "bert_unpad_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_bert_unpad: needs a GPU")
    S = 128
    lens = torch.randint(16, S + 1, (args.batch,), generator=torch.Generator().manual_seed(args.seed))
    T = int(lens.sum())
    lines = [f"BERT-base on a right-padded batch, unpadded: B {args.batch}, S {S}, dropout 0.1; lengths uniform in [16, {S}]",
             f"(seed {args.seed}: mean {lens.float().mean().item():.1f}, {int((lens == S).sum())} full), T = {T} of "
             f"{args.batch * S} tokens ({T / (args.batch * S):.3f}); {torch.cuda.get_device_name(0)}.",
             f"median of {args.rounds} alternated windows between device events (after warm-up) of {args.reps} calls "
             f"(attention), {args.layer_reps} (layer), {args.model_reps} (model); min - max of the windows.", ""]
    attention(args, lens, lines)
    layer_and_model(args, lens, lines)
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
