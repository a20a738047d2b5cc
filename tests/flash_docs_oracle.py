"""fp64 oracles of causal GQA flash attention over packed documents (the DOCS instantiations of
csrc/kernels/flash_attn.hip): tests/attn_oracle.py's flash_fwd / flash_bwd with the document mask
added to flash_scores -- query i of row b sees key j iff doc_start[b, i] <= j <= i -- and the same
rounded=True yardstick variant (bf16 at the kernels' rounding points and nowhere else).  Plain
torch on the CPU; imported by test_flash_docs_cpu.py and test_flash_docs_gpu.py.
"""
import torch

from . import attn_oracle as ao


def doc_ids_from_lengths(rows, dtype=torch.int64):
    """Per-row lists of document lengths (every list with the same sum S) -> doc_ids [B, S]: the
    documents of a row are numbered 0, 1, ..."""
    ids = [torch.repeat_interleave(torch.arange(len(r)), torch.tensor(r)) for r in rows]
    assert len({int(i.numel()) for i in ids}) == 1, "every row sums to the same S"
    return torch.stack(ids).to(dtype)


def doc_spans(lengths):
    """One row's document lengths -> [(first, one past last), ...]."""
    spans, at = [], 0
    for n in lengths:
        spans.append((at, at + n))
        at += n
    return spans


def doc_mask(doc_ids):
    """[B, 1, S, S] bool, True where query i may NOT see key j: j > i, or another document.  Written
    from the definition (same run of equal ids), not from the ops' cummax formulas."""
    ids = doc_ids.long()
    B, S = ids.shape
    run = torch.cat([torch.zeros(B, 1, dtype=torch.long), (ids[:, 1:] != ids[:, :-1]).long().cumsum(1)], dim=1)
    other = run[:, :, None] != run[:, None, :]
    return (other | torch.ones(S, S, dtype=torch.bool).triu(1))[:, None]


def flash_docs_scores(q, k, doc_ids):
    """Scaled fp64 scores [B, H, S, S], -inf where the causal or the document mask hides the key."""
    return ao.flash_scores(q, k).masked_fill(doc_mask(doc_ids), float("-inf"))


def flash_docs_fwd(q, k, v, doc_ids, rounded=False):
    """q [B, H, S, 128], k / v [B, KV, S, 128], doc_ids [B, S] -> out [B, S, H * 128], lse [B, H, S]."""
    B, H, S, D = q.shape
    G = H // k.shape[1]
    sc = flash_docs_scores(q, k, doc_ids)
    lse = torch.logsumexp(sc, -1)
    p = ao._r(torch.exp(sc - lse[..., None]), rounded)
    o = p @ v.double().repeat_interleave(G, 1)
    return ao._r(o.transpose(1, 2).reshape(B, S, H * D), rounded), lse


def flash_docs_bwd(q, k, v, out, dout, lse, doc_ids, rounded=False):
    """-> dq [B, H, S, 128], dk, dv [B, KV, S, 128], from the out and lse that are passed in."""
    B, H, S, D = q.shape
    KV = k.shape[1]
    G = H // KV
    qd = q.double()
    kk, vv = k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    do = dout.double().view(B, S, H, D).transpose(1, 2)
    o = out.double().view(B, S, H, D).transpose(1, 2)
    p = torch.exp(flash_docs_scores(q, k, doc_ids) - lse.double()[..., None])
    dsum = (do * o).sum(-1, keepdim=True)
    ds = ao._r(p * (do @ vv.transpose(-1, -2) - dsum), rounded)
    dq = ds @ kk * ao.FLASH_SCALE
    dk = (ds.transpose(-1, -2) @ qd).view(B, KV, G, S, D).sum(2) * ao.FLASH_SCALE
    dv = (ao._r(p, rounded).transpose(-1, -2) @ do).view(B, KV, G, S, D).sum(2)
    return ao._r(dq, rounded), ao._r(dk, rounded), ao._r(dv, rounded)
