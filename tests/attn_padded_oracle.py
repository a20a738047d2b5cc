"""fp64 oracles of the fused short-sequence attention kernel (csrc/kernels/attention.hip) on a
right-padded batch: per-sequence key lengths L_b, keys >= L_b out of every softmax (SDPA with a
key-padding mask).  The formulas and the bf16 rounding points (rounded=True: the yardstick) are those
of attn_oracle.short_fwd / short_bwd; the only difference is that the scores of keys >= L_b are
filled with -inf.  All S query rows are ordinary rows.  Imported by test_attention_padded_cpu.py
and test_attention_padded_gpu.py.
"""
import torch

from . import attn_oracle as ao


def key_pad(lengths, s):
    """[B, 1, 1, S] bool, True where key j >= L_b."""
    lens = torch.as_tensor(lengths, dtype=torch.int64).cpu()
    return (torch.arange(s)[None, :] >= lens[:, None])[:, None, None, :]


def _scores(q, k, lengths):
    sc = q @ k.transpose(-1, -2) * ao.SHORT_SCALE
    return sc.masked_fill(key_pad(lengths, sc.shape[-1]), float("-inf"))


def short_fwd_len(qkv, heads, lengths, keep=None, p=0.0, rounded=False):
    """qkv [B, S, 3 * H * 64], lengths [B], keep [B * H, S, S] or None -> out [B, S, H * 64],
    lse [B, H, S] (over the valid keys)."""
    b, s, _ = qkv.shape
    q, k, v = ao._split(qkv, heads)
    sc = _scores(q, k, lengths)
    lse = torch.logsumexp(sc, -1)
    pr = torch.exp(sc - lse[..., None])
    kf = ao._keepf(keep, b, heads, s, p)
    if kf is not None:
        pr = pr * kf
    o = ao._r(pr, rounded) @ v
    return ao._r(o.transpose(1, 2).reshape(b, s, heads * ao.SHORT_D), rounded), lse


def short_bwd_len(qkv, out, dout, lse, heads, lengths, keep=None, p=0.0, rounded=False):
    """-> dqkv [B, S, 3 * H * 64], from the out and lse that are passed in; dk and dv rows >= L_b
    are zeros."""
    b, s, _ = qkv.shape
    q, k, v = ao._split(qkv, heads)
    do = dout.double().view(b, s, heads, ao.SHORT_D).transpose(1, 2)
    o = out.double().view(b, s, heads, ao.SHORT_D).transpose(1, 2)
    pr = torch.exp(_scores(q, k, lengths) - lse.double()[..., None])
    dp = do @ v.transpose(-1, -2)
    pd = pr
    kf = ao._keepf(keep, b, heads, s, p)
    if kf is not None:
        pd, dp = pr * kf, dp * kf
    ds = ao._r(pr * (dp - (do * o).sum(-1, keepdim=True)), rounded)
    dv = ao._r(pd, rounded).transpose(-1, -2) @ do
    dq = ds @ k * ao.SHORT_SCALE
    dk = ds.transpose(-1, -2) @ q * ao.SHORT_SCALE
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(b, s, 3 * heads * ao.SHORT_D)
    return ao._r(dqkv, rounded)
