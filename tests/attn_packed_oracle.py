"""fp64 oracle of the fused short-sequence attention kernels (csrc/kernels/attention.hip) on a packed
batch: the tensors hold the valid tokens only, sequence b at rows [cu[b], cu[b + 1]).  It is
attn_oracle.short_fwd / short_bwd run on each sequence alone and concatenated -- nothing in it knows of
pad rows.  The keep mask is the one the kernels draw, [B * H, S, S] at the bound S the packed call runs
with (PackedSeqs.max_len), cut to [:L, :L] per sequence.  rounded=True is the bf16 yardstick of
attn_oracle.  Imported by test_attention_packed_cpu.py and test_attention_packed_gpu.py.
"""
import torch

from . import attn_oracle as ao

# the shapes of the packed tests: ((B, S, H), lengths), S the padded length the batch came from
BATCHES = [((4, 128, 2), [128, 97, 33, 1]), ((3, 96, 3), [64, 65, 31]), ((2, 32, 1), [32, 7]), ((2, 64, 5), [63, 32]),
           ((3, 128, 2), [128, 1, 17]),  # a length-1 sequence inside; the tensor ends in a partly valid key block
           ((1, 32, 1), [5]),            # one sequence, T = 5
           ((3, 128, 2), [40, 33, 64])]  # max_len 64 < seq 128


def bounds(lengths):
    """[(start, end)] of every sequence in the packed order."""
    out, at = [], 0
    for n in lengths:
        out.append((at, at + int(n)))
        at += int(n)
    return out


def _keep(keep, b, heads, n):
    return None if keep is None else keep[b * heads:(b + 1) * heads, :n, :n].contiguous()


def packed_fwd(qkv, heads, lengths, keep=None, p=0.0, rounded=False):
    """qkv [T, 3 * H * 64], keep [B * H, S, S] or None -> out [T, H * 64], lse [H, T]."""
    outs, lses = [], []
    for b, (lo, hi) in enumerate(bounds(lengths)):
        o, l = ao.short_fwd(qkv[None, lo:hi], heads, _keep(keep, b, heads, hi - lo), p, rounded=rounded)
        outs.append(o[0])
        lses.append(l[0])
    return torch.cat(outs, 0), torch.cat(lses, 1)


def packed_bwd(qkv, out, dout, lse, heads, lengths, keep=None, p=0.0, rounded=False):
    """-> dqkv [T, 3 * H * 64], from the out [T, H * 64] and lse [H, T] that are passed in."""
    grads = []
    for b, (lo, hi) in enumerate(bounds(lengths)):
        g = ao.short_bwd(qkv[None, lo:hi], out[None, lo:hi], dout[None, lo:hi], lse[None, :, lo:hi], heads,
                         _keep(keep, b, heads, hi - lo), p, rounded=rounded)
        grads.append(g[0])
    return torch.cat(grads, 0)


def packed_inputs(scale, lengths, heads, seed=0):
    """bf16 qkv [T, 3 * H * 64] = scale * randn and dout [T, H * 64] = randn (attn_oracle.short_inputs)."""
    qkv, dout = ao.short_inputs(scale, 1, sum(lengths), heads, seed=seed)
    return qkv[0], dout[0]
