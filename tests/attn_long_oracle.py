"""Inputs, shapes and a host model of the dropout mask for the chunked BERT attention kernels
(csrc/kernels/attention_long.hip: S <= 512, online softmax over 128-key chunks).  The fp64 oracles are
those of the one-tile kernels, which work at any S: attn_oracle.short_fwd / short_bwd (dense),
attn_padded_oracle (key lengths), attn_packed_oracle (packed).  Imported by test_attention_long_cpu.py
and test_attention_long_gpu.py.

long_inputs is attn_oracle.flash_inputs for this kernel: K carries a ramp of g exp2 units per 128-key
chunk along a fixed sign vector u, Q is randn + u, so a row's running max grows by about g from chunk
to chunk (FLASH_KINDS: flat 0, deferred 3, rescale 12) or is set by the first chunk (descend: 12,
reversed).  The kernels rescale O^T at every chunk, so the kinds differ in the size of the factor:
about 1, 2^-3, 2^-12, and exactly 1 after the first chunk.
"""
import math

import numpy as np
import torch

from . import attn_oracle as ao
from . import attn_packed_oracle as apk
from . import attn_padded_oracle as apo

CHUNK = 128
KINDS = list(ao.FLASH_KINDS)

# ((B, S, H), lengths): what each reaches is in the table of test_attention_long_gpu.py
PADDED = [((2, 160, 2), [160, 129]),
          ((3, 256, 1), [256, 128, 1]),
          ((2, 384, 3), [383, 257]),
          ((1, 512, 2), [512]),
          ((2, 64, 1), [64, 7])]
PACKED_ONLY = [((4, 512, 2), [512, 130, 33, 1]),
               ((2, 224, 1), [200, 150])]
PACKED = PADDED + PACKED_ONLY


def long_inputs(kind, B, S, H, seed=0):
    """bf16 qkv [B, S, 3 * H * 64] and dout [B, S, H * 64]; the ramp is the same in every head."""
    g, rev = ao.FLASH_KINDS[kind]
    D = ao.SHORT_D
    gen = torch.Generator().manual_seed(seed)
    u = (torch.randint(0, 2, (D,), generator=gen) * 2 - 1).double()
    c = 1.0 / (math.sqrt(D) * ao.LOG2E)  # u . u * c * SHORT_SCALE * LOG2E = 1 exp2 unit
    t = torch.arange(S) // CHUNK
    if rev:
        t = (S - 1) // CHUNK - t
    x = torch.randn(B, S, 3, H, D, generator=gen, dtype=torch.float64)
    x[:, :, 0] += u
    x[:, :, 1] += c * g * t.double()[None, :, None, None] * u
    dout = torch.randn(B, S, H * D, generator=gen, dtype=torch.float64)
    return x.view(B, S, 3 * H * D).to(torch.bfloat16), dout.to(torch.bfloat16)


def pack(x, lengths):
    """[B, S, ...] -> [T, ...]: the valid rows in batch order."""
    return torch.cat([x[b, :n] for b, n in enumerate(lengths)], 0).contiguous()


INPUTS = [("short", 0.8), ("short", 3.0)] + [("long", k) for k in KINDS]
LAYOUTS = ("dense", "klen", "packed")


def max_len(lengths):
    """PackedSeqs.max_len: the longest sequence rounded up to a multiple of 32."""
    return (max(lengths) + 31) // 32 * 32


def inputs(layout, batch, inp, seed):
    """bf16 (qkv, dout) of one case: [B, S, ...] for dense / klen, the valid rows [T, ...] for packed."""
    (B, S, H), lens = batch
    how, arg = inp
    if how == "short":
        qkv, dout = ao.short_inputs(arg, B, S, H, seed=seed)
    else:
        qkv, dout = long_inputs(arg, B, S, H, seed=seed)
    return (pack(qkv, lens), pack(dout, lens)) if layout == "packed" else (qkv, dout)


def reference(layout, batch, qkv, dout, keep, p):
    """fp64 oracle and bf16 yardstick of one case, the backward from the oracle's own out and lse (as bf16 /
    fp32, what the bindings are given).  keep: [B * H, S, S] (packed: at S = max_len) or None."""
    (B, S, H), lens = batch
    if layout == "dense":
        fwd = lambda r: ao.short_fwd(qkv, H, keep, p, rounded=r)  # noqa: E731
        bwd = lambda o, l, r: ao.short_bwd(qkv, o, dout, l, H, keep, p, rounded=r)  # noqa: E731
    elif layout == "klen":
        fwd = lambda r: apo.short_fwd_len(qkv, H, lens, keep, p, rounded=r)  # noqa: E731
        bwd = lambda o, l, r: apo.short_bwd_len(qkv, o, dout, l, H, lens, keep, p, rounded=r)  # noqa: E731
    else:
        fwd = lambda r: apk.packed_fwd(qkv, H, lens, keep, p, rounded=r)  # noqa: E731
        bwd = lambda o, l, r: apk.packed_bwd(qkv, o, dout, l, H, lens, keep, p, rounded=r)  # noqa: E731
    out, lse = fwd(False)
    yout, _ = fwd(True)
    out_in, lse_in = out.to(torch.bfloat16), lse.float().contiguous()
    return dict(out=out, lse=lse, yout=yout, out_in=out_in, lse_in=lse_in, grad=bwd(out_in, lse_in, False),
                ygrad=bwd(out_in, lse_in, True))


def rows(x, heads):
    """[..., H * 64] -> [..., H, 64]: the 64-wide rows rowerr is taken over."""
    return x.view(*x.shape[:-1], heads, ao.SHORT_D)


def thirds(dqkv, heads):
    """[..., 3 * H * 64] -> dq, dk, dv as [..., H, 64]."""
    return dqkv.view(*dqkv.shape[:-1], 3, heads, ao.SHORT_D).unbind(-3)


def chunk_growth(qkv, heads):
    """Growth in exp2 units, one value per (row, chunk t >= 1): the max score of chunk t minus the max
    score of the chunks before it (flash_growth over 128-key chunks, no causal mask).  Empty at S <= 128."""
    q, k, _ = ao._split(qkv, heads)
    sc = q @ k.transpose(-1, -2) * ao.SHORT_SCALE * ao.LOG2E  # [B, H, S, S]
    S = sc.shape[-1]
    tmax = torch.stack([sc[..., a:a + CHUNK].amax(-1) for a in range(0, S, CHUNK)], -1)  # [B, H, S, nt]
    return (tmax[..., 1:] - tmax.cummax(-1).values[..., :-1]).reshape(-1)


def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def keep_model(bh, S, p, seed):
    """Host model of attn_dropout_mask(like, bh, S, p, seed): uint8 [bh, S, S], 1 where element
    e = (row * S + j) mod 2^32 keeps (the 16-bit half e & 1 of mix32((e >> 1) ^ key) is >= round(p * 2^16))."""
    thr = int(p * 65536.0 + 0.5)
    key = np.uint32((seed & 0xFFFFFFFF) ^ (((seed >> 32) * 0x9E3779B9) & 0xFFFFFFFF))
    with np.errstate(over="ignore"):
        e = np.arange(bh * S * S, dtype=np.uint64).astype(np.uint32)
        h = _mix32((e >> np.uint32(1)) ^ key)
    draw = np.where(e & np.uint32(1), h >> np.uint32(16), h & np.uint32(0xFFFF))
    return torch.from_numpy((draw >= thr).astype(np.uint8)).view(bh, S, S)
