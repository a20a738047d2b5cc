"""Fused transformer row / elementwise ops (csrc/kernels/transformer.hip) with autograd.

  rms_norm(x, w, eps, residual=None)         -> y  |  (s = x + residual, y = RMSNorm(s))
  layer_norm_residual(x, o, g, b, eps, p)    -> LN(x + dropout_p(o))        (BERT post-LN)
  swiglu(gu)                                  -> silu(gu[..., :F]) * gu[..., F:]
  rope_split(qkv, cs, H, KV)                  -> q, k, v  (RoPE + head split + transpose)
  attention_qkv(qkv, H, p, mask, key_lengths) -> dropout_p(softmax(q k^T / 8)) v over the fused qkv
                                                 projection (csrc/kernels/attention.hip, S <= 128;
                                                 csrc/kernels/attention_long.hip, 128 < S <= 512;
                                                 right-padded batches by per-sequence key_lengths)
  pack_seqs(lengths, seq) / unpad / repad     -> the valid tokens of a right-padded batch as [T, ...] rows;
  attention_qkv(qkv [T, 3HD], H, p, seqs=)       attention reads sequence b at its offset (no pad rows)
  attention_causal_gqa(q, k, v, doc_bounds)   -> causal GQA flash attention, heads merged
                                                 (csrc/kernels/flash_attn.hip, head dim 128; packed
                                                 rows by per-token document bounds: doc_bounds(doc_ids))

GPU bf16 tensors (row length <= 4096, multiple of 8) take the HIP kernels; everything else
runs the plain torch composition, which is also the numerics oracle in the GPU tests.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

from .. import knobs
from ._ext import native


def _hip(*ts) -> bool:
    return all(t is not None and t.is_cuda and t.dtype == torch.bfloat16 for t in ts)


def _seed() -> int:
    # host RNG (no device sync); deterministic under torch.manual_seed
    return int(torch.randint(0, 2 ** 62, (1,)).item())


# ------------------------------------------------------------------------------ RMSNorm
def _rms_ref(x, w, eps):
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype) * w


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        x = x.contiguous()
        _, y, rstd = native().rmsnorm_fwd(x, None, w.contiguous(), float(eps))
        ctx.save_for_backward(x, w, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, rstd = ctx.saved_tensors
        dx, dw = native().rmsnorm_bwd(dy.contiguous(), x, w, rstd, None)
        return dx, dw.to(w.dtype), None


class _AddRMSNorm(torch.autograd.Function):
    """s = x + r (the residual stream, returned) and y = RMSNorm(s) in one pass; backward
    folds the stream gradient ds into the norm backward (one pass, dx = dr)."""

    @staticmethod
    def forward(ctx, x, r, w, eps):
        s, y, rstd = native().rmsnorm_fwd(x.contiguous(), r.contiguous(), w.contiguous(), float(eps))
        ctx.save_for_backward(s, w, rstd)
        # an unused stream output (the final norm discards s) arrives as None, not as a zero-filled
        # [B, S, D] tensor autograd would write first (2.6 ms per Llama step beside the serve)
        ctx.set_materialize_grads(False)
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        s, w, rstd = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(s)
        dsum, dw = native().rmsnorm_bwd(dy.contiguous(), s, w, rstd,
                                        ds.contiguous() if ds is not None else None)
        return dsum, dsum, dw.to(w.dtype), None


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None):
    D = x.shape[-1]
    ok = _hip(x) and D % 8 == 0 and D <= 4096 and w.is_cuda and w.dtype in (torch.bfloat16, torch.float32)
    if residual is None:
        return _RMSNorm.apply(x, w, eps) if ok else _rms_ref(x, w, eps)
    if ok and _hip(residual):
        return _AddRMSNorm.apply(x, residual, w, eps)
    s = x + residual
    return s, _rms_ref(s, w, eps)


# ------------------------------------------------------------------------------ LayerNorm
class _LNResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, o, gamma, beta, eps, p):
        seed = _seed()
        s, y, mean, rstd = native().layernorm_fwd(x.contiguous(), o.contiguous(), gamma.contiguous(),
                                                  beta.contiguous(), float(eps), float(p), seed)
        ctx.save_for_backward(s, gamma, mean, rstd)
        ctx.p, ctx.seed = float(p), seed
        return y

    @staticmethod
    def backward(ctx, dy):
        s, gamma, mean, rstd = ctx.saved_tensors
        dx, do, dg, db = native().layernorm_bwd(dy.contiguous(), s, gamma, mean, rstd, ctx.p, ctx.seed)
        return dx, do, dg.to(gamma.dtype), db.to(gamma.dtype), None, None


def layer_norm_residual(x: torch.Tensor, o: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                        p: float = 0.0, training: bool = True) -> torch.Tensor:
    """LayerNorm(x + dropout_p(o)) -- the BERT sublayer epilogue in one pass each way."""
    p = float(p) if training else 0.0
    D = x.shape[-1]
    if _hip(x, o) and D % 8 == 0 and D <= 4096 and gamma.dtype in (torch.bfloat16, torch.float32):
        return _LNResidual.apply(x, o, gamma, beta, eps, p)
    return F.layer_norm(x + F.dropout(o, p, training), (D,), gamma, beta, eps)


# ------------------------------------------------------------------------------ SwiGLU
class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        gu = gu.contiguous()
        ctx.save_for_backward(gu)
        return native().swiglu_fwd(gu)

    @staticmethod
    def backward(ctx, dh):
        (gu,) = ctx.saved_tensors
        return native().swiglu_bwd(dh.contiguous(), gu)


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    if _hip(gu) and gu.shape[-1] % 16 == 0:
        return _SwiGLU.apply(gu)
    g, u = gu.chunk(2, dim=-1)
    return F.silu(g) * u


# ------------------------------------------------------------------------------ RoPE
def rope_table(seq: int, hd: int, theta: float, device) -> torch.Tensor:
    """[S, hd/2, 2] fp32 (cos, sin) -- rotate-halves convention (Llama / HF)."""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, device=device).float() / hd))
    f = torch.outer(torch.arange(seq, device=device).float(), inv)
    return torch.stack([torch.cos(f), torch.sin(f)], dim=-1).contiguous()


def _rope_ref(x, cs):
    d = x.shape[-1]
    c, s = cs[..., 0][None, None].to(x.dtype), cs[..., 1][None, None].to(x.dtype)
    x1, x2 = x[..., : d // 2], x[..., d // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


class _RopeSplit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cs, H, KV):
        q, k, v = native().rope_split_fwd(qkv.contiguous(), cs, int(H), int(KV))
        ctx.save_for_backward(cs)
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        (cs,) = ctx.saved_tensors
        dq = dq if dq is not None else None
        return native().rope_split_bwd(dq.contiguous(), dk.contiguous(), dv.contiguous(), cs), None, None, None


def rope_split(qkv: torch.Tensor, cs: torch.Tensor, H: int, KV: int):
    """qkv [B, S, H + 2 KV, hd] -> q [B, H, S, hd], k/v [B, KV, S, hd] with RoPE on q and k."""
    if _hip(qkv) and qkv.shape[-1] % 16 == 0:
        return _RopeSplit.apply(qkv, cs, H, KV)
    x = qkv.transpose(1, 2)
    q, k, v = x.split([H, KV, KV], dim=1)
    return _rope_ref(q, cs), _rope_ref(k, cs), v


# ------------------------------------------------------------------------------ attention
def attention_qkv_ok(qkv: torch.Tensor, heads: int, mask) -> bool:
    """The fused kernel's domain: GPU bf16, head dim 64, S a multiple of 32 up to 128, no mask
    (a right-padded batch is given by key lengths, not by a mask: attention_qkv)."""
    return (mask is None and _hip(qkv) and qkv.dim() == 3 and qkv.shape[2] == 3 * heads * 64
            and qkv.shape[1] % 32 == 0 and 0 < qkv.shape[1] <= 128
            and knobs.enabled("fused_attn"))


# The bounds the chunked kernels (csrc/kernels/attention_long.hip) are the default route within: the
# bindings take S up to LONG_MAX_S anywhere; the route covers (SHORT_MAX_S, LONG_ROUTE_MAX_S], the
# range where profiles/bert_attn_long_probe.txt shows them at or below the SDPA route's time.
SHORT_MAX_S = 128
LONG_MAX_S = 512
LONG_ROUTE_MAX_S = 512


def attention_long_ok(qkv: torch.Tensor, heads: int, mask) -> bool:
    """The chunked kernels' domain on the default route: GPU bf16, head dim 64, S a multiple of 32 in
    (128, LONG_ROUTE_MAX_S], no mask."""
    return (mask is None and _hip(qkv) and qkv.dim() == 3 and qkv.shape[2] == 3 * heads * 64
            and qkv.shape[1] % 32 == 0 and SHORT_MAX_S < qkv.shape[1] <= LONG_ROUTE_MAX_S
            and knobs.enabled("fused_attn"))


@dataclass(frozen=True)
class PackedSeqs:
    """The packing of a right-padded batch [B, seq] into its T = sum(lengths) valid tokens, in batch
    order (``pack_seqs``).  ``cu`` int32 [B + 1] (exclusive prefix sum of the lengths), ``index`` int64
    [T] (``b * seq + i`` of every valid token) and ``pos`` int64 [T] (its position ``i``) are on the
    device; ``total`` (T), ``batch``, ``seq`` and ``max_len`` (the key bound the attention kernels run
    with: max(lengths) rounded up to a multiple of 32) are Python ints."""
    cu: torch.Tensor
    index: torch.Tensor
    pos: torch.Tensor
    total: int
    batch: int
    seq: int
    max_len: int


def pack_seqs(lengths, seq: int, device=None) -> PackedSeqs:
    """``lengths``: a list or a CPU integer tensor [B] with ``1 <= lengths[b] <= seq``.  It is read on
    the host -- T sizes every later allocation, so it has to be known there without waiting for the
    device; a CUDA tensor raises ``ValueError``.  The device tensors are uploaded ``non_blocking``."""
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda:
            raise ValueError("pack_seqs: lengths on the host (a list or a CPU tensor) -- the token total sizes "
                             "the packed tensors, and reading a CUDA tensor for it would sync the device")
        if lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
            raise ValueError("pack_seqs: integer lengths")
    lens = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1)
    seq = int(seq)
    if lens.numel() < 1 or int(lens.min()) < 1 or int(lens.max()) > seq:
        raise ValueError("pack_seqs: lengths is [B >= 1] integers in [1, seq]")
    batch = lens.numel()
    cu = torch.zeros(batch + 1, dtype=torch.int64)
    torch.cumsum(lens, 0, out=cu[1:])
    total = int(cu[-1])
    if total >= 2 ** 31:
        raise ValueError("pack_seqs: more than 2^31 - 1 tokens")
    owner = torch.repeat_interleave(torch.arange(batch), lens)
    pos = torch.arange(total) - cu[:-1][owner]
    index = owner * seq + pos
    up = lambda t: t if device is None else t.to(device, non_blocking=True)  # noqa: E731
    return PackedSeqs(cu=up(cu.to(torch.int32)), index=up(index), pos=up(pos), total=total, batch=batch, seq=seq,
                      max_len=(int(lens.max()) + 31) // 32 * 32)


def unpad(x: torch.Tensor, seqs: PackedSeqs) -> torch.Tensor:
    """[B, seq, ...] -> [T, ...]: the valid tokens in packed order (plain torch, differentiable)."""
    if x.dim() < 2 or tuple(x.shape[:2]) != (seqs.batch, seqs.seq):
        raise ValueError("unpad: x [batch, seq, ...] of the packing")
    return x.reshape(seqs.batch * seqs.seq, *x.shape[2:]).index_select(0, seqs.index)


def repad(x: torch.Tensor, seqs: PackedSeqs) -> torch.Tensor:
    """[T, ...] -> [B, seq, ...] with zeros at the pad positions (plain torch, differentiable)."""
    if x.dim() < 1 or x.shape[0] != seqs.total:
        raise ValueError("repad: x [total, ...] of the packing")
    z = x.new_zeros(seqs.batch * seqs.seq, *x.shape[1:])
    return z.index_copy(0, seqs.index, x).view(seqs.batch, seqs.seq, *x.shape[1:])


class _FusedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, p, key_lengths, cu=None, max_len=0):
        qkv = qkv.contiguous()
        seed = _seed() if p > 0 else 0
        ctx.max_len = int(max_len)
        # one tile (attention.hip) up to 128 keys, the chunked kernels (attention_long.hip) beyond
        ctx.long = (ctx.max_len if cu is not None else qkv.shape[1]) > SHORT_MAX_S
        fwd = native().attn_long_fwd if ctx.long else native().attn_fwd
        if cu is not None:  # packed: qkv [T, 3 * H * 64], sequence b at rows [cu[b], cu[b + 1])
            out, lse = fwd(qkv, heads, float(p), seed, None, cu, ctx.max_len)
            ctx.save_for_backward(qkv, out, lse, cu)
        elif key_lengths is None:
            out, lse = fwd(qkv, heads, float(p), seed)
            ctx.save_for_backward(qkv, out, lse)
        else:
            out, lse = fwd(qkv, heads, float(p), seed, key_lengths)
            ctx.save_for_backward(qkv, out, lse, key_lengths)
        ctx.heads, ctx.p, ctx.seed = heads, float(p), seed
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, *klen = ctx.saved_tensors
        bwd = native().attn_long_bwd if ctx.long else native().attn_bwd
        if ctx.max_len:
            return (bwd(qkv, out, dout.contiguous(), lse, ctx.heads, ctx.p, ctx.seed, None, klen[0], ctx.max_len),
                    None, None, None, None, None)
        return (bwd(qkv, out, dout.contiguous(), lse, ctx.heads, ctx.p, ctx.seed, *klen), None, None, None, None, None)


def key_lengths_from_mask(mask: torch.Tensor) -> torch.Tensor:
    """Per-sequence key lengths [B] of a right-padded batch from its boolean token mask [B, S] (True:
    a real token): ``mask.sum(1)``.  A CPU mask is checked to be a prefix mask (``ValueError``
    otherwise: left padding and holes are not key lengths); a GPU mask is not looked at (no sync)."""
    if mask.dim() != 2:
        raise ValueError("key_lengths_from_mask: mask [B, S]")
    m = mask.bool()
    lengths = m.sum(1)
    if not m.is_cuda:
        prefix = torch.arange(m.shape[1], device=m.device)[None, :] < lengths[:, None]
        if not torch.equal(m, prefix):
            raise ValueError("key_lengths_from_mask: not a prefix (right-padding) mask")
    return lengths


def _device_key_lengths(key_lengths: torch.Tensor, qkv: torch.Tensor) -> torch.Tensor:
    """[B] int32 on qkv's device, no sync (an int32 tensor already there passes through)."""
    if key_lengths.dim() != 1 or key_lengths.shape[0] != qkv.shape[0]:
        raise ValueError("key_lengths: one length per batch row, [B]")
    if key_lengths.is_floating_point() or key_lengths.is_complex() or key_lengths.dtype == torch.bool:
        raise ValueError("key_lengths: an integer tensor")
    return key_lengths.to(device=qkv.device, dtype=torch.int32, non_blocking=True).contiguous()


def attention_packed_ok(qkv: torch.Tensor, heads: int, seqs: PackedSeqs) -> bool:
    """The packed kernels' domain: GPU bf16, head dim 64, every sequence within 128 keys."""
    return (_hip(qkv) and qkv.shape[1] == 3 * heads * 64 and seqs.max_len <= 128 and seqs.cu.device == qkv.device
            and knobs.enabled("fused_attn"))


def attention_packed_long_ok(qkv: torch.Tensor, heads: int, seqs: PackedSeqs) -> bool:
    """The packed chunked kernels' domain on the default route: GPU bf16, head dim 64, the longest sequence
    (rounded up to 32) in (128, LONG_ROUTE_MAX_S]."""
    return (_hip(qkv) and qkv.shape[1] == 3 * heads * 64 and SHORT_MAX_S < seqs.max_len <= LONG_ROUTE_MAX_S
            and seqs.cu.device == qkv.device and knobs.enabled("fused_attn"))


def attention_qkv(qkv: torch.Tensor, heads: int, p: float = 0.0, mask: Optional[torch.Tensor] = None,
                  key_lengths: Optional[torch.Tensor] = None, seqs: Optional[PackedSeqs] = None) -> torch.Tensor:
    """Multi-head self-attention over the fused projection ``qkv`` [B, S, 3 * H * D] (q | k | v,
    heads inner) -> [B, S, H * D], dropout ``p`` on the probabilities.  On the fused kernel the
    heads are never split into separate q / k / v tensors and the output is already merged.

    ``key_lengths`` [B] (any integer dtype) describes a right-padded batch: keys at or beyond
    ``clamp(key_lengths[b], 1, S)`` of sequence b take no part in any softmax, as under SDPA with a
    key-padding mask; every query row, padded ones included, is an ordinary row.  It stays in the
    fused kernels' domain.  An arbitrary ``mask`` goes to SDPA; giving both raises ``ValueError``.

    ``seqs`` (``pack_seqs``; not with ``mask`` or ``key_lengths``): ``qkv`` is [T, 3 * H * D], the valid
    tokens of a right-padded batch only, and the result is [T, H * D]; sequence b is rows
    ``[cu[b], cu[b + 1])`` and attends to itself alone.  GPU bf16 with head dim 64 and
    ``seqs.max_len <= 512`` runs the packed instantiations of the fused kernels, which read and write no
    pad row at all; anything else is ``repad``, the ``key_lengths`` path above, ``unpad``.

    The fused domain is S (or ``seqs.max_len``) a multiple of 32: up to 128 on the one-tile kernels
    (attention.hip), from 160 to 512 on the chunked ones (attention_long.hip), with the same semantics,
    layouts and dropout draw; S > 512, ``S % 32 != 0``, CPU, fp32 and PS_AMD_DISABLE=fused_attn take SDPA."""
    if seqs is not None:
        if mask is not None or key_lengths is not None:
            raise ValueError("attention_qkv: seqs describes the whole batch: no mask, no key_lengths")
        if qkv.dim() != 2 or qkv.shape[0] != seqs.total:
            raise ValueError("attention_qkv: packed qkv [seqs.total, 3 * heads * head_dim]")
        if attention_packed_ok(qkv, heads, seqs) or attention_packed_long_ok(qkv, heads, seqs):
            return _FusedAttention.apply(qkv, heads, float(p), None, seqs.cu, seqs.max_len)
        lens = seqs.cu[1:] - seqs.cu[:-1]
        return unpad(attention_qkv(repad(qkv, seqs), heads, p, key_lengths=lens), seqs)
    if key_lengths is not None and mask is not None:
        raise ValueError("attention_qkv: give mask or key_lengths, not both")
    if attention_qkv_ok(qkv, heads, mask) or attention_long_ok(qkv, heads, mask):
        klen = None if key_lengths is None else _device_key_lengths(key_lengths, qkv)
        return _FusedAttention.apply(qkv, heads, float(p), klen, None, 0)
    b, s, _ = qkv.shape
    if key_lengths is not None:
        klen = _device_key_lengths(key_lengths, qkv).clamp(1, s)
        mask = (torch.arange(s, device=qkv.device)[None, :] < klen[:, None])[:, None, None, :]  # [B, 1, 1, S]
    q, k, v = qkv.view(b, s, 3, heads, -1).permute(2, 0, 3, 1, 4)
    a = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=p)
    return a.transpose(1, 2).reshape(b, s, -1)


# ------------------------------------------------------------------------------ causal GQA flash attention
def flash_ok(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    """The in-house causal GQA flash kernels are the default for head dim 128 (PS_AMD_DISABLE=flash_attn
    falls back to SDPA): on the Llama-3-8B shape they beat SDPA's library kernels forward and
    backward (profiles/r3_flash_v3_probe.jsonl) and end to end (profiles/r3_llama_flash_vs_sdpa.jsonl)."""
    return (_hip(q, k, v) and q.dim() == 4 and q.shape[3] == 128 and k.shape == v.shape and q.shape[2] % 128 == 0
            and q.shape[1] % k.shape[1] == 0 and knobs.enabled("flash_attn"))


def doc_bounds(doc_ids: torch.Tensor):
    """Per-token document bounds of packed rows: ``doc_ids`` [B, S] (any integer dtype) ->
    (``doc_start``, ``doc_end``), int32 [B, S] on its device, computed there without a sync.  A new
    document begins at position 0 and wherever ``doc_ids[b, i] != doc_ids[b, i - 1]`` (the values mean
    nothing else; a pad tail is one more document).  ``doc_start[b, i]`` is the first position of
    the document that holds i, ``doc_end[b, i]`` one past its last: start <= i < end, both
    non-decreasing along the row."""
    if doc_ids.dim() != 2:
        raise ValueError("doc_bounds: doc_ids [B, S]")
    if doc_ids.is_floating_point() or doc_ids.is_complex() or doc_ids.dtype == torch.bool:
        raise ValueError("doc_bounds: an integer tensor")
    b, s = doc_ids.shape
    pos = torch.arange(s, device=doc_ids.device, dtype=torch.int32).expand(b, s)
    edge = doc_ids[:, 1:] != doc_ids[:, :-1]
    one = torch.ones(b, 1, dtype=torch.bool, device=doc_ids.device)
    new = torch.cat([one, edge], dim=1)   # a document begins here
    last = torch.cat([edge, one], dim=1)  # a document ends here
    start = torch.where(new, pos, torch.zeros_like(pos)).cummax(1).values
    end = torch.where(last, pos + 1, torch.full_like(pos, s)).flip(1).cummin(1).values.flip(1)
    return start.contiguous(), end.contiguous()


def _check_doc_bounds(bounds, q: torch.Tensor):
    """(doc_start, doc_end) as int32 [B, S] tensors on q's device, no sync."""
    try:
        start, end = bounds
    except (TypeError, ValueError):
        raise ValueError("attention_causal_gqa: doc_bounds is (doc_start, doc_end)") from None
    want = (q.shape[0], q.shape[2])
    for t in (start, end):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
            raise ValueError("attention_causal_gqa: doc_start / doc_end [B, S]")
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError("attention_causal_gqa: doc_start / doc_end integer tensors")
    return tuple(t.to(device=q.device, dtype=torch.int32, non_blocking=True).contiguous() for t in (start, end))


class _FlashCausal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, doc_start=None, doc_end=None):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if doc_start is None:
            out, lse = native().fa_fwd(q, k, v)
            ctx.save_for_backward(q, k, v, out, lse)
        else:
            out, lse = native().fa_fwd(q, k, v, doc_start)
            ctx.save_for_backward(q, k, v, out, lse, doc_start, doc_end)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, *bounds = ctx.saved_tensors
        return tuple(native().fa_bwd(q, k, v, out, dout.contiguous(), lse, *bounds)) + (None, None)


def attention_causal_gqa(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, doc_bounds=None) -> torch.Tensor:
    """Causal attention with grouped KV heads: q [B, H, S, D], k / v [B, KV, S, D] -> [B, S, H * D]
    (heads merged, the output projection's input layout).

    ``doc_bounds`` = (doc_start, doc_end) (``doc_bounds(doc_ids)``; integer [B, S]) describes packed
    rows: query i of row b sees keys ``doc_start[b, i] <= j <= i`` only, its own document.  In the
    flash domain this stays on the in-house kernels, which also skip the key tiles no query of a block
    can see; off it (CPU, fp32, head dim other than 128, S % 128 != 0, PS_AMD_DISABLE=flash_attn) SDPA
    gets the dense boolean mask [B, 1, S, S] built from doc_start."""
    if doc_bounds is None:
        if flash_ok(q, k, v):
            return _FlashCausal.apply(q, k, v)
        b, _, s, _ = q.shape
        a = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=True)
        return a.transpose(1, 2).reshape(b, s, -1)
    start, end = _check_doc_bounds(doc_bounds, q)
    if flash_ok(q, k, v):
        return _FlashCausal.apply(q, k, v, start, end)
    b, _, s, _ = q.shape
    pos = torch.arange(s, device=q.device)
    mask = (pos[None, None, :] <= pos[None, :, None]) & (pos[None, None, :] >= start[:, :, None])  # [B, S(q), S(k)]
    a = F.scaled_dot_product_attention(q, k, v, attn_mask=mask[:, None], enable_gqa=True)
    return a.transpose(1, 2).reshape(b, s, -1)


# ------------------------------------------------------------------------------ fused LM-head cross-entropy
class _FusedXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, labels, ignore):
        lse, rows = native().xent_fwd(x, labels, int(ignore))
        # the kernels' rule for a scored row (xent.hip: y != ignore and 0 <= y < V): an out-of-range
        # label scores 0 and is not in the mean's denominator either (F.cross_entropy raises on
        # one; checking here would cost a host sync per step)
        V = x.shape[1]
        count = ((labels != ignore) & (labels >= 0) & (labels < V)).sum().float().reshape(1)
        ctx.save_for_backward(x, labels, lse, count)
        ctx.ignore = int(ignore)
        return (rows.sum() / count.clamp(min=1.0)).reshape(())

    @staticmethod
    def backward(ctx, go):
        x, labels, lse, count = ctx.saved_tensors
        dx = native().xent_bwd(x, labels, lse, go.float().reshape(1).contiguous(), count, ctx.ignore)
        return dx, None, None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """Mean softmax cross-entropy of ``logits`` [..., V] against ``labels`` [...] (ignore_index rows
    excluded), as F.cross_entropy.  GPU bf16 logits take the fused HIP kernels (csrc/kernels/xent.hip):
    the forward reads the logits once (per-row log-sum-exp), the backward reads them once and writes
    the bf16 gradient -- no fp32 copy of the vocab-sized activations.  PS_AMD_DISABLE=fused_xent falls back."""
    V = logits.shape[-1]
    if _hip(logits) and logits.dtype == torch.bfloat16 and knobs.enabled("fused_xent"):
        x = logits.reshape(-1, V)
        x = x if x.is_contiguous() else x.contiguous()
        return _FusedXent.apply(x, labels.reshape(-1).long().contiguous(), int(ignore_index))
    return F.cross_entropy(logits.float().reshape(-1, V), labels.reshape(-1), ignore_index=ignore_index)
