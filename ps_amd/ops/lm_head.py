"""LM-head loss without the logits (csrc/kernels/lm_head.hip) with autograd.

  linear_cross_entropy(h, w, labels) == cross_entropy(ps_linear(h, w), labels)

``h`` [..., D] bf16, ``w`` [V, D] bf16 (the ``lm_head.weight`` layout), ``labels`` [...] of any integer dtype.  The
mean runs over the scored rows (label != ignore_index and in [0, V): an out-of-range label scores 0 and is not
counted, the rule of xent.hip); no host sync.

The fused route never holds a [T, V] tensor.  Forward: a GEMM whose epilogue folds every 128-column tile of fp32
logits into per-row (max, sum-exp) partials and picks out the label's logit; a row kernel finishes lse and the
per-row loss.  Backward, chunked over the vocabulary: ``lm_head_dz`` recomputes a chunk's logits and writes
``dz = (softmax - onehot) * go / count`` as bf16 into a scratch [T, chunk_cols]; ``dW[v0:v1] = dz^T h`` is complete
after one library GEMM and lands in the rows of the destination (the parameter server's gradient slot when
``ColocatedPS`` has bound one, as ``PsLinear`` does), and ``dh += dz W[v0:v1]`` accumulates in fp32 [T, D],
rounded once after the last chunk.  No atomics: two calls are bitwise equal, and with ``labels`` fixed the loss and
``dh`` of a row do not depend on the other rows of ``h``.

Off the domain (``fused_ok``: GPU, bf16, D % 64 == 0, V % 8 == 0, T >= 1) and under PS_AMD_DISABLE=fused_head the op
is that composition itself.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import knobs
from ._ext import native
from .linear import _claim, ps_linear
from .transformer import cross_entropy

# The backward's dz scratch [T, chunk_cols] bf16 stays under this many bytes (chunk_cols: a multiple of 128).
SCRATCH_BYTES = 512 << 20


def fused_ok(h: torch.Tensor, w: torch.Tensor) -> bool:
    """The fused route's domain."""
    return (h.is_cuda and w.is_cuda and h.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and h.numel() > 0
            and w.shape[1] % 64 == 0 and w.shape[0] % 8 == 0 and w.shape[0] > 0 and knobs.enabled("fused_head"))


def default_chunk_cols(T: int, V: int) -> int:
    """The largest multiple of 128 whose scratch stays under SCRATCH_BYTES (at least 128, at most V rounded up)."""
    cols = max(128, SCRATCH_BYTES // (2 * T) // 128 * 128)
    return min(cols, (V + 127) // 128 * 128)


class _LinearXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, labels, ignore, chunk_cols, ns):
        """h [T, D], w [V, D], labels [T] int64, all contiguous; ns: vocabulary splits of the forward (0: automatic)."""
        lse, rows = native().lm_head_fwd(h, w, labels, ignore, ns)
        V = w.shape[0]
        count = ((labels != ignore) & (labels >= 0) & (labels < V)).sum().float().reshape(1)
        ctx.save_for_backward(h, w, labels, lse, count)
        ctx.ignore, ctx.chunk_cols = ignore, chunk_cols
        return (rows.sum() / count.clamp(min=1.0)).reshape(())

    @staticmethod
    def backward(ctx, go):
        h, w, labels, lse, count = ctx.saved_tensors
        (T, D), V, chunk = h.shape, w.shape[0], ctx.chunk_cols
        need_h, need_w = ctx.needs_input_grad[:2]
        go = go.float().reshape(1).contiguous()
        scratch = torch.empty(T * min(chunk, V), dtype=h.dtype, device=h.device)
        dh = torch.zeros(T, D, dtype=torch.float32, device=h.device) if need_h else None
        dw = None
        if need_w:
            dw = _claim(w)
            if dw is None:
                dw = torch.empty_like(w)
        for v0 in range(0, V, chunk):
            v1 = min(V, v0 + chunk)
            dz = scratch[:T * (v1 - v0)].view(T, v1 - v0)
            native().lm_head_dz(h, w, labels, lse, go, count, ctx.ignore, v0, dz)
            if need_w:
                torch.mm(dz.t(), h, out=dw[v0:v1])
            if need_h:
                dh += torch.mm(dz, w[v0:v1], out_dtype=torch.float32)
        return (dh.to(h.dtype) if need_h else None), dw, None, None, None, None


def linear_cross_entropy(h: torch.Tensor, w: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100,
                         chunk_cols: Optional[int] = None) -> torch.Tensor:
    """Mean softmax cross-entropy of ``h @ w.T`` against ``labels`` (module docstring); gradients to ``h`` and ``w``.
    ``chunk_cols``: vocabulary columns per backward chunk, a multiple of 128 (default: ``default_chunk_cols``)."""
    if h.shape[-1] != w.shape[-1] or w.dim() != 2 or labels.numel() * h.shape[-1] != h.numel():
        raise ValueError("linear_cross_entropy: h [..., D], w [V, D], labels [...]")
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise ValueError("linear_cross_entropy: labels is an integer tensor")
    if chunk_cols is not None and (chunk_cols <= 0 or chunk_cols % 128):
        raise ValueError("linear_cross_entropy: chunk_cols is a positive multiple of 128")
    if not fused_ok(h, w):
        return cross_entropy(ps_linear(h, w), labels.long(), ignore_index=ignore_index)
    h2 = h.reshape(-1, h.shape[-1]).contiguous()
    chunk = chunk_cols or default_chunk_cols(h2.shape[0], w.shape[0])
    return _LinearXent.apply(h2, w.contiguous(), labels.reshape(-1).long().contiguous(), int(ignore_index), chunk, 0)
