"""Mixture-of-experts FFN over routed tokens (csrc/kernels/moe.hip) with autograd.

  moe_ffn(x, idx, wts, w13, w2) -> out[t] = sum_j wts[t, j] * (swiglu(x[t] @ w13[idx[t, j]].T) @ w2[idx[t, j]].T)

``x`` [T, D] bf16, ``idx`` [T, k] integer expert ids in [0, E) (the k ids of a token distinct), ``wts`` [T, k] fp32,
``w13`` [E, 2F, D] (gate rows, then up rows, as ``LlamaBlock.w13``), ``w2`` [E, D, F].  Routing (router logits,
softmax, topk, renormalisation and their autograd) stays outside, in torch.

The fused route: ``moe_plan`` sorts the T * k (token, slot) pairs by expert into a row space in which every
expert's segment starts at a multiple of the 128-row GEMM tile (R_cap rows, sized from T, k and E alone: no host
sync), the grouped MFMA GEMMs read x (and, backward, dout times wts) through the row map while staging -- no
permuted copy of either in HBM --, the existing swiglu kernels run on the [R_cap, 2F] rows, and ``moe_combine``
folds the k rows of a token in fp32, j ascending.  No atomics: two calls are bitwise equal, and with ``idx`` fixed
``out[t]`` and ``dx[t]`` do not depend on the other tokens' x.  An id outside [0, E) contributes nothing.

Off the domain (``moe_ok``: GPU bf16, D % 64 == 0, F % 64 == 0, E <= 128, k <= 8, and a mean of at most
``ROUTE_MAX_ROWS_PER_EXPERT`` rows per expert, the measured range in which the route wins) and under
PS_AMD_DISABLE=moe_ffn the op is ``_moe_ref``, the torch composition.
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn.functional as F

from .. import knobs
from ._ext import native

MAX_EXPERTS = 128
MAX_TOP_K = 8
# The fused route is the default up to this mean number of rows per expert (T k / E).  profiles/moe_probe.txt: at
# 2048 (E 64, k 8, D 2048, F 1024) it takes a quarter to an eighth of the composition's time in every pair; at 4096
# with Mixtral's wide experts (E 8, k 2, D 4096, F 14336) the composition's library GEMMs are ahead (forward 1.25x),
# so those shapes stay on the composition.  The kernels themselves run at any size (``_MoeFFN.apply``).
ROUTE_MAX_ROWS_PER_EXPERT = 2048


def _check(x, idx, wts, w13, w2):
    if x.dim() != 2 or w13.dim() != 3 or w2.dim() != 3:
        raise ValueError("moe_ffn: x [T, D], w13 [E, 2F, D], w2 [E, D, F]")
    T, D = x.shape
    E, F2, _ = w13.shape
    if F2 % 2 or tuple(w13.shape) != (E, F2, D) or tuple(w2.shape) != (E, D, F2 // 2):
        raise ValueError("moe_ffn: w13 [E, 2F, D] and w2 [E, D, F] for x [T, D]")
    if idx.dim() != 2 or idx.shape[0] != T or tuple(wts.shape) != tuple(idx.shape):
        raise ValueError("moe_ffn: idx and wts [T, k]")
    if idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
        raise ValueError("moe_ffn: idx is an integer tensor")


def _moe_ref(x: torch.Tensor, idx: torch.Tensor, wts: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """The torch composition in x's dtype: a loop over the experts, each on the tokens its mask selects, the
    weighted outputs summed in fp32 (fp64 for fp64 inputs) through masked assignment -- no ``index_add_``.  The
    fallback off the fused domain, and the fused route's timing baseline and error yardstick."""
    from .transformer import swiglu

    acc_t = torch.promote_types(x.dtype, torch.float32)
    out = torch.zeros(x.shape, dtype=acc_t, device=x.device)
    for e in range(w13.shape[0]):
        hit = idx == e                                 # [T, k]
        sel = hit.any(1).nonzero().squeeze(1)          # tokens of expert e, ascending (a host sync)
        we = (wts.to(acc_t) * hit).sum(1)[sel]         # its weight per token (ids distinct: at most one term)
        y = swiglu(x[sel] @ w13[e].t()) @ w2[e].t()
        out[sel] = out[sel] + we[:, None] * y.to(acc_t)  # distinct rows: an assignment, not an accumulation
    return out.to(x.dtype)


def moe_ok(x: torch.Tensor, idx: torch.Tensor, wts: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor) -> bool:
    """The fused route's domain."""
    return (all(t.is_cuda and t.dtype == torch.bfloat16 for t in (x, w13, w2)) and idx.is_cuda and wts.is_cuda
            and wts.dtype == torch.float32 and x.shape[0] >= 1 and x.shape[1] % 64 == 0 and w2.shape[2] % 64 == 0
            and w13.shape[0] <= MAX_EXPERTS and 1 <= idx.shape[1] <= MAX_TOP_K
            and x.shape[0] * idx.shape[1] <= ROUTE_MAX_ROWS_PER_EXPERT * w13.shape[0] and knobs.enabled("moe_ffn"))


def moe_plan(idx: torch.Tensor, experts: int) -> List[torch.Tensor]:
    """``idx`` [T, k] on the GPU -> [row_token, row_slot, slot_row, tile_expert, counts, seg], all int32, with no
    host sync.  Row r of the permuted space holds pair ``row_slot[r] = t * k + j`` of token ``row_token[r]`` (-1:
    a pad row); pairs are in stable order by expert (ascending (t, j) within one), expert e's rows begin at
    ``seg[e]`` (a multiple of 128) and number ``counts[e]`` (what an auxiliary load-balancing loss needs);
    ``slot_row[t, j]`` is the pair's row (-1 for an id outside [0, experts)); ``tile_expert`` has one entry per
    128 rows (-1: unused).  R_cap = 128 * (ceil(T k / 128) + experts)."""
    if idx.dtype not in (torch.int32, torch.int64):
        idx = idx.long()
    return native().moe_plan(idx.contiguous(), int(experts))


class _MoeFFN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, wts, w13, w2):
        n = native()
        x, wts, w13, w2 = x.contiguous(), wts.contiguous(), w13.contiguous(), w2.contiguous()
        plan = moe_plan(idx, w13.shape[0])
        gu = n.moe_gemm(x, w13, plan, True, None, False)   # [R_cap, 2F], x gathered while staging
        h = n.swiglu_fwd(gu)
        y = n.moe_gemm(h, w2, plan, False, None, False)    # [R_cap, D]
        ctx.save_for_backward(x, wts, w13, w2, gu, h, y, *plan)
        return n.moe_combine(y, plan, wts)

    @staticmethod
    def backward(ctx, dout):
        x, wts, w13, w2, gu, h, y, *plan = ctx.saved_tensors
        n = native()
        dout = dout.contiguous()
        dwts = n.moe_combine_bwd(y, plan, dout)
        dh = n.moe_gemm(dout, w2, plan, True, wts, True)    # dY = wts * dout[token], formed while staging
        dgu = n.swiglu_bwd(dh, gu)
        dx = n.moe_combine(n.moe_gemm(dgu, w13, plan, False, None, True), plan, None)
        dw2 = n.moe_wgrad(dout, h, plan, 1, wts)            # dW2[e][d, f] = sum_r dY[r, d] H[r, f]
        dw13 = n.moe_wgrad(dgu, x, plan, 2, None)           # dW13[e][n, c] = sum_r dGU[r, n] x[token r, c]
        return dx, None, dwts, dw13, dw2


def moe_ffn(x: torch.Tensor, idx: torch.Tensor, wts: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """The mixture-of-experts FFN of the module docstring; gradients to ``x``, ``wts``, ``w13`` and ``w2``."""
    _check(x, idx, wts, w13, w2)
    if moe_ok(x, idx, wts, w13, w2):
        return _MoeFFN.apply(x, idx, wts, w13, w2)
    return _moe_ref(x, idx, wts, w13, w2)


def route(h: torch.Tensor, router_weight: torch.Tensor, top_k: int, norm_topk: bool = True):
    """Router of the MoE blocks, in torch: softmax in fp32 over the experts, ``topk``, renormalised over the k
    when ``norm_topk``.  ``h`` [T, D], ``router_weight`` [E, D] -> (idx [T, k] int64, wts [T, k] fp32)."""
    probs = F.linear(h, router_weight).float().softmax(-1)
    wts, idx = probs.topk(top_k, dim=-1)
    if norm_topk:
        wts = wts / wts.sum(-1, keepdim=True)
    return idx, wts
