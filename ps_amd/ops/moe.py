"""Mixture-of-experts FFN over routed tokens (csrc/kernels/moe.hip) with autograd.

  moe_ffn(x, idx, wts, w13, w2) -> out[t] = sum_j wts[t, j] * (swiglu(x[t] @ w13[idx[t, j]].T) @ w2[idx[t, j]].T)

``x`` [T, D] bf16, ``idx`` [T, k] integer expert ids in [0, E) (the k ids of a token distinct), ``wts`` [T, k] fp32,
``w13`` [E, 2F, D] (gate rows, then up rows, as ``LlamaBlock.w13``), ``w2`` [E, D, F].  Routing stays outside:
``route`` (router logits, softmax, topk, renormalisation and their autograd in torch, bf16 logits) or ``router``
(one GEMM with the routing in its epilogue, fp32 logits, plus the load-balancing and z losses; softmax scores, or
sigmoid scores with a selection bias and a group-limited top-k).

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

from typing import List, Optional

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


# ----------------------------------------------------------------------------------- fused router (moe_router.hip)
def _check_scoring(E: int, top_k: int, score: str, bias, n_group: int, topk_group: int, scale: float) -> None:
    """``ValueError`` for scoring arguments outside ``router``'s definition."""
    if score == "softmax":
        if bias is not None or n_group != 1 or topk_group != 1 or scale != 1.0:
            raise ValueError("router: bias, n_group, topk_group and scale belong to score='sigmoid'")
    elif score != "sigmoid":
        raise ValueError("router: score is 'softmax' or 'sigmoid'")
    elif not 1 <= topk_group <= n_group <= 32 or E % n_group:
        raise ValueError("router: E % n_group == 0 and 1 <= topk_group <= n_group <= 32")
    elif top_k > topk_group * (E // n_group):
        raise ValueError("router: top_k <= topk_group * E / n_group")
    elif bias is not None and (tuple(bias.shape) != (E,) or bias.dtype not in (torch.float32, torch.bfloat16)):
        raise ValueError("router: bias [E], fp32 or bf16")


def _router_ref(h: torch.Tensor, w: torch.Tensor, top_k: int, norm_topk: bool = True, aux_coef: float = 0.0,
                z_coef: float = 0.0, idx: Optional[torch.Tensor] = None, *, score: str = "softmax",
                bias: Optional[torch.Tensor] = None, n_group: int = 1, topk_group: int = 1, scale: float = 1.0):
    """The definition of ``router`` as a torch composition in the dtype of its inputs (bf16 inputs: the logits are a
    bf16 matmul output, as in ``route``; fp64 inputs: the high-precision reference).  ``idx`` overrides the top-k
    choice.  No host sync.  -> (idx, wts, aux)"""
    E = w.shape[0]
    _check_scoring(E, top_k, score, bias, n_group, topk_group, scale)
    z = F.linear(h, w)
    z = z.to(torch.promote_types(z.dtype, torch.float32))
    lse = torch.logsumexp(z, -1)
    if score == "sigmoid":
        s = torch.sigmoid(z)
        if idx is None:
            c = s.detach() if bias is None else s.detach() + bias.detach().to(z.dtype)
            if n_group > topk_group:  # the topk_group groups of largest (sum of their two largest c), a tie to the lower id
                per = c.view(-1, n_group, E // n_group)
                gscore = per.topk(min(2, E // n_group), dim=-1).values.sum(-1)
                kept = torch.sort(gscore, dim=-1, descending=True, stable=True).indices[:, :topk_group]
                drop = torch.ones_like(gscore, dtype=torch.bool).scatter_(1, kept, False)
                c = per.masked_fill(drop[:, :, None], float("-inf")).view(-1, E)
            idx = torch.sort(c, dim=-1, descending=True, stable=True).indices[:, :top_k]
        wts = s.gather(1, idx)
        p = s / s.sum(-1, keepdim=True)  # what the balance loss averages: DeepSeek-V3's normalised scores
    else:
        p = (z - lse[:, None]).exp()
        if idx is None:  # descending, a tie to the lower id
            idx = torch.sort(z, dim=-1, descending=True, stable=True).indices[:, :top_k]
        wts = p.gather(1, idx)
    if norm_topk:
        wts = wts / wts.sum(-1, keepdim=True)
    if score == "sigmoid":
        wts = wts * scale
    flat = idx.reshape(-1)
    counts = torch.zeros(E, dtype=torch.int64, device=z.device).scatter_add_(0, flat, torch.ones_like(flat))
    lb = E * ((counts.to(z.dtype) / flat.numel()) * p.mean(0)).sum()  # f carries no gradient, P does
    zl = (lse * lse).mean()
    return idx, wts, aux_coef * lb + z_coef * zl


def router_ok(h: torch.Tensor, w: torch.Tensor, top_k: int) -> bool:
    """The fused router's domain.  The kernel reads 16 B at a time: a contiguous view that does not start on a 16-byte
    boundary takes the composition (a non-contiguous tensor is copied, and the copy is aligned)."""
    if not (h.is_cuda and w.is_cuda and h.device == w.device):
        return False
    if any(t.is_contiguous() and t.data_ptr() % 16 for t in (h, w)):
        return False
    return (h.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and h.shape[0] >= 1
            and h.shape[1] % 64 == 0 and h.shape[1] >= 64 and 1 <= w.shape[0] <= MAX_EXPERTS
            and 1 <= top_k <= min(MAX_TOP_K, w.shape[0]) and knobs.enabled("moe_router"))


class _Router(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, top_k, norm_topk, aux_coef, z_coef, score="softmax", bias=None, n_group=1, topk_group=1,
                scale=1.0):
        """h [T, D], w [E, D] bf16 -> (idx, wts, aux, counts [E] int32)"""
        n = native()
        h, w = h.contiguous(), w.contiguous()
        sig = score == "sigmoid"
        if sig:
            bias = None if bias is None else bias.detach().float().contiguous()
            idx, wts, lse, logits, part = n.moe_router_fwd(h, w, top_k, norm_topk, 0, True, bias, n_group, topk_group, scale)
        else:
            idx, wts, lse, logits, part = n.moe_router_fwd(h, w, top_k, norm_topk)
        counts, _, stats = n.moe_router_finish(part, h.shape[0], top_k, aux_coef, z_coef)
        ctx.save_for_backward(h, w, logits, lse, idx, wts, counts)
        ctx.args = (norm_topk, aux_coef, z_coef, sig, scale)
        ctx.mark_non_differentiable(idx, counts)
        return idx, wts, stats[2], counts

    @staticmethod
    def backward(ctx, _didx, dwts, daux, _dcounts):
        h, w, logits, lse, idx, wts, counts = ctx.saved_tensors
        dwts = torch.zeros_like(wts) if dwts is None else dwts.float().contiguous()
        daux = lse.new_zeros(1) if daux is None else daux.float().reshape(1)
        dz = native().moe_router_bwd(logits, lse, idx, wts, dwts, daux, counts, *ctx.args)  # [T, E] bf16
        dh = torch.mm(dz, w) if ctx.needs_input_grad[0] else None
        dw = torch.mm(dz.t(), h) if ctx.needs_input_grad[1] else None
        return (dh, dw) + (None,) * 9


def router(h: torch.Tensor, router_weight: torch.Tensor, top_k: int, norm_topk: bool = True, aux_coef: float = 0.0,
           z_coef: float = 0.0, *, score: str = "softmax", bias: Optional[torch.Tensor] = None, n_group: int = 1,
           topk_group: int = 1, scale: float = 1.0):
    """Router with fp32 logits and the auxiliary losses.  ``h`` [T, D], ``router_weight`` [E, D] ->
    (idx [T, k] int64: the k experts of largest logit, descending, a tie to the lower id; wts [T, k]: their softmax
    probabilities, renormalised over the k when ``norm_topk``; aux: ``aux_coef`` * load-balancing loss (Switch /
    Mixtral: E sum_e f_e P_e) + ``z_coef`` * router z-loss (mean lse^2)).  Gradients to ``h`` and ``router_weight``
    from ``wts`` and ``aux``; no host sync.  On ``router_ok`` one MFMA GEMM with the routing in its epilogue
    (csrc/kernels/moe_router.hip), the logits never rounded below fp32; otherwise, and under
    PS_AMD_DISABLE=moe_router, ``_router_ref``.  ``router.last_counts`` holds the per-expert pair counts [E] int32 of
    the most recent fused call only: every call overwrites it, so with several MoE layers it is the last layer's, and
    a recomputation under activation checkpointing writes it again.  Read it right after the call it belongs to.

    ``score="sigmoid"`` (DeepSeek-V3 style; the other four keywords need it): the scores are ``s = sigmoid(z)``; the
    k experts are those of largest ``s + bias`` (``bias`` [E] fp32 or bf16, no gradient, None: zeros) -- with
    ``n_group > topk_group`` only among the ``topk_group`` groups of largest group score, a group being
    ``E / n_group`` consecutive experts and its score the sum of its two largest ``s + bias``; ties go to the lower
    id at both steps.  ``wts`` are the unbiased ``s`` of the chosen, renormalised when ``norm_topk``, times
    ``scale``; the balance loss takes ``P_e = mean_t s[t, e] / sum_e' s[t, e']``; the z-loss is unchanged."""
    if h.dim() != 2 or router_weight.dim() != 2 or h.shape[1] != router_weight.shape[1]:
        raise ValueError("router: h [T, D], router_weight [E, D]")
    if not 1 <= top_k <= router_weight.shape[0]:
        raise ValueError("router: 1 <= top_k <= E")
    n_group, topk_group, scale = int(n_group), int(topk_group), float(scale)
    _check_scoring(router_weight.shape[0], top_k, score, bias, n_group, topk_group, scale)
    if not router_ok(h, router_weight, top_k):
        return _router_ref(h, router_weight, top_k, norm_topk, aux_coef, z_coef, score=score, bias=bias, n_group=n_group,
                           topk_group=topk_group, scale=scale)
    idx, wts, aux, router.last_counts = _Router.apply(h, router_weight, int(top_k), bool(norm_topk), float(aux_coef),
                                                      float(z_coef), score, bias, n_group, topk_group, scale)
    return idx, wts, aux


router.last_counts = None
