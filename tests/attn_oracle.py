"""fp64 oracles, a bf16 rounding yardstick, a per-row error metric and input builders for the two
attention kernels (csrc/kernels/flash_attn.hip, csrc/kernels/attention.hip).  Plain torch on the
CPU; imported by test_attn_oracle_cpu.py, test_flash_rows_gpu.py and test_attention_rows_gpu.py.

Every function takes the bf16-rounded tensors the kernel gets and computes in fp64.  With
rounded=True the same formulas round to bf16 at the kernels' rounding points and nowhere else: P
(after dropout for the short kernel) before P V and P^T dO, dS before dS K and dS^T Q, and every
bf16 output tensor.  That variant is the yardstick: its row error against the exact variant is
what bf16 operands alone cost on the inputs at hand, and the GPU tests bound the kernels by a
multiple of it.

The backward oracles take out and lse as inputs, like fa_bwd / attn_bwd: P = exp(score - lse) and
D = rowsum(dO * out) with the out that was passed in.  (With D from an exact O the per-row dq
error is ill-conditioned on early rows, where dP - D cancels.)
"""
import math

import torch

LOG2E = 1.4426950408889634
FLASH_D, FLASH_SCALE, FLASH_TILE = 128, 1.0 / math.sqrt(128.0), 64
SHORT_D, SHORT_SCALE = 64, 0.125
RESCALE = 8.0  # fa_fwd_kernel's kRescale, exp2 units
FLASH_KINDS = {"flat": (0.0, False), "deferred": (3.0, False), "rescale": (12.0, False), "descend": (12.0, True)}


def bf16r(x):
    """Round an fp64 tensor to bf16, back in fp64."""
    return x.to(torch.bfloat16).double()


def _r(x, rounded):
    return bf16r(x) if rounded else x


def rowerr(a, ref):
    """max over last-dim rows r of |a_r - ref_r| / (|ref_r| + 0.05 rms_r |ref_r|)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    n = ref.norm(dim=-1)
    floor = 0.05 * n.pow(2).mean().sqrt()
    return ((a - ref).norm(dim=-1) / (n + floor)).max().item()


def relerr(a, ref):
    """The suite's older metric: Frobenius error of the whole tensor over its norm."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).norm() / ref.norm()).item()


# ------------------------------------------------------------------ causal GQA flash attention
def flash_scores(q, k):
    """Scaled, causally masked fp64 scores [B, H, S, S] (future keys -inf)."""
    G = q.shape[1] // k.shape[1]
    S = q.shape[2]
    sc = q.double() @ k.double().repeat_interleave(G, 1).transpose(-1, -2) * FLASH_SCALE
    return sc.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))


def flash_fwd(q, k, v, rounded=False):
    """q [B, H, S, 128], k / v [B, KV, S, 128] -> out [B, S, H * 128], lse [B, H, S]."""
    B, H, S, D = q.shape
    G = H // k.shape[1]
    sc = flash_scores(q, k)
    lse = torch.logsumexp(sc, -1)
    p = _r(torch.exp(sc - lse[..., None]), rounded)
    o = p @ v.double().repeat_interleave(G, 1)
    return _r(o.transpose(1, 2).reshape(B, S, H * D), rounded), lse


def flash_bwd(q, k, v, out, dout, lse, rounded=False):
    """-> dq [B, H, S, 128], dk, dv [B, KV, S, 128], from the out and lse that are passed in."""
    B, H, S, D = q.shape
    KV = k.shape[1]
    G = H // KV
    qd = q.double()
    kk, vv = k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    do = dout.double().view(B, S, H, D).transpose(1, 2)
    o = out.double().view(B, S, H, D).transpose(1, 2)
    p = torch.exp(flash_scores(q, k) - lse.double()[..., None])
    dsum = (do * o).sum(-1, keepdim=True)
    ds = _r(p * (do @ vv.transpose(-1, -2) - dsum), rounded)
    dq = ds @ kk * FLASH_SCALE
    dk = (ds.transpose(-1, -2) @ qd).view(B, KV, G, S, D).sum(2) * FLASH_SCALE
    dv = (_r(p, rounded).transpose(-1, -2) @ do).view(B, KV, G, S, D).sum(2)
    return _r(dq, rounded), _r(dk, rounded), _r(dv, rounded)


def flash_inputs(kind, B, H, KV, S, seed=0):
    """bf16 q, k, v, dout whose scores ramp by about g exp2 units per 64-key tile along a fixed
    direction u: flat (g = 0), deferred (3, ascending), rescale (12, ascending), descend (12,
    descending).  Under an ascending ramp every row's future keys outscore its visible ones."""
    g, rev = FLASH_KINDS[kind]
    gen = torch.Generator().manual_seed(seed)
    u = (torch.randint(0, 2, (FLASH_D,), generator=gen) * 2 - 1).double()
    c = 1.0 / (math.sqrt(FLASH_D) * LOG2E)
    t = torch.arange(S) // FLASH_TILE
    if rev:
        t = (S - 1) // FLASH_TILE - t
    q = torch.randn(B, H, S, FLASH_D, generator=gen, dtype=torch.float64) + u
    k = torch.randn(B, KV, S, FLASH_D, generator=gen, dtype=torch.float64) + c * g * t.double()[:, None] * u
    v = torch.randn(B, KV, S, FLASH_D, generator=gen, dtype=torch.float64)
    dout = torch.randn(B, S, H * FLASH_D, generator=gen, dtype=torch.float64)
    return tuple(x.to(torch.bfloat16) for x in (q, k, v, dout))


def flash_growth(q, k):
    """Growth in exp2 units, one value per (row i, tile t >= 1 with a visible key): the max visible
    score of tile t minus the max visible score of the tiles before it."""
    sc = flash_scores(q, k) * LOG2E
    S = sc.shape[-1]
    nt = S // FLASH_TILE
    tmax = sc.view(*sc.shape[:-1], nt, FLASH_TILE).amax(-1)  # [B, H, S, nt]
    grow = tmax[..., 1:] - tmax.cummax(-1).values[..., :-1]
    seen = torch.arange(1, nt)[None, :] * FLASH_TILE <= torch.arange(S)[:, None]  # [S, nt - 1]
    return grow[seen.expand_as(grow)]


# ------------------------------------------------------------------ fused short-sequence attention
def short_rkeep(p):
    """1 / (1 - p_eff), p_eff = round(p * 65536) / 65536, as launch_attn_fwd computes it."""
    thr = int(p * 65536.0 + 0.5)
    return 65536.0 / (65536.0 - thr) if thr > 0 else 1.0


def short_p_eff(p):
    return int(p * 65536.0 + 0.5) / 65536.0


def _split(qkv, heads):
    b, s, _ = qkv.shape
    return qkv.double().view(b, s, 3, heads, SHORT_D).permute(2, 0, 3, 1, 4)  # 3 x [B, H, S, 64]


def _keepf(keep, b, heads, s, p):
    if keep is None:
        return None
    return keep.double().cpu().view(b, heads, s, s) * short_rkeep(p)


def short_fwd(qkv, heads, keep=None, p=0.0, rounded=False):
    """qkv [B, S, 3 * H * 64], keep [B * H, S, S] or None -> out [B, S, H * 64], lse [B, H, S]."""
    b, s, _ = qkv.shape
    q, k, v = _split(qkv, heads)
    sc = q @ k.transpose(-1, -2) * SHORT_SCALE
    lse = torch.logsumexp(sc, -1)
    pr = torch.exp(sc - lse[..., None])
    kf = _keepf(keep, b, heads, s, p)
    if kf is not None:
        pr = pr * kf
    o = _r(pr, rounded) @ v
    return _r(o.transpose(1, 2).reshape(b, s, heads * SHORT_D), rounded), lse


def short_bwd(qkv, out, dout, lse, heads, keep=None, p=0.0, rounded=False):
    """-> dqkv [B, S, 3 * H * 64], from the out and lse that are passed in."""
    b, s, _ = qkv.shape
    q, k, v = _split(qkv, heads)
    do = dout.double().view(b, s, heads, SHORT_D).transpose(1, 2)
    o = out.double().view(b, s, heads, SHORT_D).transpose(1, 2)
    pr = torch.exp(q @ k.transpose(-1, -2) * SHORT_SCALE - lse.double()[..., None])
    dp = do @ v.transpose(-1, -2)
    pd = pr
    kf = _keepf(keep, b, heads, s, p)
    if kf is not None:
        pd, dp = pr * kf, dp * kf
    ds = _r(pr * (dp - (do * o).sum(-1, keepdim=True)), rounded)
    dv = _r(pd, rounded).transpose(-1, -2) @ do
    dq = ds @ k * SHORT_SCALE
    dk = ds.transpose(-1, -2) @ q * SHORT_SCALE
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(b, s, 3 * heads * SHORT_D)
    return _r(dqkv, rounded)


def short_inputs(scale, B, S, H, seed=0):
    """bf16 qkv = scale * randn (0.8: nearly flat softmax; 3.0: peaked) and dout = randn."""
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, 3 * H * SHORT_D, generator=gen, dtype=torch.float64) * scale
    dout = torch.randn(B, S, H * SHORT_D, generator=gen, dtype=torch.float64)
    return qkv.to(torch.bfloat16), dout.to(torch.bfloat16)


def short_row_max_prob(qkv, heads):
    """Per-row max softmax probability [B, H, S]."""
    q, k, _ = _split(qkv, heads)
    return torch.softmax(q @ k.transpose(-1, -2) * SHORT_SCALE, -1).amax(-1)
