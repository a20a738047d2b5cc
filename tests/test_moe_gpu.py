"""The fused mixture-of-experts FFN (csrc/kernels/moe.hip, ops/moe.py) against one fp64 oracle: every expert
evaluated densely on every token, then selected.  The bound is relative to the bf16 torch composition
(``_moe_ref``): both round the intermediate activations to bf16 at the same places but accumulate in different
orders, so per tensor the fused maximum error (relative to the tensor's maximum) stays within 2x the composition's.
Routing is hand-made so that every edge of the plan is hit at the smallest sizes (row tile 128)."""
import functools

import pytest
import torch

from ps_amd import knobs
from ps_amd.models.transformer import LlamaBlock, LlamaConfig
from ps_amd.ops import moe as M
from ps_amd.ops import transformer as TR
from ps_amd.ops._ext import native

pytestmark = pytest.mark.gpu

NAMES = ("out", "dx", "dwts", "dw13", "dw2")
# name -> (T, E, k, D, F)
CASES = {"skew": (384, 4, 2, 256, 192), "top1": (200, 4, 1, 128, 64), "all": (96, 8, 8, 64, 128),
         "odd": (131, 4, 2, 192, 64)}


def _routing(name, T, E, k):
    if name == "skew":  # expert 3: no token; expert 2: exactly token 0; expert 0: all 384 (3 tiles); expert 1: 383
        idx = torch.tensor([[0, 1]]).repeat(T, 1)
        idx[0, 1] = 2
        return idx
    if name == "all":
        return torch.arange(E).repeat(T, 1)
    g = torch.Generator().manual_seed(T)
    return torch.rand(T, E, generator=g).argsort(1)[:, :k].contiguous()  # distinct ids per token, uneven counts


def _oracle(x, idx, wts, w13, w2):
    """fp64: all experts on all tokens, then select."""
    gu = torch.einsum("td,end->etn", x, w13)
    f = w13.shape[1] // 2
    y = torch.einsum("etf,edf->etd", torch.nn.functional.silu(gu[..., :f]) * gu[..., f:], w2)  # [E, T, D]
    pick = y[idx, torch.arange(x.shape[0], device=x.device)[:, None]]  # [T, k, D]
    return (wts[..., None] * pick).sum(1)


def _run(fn, x, idx, wts, w13, w2, dout):
    x, wts, w13, w2 = (t.detach().clone().requires_grad_() for t in (x, wts, w13, w2))
    out = fn(x, idx, wts, w13, w2)
    node = type(out.grad_fn).__name__
    out.backward(dout.to(out.dtype))
    return (out.detach(), x.grad, wts.grad, w13.grad, w2.grad), node


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, the output gradient and the fp64 results; read-only."""
    T, E, k, D, F = CASES[name]
    g = torch.Generator().manual_seed(D + F)
    x = torch.randn(T, D, generator=g).bfloat16().cuda()
    w13 = (torch.randn(E, 2 * F, D, generator=g) / D ** 0.5).bfloat16().cuda()
    w2 = (torch.randn(E, D, F, generator=g) / F ** 0.5).bfloat16().cuda()
    wts = (0.25 + torch.rand(T, k, generator=g)).cuda()
    dout = torch.randn(T, D, generator=g).bfloat16().cuda()
    idx = _routing(name, T, E, k).cuda()
    ref, _ = _run(_oracle, x.double(), idx, wts.double(), w13.double(), w2.double(), dout)
    return (x, idx, wts, w13, w2, dout), ref


@pytest.mark.parametrize("name", list(CASES))
def test_fused_within_2x_of_composition(name, monkeypatch):
    args, ref = _case(name)
    fused, fn = _run(M.moe_ffn, *args)
    assert "MoeFFN" in fn  # the HIP path, not the composition
    again, _ = _run(M.moe_ffn, *args)
    monkeypatch.setenv(knobs.ENV, "moe_ffn")
    comp, fn = _run(M.moe_ffn, *args)
    assert "MoeFFN" not in fn
    for what, f, a, c, r in zip(NAMES, fused, again, comp, ref):
        assert f.dtype == c.dtype and f.shape == c.shape
        assert torch.equal(f, a), what  # two calls, bitwise
        ef, ec = (((t.double() - r).abs().max() / r.abs().max()).item() for t in (f, c))
        print(f"moe {name} {what}: fused {ef:.3e} composition {ec:.3e} ratio {ef / max(ec, 1e-300):.3f}")
        assert ef <= 2 * ec, what
    if name == "skew":  # the expert without a token: exact zeros
        assert not fused[3][3].any() and not fused[4][3].any()


def test_a_token_does_not_depend_on_the_others():
    (x, idx, wts, w13, w2, dout), _ = _case("skew")
    keep = torch.arange(0, x.shape[0], 7, device="cuda")
    x2 = -3 * x.flip(0)
    x2[keep] = x[keep]
    a, _ = _run(M.moe_ffn, x, idx, wts, w13, w2, dout)
    b, _ = _run(M.moe_ffn, x2, idx, wts, w13, w2, dout)
    assert torch.equal(a[0][keep], b[0][keep]) and torch.equal(a[1][keep], b[1][keep])
    assert not torch.equal(a[0], b[0])


def test_plan_layout_and_ids_off_the_range():
    T, E, k = 131, 4, 2
    idx = _routing("odd", T, E, k).cuda()
    idx[5, 1], idx[77, 0] = E, -1  # map to no row
    row_token, row_slot, slot_row, tile_expert, counts, seg = (t.cpu() for t in M.moe_plan(idx.int(), E))
    ids = idx.cpu().reshape(-1)
    assert row_token.numel() == 128 * ((T * k + 127) // 128 + E) and slot_row[5, 1] == -1 and slot_row[77, 0] == -1
    assert counts.tolist() == [(ids == e).sum().item() for e in range(E)]
    for e in range(E):
        pairs = (ids == e).nonzero().squeeze(1).int()  # ascending (t, j): the stable order
        s = seg[e].item()
        assert s % 128 == 0 and torch.equal(row_slot[s:s + len(pairs)], pairs)
        assert torch.equal(row_token[s:s + len(pairs)], pairs // k)
        assert torch.equal(slot_row.reshape(-1)[pairs.long()], torch.arange(s, s + len(pairs), dtype=torch.int32))
        assert (tile_expert[s // 128:(s + len(pairs) + 127) // 128] == e).all()
    assert (row_slot >= 0).sum() == counts.sum() and (tile_expert >= 0).sum() == ((counts + 127) // 128).sum()
    x = torch.randn(T, 64).bfloat16().cuda()
    w13, w2 = torch.randn(E, 128, 64).bfloat16().cuda() / 8, torch.randn(E, 64, 64).bfloat16().cuda() / 8
    wts = torch.rand(T, k).cuda()
    assert torch.equal(M.moe_ffn(x, idx, wts, w13, w2), M.moe_ffn(x, idx.clamp(-1, E).int(), wts, w13, w2))
    assert torch.isfinite(M.moe_ffn(x, idx, wts, w13, w2).float()).all()


def test_llama_block_takes_the_fused_route(monkeypatch):
    ran = []
    real = M._MoeFFN.apply
    monkeypatch.setattr(M._MoeFFN, "apply", lambda *a: ran.append(1) or real(*a))
    c = LlamaConfig.tiny_moe()
    torch.manual_seed(0)
    blk = LlamaBlock(c).cuda().bfloat16()
    x = torch.randn(2, 128, c.hidden, device="cuda").bfloat16()
    cs = TR.rope_table(128, c.hidden // c.heads, c.rope_theta, "cuda")
    _, on = blk(x, None, cs)
    assert ran == [1]
    monkeypatch.setenv(knobs.ENV, "moe_ffn")
    _, off = blk(x, None, cs)
    assert ran == [1]
    assert (on.float() - off.float()).abs().max() <= 0.05 * off.float().abs().max()


def test_bindings_refuse_what_does_not_fit():
    n = native()
    idx = torch.zeros(4, 2, dtype=torch.int32, device="cuda")
    plan = n.moe_plan(idx, 2)
    with pytest.raises(RuntimeError):
        n.moe_plan(idx, 129)
    with pytest.raises(RuntimeError):  # K not a multiple of 64
        n.moe_gemm(torch.zeros(4, 32, device="cuda").bfloat16(), torch.zeros(2, 64, 32, device="cuda").bfloat16(),
                   plan, True, None, False)
    with pytest.raises(RuntimeError):  # ungathered operand without R_cap rows
        n.moe_gemm(torch.zeros(4, 64, device="cuda").bfloat16(), torch.zeros(2, 64, 64, device="cuda").bfloat16(),
                   plan, False, None, False)
