"""The mixture-of-experts FFN off the GPU: the torch composition, the model plumbing, the route's registration."""
import torch

from ps_amd import knobs
from ps_amd.models.transformer import LlamaConfig, LlamaForCausalLM
from ps_amd.ops.moe import moe_ffn


def test_cpu_fp32_matches_the_dense_fp64_oracle():
    T, E, k, D, F = 37, 4, 2, 16, 24
    g = torch.Generator().manual_seed(0)
    x, wts = torch.randn(T, D, generator=g), torch.rand(T, k, generator=g)
    w13, w2 = torch.randn(E, 2 * F, D, generator=g) / 4, torch.randn(E, D, F, generator=g) / 5
    idx = torch.rand(T, E, generator=g).argsort(1)[:, :k]
    out = moe_ffn(x, idx, wts, w13, w2)
    gu = torch.einsum("td,end->etn", x.double(), w13.double())
    y = torch.einsum("etf,edf->etd", torch.nn.functional.silu(gu[..., :F]) * gu[..., F:], w2.double())
    ref = (wts.double()[..., None] * y[idx, torch.arange(T)[:, None]]).sum(1)
    assert out.dtype == torch.float32
    assert (out.double() - ref).abs().max() <= 64 * 2.0 ** -24 * ref.abs().max()  # fp32 rounding over D + F terms


def test_tiny_moe_model_trains_one_step():
    torch.manual_seed(0)
    c = LlamaConfig.tiny_moe()
    m = LlamaForCausalLM(c)
    ids = torch.randint(0, c.vocab, (2, 16))
    loss = m(ids, labels=ids)
    loss.backward()
    assert torch.isfinite(loss)
    blk = m.layers[0]
    for p in (blk.router.weight, blk.w13_e, blk.w2_e):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
    assert tuple(blk.w13_e.shape) == (4, 128, 64) and tuple(blk.w2_e.shape) == (4, 64, 64)


def test_no_experts_keeps_the_dense_parameter_names():
    names = [n for n, _ in LlamaForCausalLM(LlamaConfig.tiny()).layers[0].named_parameters()]
    assert names == ["attn_norm.weight", "wqkv.weight", "wo.weight", "mlp_norm.weight", "w13.weight", "w2.weight"]
    moe = [n for n, _ in LlamaForCausalLM(LlamaConfig.tiny_moe()).layers[0].named_parameters()]
    assert "w13.weight" not in moe and {"router.weight", "w13_e", "w2_e"} <= set(moe)


def test_route_is_registered():
    assert "moe_ffn" in knobs.ROUTES
    c = LlamaConfig.mixtral_8x7b()
    assert (c.hidden, c.layers, c.heads, c.kv_heads, c.moe_experts, c.moe_top_k, c.ffn, c.vocab) == \
        (4096, 32, 32, 8, 8, 2, 14336, 32000)
