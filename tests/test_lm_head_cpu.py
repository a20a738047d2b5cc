"""ops.lm_head off the fused domain (CPU): the op is the composition cross_entropy(ps_linear(h, w), labels) itself,
the config flag reaches LlamaForCausalLM.forward, and the route has its switch."""
import dataclasses

import pytest
import torch

from ps_amd import knobs
from ps_amd.models.transformer import LlamaConfig, LlamaForCausalLM
from ps_amd.ops.linear import ps_linear
from ps_amd.ops.lm_head import default_chunk_cols, linear_cross_entropy
from ps_amd.ops.transformer import cross_entropy


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fallback_is_the_composition(dtype):
    g = torch.Generator().manual_seed(0)
    h, w = torch.randn(3, 5, 64, generator=g).to(dtype), torch.randn(72, 64, generator=g).to(dtype)
    y = torch.randint(0, 72, (3, 5), generator=g, dtype=torch.int32)
    y[0, 0] = -100
    out = []
    for fn in (linear_cross_entropy, lambda h, w, y: cross_entropy(ps_linear(h, w), y.long())):
        a, b = h.clone().requires_grad_(), w.clone().requires_grad_()
        loss = fn(a, b, y)
        loss.backward()
        out.append((loss.detach(), a.grad, b.grad))
    assert all(torch.equal(p, q) for p, q in zip(*out))
    with pytest.raises(ValueError):
        linear_cross_entropy(h, w, y, chunk_cols=100)


def test_config_flag_route_and_default_chunk():
    assert "fused_head" in knobs.ROUTES and LlamaConfig().fused_head is False
    c = LlamaConfig.tiny()
    torch.manual_seed(0)
    off = LlamaForCausalLM(c)
    on = LlamaForCausalLM(dataclasses.replace(c, fused_head=True))
    on.load_state_dict(off.state_dict())
    ids = torch.randint(0, c.vocab, (2, 16))
    assert torch.equal(on(ids, labels=ids), off(ids, labels=ids)) and torch.equal(on(ids), off(ids))
    assert default_chunk_cols(16384, 128256) == 16384 and default_chunk_cols(8, 264) == 384
    assert default_chunk_cols(1 << 24, 128256) == 128
