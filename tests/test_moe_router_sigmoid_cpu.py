"""ops.moe.router with sigmoid scores off the GPU: ``_router_ref``'s group-limited choice on a hand-computed example,
its gradients against finite differences in fp64, and the new config fields."""
import dataclasses

import pytest
import torch

from ps_amd.models.transformer import LlamaBlock, LlamaConfig, LlamaForCausalLM
from ps_amd.ops import moe as M


def test_chosen_experts_lie_in_the_kept_group():
    # z[t, e] = w[e, t]; two groups of two, one kept.  Row 0: s = (.953, .047 | .731, .818), group scores with the
    # bias 1.10 < 1.55: group 1 is kept although expert 0 has the largest score.  Row 1: all s = .5, the bias on
    # expert 1 lifts group 0 (1.1 > 1.0) and puts expert 1 first; the weights are the unbiased scores.
    h = torch.eye(2, dtype=torch.float64)
    w = torch.tensor([[3.0, 0.0], [-3.0, 0.0], [1.0, 0.0], [1.5, 0.0]], dtype=torch.float64)
    bias = torch.tensor([0.0, 0.1, 0.0, 0.0])
    kw = dict(score="sigmoid", n_group=2, topk_group=1, scale=2.5)
    idx, wts, _ = M.router(h, w, 2, True, bias=bias, **kw)
    assert idx.tolist() == [[3, 2], [1, 0]]
    s = torch.sigmoid(torch.tensor([1.5, 1.0], dtype=torch.float64))
    assert torch.allclose(wts, torch.stack([2.5 * s / s.sum(), torch.tensor([1.25, 1.25], dtype=torch.float64)]))
    assert M.router(h, w, 2, True, **kw)[0].tolist() == [[3, 2], [0, 1]]  # no bias: the tie goes to group 0, expert 0
    assert M.router(h, w, 2, True, score="sigmoid", n_group=2, topk_group=2)[0].tolist() == [[0, 3], [0, 1]]  # no limit


@pytest.mark.parametrize("norm", [True, False])
def test_reference_gradients_in_fp64(norm):
    g = torch.Generator().manual_seed(0)
    h = torch.randn(5, 8, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(6, 8, generator=g, dtype=torch.float64) / 3).requires_grad_()
    bias = torch.rand(6, generator=g) * 0.2 - 0.1
    kw = dict(score="sigmoid", bias=bias, n_group=3, topk_group=2, scale=2.5)
    idx = M._router_ref(h, w, 2, norm, **kw)[0]  # fixed: the function is smooth
    assert torch.autograd.gradcheck(lambda a, b: M._router_ref(a, b, 2, norm, 0.5, 0.25, idx, **kw)[1:], (h, w))


def test_config_defaults_state_dict_keys_and_bias_update():
    c = LlamaConfig.tiny_moe()
    assert (c.moe_score, c.moe_n_group, c.moe_topk_group, c.moe_route_scale, c.moe_bias_balance) == \
        ("softmax", 1, 1, 1.0, False)
    assert sorted(LlamaBlock(c).state_dict()) == ["attn_norm.weight", "mlp_norm.weight", "router.weight", "w13_e",
                                                  "w2_e", "wo.weight", "wqkv.weight"]
    torch.manual_seed(0)
    m = LlamaForCausalLM(dataclasses.replace(c, moe_score="sigmoid", moe_bias_balance=True, moe_n_group=2))
    assert all("router_bias" in blk.state_dict() for blk in m.layers)
    m(torch.randint(0, c.vocab, (2, 16)))
    counts = [blk.last_counts.float() for blk in m.layers]
    m.update_router_bias(1e-2)
    for blk, n in zip(m.layers, counts):
        assert n.sum() == 2 * 16 * c.moe_top_k and torch.equal(blk.router_bias, 1e-2 * torch.sign(n.mean() - n))
