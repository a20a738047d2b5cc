"""Per-head QK RMSNorm in rope_split and LlamaConfig.qk_norm: the composition path and the model plumbing."""
import dataclasses

import pytest
import torch

from ps_amd.models.transformer import LlamaConfig, LlamaForCausalLM, param_count
from ps_amd.ops import transformer as T

B, S, H, KV, HD = 2, 5, 4, 2, 16  # LlamaConfig.tiny() heads and head dim


def _ref64(qkv, cs, wq, wk, eps):
    """q, k, v in fp64, written out: normalise each head row, scale, rotate halves."""
    q, k, v = qkv.transpose(1, 2).split([H, KV, KV], dim=1)
    c, s = cs[..., 0].double(), cs[..., 1].double()

    def nr(x, w):
        y = x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps) * w
        y1, y2 = y[..., :HD // 2], y[..., HD // 2:]
        return torch.cat([y1 * c - y2 * s, y2 * c + y1 * s], dim=-1)

    return nr(q, wq), nr(k, wk), v


def test_op_against_fp64():
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, S, H + 2 * KV, HD, generator=g)
    wq, wk = (0.5 + torch.rand(HD, generator=g) for _ in range(2))
    cs = T.rope_table(S, HD, 500000.0, "cpu")
    grads = [torch.randn(B, h, S, HD, generator=g) for h in (H, KV, KV)]
    res = []
    for dt in (torch.float32, torch.float64):
        a, wa, wb = (t.clone().to(dt).requires_grad_() for t in (qkv, wq, wk))
        out = T.rope_split(a, cs, H, KV, wa, wb, 1e-6) if dt == torch.float32 else _ref64(a, cs, wa, wb, 1e-6)
        torch.autograd.backward(out, [t.to(dt) for t in grads])
        res.append(tuple(out) + (a.grad, wa.grad, wb.grad))
    for got, want in zip(*res):
        # fp32 against fp64: a few hundred roundings of 6e-8 on values of order 1 - 10
        torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError):  # one weight without the other
        T.rope_split(qkv, cs, H, KV, q_norm=wq)


def _closed_form(c):
    hd = c.hidden // c.heads
    block = (2 * c.hidden + c.hidden * (c.heads + 2 * c.kv_heads) * hd + c.heads * hd * c.hidden
             + 3 * c.ffn * c.hidden + (2 * hd if c.qk_norm else 0))
    return 2 * c.vocab * c.hidden + c.hidden + c.layers * block


def test_state_dict_and_parameter_count():
    c = LlamaConfig.tiny()
    hd = c.hidden // c.heads
    plain, normed = LlamaForCausalLM(c), LlamaForCausalLM(dataclasses.replace(c, qk_norm=True))
    keys = set(plain.state_dict())
    assert not any("q_norm" in k or "k_norm" in k for k in keys) and param_count(plain) == _closed_form(c)
    new = {k: v for k, v in normed.state_dict().items() if k not in keys}
    assert len(new) == 2 * c.layers and set(normed.state_dict()) - set(new) == keys
    assert all(tuple(v.shape) == (hd,) for v in new.values())
    assert param_count(normed) == param_count(plain) + 2 * c.layers * hd


def test_qwen3_8b_config_arithmetic():
    c = LlamaConfig.qwen3_8b()
    assert (c.hidden, c.layers, c.heads, c.kv_heads, c.ffn, c.vocab) == (4096, 36, 32, 8, 12288, 151936)
    assert (c.rope_theta, c.eps, c.qk_norm) == (1e6, 1e-6, True)
    cut = dataclasses.replace(c, layers=2)
    with torch.device("meta"):  # shapes only: no 5 GB of weights
        m = LlamaForCausalLM(cut)
    assert param_count(m) == _closed_form(cut)


def test_training_smoke():
    torch.manual_seed(0)
    c = dataclasses.replace(LlamaConfig.tiny(), qk_norm=True)
    m = LlamaForCausalLM(c)
    ids = torch.randint(0, c.vocab, (2, 16))
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    losses = []
    for step in range(4):
        opt.zero_grad()
        loss = m(ids, ids)
        loss.backward()
        if step == 0:
            for p in (p for layer in m.layers for p in (layer.q_norm, layer.k_norm)):
                assert torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
        losses.append(loss.item())
        opt.step()
    assert losses[3] < losses[0]  # three optimizer steps on a fixed batch
