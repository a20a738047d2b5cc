"""Head dim 64 above the attention op, the parts that need no GPU: the Llama-3.2-1B shapes, and a two-layer
model at head dim 64 forward and backward, with and without doc_ids -- nothing above the op assumes 128."""
import pytest
import torch

from ps_amd.models.transformer import LlamaConfig, LlamaForCausalLM


def test_llama32_1b_shapes():
    c = LlamaConfig.llama32_1b()
    assert (c.vocab, c.hidden, c.layers, c.ffn, c.rope_theta) == (128256, 2048, 16, 8192, 500000.0)
    assert c.hidden // c.heads == 64 and c.heads // c.kv_heads == 4


@pytest.mark.parametrize("lengths", [None, (80, 47, 1)], ids=["plain", "docs"])
def test_two_layer_model_at_head_dim_64(lengths):
    S = 128
    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig(vocab=256, hidden=128, layers=2, heads=2, kv_heads=1, ffn=256, max_seq=S)).float()
    ids = torch.randint(0, 256, (1, S))
    doc_ids = None if lengths is None else torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths))[None]
    loss = m(ids, ids.roll(-1, 1), doc_ids=doc_ids)
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    with torch.no_grad():
        logits = m(ids, doc_ids=doc_ids)
        assert logits.shape == (1, S, 256)
        s = 0
        for n in lengths or (S,):  # every document run alone gives the packed row's logits
            torch.testing.assert_close(logits[:, s:s + n], m(ids[:, s:s + n]), rtol=0, atol=1e-5)
            s += n
