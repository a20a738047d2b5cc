"""Packed documents, the parts that need no GPU: doc_bounds, the fp64 document oracle against the
plain oracle on each document alone, attention_causal_gqa's SDPA path with doc_bounds,
LlamaForCausalLM with doc_ids (logits and loss of a packed row against its documents run alone)
and packed_lm_batch."""
import pytest
import torch

from ps_amd.models.transformer import LlamaConfig, LlamaForCausalLM, packed_lm_batch
from ps_amd.ops.transformer import attention_causal_gqa, doc_bounds

from . import attn_oracle as ao
from . import flash_docs_oracle as fo


# ------------------------------------------------------------------ 1. doc_bounds
BOUND_ROWS = [[80, 48], [64, 1, 63], [128], [1] * 128]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_doc_bounds_on_hand_written_rows(dtype):
    ids = fo.doc_ids_from_lengths(BOUND_ROWS, dtype)
    ids = ids * 7 + 3  # the values mean nothing but "changed"
    ids[1, 64] = -5
    start, end = doc_bounds(ids)
    assert start.dtype == torch.int32 and end.dtype == torch.int32
    assert start.shape == ids.shape and end.shape == ids.shape and start.device == ids.device
    for b, lengths in enumerate(BOUND_ROWS):
        want_s = torch.cat([torch.full((e - s,), s) for s, e in fo.doc_spans(lengths)]).int()
        want_e = torch.cat([torch.full((e - s,), e) for s, e in fo.doc_spans(lengths)]).int()
        assert torch.equal(start[b], want_s), lengths
        assert torch.equal(end[b], want_e), lengths
    pos = torch.arange(128)[None]
    assert bool(((start <= pos) & (pos < end)).all())
    assert bool((start[:, 1:] >= start[:, :-1]).all()) and bool((end[:, 1:] >= end[:, :-1]).all())


def test_doc_bounds_ids_may_repeat_after_a_gap():
    """Only a change starts a document: ids 0 0 1 1 0 0 are three documents."""
    start, end = doc_bounds(torch.tensor([[0, 0, 1, 1, 0, 0]]))
    assert start.tolist() == [[0, 0, 2, 2, 4, 4]] and end.tolist() == [[2, 2, 4, 4, 6, 6]]


def test_doc_bounds_errors():
    with pytest.raises(ValueError):
        doc_bounds(torch.zeros(2, 8))
    with pytest.raises(ValueError):
        doc_bounds(torch.zeros(2, 8, dtype=torch.bool))
    with pytest.raises(ValueError):
        doc_bounds(torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError):
        doc_bounds(torch.zeros(1, 2, 8, dtype=torch.int64))


# ------------------------------------------------------------------ 2. the oracle
@pytest.mark.parametrize("lengths", [[80, 48], [1, 1, 2, 4, 8, 16, 32, 64]], ids=["80-48", "pow2"])
def test_oracle_on_a_packed_row_is_the_plain_oracle_on_each_document(lengths):
    H, KV, S, D = 4, 2, 128, ao.FLASH_D
    q, k, v, dout = ao.flash_inputs("rescale", 1, H, KV, S, seed=3)
    ids = fo.doc_ids_from_lengths([lengths])
    out, lse = fo.flash_docs_fwd(q, k, v, ids)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    out_in, lse_in = out.to(torch.bfloat16), lse.float()
    dq, dk, dv = fo.flash_docs_bwd(q, k, v, out_in, dout, lse_in, ids)
    tol = dict(rtol=0, atol=1e-10)
    for s, e in fo.doc_spans(lengths):
        qa, ka, va, da = q[:, :, s:e], k[:, :, s:e], v[:, :, s:e], dout[:, s:e]
        o1, l1 = ao.flash_fwd(qa, ka, va)
        torch.testing.assert_close(out[:, s:e], o1, **tol)
        torch.testing.assert_close(lse[:, :, s:e], l1, **tol)
        g1 = ao.flash_bwd(qa, ka, va, out_in[:, s:e], da, lse_in[:, :, s:e])
        for got, want in zip((dq, dk, dv), g1):
            torch.testing.assert_close(got[:, :, s:e], want, **tol)


def test_oracle_mask_differs_from_the_plain_oracle():
    q, k, v, _ = ao.flash_inputs("flat", 1, 2, 1, 128, seed=4)
    ids = fo.doc_ids_from_lengths([[80, 48]])
    out, _ = fo.flash_docs_fwd(q, k, v, ids)
    plain, _ = ao.flash_fwd(q, k, v)
    torch.testing.assert_close(out[:, :80], plain[:, :80], rtol=0, atol=1e-12)
    assert (out[:, 80:] - plain[:, 80:]).abs().max().item() > 1e-2


# ------------------------------------------------------------------ 3. the op on the CPU (SDPA path)
@pytest.mark.parametrize("lengths", [[80, 48], [64, 1, 63]], ids=["80-48", "64-1-63"])
def test_op_with_doc_bounds_is_the_plain_op_on_each_document(lengths):
    B, H, KV, S, D = 2, 4, 2, 128, 16
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B, h, S, D, generator=g).requires_grad_() for h in (H, KV, KV))
    dout = torch.randn(B, S, H * D, generator=g)
    ids = fo.doc_ids_from_lengths([lengths] * B)
    out = attention_causal_gqa(q, k, v, doc_bounds=doc_bounds(ids))
    assert out.shape == (B, S, H * D)
    grads = torch.autograd.grad(out, (q, k, v), dout)
    for s, e in fo.doc_spans(lengths):
        qa, ka, va = (t.detach()[:, :, s:e].clone().requires_grad_() for t in (q, k, v))
        o1 = attention_causal_gqa(qa, ka, va)
        g1 = torch.autograd.grad(o1, (qa, ka, va), dout[:, s:e])
        torch.testing.assert_close(out[:, s:e], o1, rtol=0, atol=1e-5)
        for got, want in zip(grads, g1):
            torch.testing.assert_close(got[:, :, s:e], want, rtol=0, atol=1e-5)


def test_op_rejects_bounds_of_another_shape():
    q, k, v = torch.randn(2, 4, 128, 16), torch.randn(2, 2, 128, 16), torch.randn(2, 2, 128, 16)
    start, end = doc_bounds(fo.doc_ids_from_lengths([[80, 48]] * 2))
    with pytest.raises(ValueError):
        attention_causal_gqa(q, k, v, doc_bounds=(start[:1], end[:1]))
    with pytest.raises(ValueError):
        attention_causal_gqa(q, k, v, doc_bounds=(start[:, :64], end[:, :64]))
    with pytest.raises(ValueError):
        attention_causal_gqa(q, k, v, doc_bounds=(start, end[:, :64]))
    with pytest.raises(ValueError):
        attention_causal_gqa(q, k, v, doc_bounds=start)


# ------------------------------------------------------------------ 4. the model
def test_llama_packed_row_is_its_documents_run_alone():
    lengths = [80, 47, 1]
    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig.tiny()).float().eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(10.0)
    ids, labels, doc_ids = packed_lm_batch(1, 128, 512, [lengths], seed=1)
    with torch.no_grad():
        packed = m(ids, doc_ids=doc_ids)
        unmasked = m(ids)
        loss = m(ids, labels, doc_ids=doc_ids)
        worst, leak, total, count = 0.0, 0.0, 0.0, 0
        for i, (s, e) in enumerate(fo.doc_spans(lengths)):
            alone = m(ids[:, s:e])
            worst = max(worst, (packed[:, s:e] - alone).abs().max().item())
            if i > 0:
                leak = max(leak, (unmasked[:, s:e] - alone).abs().max().item())
            if e - s > 1:  # a one-token document has no target
                total += m(ids[:, s:e], labels[:, s:e]).item() * (e - s - 1)
                count += e - s - 1
    print(f"packed vs alone: {worst:.3g}; without doc_ids: {leak:.3g}; logit scale {packed.abs().max().item():.3g}")
    assert worst <= 1e-4
    assert leak > 1.0
    assert abs(loss.item() - total / count) <= 1e-5


def test_llama_doc_ids_of_another_shape_raise():
    m = LlamaForCausalLM(LlamaConfig.tiny()).float().eval()
    ids = torch.zeros(1, 128, dtype=torch.int64)
    with pytest.raises(ValueError):
        m(ids, doc_ids=torch.zeros(1, 64, dtype=torch.int64))


# ------------------------------------------------------------------ 5. packed_lm_batch
def test_packed_lm_batch():
    rows = [[80, 48], [64, 1, 63], [128]]
    ids, labels, doc_ids = packed_lm_batch(3, 128, 512, rows, seed=2)
    for t in (ids, labels, doc_ids):
        assert t.shape == (3, 128) and t.dtype == torch.int64
    assert int(ids.min()) >= 0 and int(ids.max()) < 512
    assert torch.equal(labels, ids)
    for b, r in enumerate(rows):
        assert torch.unique_consecutive(doc_ids[b], return_counts=True)[1].tolist() == r
    again = packed_lm_batch(3, 128, 512, rows, seed=2)
    assert all(torch.equal(a, b) for a, b in zip((ids, labels, doc_ids), again))
    with pytest.raises(ValueError):
        packed_lm_batch(2, 128, 512, [[80, 48], [64, 63]])
    with pytest.raises(ValueError):
        packed_lm_batch(2, 128, 512, [[128]])
