"""Right-padded batches without a GPU: the padded attention oracle against the existing one, the
attention_qkv key_lengths fallback against SDPA with the explicit mask, mlm_batch with lengths,
and a tiny BertForMLM whose loss and gradients do not see what the pad tokens are."""
import pytest
import torch
import torch.nn.functional as F

from ps_amd.models.transformer import BertConfig, BertForMLM, mlm_batch
from ps_amd.ops.transformer import attention_qkv, key_lengths_from_mask

from . import attn_oracle as ao
from . import attn_padded_oracle as apo

B, S, H = 3, 64, 2
LENS = [64, 33, 1]
ROUND_OFF = 1e-12  # fp64 sums of 64 terms of size O(1 - 10), reordered


def _thirds(dqkv, heads):
    b, s, _ = dqkv.shape
    return dqkv.view(b, s, 3, heads, ao.SHORT_D).unbind(2)


def _close(a, b):
    assert (a - b).abs().max().item() <= ROUND_OFF * max(1.0, b.abs().max().item())


# ------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("scale", [0.8, 3.0])
def test_padded_oracle_is_the_unpadded_oracle_on_each_truncated_sequence(scale, p):
    qkv, dout = ao.short_inputs(scale, B, S, H, seed=3)
    keep = None
    if p > 0:
        keep = (torch.rand(B * H, S, S, generator=torch.Generator().manual_seed(1)) >= p).to(torch.uint8)
    out, lse = apo.short_fwd_len(qkv, H, LENS, keep, p)
    # the truncated sequence has no queries >= L: take their dout out of the padded batch too
    valid = torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]
    dout0 = dout * valid[..., None]
    out_in, lse_in = out.to(torch.bfloat16), lse.float()
    grad = apo.short_bwd_len(qkv, out_in, dout0, lse_in, H, LENS, keep, p)
    for b, L in enumerate(LENS):
        kb = None if keep is None else keep[b * H:(b + 1) * H, :L, :L].contiguous()
        tout, tlse = ao.short_fwd(qkv[b:b + 1, :L], H, kb, p)
        _close(out[b:b + 1, :L], tout)
        _close(lse[b:b + 1, :, :L], tlse)
        tgrad = ao.short_bwd(qkv[b:b + 1, :L], out_in[b:b + 1, :L], dout[b:b + 1, :L], lse_in[b:b + 1, :, :L], H, kb, p)
        for got, ref in zip(_thirds(grad[b:b + 1, :L].contiguous(), H), _thirds(tgrad, H)):
            _close(got, ref)
    # with every query's dout in: dk and dv rows >= L are zeros
    full = apo.short_bwd_len(qkv, out_in, dout, lse_in, H, LENS, keep, p)
    for b, L in enumerate(LENS):
        _, dk, dv = _thirds(full[b:b + 1], H)
        assert bool((dk[:, L:] == 0).all()) and bool((dv[:, L:] == 0).all())
        assert bool((dv[:, :L] != 0).all())  # (dk of a single key is zero: its softmax is constant)


@pytest.mark.parametrize("rounded", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_padded_oracle_with_full_lengths_equals_the_existing_oracle_exactly(p, rounded):
    qkv, dout = ao.short_inputs(3.0, 2, 96, 3, seed=4)
    keep = None
    if p > 0:
        keep = (torch.rand(2 * 3, 96, 96, generator=torch.Generator().manual_seed(2)) >= p).to(torch.uint8)
    out, lse = ao.short_fwd(qkv, 3, keep, p, rounded=rounded)
    pout, plse = apo.short_fwd_len(qkv, 3, [96, 96], keep, p, rounded=rounded)
    assert torch.equal(out, pout) and torch.equal(lse, plse)
    out_in, lse_in = out.to(torch.bfloat16), lse.float()
    assert torch.equal(ao.short_bwd(qkv, out_in, dout, lse_in, 3, keep, p, rounded=rounded),
                       apo.short_bwd_len(qkv, out_in, dout, lse_in, 3, [96, 96], keep, p, rounded=rounded))


# ------------------------------------------------------------------ 2. the op on the CPU
def _sdpa(qkv, heads, mask):
    b, s, _ = qkv.shape
    q, k, v = qkv.view(b, s, 3, heads, -1).permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(b, s, -1)


def _prefix(lengths, s):
    return torch.arange(s)[None, :] < torch.as_tensor(lengths)[:, None]


def test_attention_qkv_key_lengths_is_sdpa_with_the_key_mask_cpu():
    torch.manual_seed(0)
    qkv = torch.randn(B, S, 3 * H * 64)
    x = qkv.clone().requires_grad_()
    y = qkv.clone().requires_grad_()
    got = attention_qkv(x, H, 0.0, key_lengths=torch.tensor(LENS))
    ref = _sdpa(y, H, _prefix(LENS, S)[:, None, None, :])
    torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6)
    w = torch.randn_like(ref)
    (got * w).sum().backward()
    (ref * w).sum().backward()
    torch.testing.assert_close(x.grad, y.grad, rtol=1e-5, atol=1e-6)
    k, v = x.grad.view(B, S, 3, H * 64).unbind(2)[1:]
    for b, L in enumerate(LENS):
        assert bool((k[b, L:] == 0).all()) and bool((v[b, L:] == 0).all())


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.int16])
def test_attention_qkv_key_lengths_clamp_to_1_S_cpu(dtype):
    torch.manual_seed(1)
    qkv = torch.randn(4, 32, 3 * 64)
    got = attention_qkv(qkv, 1, 0.0, key_lengths=torch.tensor([0, -5, 33, 1000], dtype=dtype))
    ref = attention_qkv(qkv, 1, 0.0, key_lengths=torch.tensor([1, 1, 32, 32]))
    assert torch.equal(got, ref)
    torch.testing.assert_close(ref[2:], attention_qkv(qkv[2:], 1, 0.0), rtol=1e-6, atol=1e-6)  # full: unmasked
    assert bool(torch.isfinite(got).all())


def test_attention_qkv_mask_with_key_lengths_raises():
    qkv = torch.randn(2, 32, 3 * 64)
    with pytest.raises(ValueError):
        attention_qkv(qkv, 1, 0.0, mask=torch.ones(2, 1, 32, 32, dtype=torch.bool), key_lengths=torch.tensor([32, 3]))
    with pytest.raises(ValueError):
        attention_qkv(qkv, 1, 0.0, key_lengths=torch.tensor([32, 3, 4]))  # not one per batch row
    with pytest.raises(ValueError):
        attention_qkv(qkv, 1, 0.0, key_lengths=torch.tensor([32.0, 3.0]))


def test_key_lengths_from_mask_round_trips_a_prefix_mask_and_rejects_others():
    lens = torch.tensor([5, 1, 32, 17])
    mask = _prefix(lens, 32)
    assert torch.equal(key_lengths_from_mask(mask), lens)
    assert torch.equal(key_lengths_from_mask(mask.long()), lens)
    left = mask.flip(1)  # left padding
    with pytest.raises(ValueError):
        key_lengths_from_mask(left)
    hole = mask.clone()
    hole[2, 7] = False
    with pytest.raises(ValueError):
        key_lengths_from_mask(hole)
    with pytest.raises(ValueError):
        key_lengths_from_mask(mask[0])


# ------------------------------------------------------------------ 3. mlm_batch
@pytest.mark.parametrize("with_positions", [False, True])
def test_mlm_batch_without_lengths_is_unchanged(with_positions):
    a = mlm_batch(8, 20, vocab=300, seed=1, with_positions=with_positions)
    b = mlm_batch(8, 20, vocab=300, seed=1, with_positions=with_positions, lengths=None)
    assert len(a) == len(b) == (3 if with_positions else 2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # and what it always was: full-length sequences, round(0.15 * 20) = 3 [MASK]s each
    ids, labels = a[0], a[1]
    assert bool((ids >= 103).all()) and bool(((ids == 103).sum(1) == 3).all())
    assert bool(((labels != -100) == (ids == 103)).all())


@pytest.mark.parametrize("lengths", [[20, 13, 1, 7, 20, 2], 9])
def test_mlm_batch_with_lengths(lengths):
    nb, s = 6, 20
    ids, labels, positions, lens = mlm_batch(nb, s, vocab=300, seed=2, with_positions=True, lengths=lengths)
    want = torch.tensor(lengths).expand(nb) if isinstance(lengths, int) else torch.tensor(lengths)
    assert torch.equal(lens, want) and lens.dtype == torch.int64
    ids2, labels2, lens2 = mlm_batch(nb, s, vocab=300, seed=2, lengths=lengths)
    assert torch.equal(ids, ids2) and torch.equal(labels, labels2) and torch.equal(lens, lens2)
    pad = torch.arange(s)[None, :] >= lens[:, None]
    assert bool((ids[pad] == 0).all()) and bool((labels[pad] == -100).all())
    assert bool((ids[~pad] >= 103).all())
    npred = torch.tensor([max(1, int(round(0.15 * n))) for n in lens.tolist()])
    masked = labels != -100
    assert torch.equal(masked.sum(1), npred)
    assert bool(((ids == 103) == masked).all())
    assert positions.shape == (nb, int(npred.max()))
    at = labels.gather(1, positions)  # the label the head sees at each position
    assert torch.equal((at != -100).sum(1), npred)  # every masked token once, fillers ignored
    assert bool((positions[at != -100] < lens[:, None].expand_as(positions)[at != -100]).all())
    # a filler repeats a valid position where the sequence has an unmasked one
    some = (lens > npred)[:, None].expand_as(positions)
    assert bool((positions[some] < lens[:, None].expand_as(positions)[some]).all())


def test_mlm_batch_rejects_lengths_out_of_range():
    for bad in (0, 21, [20, 0], [1, 2, 3]):
        with pytest.raises(ValueError):
            mlm_batch(2, 20, vocab=300, lengths=bad)


# ------------------------------------------------------------------ 4. the model
def test_bert_loss_and_gradients_do_not_see_the_pad_ids_cpu():
    torch.manual_seed(0)
    c = BertConfig(vocab=512, hidden=128, layers=2, heads=2, ffn=256, max_pos=64, dropout=0.0)
    m = BertForMLM(c)
    with torch.no_grad():  # the 0.02 init attends nearly uniformly: make the scores count
        for w in m.parameters():
            if w.dim() > 1:
                w.mul_(10.0)
    ids, labels, positions, lens = mlm_batch(B, S, vocab=512, seed=5, with_positions=True, lengths=LENS)
    pad = torch.arange(S)[None, :] >= lens[:, None]
    other = torch.where(pad, torch.randint(1, 512, (B, S), generator=torch.Generator().manual_seed(6)), ids)
    assert bool((other[pad] != ids[pad]).all())
    res = []
    for x in (ids, other):
        m.zero_grad()
        loss = m(x, labels, positions, lengths=lens)
        loss.backward()
        res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    (l0, g0), (l1, g1) = res
    assert abs(l0.item() - l1.item()) <= 1e-6 * abs(l0.item())
    for n in g0:
        assert (g0[n] - g1[n]).abs().max().item() <= 1e-6 * g0[n].abs().max().item(), n
    # without the lengths the pad ids are attended to, and the loss moves
    assert abs(m(ids, labels, positions).item() - m(other, labels, positions).item()) > 1e-4 * abs(l0.item())
