"""Unpadded BERT without a GPU: the packed attention oracle against the padded one, pack_seqs and its
errors, unpad / repad, the attention_qkv(seqs=) fallback against SDPA on each sequence alone,
mlm_batch(packed=True), and a tiny fp32 BertForMLM whose loss and gradients with seqs= are those with
lengths=."""
import pytest
import torch
import torch.nn.functional as F

from ps_amd.models.transformer import BertConfig, BertForMLM, BertLayer, mlm_batch
from ps_amd.ops.transformer import PackedSeqs, attention_qkv, pack_seqs, repad, unpad

from . import attn_packed_oracle as apk
from . import attn_padded_oracle as apo

ROUND_OFF = 1e-12  # fp64 sums of up to 128 terms of size O(1 - 10), reordered
BID = lambda b: "x".join(map(str, b[0])) + "-" + "_".join(map(str, b[1]))  # noqa: E731


def _close(a, b):
    assert (a - b).abs().max().item() <= ROUND_OFF * max(1.0, b.abs().max().item())


# ------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("scale", [0.8, 3.0])
@pytest.mark.parametrize("batch", apk.BATCHES, ids=BID)
def test_packed_oracle_is_the_padded_oracle_at_the_valid_rows(batch, scale, p):
    (B, S, H), lens = batch
    seqs = pack_seqs(lens, S)
    M = seqs.max_len
    qkv, dout = apk.packed_inputs(scale, lens, H, seed=3)
    keep = None
    if p > 0:
        keep = (torch.rand(B * H, M, M, generator=torch.Generator().manual_seed(1)) >= p).to(torch.uint8)
    out, lse = apk.packed_fwd(qkv, H, lens, keep, p)
    assert out.shape == (seqs.total, H * 64) and lse.shape == (H, seqs.total)
    out_in, lse_in = out.to(torch.bfloat16), lse.float()
    grad = apk.packed_bwd(qkv, out_in, dout, lse_in, H, lens, keep, p)
    # the same batch re-padded to the bound the packed kernels run with; dout with zero pad rows
    short = PackedSeqs(cu=seqs.cu, index=seqs.index // S * M + seqs.pos, pos=seqs.pos, total=seqs.total, batch=B, seq=M,
                       max_len=M)
    pq, pdo = repad(qkv, short), repad(dout, short)
    pout, plse = apo.short_fwd_len(pq, H, lens, keep, p)
    _close(unpad(pout, short), out)
    _close(unpad(plse.transpose(1, 2), short).t(), lse)
    pgrad = apo.short_bwd_len(pq, repad(out_in, short), pdo, repad(lse_in.t().contiguous(), short).transpose(1, 2),
                              H, lens, keep, p)
    _close(unpad(pgrad, short), grad)


# ------------------------------------------------------------------ 2. pack_seqs, unpad, repad
@pytest.mark.parametrize("batch", apk.BATCHES, ids=BID)
@pytest.mark.parametrize("as_tensor", [False, True])
def test_pack_seqs_fields(batch, as_tensor):
    (B, S, _), lens = batch
    seqs = pack_seqs(torch.tensor(lens, dtype=torch.int32) if as_tensor else lens, S)
    assert isinstance(seqs.total, int) and seqs.total == sum(lens)
    assert (seqs.batch, seqs.seq) == (B, S)
    assert seqs.max_len == -(-max(lens) // 32) * 32 and seqs.max_len % 32 == 0 and max(lens) <= seqs.max_len <= S
    assert seqs.cu.dtype == torch.int32 and seqs.cu.tolist() == [sum(lens[:i]) for i in range(B + 1)]
    want = [(b, i) for b in range(B) for i in range(lens[b])]
    assert seqs.index.dtype == torch.int64 and seqs.index.tolist() == [b * S + i for b, i in want]
    assert seqs.pos.dtype == torch.int64 and seqs.pos.tolist() == [i for _, i in want]


def test_pack_seqs_errors():
    for bad in ([0, 3], [33], [], [4, -1]):
        with pytest.raises(ValueError):
            pack_seqs(bad, 32)
    with pytest.raises(ValueError):
        pack_seqs(torch.tensor([3.0, 4.0]), 32)
    with pytest.raises(ValueError, match="host"):
        pack_seqs(_FakeCuda([3, 4]), 32)


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: pack_seqs must refuse before it reads a value."""

    @staticmethod
    def __new__(cls, data):
        return torch.Tensor._make_subclass(cls, torch.tensor(data))

    @property
    def is_cuda(self):
        return True


@pytest.mark.parametrize("batch", apk.BATCHES, ids=BID)
def test_unpad_repad_round_trip_and_gradients(batch):
    (B, S, _), lens = batch
    seqs = pack_seqs(lens, S)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, S, 3, 5, generator=g, dtype=torch.float64).requires_grad_()
    valid = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None])[:, :, None, None]
    u = unpad(x, seqs)
    assert u.shape == (seqs.total, 3, 5)
    for b, (lo, hi) in enumerate(apk.bounds(lens)):
        assert torch.equal(u[lo:hi], x[b, :hi - lo])
    r = repad(u, seqs)
    assert torch.equal(r, x * valid)  # zeros at the pads
    assert torch.equal(unpad(r, seqs), u)
    w = torch.randn(seqs.total, 3, 5, generator=g, dtype=torch.float64)
    (u * w).sum().backward()
    assert torch.equal(x.grad, repad(w, seqs))  # unpad's gradient is repad
    t = u.detach().clone().requires_grad_()
    w2 = torch.randn(B, S, 3, 5, generator=g, dtype=torch.float64)
    (repad(t, seqs) * w2).sum().backward()
    assert torch.equal(t.grad, unpad(w2, seqs))  # and the other way round
    with pytest.raises(ValueError):
        unpad(x[:, :-1], seqs)
    with pytest.raises(ValueError):
        repad(u[:-1], seqs)


# ------------------------------------------------------------------ 3. the op on the CPU
@pytest.mark.parametrize("batch", apk.BATCHES, ids=BID)
def test_attention_qkv_seqs_is_sdpa_on_each_sequence_cpu(batch):
    (B, S, H), lens = batch
    seqs = pack_seqs(lens, S)
    torch.manual_seed(0)
    qkv = torch.randn(seqs.total, 3 * H * 64)
    x, y = qkv.clone().requires_grad_(), qkv.clone().requires_grad_()
    got = attention_qkv(x, H, 0.0, seqs=seqs)
    assert got.shape == (seqs.total, H * 64)
    refs = []
    for lo, hi in apk.bounds(lens):
        q, k, v = y[lo:hi].view(1, hi - lo, 3, H, 64).permute(2, 0, 3, 1, 4)
        refs.append(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(hi - lo, H * 64))
    ref = torch.cat(refs, 0)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)
    w = torch.randn_like(ref)
    (got * w).sum().backward()
    (ref * w).sum().backward()
    torch.testing.assert_close(x.grad, y.grad, rtol=1e-4, atol=1e-5)


def test_attention_qkv_seqs_with_mask_or_key_lengths_raises():
    seqs = pack_seqs([32, 3], 32)
    qkv = torch.randn(35, 3 * 64)
    with pytest.raises(ValueError):
        attention_qkv(qkv, 1, 0.0, key_lengths=torch.tensor([32, 3]), seqs=seqs)
    with pytest.raises(ValueError):
        attention_qkv(qkv, 1, 0.0, mask=torch.ones(2, 1, 32, 32, dtype=torch.bool), seqs=seqs)
    with pytest.raises(ValueError):
        attention_qkv(qkv[:-1], 1, 0.0, seqs=seqs)  # not T rows
    with pytest.raises(ValueError):
        attention_qkv(qkv.view(1, 35, -1), 1, 0.0, seqs=seqs)


# ------------------------------------------------------------------ 4. mlm_batch
@pytest.mark.parametrize("with_positions", [False, True])
def test_mlm_batch_packed_appends_the_packing_and_changes_nothing_else(with_positions):
    lens = [20, 13, 1, 7, 20, 2]
    a = mlm_batch(6, 20, vocab=300, seed=2, with_positions=with_positions, lengths=lens)
    b = mlm_batch(6, 20, vocab=300, seed=2, with_positions=with_positions, lengths=lens, packed=True)
    assert len(b) == len(a) + 1
    for x, y in zip(a, b):
        assert torch.equal(x, y) and x.dtype == y.dtype
    seqs = b[-1]
    assert isinstance(seqs, PackedSeqs) and seqs.total == sum(lens) and (seqs.batch, seqs.seq) == (6, 20)
    assert seqs.cu.tolist() == pack_seqs(lens, 20).cu.tolist()
    with pytest.raises(ValueError):
        mlm_batch(6, 20, vocab=300, packed=True)  # no lengths: nothing to pack


# ------------------------------------------------------------------ 5. the model
def _tiny(S):
    torch.manual_seed(0)
    c = BertConfig(vocab=512, hidden=128, layers=2, heads=2, ffn=256, max_pos=S, dropout=0.1)
    m = BertForMLM(c)
    with torch.no_grad():  # the 0.02 init attends nearly uniformly: make the scores count
        for w in m.parameters():
            if w.dim() > 1:
                w.mul_(10.0)
    return m.eval()


@pytest.mark.parametrize("with_positions", [False, True])
def test_bert_seqs_is_lengths_cpu(with_positions):
    B, S, lens = 4, 32, [32, 19, 1, 8]
    m = _tiny(S)
    ids, labels, positions, lengths, seqs = mlm_batch(B, S, vocab=512, seed=5, with_positions=True, lengths=lens,
                                                      packed=True)
    pos = positions if with_positions else None
    res = []
    for kw in (dict(lengths=lengths), dict(seqs=seqs)):
        m.zero_grad()
        loss = m(ids, labels, pos, **kw)
        loss.backward()
        res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    (l0, g0), (l1, g1) = res
    assert bool(torch.isfinite(l0)) and abs(l0.item() - l1.item()) <= 1e-5 * abs(l0.item())
    for n in g0:
        assert (g0[n] - g1[n]).abs().max().item() <= 1e-5 * g0[n].abs().max().item(), n
    # logits: at the positions as ever; without them [T, V] in packed order
    with torch.no_grad():
        ref = m(ids, None, pos, lengths=lengths)
        got = m(ids, None, pos, seqs=seqs)
    if with_positions:
        assert got.shape == ref.shape == (B * positions.shape[1], 512)
        real = (labels.gather(1, positions) != -100).reshape(-1)  # a filler may sit on a pad row
        torch.testing.assert_close(got[real], ref[real], rtol=1e-4, atol=1e-4)
    else:
        assert got.shape == (seqs.total, 512)
        torch.testing.assert_close(got, unpad(ref.view(B, S, 512), seqs), rtol=1e-4, atol=1e-4)


def test_bert_layer_seqs_runs_on_the_valid_tokens_cpu():
    B, S, lens = 3, 32, [32, 5, 17]
    m = _tiny(S)
    layer: BertLayer = m.layers[0]
    seqs = pack_seqs(lens, S)
    x = torch.randn(B, S, 128, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = layer(x, key_lengths=torch.tensor(lens))
        got = layer(unpad(x, seqs), seqs=seqs)
    assert got.shape == (seqs.total, 128)
    torch.testing.assert_close(got, unpad(ref, seqs), rtol=1e-4, atol=1e-4)


def test_bert_lengths_with_seqs_raises():
    m = _tiny(32)
    ids, labels, lengths, seqs = mlm_batch(2, 32, vocab=512, seed=5, lengths=[32, 4], packed=True)
    with pytest.raises(ValueError):
        m(ids, labels, lengths=lengths, seqs=seqs)
    with pytest.raises(ValueError):
        m(ids[:, :16], labels[:, :16], seqs=seqs)  # not the batch the packing describes
