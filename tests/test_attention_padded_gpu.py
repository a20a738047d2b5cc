"""Fused short-sequence attention (csrc/kernels/attention.hip) on right-padded batches: per-sequence
key lengths L_b, keys >= L_b out of every softmax.  Shapes and lengths reach every branch of the
kernels: a full sequence, a partly valid last key block, key waves padded in full, one single key,
lengths on, one past and one short of a 32-key block edge.

1. every 64-wide row of out and of the q, k and v thirds of dqkv against the fp64 oracle of
   tests/attn_padded_oracle.py, bounded by three times the row error of the bf16 rounding yardstick on
   the same inputs and keep mask (the bound of test_attention_rows_gpu.py); the backward is fed the
   oracle's out and lse;
2. dk and dv rows >= L_b are exact zeros;
3. lengths all equal to S give bitwise what the calls without lengths give;
4. what the pad rows of k and v hold cannot leak: +-1e4 randn there changes no bit of any output;
5. two calls are bitwise equal;
6. attention_qkv(key_lengths=) with autograd: the fused kernels against SDPA with the key mask;
7. a tiny BertForMLM: loss and gradients bitwise unchanged when the pad ids are replaced.

Observed on MI355X: rowerr(kernel) / rowerr(yardstick) is 1.00 in 63 of the 64 (case, tensor) pairs of
test 1 and 0.95 in one (the bound is 3; the yardstick's own rowerr is 0.0028 - 0.0045); tests 2 - 5 and
7 hold bitwise, no library GEMM breaks the bit equality of test 7.
"""
import functools

import pytest
import torch

from ps_amd.models.transformer import BertConfig, BertForMLM, mlm_batch
from ps_amd.ops import native
from ps_amd.ops import transformer as T

from . import attn_oracle as ao
from . import attn_padded_oracle as apo

pytestmark = pytest.mark.gpu
DEV = "cuda"

BATCHES = [((4, 128, 2), [128, 97, 33, 1]), ((3, 96, 3), [64, 65, 31]), ((2, 32, 1), [32, 7]), ((2, 64, 5), [63, 32])]
FACTOR = 3.0
HIGH = 7 << 40

CASES = [(batch, scale, p) for batch in BATCHES for scale in (0.8, 3.0) for p in (0.0, 0.1)]
PAIRS = [(batch, p) for batch in BATCHES for p in (0.0, 0.1)]


def _seed(i):
    return 12345 + (HIGH if i % 2 else 0)  # the p = 0.1 cases: a seed above 2^32


def _id(case):
    i, (((B, S, H), _), scale, p) = case
    return f"{B}x{S}x{H}-s{scale}-p{p}-{'hi' if _seed(i) >> 32 else 'lo'}"


def _pid(pair):
    ((B, S, H), _), p = pair
    return f"{B}x{S}x{H}-p{p}"


def _thirds(dqkv, heads):
    b, s, _ = dqkv.shape
    return dqkv.view(b, s, 3, heads, ao.SHORT_D).unbind(2)


def _klen(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs, keep mask, fp64 oracle and yardstick of one case, computed once and left unchanged."""
    ((B, S, H), lens), scale, p = CASES[i]
    seed = _seed(i)
    qkv, dout = ao.short_inputs(scale, B, S, H, seed=100 + i)
    keep = native().attn_dropout_mask(qkv.to(DEV), B * H, S, p, seed).cpu() if p > 0 else None
    out, lse = apo.short_fwd_len(qkv, H, lens, keep, p)
    yout, _ = apo.short_fwd_len(qkv, H, lens, keep, p, rounded=True)
    out_in, lse_in = out.to(torch.bfloat16), lse.float()  # what attn_bwd is given
    grad = apo.short_bwd_len(qkv, out_in, dout, lse_in, H, lens, keep, p)
    ygrad = apo.short_bwd_len(qkv, out_in, dout, lse_in, H, lens, keep, p, rounded=True)
    return dict(qkv=qkv, dout=dout, H=H, p=p, seed=seed, lens=lens, out=out, lse=lse, yout=yout, out_in=out_in,
                lse_in=lse_in, grad=grad, ygrad=ygrad)


def _bound(name, tag, got, ref, yard):
    e, y = ao.rowerr(got, ref), ao.rowerr(yard, ref)
    print(f"RATIO padded {tag} {name}: kernel {e:.5f} yardstick {y:.5f} ratio {e / y:.2f}")
    assert y > 0
    assert e <= FACTOR * y, (name, e, y)


def _bwd(c, qkv=None):
    return native().attn_bwd((c["qkv"] if qkv is None else qkv).to(DEV), c["out_in"].to(DEV), c["dout"].to(DEV),
                             c["lse_in"].to(DEV), c["H"], c["p"], c["seed"], _klen(c["lens"]))


# ------------------------------------------------------------------ 1. per row against the oracle
@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=_id)
def test_padded_forward_rows(case):
    c = _case(case[0])
    H = c["H"]
    out, lse = native().attn_fwd(c["qkv"].to(DEV), H, c["p"], c["seed"], _klen(c["lens"]))
    rows = lambda x: x.view(*x.shape[:2], H, ao.SHORT_D)  # noqa: E731
    _bound("out", _id(case), rows(out), rows(c["out"]), rows(c["yout"]))
    torch.testing.assert_close(lse.cpu(), c["lse"].float(), rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=_id)
def test_padded_backward_rows(case):
    c = _case(case[0])
    H = c["H"]
    dqkv = _bwd(c)
    assert dqkv.shape == c["grad"].shape
    for name, g, ref, yard in zip(("dq", "dk", "dv"), _thirds(dqkv, H), _thirds(c["grad"], H), _thirds(c["ygrad"], H)):
        _bound(name, _id(case), g, ref, yard)


# ------------------------------------------------------------------ 2. dk, dv of pad rows
@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=_id)
def test_padded_backward_pad_rows_are_exact_zeros(case):
    c = _case(case[0])
    dq, dk, dv = _thirds(_bwd(c), c["H"])
    for b, L in enumerate(c["lens"]):
        assert bool((dk[b, L:] == 0).all()) and bool((dv[b, L:] == 0).all()), (b, L)
        assert bool((dv[b, :L] != 0).any(-1).all()), (b, L)  # and every valid row was written
    assert bool(torch.isfinite(dq.float()).all())


# ------------------------------------------------------------------ 3. lengths = S
def _inputs(pair, scale, seed):
    ((B, S, H), lens), p = pair
    qkv, dout = ao.short_inputs(scale, B, S, H, seed=seed)
    return qkv.to(DEV), dout.to(DEV), H, lens, p, 777 + (HIGH if p > 0 else 0)


def _run(qkv, dout, H, p, seed, klen):
    out, lse = native().attn_fwd(qkv, H, p, seed, klen)
    return out, lse, native().attn_bwd(qkv, out, dout, lse, H, p, seed, klen)


@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_full_lengths_are_bitwise_the_unpadded_kernels(pair):
    qkv, dout, H, _, p, seed = _inputs(pair, 0.8, 31)
    full = _klen([qkv.shape[1]] * qkv.shape[0])
    out, lse = native().attn_fwd(qkv, H, p, seed)  # (c) the calls without key_lengths
    dqkv = native().attn_bwd(qkv, out, dout, lse, H, p, seed)
    for got, ref in zip(_run(qkv, dout, H, p, seed, full), (out, lse, dqkv)):
        assert torch.equal(got, ref)


# ------------------------------------------------------------------ 4. pad content cannot leak
@pytest.mark.parametrize("scale", [0.8, 3.0])
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_pad_rows_cannot_leak(pair, scale):
    qkv, dout, H, lens, p, seed = _inputs(pair, scale, 32)
    B, S, _ = qkv.shape
    pad = (torch.arange(S, device=DEV)[None, :] >= _klen(lens)[:, None])[:, :, None, None]  # [B, S, 1, 1]
    g = torch.Generator().manual_seed(33)
    noise = (torch.randn(B, S, 3, H * 64, generator=g) * 1e4).to(DEV).bfloat16()
    kv = torch.tensor([False, True, True], device=DEV)[None, None, :, None]
    loud = torch.where(pad & kv, noise, qkv.view(B, S, 3, H * 64)).view_as(qkv).contiguous()
    assert bool(torch.isfinite(loud.float()).all()) and not torch.equal(loud, qkv)
    klen = _klen(lens)
    ref = _run(qkv, dout, H, p, seed, klen)
    got = _run(loud, dout, H, p, seed, klen)
    for a, b in zip(got, ref):
        assert bool(torch.isfinite(a.float()).all())
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_padded_kernels_are_deterministic(pair):
    qkv, dout, H, lens, p, seed = _inputs(pair, 3.0, 34)
    klen = _klen(lens)
    for a, b in zip(_run(qkv, dout, H, p, seed, klen), _run(qkv, dout, H, p, seed, klen)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 6. the op
def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.mark.parametrize("batch", BATCHES, ids=lambda b: "x".join(map(str, b[0])))
def test_attention_qkv_key_lengths_fused_matches_sdpa(batch, monkeypatch):
    (B, S, H), lens = batch
    qkv, dout = ao.short_inputs(0.8, B, S, H, seed=35)
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    lengths = torch.tensor(lens)  # int64 on the host: the op converts
    calls = []
    real = T._FusedAttention.apply
    monkeypatch.setattr(T._FusedAttention, "apply", lambda *a: calls.append(a[3]) or real(*a))
    res = []
    for route in ("", "fused_attn"):
        monkeypatch.setenv("PS_AMD_DISABLE", route)
        x = qkv.clone().requires_grad_()
        y = T.attention_qkv(x, H, 0.0, key_lengths=lengths)
        y.backward(dout)
        res.append((y.detach(), x.grad))
    assert len(calls) == 1 and calls[0].dtype == torch.int32 and calls[0].is_cuda  # fused once, SDPA once
    (y, g), (ry, rg) = res
    assert _rel(y, ry) < 1e-2
    for name, a, b in zip("qkv", _thirds(g, H), _thirds(rg, H)):
        assert _rel(a, b) < 2e-2, name
    # an arbitrary mask still goes to SDPA, also where it says the same
    monkeypatch.setenv("PS_AMD_DISABLE", "")
    mask = (torch.arange(S, device=DEV)[None, :] < lengths.to(DEV)[:, None])[:, None, None, :]
    ym = T.attention_qkv(qkv, H, 0.0, mask=mask)
    assert len(calls) == 1
    assert _rel(ym, ry) < 1e-2
    assert torch.equal(T.key_lengths_from_mask(mask[:, 0, 0]).cpu(), lengths)  # on the GPU: no check, no sync


# ------------------------------------------------------------------ 7. the model
def test_bert_loss_and_gradients_do_not_see_the_pad_ids_gpu():
    torch.manual_seed(0)
    B, S, lens = 3, 64, [64, 33, 1]
    c = BertConfig(vocab=512, hidden=128, layers=2, heads=2, ffn=256, max_pos=64, dropout=0.0)
    m = BertForMLM(c)
    with torch.no_grad():  # the 0.02 init attends nearly uniformly: make the scores count
        for w in m.parameters():
            if w.dim() > 1:
                w.mul_(10.0)
    m = m.to(DEV).to(torch.bfloat16)
    ids, labels, positions, lengths = mlm_batch(B, S, vocab=512, seed=5, with_positions=True, lengths=lens, device=DEV)
    pad = torch.arange(S, device=DEV)[None, :] >= lengths[:, None]
    rnd = torch.randint(1, 512, (B, S), generator=torch.Generator().manual_seed(6)).to(DEV)
    other = torch.where(pad, rnd, ids)
    res = []
    for x in (ids, other):
        m.zero_grad()
        loss = m(x, labels, positions, lengths=lengths)
        loss.backward()
        res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    (l0, g0), (l1, g1) = res
    assert bool(torch.isfinite(l0))
    assert torch.equal(l0, l1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    # without the lengths the pad ids are attended to, and the loss moves
    assert m(ids, labels, positions).item() != m(other, labels, positions).item()
