"""Fused short-sequence attention (csrc/kernels/attention.hip) on packed batches -- the tensors hold the
valid tokens only, sequence b at rows [cu[b], cu[b + 1]) -- and the unpadded BertForMLM on top of it.
The shapes (tests/attn_packed_oracle.py BATCHES) reach every branch of the PACK kernels: a full
sequence, partly valid query waves and key blocks, waves beyond L, a single token, a length-1 sequence
between two others, a tensor that ends inside a partly valid key block, one sequence of 5 tokens,
max_len below the padded length.

1. every 64-wide row of out and of the q, k and v thirds of dqkv against the fp64 oracle of
   tests/attn_packed_oracle.py, bounded by three times the row error of the bf16 rounding yardstick on the
   same inputs and keep mask, lse to rtol 1e-3 / atol 2e-3 (the rules of test_attention_padded_gpu.py); the
   backward is fed the oracle's out and lse;
2. out, lse and dqkv are bitwise the valid rows of the key_lengths call on the re-padded input (S =
   max_len, the same seed, dout with zero pad rows);
3. sequence b's rows do not change by a bit when every other sequence's tokens and dout rows are replaced
   by +-1e4 randn;
4. every row is written: the whole tensors of test 1 are finite and within the bound, nothing pre-filled;
5. two calls are bitwise equal;
6. attention_qkv(seqs=) with autograd: the packed kernels against the repad / SDPA / unpad fallback;
7. a tiny BertForMLM: seqs= against lengths=, each against the fp32 model; bitwise repeatable under
   dropout; no host sync;
8. SplitKLinear's weight and bias gradient at a row count only packing makes (T = 4099).

The bound of test 7: err(seqs) <= 2 * err(lengths) + FLOOR per tensor, err the relative Frobenius error
against the same model in fp32.  The two bf16 runs differ in GEMM row counts only, so their errors are two
draws from one rounding distribution, hence the factor 2.  FLOOR = 1e-3 lies below every error the padded
run shows on MI355X (loss 1.70e-3; gradients 1.31e-2 (head_ln.bias, head_bias) to 7.96e-2 (pos.weight)), so
it decides nothing unless a padded draw comes out near zero.  Observed on MI355X: the seqs= errors equal the
lengths= errors to three digits (loss 1.70e-3 both; the largest difference is 6.78e-2 against 6.79e-2,
word.weight), with and without positions; rowerr(kernel) / rowerr(yardstick) is 1.00 in all 112 (case,
tensor) pairs of test 1 (the yardstick's own rowerr is 0.0020 - 0.0046); tests 2, 3 and 5 hold bitwise.
"""
import functools
import warnings

import pytest
import torch

from ps_amd.models.transformer import BertConfig, BertForMLM, mlm_batch
from ps_amd.ops import native
from ps_amd.ops import transformer as T
from ps_amd.ops.dense import SplitKLinear, _wgrad_ok

from . import attn_oracle as ao
from . import attn_packed_oracle as apk

pytestmark = pytest.mark.gpu
DEV = "cuda"

BATCHES = apk.BATCHES
FACTOR = 3.0
HIGH = 7 << 40
FLOOR = 1e-3

CASES = [(batch, scale, p) for batch in BATCHES for scale in (0.8, 3.0) for p in (0.0, 0.1)]
PAIRS = [(batch, p) for batch in BATCHES for p in (0.0, 0.1)]


def _seed(i):
    return 12345 + (HIGH if i % 2 else 0)  # the p = 0.1 cases: a seed above 2^32


def _bid(batch):
    return "x".join(map(str, batch[0])) + "-" + "_".join(map(str, batch[1]))


def _id(case):
    i, (batch, scale, p) = case
    return f"{_bid(batch)}-s{scale}-p{p}-{'hi' if _seed(i) >> 32 else 'lo'}"


def _pid(pair):
    return f"{_bid(pair[0])}-p{pair[1]}"


def _thirds(dqkv, heads):
    return dqkv.view(dqkv.shape[0], 3, heads, ao.SHORT_D).unbind(1)


def _seqs(batch):
    (_, S, _), lens = batch
    return T.pack_seqs(lens, S, DEV)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs, keep mask, fp64 oracle and yardstick of one case, computed once and left unchanged."""
    batch, scale, p = CASES[i]
    (B, S, H), lens = batch
    seqs = _seqs(batch)
    seed = _seed(i)
    qkv, dout = apk.packed_inputs(scale, lens, H, seed=100 + i)
    M = seqs.max_len
    keep = native().attn_dropout_mask(qkv.to(DEV), B * H, M, p, seed).cpu() if p > 0 else None
    out, lse = apk.packed_fwd(qkv, H, lens, keep, p)
    yout, _ = apk.packed_fwd(qkv, H, lens, keep, p, rounded=True)
    out_in, lse_in = out.to(torch.bfloat16), lse.float().contiguous()  # what attn_bwd is given
    grad = apk.packed_bwd(qkv, out_in, dout, lse_in, H, lens, keep, p)
    ygrad = apk.packed_bwd(qkv, out_in, dout, lse_in, H, lens, keep, p, rounded=True)
    return dict(qkv=qkv, dout=dout, H=H, p=p, seed=seed, lens=lens, seqs=seqs, out=out, lse=lse, yout=yout,
                out_in=out_in, lse_in=lse_in, grad=grad, ygrad=ygrad)


def _bound(name, tag, got, ref, yard):
    assert got.shape == ref.shape and bool(torch.isfinite(got.float()).all()), name  # 4: no NaN, no row missing
    e, y = ao.rowerr(got, ref), ao.rowerr(yard, ref)
    print(f"RATIO packed {tag} {name}: kernel {e:.5f} yardstick {y:.5f} ratio {e / y:.2f}")
    assert y > 0
    assert e <= FACTOR * y, (name, e, y)


# ------------------------------------------------------------------ 1, 4. per row against the oracle
@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=_id)
def test_packed_forward_rows(case):
    c = _case(case[0])
    H, seqs = c["H"], c["seqs"]
    out, lse = native().attn_fwd(c["qkv"].to(DEV), H, c["p"], c["seed"], None, seqs.cu, seqs.max_len)
    assert out.shape == (seqs.total, H * 64) and lse.shape == (H, seqs.total)
    rows = lambda x: x.view(x.shape[0], H, ao.SHORT_D)  # noqa: E731
    _bound("out", _id(case), rows(out), rows(c["out"]), rows(c["yout"]))
    torch.testing.assert_close(lse.cpu(), c["lse"].float(), rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=_id)
def test_packed_backward_rows(case):
    c = _case(case[0])
    H, seqs = c["H"], c["seqs"]
    dqkv = native().attn_bwd(c["qkv"].to(DEV), c["out_in"].to(DEV), c["dout"].to(DEV), c["lse_in"].to(DEV), H, c["p"],
                             c["seed"], None, seqs.cu, seqs.max_len)
    assert dqkv.shape == c["grad"].shape
    for name, g, ref, yard in zip(("dq", "dk", "dv"), _thirds(dqkv, H), _thirds(c["grad"], H), _thirds(c["ygrad"], H)):
        _bound(name, _id(case), g, ref, yard)


# ------------------------------------------------------------------ 2. bitwise the padded kernels
def _inputs(pair, scale, seed):
    batch, p = pair
    (_, _, H), lens = batch
    qkv, dout = apk.packed_inputs(scale, lens, H, seed=seed)
    return qkv.to(DEV), dout.to(DEV), H, lens, _seqs(batch), p, 777 + (HIGH if p > 0 else 0)


def _run(qkv, dout, H, p, seed, seqs):
    out, lse = native().attn_fwd(qkv, H, p, seed, None, seqs.cu, seqs.max_len)
    return out, lse, native().attn_bwd(qkv, out, dout, lse, H, p, seed, None, seqs.cu, seqs.max_len)


@pytest.mark.parametrize("scale", [0.8, 3.0])
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_packed_is_bitwise_the_key_lengths_call_on_the_repadded_batch(pair, scale):
    qkv, dout, H, lens, seqs, p, seed = _inputs(pair, scale, 41)
    M, B = seqs.max_len, seqs.batch
    short = T.pack_seqs(lens, M, DEV)  # the batch padded to the bound the packed kernels run with
    klen = torch.tensor(lens, dtype=torch.int32, device=DEV)
    pq, pdo = T.repad(qkv, short).contiguous(), T.repad(dout, short).contiguous()  # zero pad rows
    pout, plse = native().attn_fwd(pq, H, p, seed, klen)
    pgrad = native().attn_bwd(pq, pout, pdo, plse, H, p, seed, klen)
    out, lse, dqkv = _run(qkv, dout, H, p, seed, seqs)
    assert pout.shape == (B, M, H * 64)
    assert torch.equal(out, T.unpad(pout, short))
    assert torch.equal(lse, T.unpad(plse.transpose(1, 2), short).t())
    assert torch.equal(dqkv, T.unpad(pgrad, short))


# ------------------------------------------------------------------ 3. isolation
@pytest.mark.parametrize("scale", [0.8, 3.0])
@pytest.mark.parametrize("pair", [x for x in PAIRS if x[0][0][0] > 1], ids=_pid)
def test_other_sequences_cannot_leak(pair, scale):
    qkv, dout, H, lens, seqs, p, seed = _inputs(pair, scale, 42)
    g = torch.Generator().manual_seed(43)
    loud_qkv = (torch.randn(qkv.shape, generator=g) * 1e4).to(DEV).bfloat16()
    loud_dout = (torch.randn(dout.shape, generator=g) * 1e4).to(DEV).bfloat16()
    ref = _run(qkv, dout, H, p, seed, seqs)
    for lo, hi in apk.bounds(lens):
        own = torch.zeros(seqs.total, 1, dtype=torch.bool, device=DEV)
        own[lo:hi] = True
        got = _run(torch.where(own, qkv, loud_qkv), torch.where(own, dout, loud_dout), H, p, seed, seqs)
        for name, a, b in zip(("out", "lse", "dqkv"), got, ref):
            a, b = (a[:, lo:hi], b[:, lo:hi]) if name == "lse" else (a[lo:hi], b[lo:hi])
            assert bool(torch.isfinite(a.float()).all()), (name, lo)
            assert torch.equal(a, b), (name, lo)


# ------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_packed_kernels_are_deterministic(pair):
    qkv, dout, H, _, seqs, p, seed = _inputs(pair, 3.0, 44)
    for a, b in zip(_run(qkv, dout, H, p, seed, seqs), _run(qkv, dout, H, p, seed, seqs)):
        assert torch.equal(a, b)


def test_packed_bindings_check_their_arguments():
    qkv = torch.zeros(8, 3 * 64, device=DEV, dtype=torch.bfloat16)
    cu = torch.tensor([0, 5, 8], dtype=torch.int32, device=DEV)
    klen = torch.tensor([5, 3], dtype=torch.int32, device=DEV)
    f = native().attn_fwd
    for bad in (lambda: f(qkv, 1, 0.0, 0, klen, cu, 32),          # both descriptions
                lambda: f(qkv, 1, 0.0, 0, None, cu, 48),          # max_len % 32
                lambda: f(qkv, 1, 0.0, 0, None, cu, 160),         # max_len > 128
                lambda: f(qkv, 1, 0.0, 0, None, cu, 0),
                lambda: f(qkv, 1, 0.0, 0, None, cu[:1], 32),      # B + 1 >= 2
                lambda: f(qkv, 1, 0.0, 0, None, cu.long(), 32),
                lambda: f(qkv, 1, 0.0, 0, None, cu.cpu(), 32),
                lambda: f(qkv.view(1, 8, -1), 1, 0.0, 0, None, cu, 32),
                lambda: f(qkv, 1, 0.0, 0, None, None, 32)):       # max_len without cu_seqlens
        with pytest.raises(RuntimeError):
            bad()
    out, lse = f(qkv, 1, 0.0, 0, None, cu, 32)
    b = native().attn_bwd
    with pytest.raises(RuntimeError):
        b(qkv, out, out, lse.t().contiguous(), 1, 0.0, 0, None, cu, 32)  # lse [H, T]
    with pytest.raises(RuntimeError):
        b(qkv, out[:-1], out[:-1], lse, 1, 0.0, 0, None, cu, 32)
    with pytest.raises(ValueError, match="host"):
        T.pack_seqs(klen, 32)  # lengths on the device


# ------------------------------------------------------------------ 6. the op
def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.mark.parametrize("batch", BATCHES, ids=_bid)
def test_attention_qkv_seqs_fused_matches_its_fallback(batch, monkeypatch):
    (_, _, H), lens = batch
    seqs = _seqs(batch)
    qkv, dout = apk.packed_inputs(0.8, lens, H, seed=45)
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    calls = []
    real = T._FusedAttention.apply
    monkeypatch.setattr(T._FusedAttention, "apply", lambda *a: calls.append(a[4]) or real(*a))
    res = []
    for route in ("", "fused_attn"):
        monkeypatch.setenv("PS_AMD_DISABLE", route)
        x = qkv.clone().requires_grad_()
        y = T.attention_qkv(x, H, 0.0, seqs=seqs)
        y.backward(dout)
        res.append((y.detach(), x.grad))
    assert len(calls) == 1 and calls[0] is seqs.cu  # packed kernels once, repad / SDPA / unpad once
    (y, g), (ry, rg) = res
    assert y.shape == ry.shape == (seqs.total, H * 64)
    assert _rel(y, ry) < 1e-2
    for name, a, b in zip("qkv", _thirds(g, H), _thirds(rg, H)):
        assert _rel(a, b) < 2e-2, name


# ------------------------------------------------------------------ 7. the model
MB, MS, MLENS = 4, 64, [64, 33, 1, 20]


def _tiny(dropout):
    torch.manual_seed(0)
    c = BertConfig(vocab=512, hidden=128, layers=2, heads=2, ffn=256, max_pos=MS, dropout=dropout)
    m = BertForMLM(c)
    with torch.no_grad():  # the 0.02 init attends nearly uniformly: make the scores count
        for w in m.parameters():
            if w.dim() > 1:
                w.mul_(10.0)
    return m.to(DEV)


def _loss_and_grads(m, ids, labels, pos, **kw):
    m.zero_grad()
    loss = m(ids, labels, pos, **kw)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}


@functools.lru_cache(maxsize=None)
def _model_batch():
    return mlm_batch(MB, MS, vocab=512, seed=5, with_positions=True, lengths=MLENS, device=DEV, packed=True)


@pytest.mark.parametrize("with_positions", [False, True])
def test_bert_seqs_is_as_close_to_fp32_as_lengths(with_positions):
    ids, labels, positions, lengths, seqs = _model_batch()
    pos = positions if with_positions else None
    m32 = _tiny(0.0).eval()
    l32, g32 = _loss_and_grads(m32, ids, labels, pos, lengths=lengths)
    m = _tiny(0.0).to(torch.bfloat16).eval()
    lp, gp = _loss_and_grads(m, ids, labels, pos, lengths=lengths)
    ls, gs = _loss_and_grads(m, ids, labels, pos, seqs=seqs)
    assert bool(torch.isfinite(ls))
    ep, es = abs(lp.item() - l32.item()) / abs(l32.item()), abs(ls.item() - l32.item()) / abs(l32.item())
    print(f"MODEL positions={with_positions} loss: lengths {ep:.2e} seqs {es:.2e}")
    assert es <= 2 * ep + FLOOR
    for n in g32:
        if g32[n].norm().item() == 0:
            assert gs[n].float().norm().item() == 0, n
            continue
        ep, es = _rel(gp[n], g32[n]), _rel(gs[n], g32[n])
        print(f"MODEL positions={with_positions} {n}: lengths {ep:.2e} seqs {es:.2e}")
        assert es <= 2 * ep + FLOOR, n


def test_bert_seqs_with_dropout_is_repeatable_and_finite():
    ids, labels, positions, _, seqs = _model_batch()
    m = _tiny(0.1).to(torch.bfloat16).train()
    res = []
    for _ in range(2):
        torch.manual_seed(11)
        res.append(_loss_and_grads(m, ids, labels, positions, seqs=seqs))
    (l0, g0), (l1, g1) = res
    assert bool(torch.isfinite(l0)) and torch.equal(l0, l1)
    for n in g0:
        assert bool(torch.isfinite(g0[n].float()).all()), n
        assert torch.equal(g0[n], g1[n]), n


def test_bert_seqs_forward_and_backward_do_not_sync():
    ids, labels, positions, _, seqs = _model_batch()
    m = _tiny(0.1).to(torch.bfloat16).train()
    for pos in (positions, None):  # warm-up: lazy initialisations may sync
        _loss_and_grads(m, ids, labels, pos, seqs=seqs)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            m.zero_grad()
            m(ids, labels, positions, seqs=seqs).backward()
            m(ids, labels, None, seqs=seqs).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()]


# ------------------------------------------------------------------ 8. weight gradient at odd T
def test_splitk_linear_weight_gradient_at_odd_row_count():
    Tn, K, N = 4099, 768, 768
    g = torch.Generator().manual_seed(Tn + K + N)
    x = torch.randn(Tn, K, generator=g).bfloat16().to(DEV)
    dy = torch.randn(Tn, N, generator=g).bfloat16().to(DEV)
    assert _wgrad_ok(x, dy)
    ref = dy.float().t() @ x.float()
    dw, db = native().linear_wgrad_db(dy, x)  # the kernel's own outputs, test_splitk_gpu.py's tolerances
    assert _rel(dw, ref) < 5e-3
    torch.testing.assert_close(db, dy.float().sum(0), rtol=1e-4, atol=1e-2)
    lin = SplitKLinear(K, N).to(DEV).bfloat16()
    lin(x.clone().requires_grad_()).backward(dy)
    assert lin.weight.grad.shape == (N, K)
    assert _rel(lin.weight.grad, ref) < 5e-3
    assert _rel(lin.bias.grad, dy.float().sum(0)) < 1e-2
