"""Chunked BERT attention (csrc/kernels/attention_long.hip: S a multiple of 32 up to 512, online softmax
over 128-key chunks) in its three layouts -- dense, per-sequence key lengths, packed -- through the
bindings attn_long_fwd / attn_long_bwd, the op attention_qkv and BertForMLM.

Shapes (tests/attn_long_oracle.py) and what each reaches:

  (2, 160, 2) [160, 129]          two chunks, the last one a single 32-key block; a second query block of 32
                                  rows; L one past a chunk edge
  (3, 256, 1) [256, 128, 1]       L on the chunk edge (the second chunk skipped whole); a single key
  (2, 384, 3) [383, 257]          three chunks (two rescales); one short of S; one past an edge
  (1, 512, 2) [512]               the top of the domain, 4 x 4 blocks
  (2, 64, 1)  [64, 7]             below one chunk, through the long bindings
  packed only (4, 512, 2) [512, 130, 33, 1]   long and short sequences side by side, query blocks beyond L
  packed only (2, 224, 1) [200, 150]          max_len not a multiple of 128

Inputs: short_inputs at scales 0.8 and 3.0 and every kind of long_inputs (a ramp of 0, 3, 12 exp2 units per
chunk, ascending, and 12 descending: the online rescale factor is about 1, 2^-3, 2^-12, or 1 after the first
chunk).  The kernels rescale at every chunk, there is no threshold with two sides.

1. every 64-wide row of out and of the q, k and v thirds of dqkv against the fp64 oracle, bounded by three
   times the row error of the bf16 rounding yardstick on the same inputs and keep mask (the bound of
   test_attention_rows_gpu.py), lse to rtol 1e-3 / atol 2e-3; p in {0, 0.1}, the p = 0.1 seed above 2^32; the
   backward is fed the oracle's out and lse.  The yardstick is the one of the one-tile kernels (it rounds
   the normalised P); the chunked forward rounds P before the normalisation, which is the same relative
   rounding, and the ratios show it;
2. padded layout: dk and dv rows >= L are exact zeros, every valid dv row is written, dq is finite;
3. bitwise: lengths all S give the dense result; packed rows are the valid rows of the key-length call at
   S = max_len with the same seed; +-1e4 randn in the K / V pad rows, or in the other sequences' tokens,
   changes no bit; two calls are equal;
4. the chunked and the one-tile family at (2, 128, 2) and (2, 64, 1): both within the bound of test 1 around
   the same oracle (not bitwise equal: the rounding points differ);
5. the bindings check their arguments;
6. attention_qkv (dense, key_lengths=, seqs=) with autograd at (2, 160, 2) and (1, 512, 2): the chunked
   kernels once on the default route, bitwise the binding's output, against the SDPA route; S = 544 and an
   arbitrary mask still go to SDPA;
7. a tiny BertForMLM at S = 192: loss and gradients bitwise unchanged when the pad ids are replaced
   (lengths=); the seqs= loss as close to the fp32 model's as the lengths= loss (the bound of
   test_attention_packed_gpu.py: err(seqs) <= 2 * err(lengths) + 1e-3).

Observed on MI355X (profiles/bert_attn_long_gpu_tests.txt), rowerr(kernel) / rowerr(yardstick) over the 204
cases of test 1: out 0.57 - 1.10 (mean 0.81: rounding the unnormalised P is on average the smaller error), dq
0.98 - 1.00, dk 0.99 - 1.07, dv 0.92 - 1.05; the bound is 3; the yardstick's own rowerr is 0.0023 - 0.0198 (the
largest on the descend and rescale inputs).  Test 4: the chunked family out 0.61 - 1.03 and dq, dk, dv 1.00, the
one-tile family 1.00 throughout.  Tests 2 and 3 hold bitwise.  Test 7: loss error against fp32 1.32e-4 with
lengths= and with seqs=.
"""
import functools

import pytest
import torch

from ps_amd.models.transformer import BertConfig, BertForMLM, mlm_batch
from ps_amd.ops import native
from ps_amd.ops import transformer as T

from . import attn_long_oracle as alo
from . import attn_oracle as ao
from . import attn_packed_oracle as apk

pytestmark = pytest.mark.gpu
DEV = "cuda"

FACTOR = 3.0
HIGH = 7 << 40
FLOOR = 1e-3

CASES = [(layout, batch, inp, p)
         for layout in alo.LAYOUTS
         for batch in (alo.PACKED if layout == "packed" else alo.PADDED)
         for inp in alo.INPUTS
         for p in (0.0, 0.1)]
PAIRS = [(batch, p) for batch in alo.PADDED for p in (0.0, 0.1)]
PACKED_PAIRS = [(batch, p) for batch in alo.PACKED for p in (0.0, 0.1)]


def _bid(batch):
    return "x".join(map(str, batch[0])) + "-" + "_".join(map(str, batch[1]))


def _id(case):
    _, (layout, batch, inp, p) = case
    return f"{layout}-{_bid(batch)}-{inp[0]}{inp[1]}-p{p}"


def _pid(pair):
    return f"{_bid(pair[0])}-p{pair[1]}"


def _seed(p):
    return 12345 + (HIGH if p > 0 else 0)  # the p = 0.1 cases: a seed above 2^32


def _klen(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def _extra(layout, batch):
    """The arguments after seed that describe the layout to the bindings."""
    (_, S, _), lens = batch
    if layout == "dense":
        return ()
    if layout == "klen":
        return (_klen(lens),)
    seqs = T.pack_seqs(lens, S, DEV)
    assert seqs.max_len == alo.max_len(lens)
    return (None, seqs.cu, seqs.max_len)


def _mask(batch, layout, p, seed):
    (B, S, H), lens = batch
    if p == 0:
        return None
    like = torch.zeros(1, device=DEV)
    return native().attn_dropout_mask(like, B * H, alo.max_len(lens) if layout == "packed" else S, p, seed).cpu()


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs, keep mask, fp64 oracle and yardstick of one case, computed once and left unchanged."""
    layout, batch, inp, p = CASES[i]
    seed = _seed(p)
    qkv, dout = alo.inputs(layout, batch, inp, seed=100 + i)
    keep = _mask(batch, layout, p, seed)
    c = alo.reference(layout, batch, qkv, dout, keep, p)
    c.update(qkv=qkv, dout=dout, H=batch[0][2], p=p, seed=seed, extra=_extra(layout, batch))
    return c


def _bound(name, tag, got, ref, yard):
    assert got.shape == ref.shape and bool(torch.isfinite(got.float()).all()), name
    e, y = ao.rowerr(got, ref), ao.rowerr(yard, ref)
    print(f"RATIO long {tag} {name}: kernel {e:.5f} yardstick {y:.5f} ratio {e / y:.2f}")
    assert y > 0
    assert e <= FACTOR * y, (name, e, y)


# ------------------------------------------------------------------ 1. per row against the oracle
@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=_id)
def test_long_forward_rows(case):
    c = _case(case[0])
    H = c["H"]
    out, lse = native().attn_long_fwd(c["qkv"].to(DEV), H, c["p"], c["seed"], *c["extra"])
    _bound("out", _id(case), alo.rows(out, H), alo.rows(c["out"], H), alo.rows(c["yout"], H))
    assert lse.shape == c["lse"].shape
    torch.testing.assert_close(lse.cpu(), c["lse"].float(), rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=_id)
def test_long_backward_rows(case):
    c = _case(case[0])
    H = c["H"]
    dqkv = native().attn_long_bwd(c["qkv"].to(DEV), c["out_in"].to(DEV), c["dout"].to(DEV), c["lse_in"].to(DEV), H,
                                  c["p"], c["seed"], *c["extra"])
    assert dqkv.shape == c["grad"].shape
    for name, g, ref, yard in zip(("dq", "dk", "dv"), alo.thirds(dqkv, H), alo.thirds(c["grad"], H),
                                  alo.thirds(c["ygrad"], H)):
        _bound(name, _id(case), g, ref, yard)


def test_mask_model_is_the_device_mask():
    like = torch.zeros(1, device=DEV)
    for bh, S, seed in ((4, 160, _seed(0.1)), (2, 512, 99)):
        assert torch.equal(native().attn_dropout_mask(like, bh, S, 0.1, seed).cpu(), alo.keep_model(bh, S, 0.1, seed))


# ------------------------------------------------------------------ 2. dk, dv of pad rows
def _inputs(pair, inp, seed, layout="klen"):
    batch, p = pair
    qkv, dout = alo.inputs(layout, batch, inp, seed=seed)
    return qkv.to(DEV), dout.to(DEV), batch[0][2], batch[1], p, 777 + (HIGH if p > 0 else 0)


def _run(qkv, dout, H, p, seed, *extra):
    out, lse = native().attn_long_fwd(qkv, H, p, seed, *extra)
    return out, lse, native().attn_long_bwd(qkv, out, dout, lse, H, p, seed, *extra)


@pytest.mark.parametrize("inp", [("short", 3.0), ("long", "deferred")], ids=lambda x: f"{x[0]}{x[1]}")
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_long_backward_pad_rows_are_exact_zeros(pair, inp):
    qkv, dout, H, lens, p, seed = _inputs(pair, inp, 30)
    dqkv = _run(qkv, dout, H, p, seed, _klen(lens))[2]
    dq, dk, dv = alo.thirds(dqkv, H)
    for b, L in enumerate(lens):
        assert bool((dk[b, L:] == 0).all()) and bool((dv[b, L:] == 0).all()), (b, L)
        assert bool((dv[b, :L] != 0).any(-1).all()), (b, L)  # and every valid row was written
    assert bool(torch.isfinite(dq.float()).all())


# ------------------------------------------------------------------ 3. bitwise properties
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_full_lengths_are_bitwise_the_dense_call(pair):
    qkv, dout, H, _, p, seed = _inputs(pair, ("short", 0.8), 31)
    full = _klen([qkv.shape[1]] * qkv.shape[0])
    for got, ref in zip(_run(qkv, dout, H, p, seed, full), _run(qkv, dout, H, p, seed)):
        assert torch.equal(got, ref)


@pytest.mark.parametrize("inp", [("short", 0.8), ("long", "rescale")], ids=lambda x: f"{x[0]}{x[1]}")
@pytest.mark.parametrize("pair", PACKED_PAIRS, ids=_pid)
def test_packed_is_bitwise_the_key_lengths_call_on_the_repadded_batch(pair, inp):
    qkv, dout, H, lens, p, seed = _inputs(pair, inp, 41, layout="packed")
    seqs = T.pack_seqs(lens, pair[0][0][1], DEV)
    M, B = seqs.max_len, seqs.batch
    short = T.pack_seqs(lens, M, DEV)  # the batch padded to the bound the packed kernels run with
    pq, pdo = T.repad(qkv, short).contiguous(), T.repad(dout, short).contiguous()  # zero pad rows
    pout, plse, pgrad = _run(pq, pdo, H, p, seed, _klen(lens))
    out, lse, dqkv = _run(qkv, dout, H, p, seed, None, seqs.cu, M)
    assert pout.shape == (B, M, H * 64) and out.shape == (seqs.total, H * 64) and lse.shape == (H, seqs.total)
    assert torch.equal(out, T.unpad(pout, short))
    assert torch.equal(lse, T.unpad(plse.transpose(1, 2), short).t())
    assert torch.equal(dqkv, T.unpad(pgrad, short))


@pytest.mark.parametrize("inp", [("short", 0.8), ("short", 3.0)], ids=lambda x: f"{x[0]}{x[1]}")
@pytest.mark.parametrize("pair", PAIRS, ids=_pid)
def test_pad_rows_cannot_leak(pair, inp):
    qkv, dout, H, lens, p, seed = _inputs(pair, inp, 32)
    B, S, _ = qkv.shape
    pad = (torch.arange(S, device=DEV)[None, :] >= _klen(lens)[:, None])[:, :, None, None]  # [B, S, 1, 1]
    g = torch.Generator().manual_seed(33)
    noise = (torch.randn(B, S, 3, H * 64, generator=g) * 1e4).to(DEV).bfloat16()
    kv = torch.tensor([False, True, True], device=DEV)[None, None, :, None]
    loud = torch.where(pad & kv, noise, qkv.view(B, S, 3, H * 64)).view_as(qkv).contiguous()
    assert bool(torch.isfinite(loud.float()).all())
    assert torch.equal(loud, qkv) == (min(lens) == S)
    klen = _klen(lens)
    for a, b in zip(_run(loud, dout, H, p, seed, klen), _run(qkv, dout, H, p, seed, klen)):
        assert bool(torch.isfinite(a.float()).all())
        assert torch.equal(a, b)


@pytest.mark.parametrize("pair", [x for x in PACKED_PAIRS if x[0][0][0] > 1], ids=_pid)
def test_other_sequences_cannot_leak(pair):
    qkv, dout, H, lens, p, seed = _inputs(pair, ("short", 3.0), 42, layout="packed")
    extra = _extra("packed", pair[0])
    g = torch.Generator().manual_seed(43)
    loud_qkv = (torch.randn(qkv.shape, generator=g) * 1e4).to(DEV).bfloat16()
    loud_dout = (torch.randn(dout.shape, generator=g) * 1e4).to(DEV).bfloat16()
    ref = _run(qkv, dout, H, p, seed, *extra)
    for lo, hi in apk.bounds(lens):
        own = torch.zeros(qkv.shape[0], 1, dtype=torch.bool, device=DEV)
        own[lo:hi] = True
        got = _run(torch.where(own, qkv, loud_qkv), torch.where(own, dout, loud_dout), H, p, seed, *extra)
        for name, a, b in zip(("out", "lse", "dqkv"), got, ref):
            a, b = (a[:, lo:hi], b[:, lo:hi]) if name == "lse" else (a[lo:hi], b[lo:hi])
            assert bool(torch.isfinite(a.float()).all()), (name, lo)
            assert torch.equal(a, b), (name, lo)


@pytest.mark.parametrize("layout,pair", [("klen", x) for x in PAIRS] + [("packed", x) for x in PACKED_PAIRS],
                         ids=lambda x: x if isinstance(x, str) else _pid(x))
def test_long_kernels_are_deterministic(layout, pair):
    qkv, dout, H, _, p, seed = _inputs(pair, ("long", "rescale"), 44, layout=layout)
    extra = _extra(layout, pair[0])
    for a, b in zip(_run(qkv, dout, H, p, seed, *extra), _run(qkv, dout, H, p, seed, *extra)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 4. the two families
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("scale", [0.8, 3.0])
@pytest.mark.parametrize("batch", [((2, 128, 2), [128, 97]), ((2, 64, 1), [64, 7])], ids=_bid)
def test_the_two_families_agree(batch, scale, p):
    (B, S, H), lens = batch
    seed = _seed(p)
    qkv, dout = ao.short_inputs(scale, B, S, H, seed=50)
    keep = _mask(batch, "klen", p, seed)
    for layout in ("dense", "klen"):
        c = alo.reference(layout, batch, qkv, dout, keep, p)
        extra = _extra(layout, batch)
        for fam, fwd, bwd in (("long", native().attn_long_fwd, native().attn_long_bwd),
                              ("short", native().attn_fwd, native().attn_bwd)):
            tag = f"{fam}-{layout}-{_bid(batch)}-s{scale}-p{p}"
            out, lse = fwd(qkv.to(DEV), H, p, seed, *extra)
            _bound("out", tag, alo.rows(out, H), alo.rows(c["out"], H), alo.rows(c["yout"], H))
            torch.testing.assert_close(lse.cpu(), c["lse"].float(), rtol=1e-3, atol=2e-3)
            dqkv = bwd(qkv.to(DEV), c["out_in"].to(DEV), dout.to(DEV), c["lse_in"].to(DEV), H, p, seed, *extra)
            for name, g, ref, yard in zip(("dq", "dk", "dv"), alo.thirds(dqkv, H), alo.thirds(c["grad"], H),
                                          alo.thirds(c["ygrad"], H)):
                _bound(name, tag, g, ref, yard)


# ------------------------------------------------------------------ 5. the bindings' checks
def test_long_bindings_check_their_arguments():
    f, b = native().attn_long_fwd, native().attn_long_bwd
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=torch.bfloat16)  # noqa: E731
    qkv = z(8, 3 * 64)
    cu = torch.tensor([0, 5, 8], dtype=torch.int32, device=DEV)
    klen = torch.tensor([5, 3], dtype=torch.int32, device=DEV)
    for bad in (lambda: f(z(1, 544, 3 * 64), 1, 0.0, 0),             # S > 512
                lambda: f(z(1, 48, 3 * 64), 1, 0.0, 0),              # S % 32
                lambda: f(z(1, 64, 3 * 64).float(), 1, 0.0, 0),
                lambda: f(qkv, 1, 0.0, 0, klen, cu, 32),             # both descriptions
                lambda: f(qkv, 1, 0.0, 0, None, None, 32),           # max_len without cu_seqlens
                lambda: f(qkv, 1, 0.0, 0, None, cu, 544),
                lambda: f(qkv, 1, 0.0, 0, None, cu, 48),
                lambda: f(qkv, 1, 0.0, 0, None, cu, 0),
                lambda: f(qkv, 1, 0.0, 0, None, cu.long(), 32),      # dtype of cu
                lambda: f(qkv, 1, 0.0, 0, None, cu.cpu(), 32),       # device of cu
                lambda: f(z(2, 160, 3 * 64), 1, 0.0, 0, klen.long()),
                lambda: f(z(2, 160, 3 * 64), 1, 0.0, 0, klen.cpu())):
        with pytest.raises(RuntimeError):
            bad()
    out, lse = f(qkv, 1, 0.0, 0, None, cu, 32)
    with pytest.raises(RuntimeError):
        b(qkv, out, out, lse.t().contiguous(), 1, 0.0, 0, None, cu, 32)  # packed lse is [H, T]
    with pytest.raises(RuntimeError):
        b(qkv, out[:-1], out[:-1], lse, 1, 0.0, 0, None, cu, 32)
    x = z(2, 160, 3 * 64)
    out, lse = f(x, 1, 0.0, 0)
    with pytest.raises(RuntimeError):
        b(x, out, out, lse[:, :, :128].contiguous(), 1, 0.0, 0)
    with pytest.raises(RuntimeError):  # the one-tile bindings keep their bound
        native().attn_fwd(x, 1, 0.0, 0)


# ------------------------------------------------------------------ 6. the op
def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.mark.parametrize("layout", alo.LAYOUTS)
@pytest.mark.parametrize("batch", [alo.PADDED[0], alo.PADDED[3]], ids=_bid)
def test_attention_qkv_takes_the_long_kernels_and_matches_sdpa(batch, layout, monkeypatch):
    (B, S, H), lens = batch
    qkv, dout = alo.inputs(layout, batch, ("short", 0.8), seed=35)
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    kw, extra = {}, _extra(layout, batch)
    if layout == "klen":
        kw = dict(key_lengths=torch.tensor(lens))  # int64 on the host: the op converts
    elif layout == "packed":
        kw = dict(seqs=T.pack_seqs(lens, S, DEV))
    assert (T.attention_packed_long_ok(qkv, H, kw["seqs"]) if layout == "packed" else T.attention_long_ok(qkv, H, None))
    calls = []
    real = T._FusedAttention.apply
    monkeypatch.setattr(T._FusedAttention, "apply", lambda *a: calls.append(a) or real(*a))
    res = []
    for route in ("", "fused_attn"):
        monkeypatch.setenv("PS_AMD_DISABLE", route)
        x = qkv.clone().requires_grad_()
        y = T.attention_qkv(x, H, 0.0, **kw)
        y.backward(dout)
        res.append((y.detach(), x.grad))
    assert len(calls) == 1  # the fused kernels once, SDPA once
    (y, g), (ry, rg) = res
    assert torch.equal(y, native().attn_long_fwd(qkv, H, 0.0, 0, *extra)[0])
    assert y.shape == ry.shape
    assert _rel(y, ry) < 1e-2
    for name, a, b in zip("qkv", alo.thirds(g, H), alo.thirds(rg, H)):
        assert _rel(a, b) < 2e-2, name


def test_attention_qkv_off_the_long_domain_goes_to_sdpa(monkeypatch):
    monkeypatch.setenv("PS_AMD_DISABLE", "")
    calls = []
    real = T._FusedAttention.apply
    monkeypatch.setattr(T._FusedAttention, "apply", lambda *a: calls.append(a) or real(*a))
    H = 2
    big, _ = ao.short_inputs(0.8, 1, 544, H, seed=36)
    assert T.attention_qkv(big.to(DEV), H, 0.0).shape == (1, 544, H * 64)
    odd, _ = ao.short_inputs(0.8, 1, 200, H, seed=36)
    assert T.attention_qkv(odd.to(DEV), H, 0.0).shape == (1, 200, H * 64)
    qkv, _ = ao.short_inputs(0.8, 2, 160, H, seed=36)
    qkv, lengths = qkv.to(DEV), torch.tensor([160, 129], device=DEV)
    mask = (torch.arange(160, device=DEV)[None, :] < lengths[:, None])[:, None, None, :]
    ym = T.attention_qkv(qkv, H, 0.0, mask=mask)
    assert not calls
    yk = T.attention_qkv(qkv, H, 0.0, key_lengths=lengths)
    assert len(calls) == 1
    assert _rel(ym, yk) < 1e-2


# ------------------------------------------------------------------ 7. the model
MB, MS, MLENS = 3, 192, [192, 129, 1]


def _tiny():
    torch.manual_seed(0)
    c = BertConfig(vocab=512, hidden=128, layers=2, heads=2, ffn=256, max_pos=MS, dropout=0.0)
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


def test_bert_at_192_does_not_see_the_pad_ids_and_seqs_matches_lengths(monkeypatch):
    ids, labels, positions, lengths, seqs = mlm_batch(MB, MS, vocab=512, seed=5, with_positions=True, lengths=MLENS,
                                                      device=DEV, packed=True)
    assert seqs.max_len == MS
    calls = []
    real = T._FusedAttention.apply
    monkeypatch.setattr(T._FusedAttention, "apply", lambda *a: calls.append(a) or real(*a))
    m = _tiny().to(torch.bfloat16).eval()
    pad = torch.arange(MS, device=DEV)[None, :] >= lengths[:, None]
    rnd = torch.randint(1, 512, (MB, MS), generator=torch.Generator().manual_seed(6)).to(DEV)
    other = torch.where(pad, rnd, ids)
    l0, g0 = _loss_and_grads(m, ids, labels, positions, lengths=lengths)
    l1, g1 = _loss_and_grads(m, other, labels, positions, lengths=lengths)
    assert len(calls) == 4  # two layers, twice: the in-house kernels at S = 192
    assert bool(torch.isfinite(l0)) and torch.equal(l0, l1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert m(ids, labels, positions).item() != m(other, labels, positions).item()  # without the lengths it moves
    ls, _ = _loss_and_grads(m, ids, labels, positions, seqs=seqs)
    l32, _ = _loss_and_grads(_tiny().eval(), ids, labels, positions, lengths=lengths)
    ep, es = abs(l0.item() - l32.item()) / abs(l32.item()), abs(ls.item() - l32.item()) / abs(l32.item())
    print(f"MODEL S={MS} loss: lengths {ep:.2e} seqs {es:.2e}")
    assert es <= 2 * ep + FLOOR
