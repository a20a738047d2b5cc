"""Causal GQA flash attention at head dim 64 (csrc/kernels/flash_attn_d64.hip): every 64-wide row of
out, dq, dk and dv against the fp64 reference below, bounded by three times the row error of the same
reference rounded to bf16 at the kernels' rounding points (the bound and metric of
test_flash_rows_gpu.py); lse with that file's bound; document bounds; bitwise blindness of a causal
prefix and of documents to each other; the op's route.  The backward is fed the reference's out and lse.

Observed on MI355X, rowerr(kernel) / rowerr(yardstick), min - max over the cases (the bound is 3); in
brackets the yardstick's own rowerr:

    kind      out                            dq                     dk                     dv
    flat      0.82 - 0.98 (0.0036 - 0.0042)  1.00 (0.0036 - 0.0042)  1.00 (0.0031 - 0.0043)  1.00 (0.0031 - 0.0038)
    rescale   0.68 - 1.07 (0.0040 - 0.0044)  1.00 (0.0067 - 0.0398)  1.00 (0.0045 - 0.0062)  1.00 (0.0029 - 0.0040)

The launch code switches kernel variant on S % 256 alone (384 against 256 / 512), so the four shapes of
test_flash_rows_gpu.py's choice cover it.
"""
import functools
import math

import pytest
import torch

import ps_amd.ops.transformer as T
from ps_amd.ops import native

from .attn_oracle import LOG2E, bf16r, rowerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, SCALE, FACTOR = 64, 0.125, 3.0
NAMES = ("out", "lse", "dq", "dk", "dv")

SHAPES = [
    (1, 4, 1, 512),  # G = 4 as in the 1B model; several query blocks
    (1, 2, 1, 384),  # S % 256 != 0: the 4-wave forward / dQ kernels
    (1, 8, 8, 256),  # 8 units: the XCD order
    (3, 8, 8, 128),  # one block per unit; three rounds of the XCD order
]
DOC_CASES = [
    # boundaries inside a 32-key slice, a one-token document, a boundary on a tile edge
    ((1, 4, 1, 384), ((70, 1, 185, 128),)),
    ((2, 8, 8, 256), ((256,), (33, 223))),
]
CASES = [(s, None) for s in SHAPES] + DOC_CASES


def _cid(case):
    return "x".join(map(str, case[0])) + ("" if case[1] is None else "-docs")


def _row_start(row):
    """doc_start of one row from its document lengths."""
    out, s = [], 0
    for n in row:
        out += [s] * n
        s += n
    return out


def inputs(kind, B, H, KV, S, seed=0):
    """flat: randn.  rescale: k ramps by 12 exp2 units per 64-key tile along a +-1 direction q carries."""
    gen = torch.Generator().manual_seed(seed)
    u = (torch.randint(0, 2, (D,), generator=gen) * 2 - 1).double() * (kind == "rescale")
    ramp = 12.0 / (math.sqrt(D) * LOG2E) * (torch.arange(S) // 64).double()[:, None] * u
    q = torch.randn(B, H, S, D, generator=gen, dtype=torch.float64) + u
    k = torch.randn(B, KV, S, D, generator=gen, dtype=torch.float64) + ramp
    v = torch.randn(B, KV, S, D, generator=gen, dtype=torch.float64)
    dout = torch.randn(B, S, H * D, generator=gen, dtype=torch.float64)
    return tuple(x.to(torch.bfloat16) for x in (q, k, v, dout))


def reference(q, k, v, dout, start=None, out=None, lse=None, rounded=False):
    """fp64 out, lse, dq, dk, dv; the gradients from the out and lse passed in (else its own).  rounded:
    bf16 at the kernels' rounding points (P, dS, every bf16 output)."""
    r = bf16r if rounded else (lambda x: x)
    B, H, S, _ = q.shape
    KV = k.shape[1]
    G = H // KV
    kk, vv = k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    pos = torch.arange(S)
    hidden = pos[None, :] > pos[:, None]  # [S(q), S(k)]
    if start is not None:
        hidden = hidden | (pos[None, None, :] < start[:, :, None])  # [B, S, S]
        hidden = hidden[:, None]
    sc = (q.double() @ kk.transpose(-1, -2) * SCALE).masked_fill(hidden, float("-inf"))
    lse0 = torch.logsumexp(sc, -1)
    out0 = r(r(torch.exp(sc - lse0[..., None])) @ vv).transpose(1, 2).reshape(B, S, H * D)
    out, lse = (out0 if out is None else out), (lse0 if lse is None else lse)
    do = dout.double().view(B, S, H, D).transpose(1, 2)
    o = out.double().view(B, S, H, D).transpose(1, 2)
    p = torch.exp(sc - lse.double()[..., None])
    ds = r(p * (do @ vv.transpose(-1, -2) - (do * o).sum(-1, keepdim=True)))
    dq = ds @ kk * SCALE
    dk = (ds.transpose(-1, -2) @ q.double()).view(B, KV, G, S, D).sum(2) * SCALE
    dv = (r(p).transpose(-1, -2) @ do).view(B, KV, G, S, D).sum(2)
    return out0, lse0, r(dq), r(dk), r(dv)


@functools.lru_cache(maxsize=None)
def _case(kind, case):
    """Inputs, reference and yardstick of one case, computed once and left unchanged."""
    shape, rows = case
    x = inputs(kind, *shape)
    start = None if rows is None else torch.tensor([_row_start(r) for r in rows])
    out, lse = reference(*x, start)[:2]
    fed = dict(out=out.to(torch.bfloat16), lse=lse.float())  # what fa_bwd is given
    return x, start, fed, reference(*x, start, **fed), reference(*x, start, **fed, rounded=True)


def _bounds(start):
    """(doc_start, doc_end) on the device, or () for a case without documents."""
    return () if start is None else T.doc_bounds(start.to(DEV))  # doc_start identifies the document


def _run(q, k, v, dout, bounds=()):
    out, lse = native().fa_fwd(q, k, v, *bounds[:1])
    return (out, lse) + tuple(native().fa_bwd(q, k, v, out, dout, lse, *bounds))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _rows(name, t, s, e):
    return t[:, s:e] if name == "out" else t[:, :, s:e]


@pytest.mark.parametrize("kind", ["flat", "rescale"])
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_rows_against_reference(case, kind):
    (q, k, v, dout), start, fed, ref, yard = _case(kind, case)
    q, k, v, dout = (t.to(DEV) for t in (q, k, v, dout))
    bounds = _bounds(start)
    out, lse = native().fa_fwd(q, k, v, *bounds[:1])
    got = (out, lse) + tuple(native().fa_bwd(q, k, v, fed["out"].to(DEV), dout, fed["lse"].to(DEV), *bounds))
    for name, g, r, y in zip(NAMES, got, ref, yard):
        if name == "lse":
            torch.testing.assert_close(g.cpu(), r.float(), rtol=1e-3, atol=2e-3)
            continue
        if name == "out":
            g, r, y = (t.reshape(*t.shape[:2], -1, D) for t in (g, r, y))
        assert g.shape == r.shape
        e, ye = rowerr(g, r), rowerr(y, r)
        print(f"RATIO flash_d64 {kind} {_cid(case)} {name}: kernel {e:.5f} yardstick {ye:.5f} ratio {e / ye:.2f}")
        assert ye > 0 and e <= FACTOR * ye, (name, e, ye)


@pytest.mark.parametrize("case", DOC_CASES, ids=_cid)
def test_documents_bitwise(case):
    """(a) One document per row is bitwise the call without bounds.  (b) Changing q / k / v / dout of
    document 0 of every row changes no bit of the other documents' rows."""
    shape, rows = case
    B, _, _, S = shape
    q, k, v, dout = (t.to(DEV) for t in inputs("rescale", *shape, seed=1))
    one = (torch.zeros(B, S, dtype=torch.int32, device=DEV), torch.full((B, S), S, dtype=torch.int32, device=DEV))
    for name, a, b in zip(NAMES, _run(q, k, v, dout), _run(q, k, v, dout, one)):
        assert torch.equal(_bits(a), _bits(b)), name
    bounds = _bounds(torch.tensor([_row_start(r) for r in rows]))
    base = _run(q, k, v, dout, bounds)
    q2, k2, v2, dout2 = (t.clone() for t in (q, k, v, dout))
    g = torch.Generator().manual_seed(0)
    for b, row in enumerate(rows):
        for x in (q2, k2, v2):
            x[b, :, :row[0]] = (8 * torch.randn(x[b, :, :row[0]].shape, generator=g)).bfloat16().to(DEV)
        dout2[b, :row[0]] = (8 * torch.randn(dout[b, :row[0]].shape, generator=g)).bfloat16().to(DEV)
    got = _run(q2, k2, v2, dout2, bounds)
    for name, a, c in zip(NAMES, base, got):
        for b, row in enumerate(rows):
            assert not torch.equal(_rows(name, a[b:b + 1], 0, row[0]), _rows(name, c[b:b + 1], 0, row[0])), name
            assert torch.equal(_bits(_rows(name, a[b:b + 1], row[0], S)), _bits(_rows(name, c[b:b + 1], row[0], S))), name


@pytest.mark.parametrize("t", [32, 96, 160])
def test_causal_prefix_bitwise(t):
    """Rows < t of out / lse / dq are blind to k, v at positions >= t; rows >= t of dk / dv are blind to q,
    dout, out, lse at positions < t."""
    q, k, v, dout = (x.to(DEV) for x in inputs("rescale", 1, 2, 1, 256, seed=2))
    g = torch.Generator().manual_seed(t)
    noise = lambda x: (8 * torch.randn(x.shape, generator=g)).bfloat16().to(DEV)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, t:], v2[:, :, t:] = noise(k[:, :, t:]), noise(v[:, :, t:])
    a, b = _run(q, k, v, dout), _run(q, k2, v2, dout)
    assert not torch.equal(a[0][:, t:], b[0][:, t:])  # the change is seen where it may be
    for name, x, y in list(zip(NAMES, a, b))[:3]:
        assert torch.equal(_bits(_rows(name, x, 0, t)), _bits(_rows(name, y, 0, t))), name
    out, lse = a[:2]
    q2, dout2, out2, lse2 = q.clone(), dout.clone(), out.clone(), lse.clone()
    q2[:, :, :t], dout2[:, :t], out2[:, :t] = noise(q[:, :, :t]), noise(dout[:, :t]), noise(out[:, :t])
    lse2[:, :, :t] += 1.0
    _, dk2, dv2 = native().fa_bwd(q2, k, v, out2, dout2, lse2)
    assert not torch.equal(a[3][:, :, :t], dk2[:, :, :t])
    assert torch.equal(_bits(a[3][:, :, t:]), _bits(dk2[:, :, t:]))
    assert torch.equal(_bits(a[4][:, :, t:]), _bits(dv2[:, :, t:]))


@pytest.mark.parametrize("docs", [False, True], ids=["plain", "docs"])
def test_op_stays_on_flash_and_matches_sdpa(docs, monkeypatch):
    q, k, v, dout = (x.to(DEV) for x in inputs("flat", 1, 4, 1, 256, seed=5))
    bounds = T.doc_bounds(torch.tensor([_row_start((100, 156))])) if docs else None
    calls, real = [], T._FlashCausal.apply
    monkeypatch.setattr(T._FlashCausal, "apply", lambda *a: (calls.append(len(a)), real(*a))[1])
    res = []
    for off in ("", "flash_attn"):
        monkeypatch.setenv("PS_AMD_DISABLE", off)
        qi, ki, vi = (t.clone().requires_grad_() for t in (q, k, v))
        out = T.attention_causal_gqa(qi, ki, vi, doc_bounds=bounds)
        res.append((out.detach(),) + torch.autograd.grad(out, (qi, ki, vi), dout))
    assert calls == [5 if docs else 3]  # the flash route ran exactly once
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()
    (o, *g), (ro, *rg) = res
    assert bool(torch.isfinite(o.float()).all()) and rel(o, ro) < 1e-2
    for a, b in zip(g, rg):
        assert rel(a, b) < 2e-2
