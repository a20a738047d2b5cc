"""Causal GQA flash attention over packed documents (the DOCS instantiations of
csrc/kernels/flash_attn.hip): every 128-wide row of out, dq, dk and dv against the fp64 document
oracle (tests/flash_docs_oracle.py), bounded by three times the row error of the bf16 rounding
yardstick on the same inputs (the factor and metric of test_flash_rows_gpu.py); lse with that
file's bound; one document per row bitwise equal to the plain kernels; bitwise isolation of the
documents from each other; determinism; the op against its SDPA route; the model.  The backward is
fed the oracle's out and lse.  Each layout is the smallest shape that reaches its branch.

Observed on MI355X, rowerr(kernel) / rowerr(yardstick), min - max over the six layouts (the bound
is 3); in brackets the yardstick's own rowerr, the quantity the bound is a multiple of:

    kind      out                            dq                     dk                     dv
    flat      0.74 - 0.98 (0.0036 - 0.0040)  1.00 (0.0034 - 0.0040)  1.00 (0.0044 - 0.0063)  1.00 (0.0030 - 0.0036)
    rescale   0.65 - 0.77 (0.0035 - 0.0040)  1.00 (0.0045 - 0.0248)  1.00 (0.0040 - 0.0057)  1.00 (0.0031 - 0.0040)
    descend   0.67 - 0.75 (0.0037 - 0.0041)  1.00 (0.0047 - 0.0290)  1.00 (0.0043 - 0.0073)  1.00 (0.0031 - 0.0036)

As in test_flash_rows_gpu.py the gradients agree with the yardstick to the printed digits (same
rounding points, fp32 in between) and out differs because the kernel rounds P before the division
by l.  Under descend one leaked key of an earlier document would outweigh every visible key by
2^12 per tile: the ratios there are those of the other kinds.
"""
import functools

import pytest
import torch

import ps_amd.ops.transformer as T
from ps_amd.ops import native

from . import attn_oracle as ao
from . import flash_docs_oracle as fo
from .test_flash_rows_gpu import SHAPES as PLAIN_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"

LAYOUTS = [
    # 4-wave path, one block; the boundary is inside the wave of queries 64..95, which still processes
    # tile 0 for its lanes 64..79 while lanes 80..95 see none of it
    ((1, 4, 2, 128), ((80, 48),)),
    # 4-wave, three blocks: boundaries one past a tile edge, on a block edge, one past a block edge
    ((1, 2, 1, 384), ((65, 63, 129, 127),)),
    # 8-wave path, XCD order: boundaries on tile edges and a one-token document
    ((1, 8, 8, 256), ((64, 64, 1, 63, 64),)),
    # the second block starts its key loop at tile 4; key blocks 0 and 1 end their query stages at 256
    ((1, 4, 2, 512), ((256, 256),)),
    # G = 4, different rows, a document across a block edge, a boundary one short of a wave edge
    ((2, 4, 1, 512), ((300, 212), (31, 1, 480))),
    # 24 units, three rounds of the XCD order
    ((3, 8, 8, 128), ((128,), (1, 1, 2, 4, 8, 16, 32, 64), (127, 1))),
]
KINDS = ["flat", "rescale", "descend"]
FACTOR = 3.0


def _lid(layout):
    return "x".join(map(str, layout[0]))


def _heads(out):
    return out.view(*out.shape[:2], -1, ao.FLASH_D)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _bounds(rows):
    """doc_start, doc_end on the device from per-row length lists."""
    return T.doc_bounds(fo.doc_ids_from_lengths(rows).to(DEV))


@functools.lru_cache(maxsize=None)
def _case(kind, layout):
    """Inputs, fp64 oracle and yardstick of one case, computed once and left unchanged."""
    shape, rows = layout
    q, k, v, dout = ao.flash_inputs(kind, *shape, seed=0)
    ids = fo.doc_ids_from_lengths(rows)
    out, lse = fo.flash_docs_fwd(q, k, v, ids)
    yout, _ = fo.flash_docs_fwd(q, k, v, ids, rounded=True)
    out_in, lse_in = out.to(torch.bfloat16), lse.float()  # what fa_bwd is given
    grads = fo.flash_docs_bwd(q, k, v, out_in, dout, lse_in, ids)
    ygrads = fo.flash_docs_bwd(q, k, v, out_in, dout, lse_in, ids, rounded=True)
    return dict(q=q, k=k, v=v, dout=dout, out=out, lse=lse, yout=yout, out_in=out_in, lse_in=lse_in, grads=grads,
                ygrads=ygrads)


def _bound(name, kind, layout, got, ref, yard):
    e, y = ao.rowerr(got, ref), ao.rowerr(yard, ref)
    print(f"RATIO flash_docs {kind} {_lid(layout)} {name}: kernel {e:.5f} yardstick {y:.5f} ratio {e / max(y, 1e-30):.2f}")
    assert y > 0
    assert e <= FACTOR * y, (name, e, y)


# ------------------------------------------------------------------ 1, 2. per row against the oracle
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=_lid)
def test_flash_docs_forward_rows(layout, kind):
    c = _case(kind, layout)
    start, _ = _bounds(layout[1])
    out, lse = native().fa_fwd(*(c[n].to(DEV) for n in "qkv"), start)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
    _bound("out", kind, layout, _heads(out), _heads(c["out"]), _heads(c["yout"]))
    torch.testing.assert_close(lse.cpu(), c["lse"].float(), rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=_lid)
def test_flash_docs_backward_rows(layout, kind):
    c = _case(kind, layout)
    start, end = _bounds(layout[1])
    got = native().fa_bwd(*(c[n].to(DEV) for n in ("q", "k", "v", "out_in", "dout", "lse_in")), start, end)
    for name, g, ref, yard in zip(("dq", "dk", "dv"), got, c["grads"], c["ygrads"]):
        assert g.shape == ref.shape
        assert bool(torch.isfinite(g.float()).all()), name
        _bound(name, kind, layout, g, ref, yard)


# ------------------------------------------------------------------ 3. one document is the plain kernel
def _run(q, k, v, dout, bounds=None):
    """Full forward + backward -> out, lse, dq, dk, dv."""
    nat = native()
    if bounds is None:
        out, lse = nat.fa_fwd(q, k, v)
        return (out, lse) + tuple(nat.fa_bwd(q, k, v, out, dout, lse))
    out, lse = nat.fa_fwd(q, k, v, bounds[0])
    return (out, lse) + tuple(nat.fa_bwd(q, k, v, out, dout, lse, *bounds))


NAMES = ("out", "lse", "dq", "dk", "dv")


@pytest.mark.parametrize("shape", PLAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_document_per_row_is_bitwise_the_plain_kernels(shape):
    B, _, _, S = shape
    q, k, v, dout = (x.to(DEV) for x in ao.flash_inputs("rescale", *shape, seed=1))
    start = torch.zeros(B, S, dtype=torch.int32, device=DEV)
    end = torch.full((B, S), S, dtype=torch.int32, device=DEV)
    plain = _run(q, k, v, dout)
    docs = _run(q, k, v, dout, (start, end))
    for name, a, b in zip(NAMES, plain, docs):
        assert torch.equal(_bits(a), _bits(b)), name


# ------------------------------------------------------------------ 4, 5. isolation
def _rows(name, t, s, e):
    """Rows s..e of a result along its sequence axis (out is [B, S, H * D], the others [B, heads, S, ...])."""
    return t[:, s:e] if name == "out" else t[:, :, s:e]


ALIGNED = [
    ((1, 4, 2, 512), (256, 256)),
    ((1, 8, 8, 256), (64, 32, 96, 64)),
    ((1, 2, 1, 384), (128, 160, 96)),
]


@pytest.mark.parametrize("layout", ALIGNED, ids=_lid)
def test_documents_are_bitwise_isolated_at_wave_aligned_boundaries(layout):
    """Replacing q, k, v, dout inside one document changes no bit of any other document's rows of out,
    lse, dq, dk, dv (full forward + backward), and does change its own.  Boundaries are multiples of
    32: the forward's deferred rescale is decided per wave, so a neighbour inside the same wave may
    legitimately move the last bit."""
    shape, lengths = layout
    q, k, v, dout = (x.to(DEV) for x in ao.flash_inputs("rescale", *shape, seed=2))
    bounds = _bounds([lengths])
    base = _run(q, k, v, dout, bounds)
    spans = fo.doc_spans(lengths)
    for d, (s, e) in enumerate(spans):
        g = torch.Generator().manual_seed(d)
        q2, k2, v2, dout2 = q.clone(), k.clone(), v.clone(), dout.clone()
        for x in (q2, k2, v2):
            x[:, :, s:e] = (8 * torch.randn(x[:, :, s:e].shape, generator=g)).bfloat16().to(DEV)
        dout2[:, s:e] = (8 * torch.randn(dout[:, s:e].shape, generator=g)).bfloat16().to(DEV)
        got = _run(q2, k2, v2, dout2, bounds)
        for name, a, b in zip(NAMES, base, got):
            assert not torch.equal(_rows(name, a, s, e), _rows(name, b, s, e)), (name, d)
            for d2, (s2, e2) in enumerate(spans):
                if d2 != d:
                    assert torch.equal(_bits(_rows(name, a, s2, e2)), _bits(_rows(name, b, s2, e2))), (name, d, d2)


@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[1]], ids=_lid)
def test_backward_is_bitwise_isolated_at_any_boundary(layout):
    """dq, dk, dv rows of the other documents do not change by one bit when q, dout, out, lse, k and v
    change inside one document."""
    shape, rows = layout
    lengths = rows[0]
    q, k, v, dout = (x.to(DEV) for x in ao.flash_inputs("rescale", *shape, seed=3))
    bounds = _bounds(rows)
    out, lse = native().fa_fwd(q, k, v, bounds[0])
    base = native().fa_bwd(q, k, v, out, dout, lse, *bounds)
    spans = fo.doc_spans(lengths)
    for d, (s, e) in enumerate(spans):
        g = torch.Generator().manual_seed(d)
        q2, k2, v2, dout2, out2, lse2 = (x.clone() for x in (q, k, v, dout, out, lse))
        for x in (q2, k2, v2):
            x[:, :, s:e] = (8 * torch.randn(x[:, :, s:e].shape, generator=g)).bfloat16().to(DEV)
        for x in (dout2, out2):
            x[:, s:e] = (8 * torch.randn(x[:, s:e].shape, generator=g)).bfloat16().to(DEV)
        lse2[:, :, s:e] += 1.0
        got = native().fa_bwd(q2, k2, v2, out2, dout2, lse2, *bounds)
        for name, a, b in zip(("dq", "dk", "dv"), base, got):
            assert not torch.equal(a[:, :, s:e], b[:, :, s:e]), (name, d)
            for d2, (s2, e2) in enumerate(spans):
                if d2 != d:
                    assert torch.equal(_bits(a[:, :, s2:e2]), _bits(b[:, :, s2:e2])), (name, d, d2)


# ------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("layout", LAYOUTS, ids=_lid)
def test_flash_docs_is_deterministic(layout):
    shape, rows = layout
    q, k, v, dout = (x.to(DEV) for x in ao.flash_inputs("rescale", *shape, seed=4))
    bounds = _bounds(rows)
    a = _run(q, k, v, dout, bounds)
    b = _run(q, k, v, dout, bounds)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(_bits(x), _bits(y)), name


# ------------------------------------------------------------------ 7. the op
def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[2], LAYOUTS[4]], ids=_lid)
def test_op_with_doc_bounds_flash_matches_sdpa(layout, monkeypatch):
    shape, rows = layout
    q, k, v, dout = (x.to(DEV) for x in ao.flash_inputs("flat", *shape, seed=5))
    ids = fo.doc_ids_from_lengths(rows)  # int64, on the host
    calls = []
    real = T._FlashCausal.apply

    def spy(*a):
        calls.append(len(a))
        return real(*a)

    monkeypatch.setattr(T._FlashCausal, "apply", spy)
    res = []
    for off in ("", "flash_attn"):
        monkeypatch.setenv("PS_AMD_DISABLE", off)
        qi, ki, vi = (t.clone().requires_grad_() for t in (q, k, v))
        out = T.attention_causal_gqa(qi, ki, vi, doc_bounds=T.doc_bounds(ids))
        res.append((out.detach(),) + torch.autograd.grad(out, (qi, ki, vi), dout))
    assert calls == [5]  # the flash route ran exactly once, with both bound tensors
    (o, *g), (ro, *rg) = res
    assert bool(torch.isfinite(o.float()).all())
    assert _rel(o, ro) < 1e-2
    for a, b in zip(g, rg):
        assert _rel(a, b) < 2e-2


# ------------------------------------------------------------------ 8. the model
def test_llama_with_doc_ids_isolates_documents_and_trains():
    from ps_amd.models.transformer import LlamaConfig, LlamaForCausalLM, packed_lm_batch

    c = LlamaConfig(vocab=512, hidden=512, layers=2, heads=4, kv_heads=2, ffn=1024, max_seq=256)
    torch.manual_seed(0)
    m = LlamaForCausalLM(c).to(DEV).to(torch.bfloat16).eval()
    ids, labels, doc_ids = packed_lm_batch(1, 256, c.vocab, [[128, 128]], seed=6, device=DEV)
    ids2 = ids.clone()
    ids2[:, :128] = (ids[:, :128] + 1 + torch.arange(128, device=DEV)) % c.vocab
    with torch.no_grad():
        a, b = m(ids, doc_ids=doc_ids), m(ids2, doc_ids=doc_ids)
        pa, pb = m(ids), m(ids2)
    assert not torch.equal(a[:, :128], b[:, :128])
    assert torch.equal(_bits(a[:, 128:]), _bits(b[:, 128:]))
    assert not torch.equal(pa[:, 128:], pb[:, 128:])
    for ckpt in (False, True):
        m.checkpointing = ckpt
        m.train()
        m.zero_grad()
        loss = m(ids, labels, doc_ids=doc_ids)
        loss.backward()
        assert bool(torch.isfinite(loss))
        for n, p in m.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all()), (ckpt, n)
