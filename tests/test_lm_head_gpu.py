"""The fused LM-head loss (csrc/kernels/lm_head.hip, ops/lm_head.py) against fp64: z = h.double() @ w.double().T,
F.cross_entropy, autograd.  The yardstick is the bf16 composition cross_entropy(ps_linear(h, w), labels) on the
same inputs (PS_AMD_DISABLE=fused_head): the fused path never rounds a logit, so its per-row loss error stays within
the composition's; dh and dW round dz to bf16 at the same place but sum in another order, so their maximum error
stays within 2x the composition's.  Shapes: a row-tile tail, 1 / 2 / 3 K stages, a vocabulary tail of 8 columns,
several tiles per split, several backward chunks with a partial last one."""
import dataclasses
import functools

import pytest
import torch
import torch.nn.functional as F

from ps_amd import knobs
from ps_amd.models import transformer as TM
from ps_amd.ops import lm_head as L
from ps_amd.ops._ext import native
from ps_amd.ops.linear import GradDst, ps_linear

pytestmark = pytest.mark.gpu

CASES = [(200, 128, 264, 128, 1), (200, 64, 264, 128, 3), (136, 192, 1032, 384, 2)]  # T, D, V, chunk_cols, NS


def _fp64(h, w, y):
    """-> per-row loss, dh, dW of the mean over the scored rows, in fp64"""
    hd, wd = h.double().requires_grad_(), w.double().requires_grad_()
    scored = (y >= 0) & (y < w.shape[0])
    rows = F.cross_entropy(hd @ wd.T, torch.where(scored, y, -100), reduction="none")
    (rows.sum() / scored.sum().clamp(min=1)).backward()
    return rows.detach(), hd.grad, wd.grad


@functools.lru_cache(maxsize=None)
def _case(T, D, V, scale):
    """Inputs and the fp64 results; read-only."""
    g = torch.Generator().manual_seed(T + D + V)
    h = (scale * torch.randn(T, D, generator=g)).bfloat16().cuda()
    w = (0.05 * torch.randn(V, D, generator=g)).bfloat16().cuda()
    y = torch.randint(0, V, (T,), generator=g)
    y[::7] = -100
    y[1], y[2] = V - 1, V + 5  # in the tail tile; out of range: not scored
    y = y.cuda()
    return (h, w, y), _fp64(h, w, y)


def _grads(fn, h, w, y):
    h, w = h.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    loss = fn(h, w, y)
    loss.backward()
    return loss.detach(), h.grad, w.grad


@pytest.mark.parametrize("scale", [1.0, 8.0])
@pytest.mark.parametrize("T,D,V,chunk,ns", CASES)
def test_fused_against_fp64_and_the_composition(T, D, V, chunk, ns, scale, monkeypatch):
    (h, w, y), ref = _case(T, D, V, scale)
    fused_fn = lambda h, w, y: L._LinearXent.apply(h, w, y, -100, chunk, ns)  # noqa: E731
    fused = (native().lm_head_fwd(h, w, y, -100, ns)[1],) + _grads(fused_fn, h, w, y)[1:]
    again = (native().lm_head_fwd(h, w, y, -100, ns)[1],) + _grads(fused_fn, h, w, y)[1:]
    monkeypatch.setenv(knobs.ENV, "fused_head")
    comp = (native().xent_fwd(ps_linear(h, w), y, -100)[1],) + _grads(L.linear_cross_entropy, h, w, y)[1:]
    for what, bound, f, a, c, r in zip(("loss_row", "dh", "dW"), (1, 2, 2), fused, again, comp, ref):
        assert f.dtype == c.dtype and f.shape == c.shape
        assert torch.equal(f, a), what  # two calls, bitwise
        ef, ec = ((t.double() - r).abs().max().item() for t in (f, c))
        print(f"lm_head T={T} D={D} V={V} scale={scale} {what}: fused {ef:.3e} composition {ec:.3e} "
              f"ratio {ef / max(ec, 1e-300):.3f}")
        assert ef <= bound * ec, what
    unscored = (y < 0) | (y >= V)
    assert not fused[0][unscored].any() and not fused[1][unscored].any()  # exact zeros


def test_a_row_does_not_depend_on_the_others():
    T, D, V, chunk, ns = CASES[2]
    (h, w, y), _ = _case(T, D, V, 1.0)
    keep = torch.arange(1, T, 5, device="cuda")
    h2 = -3 * h.flip(0)
    h2[keep] = h[keep]
    fn = lambda h, w, y: L._LinearXent.apply(h, w, y, -100, chunk, ns)  # noqa: E731
    a, b = _grads(fn, h, w, y), _grads(fn, h2, w, y)
    ra, rb = (native().lm_head_fwd(x, w, y, -100, ns)[1] for x in (h, h2))
    assert torch.equal(ra[keep], rb[keep]) and torch.equal(a[1][keep], b[1][keep])
    assert not torch.equal(ra, rb)


def test_all_rows_ignored():
    (h, w, y), _ = _case(*CASES[0][:3], 1.0)
    loss, dh, dw = _grads(L.linear_cross_entropy, h, w, torch.full_like(y, -100))
    assert loss.item() == 0 and not dh.any() and not dw.any()


def test_route_is_taken_on_the_domain_only(monkeypatch):
    ran = []
    real = L._LinearXent.apply
    monkeypatch.setattr(L._LinearXent, "apply", lambda *a: ran.append(1) or real(*a))
    y = torch.arange(16, device="cuda")
    for V, D, dt, want in ((264, 64, torch.bfloat16, 1), (260, 64, torch.bfloat16, 0), (264, 96, torch.bfloat16, 0),
                           (264, 64, torch.float32, 0)):
        ran.clear()
        h, w = torch.randn(2, 8, D, device="cuda", dtype=dt), torch.randn(V, D, device="cuda", dtype=dt) / 8
        assert torch.isfinite(L.linear_cross_entropy(h, w, y.view(2, 8).int()))
        assert len(ran) == want, (V, D, dt)


def test_bindings_refuse_what_does_not_fit():
    n = native()
    h, w = torch.zeros(16, 64, device="cuda").bfloat16(), torch.zeros(264, 64, device="cuda").bfloat16()
    y = torch.zeros(16, dtype=torch.int64, device="cuda")
    lse, one = torch.zeros(16, device="cuda"), torch.ones(1, device="cuda")
    n.lm_head_dz(h, w, y, lse, one, one, -100, 128, torch.empty(16, 136, device="cuda").bfloat16())  # fits
    for bad in ((h.float(), w, y), (h, w.float(), y), (h.t().contiguous().t(), w, y), (h, w[:, :32].contiguous(), y),
                (h, w[:260], y), (h, w, y.int()), (h, w, y[:8])):
        with pytest.raises(RuntimeError):
            n.lm_head_fwd(*bad, -100, 0)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    for v0, dz in ((136, torch.empty(16, 136, **bf)), (128, torch.empty(8, 128, **bf)), (4, torch.empty(16, 128, **bf)),
                   (0, torch.empty(16, 128, device="cuda"))):  # past V, rows, v0 % 8, dtype
        with pytest.raises(RuntimeError):
            n.lm_head_dz(h, w, y, lse, one, one, -100, v0, dz)


def test_llama_fused_head_flag(monkeypatch):
    seen = []
    real = TM.linear_cross_entropy
    monkeypatch.setattr(TM, "linear_cross_entropy", lambda h, w, y, **k: seen.append((h, y)) or real(h, w, y, **k))
    c = TM.LlamaConfig.tiny()
    torch.manual_seed(0)
    off = TM.LlamaForCausalLM(c).cuda().bfloat16()
    on = TM.LlamaForCausalLM(dataclasses.replace(c, fused_head=True)).cuda().bfloat16()
    on.load_state_dict(off.state_dict())  # the same parameter names
    wt = on.lm_head.weight
    slot = torch.zeros(wt.numel(), device="cuda", dtype=wt.dtype)
    wt._ps_gdst = GradDst(slot, 0, wt.numel(), wt.shape)
    ids = torch.randint(0, c.vocab, (2, 128), device="cuda")
    got = []
    for m in (on, off):
        loss = m(ids, labels=ids)
        loss.backward()
        got.append((loss.detach(), m.lm_head.weight.grad))
    assert len(seen) == 1 and wt._ps_gdst.claimed and wt.grad.data_ptr() == slot.data_ptr()  # landed in the slot
    h, y = seen[0]
    rows, _, dw = _fp64(h.detach().reshape(-1, c.hidden), wt.detach(), y.reshape(-1))
    ref = (rows.sum() / (y != -100).sum(), dw)
    for what, bound, f, o, r in zip(("loss", "dW"), (1, 2), got[0], got[1], ref):
        ef, ec = ((t.double() - r).abs().max().item() for t in (f, o))
        print(f"llama tiny fused_head {what}: fused {ef:.3e} composition {ec:.3e}")
        assert ef <= bound * ec, what
