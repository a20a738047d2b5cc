"""The fused MoE router (csrc/kernels/moe_router.hip, ops.moe.router) against ``_router_ref`` in fp64.

Shapes: T 1 (one row alone), 200 (full row tiles plus a partial one) and 1100 (35 row tiles: the finish kernel's 16
waves fold several partial rows each, the last waves none); D 64 (one K stage), 192 (an odd number of stages,
wrapping the double buffer) and 384 (6 stages, the fewest at which the 4-stage register ring refills in the prologue
and in the loop, starts a second trip and ends ragged; the derived bound grows as D^1.5, and at 576 the fp64
reference alone leaves about 2 % of the rows with E 128 unresolved, at 384 about 1 %);
(E, k) below one lane group, one column per lane, E no multiple of 32, and the full width.  The logit bound is the
fp32 dot-product bound D 2^-23 max(|h| |Wr|^T); the gradients are held to 2x the error of the bf16 composition with
the same selection, the project's rule for the MoE and LM-head kernels.  The order inside a top-k is checked where
the logits are exact (integers) and, on random inputs, on the rows whose adjacent fp64 gaps down to the (k+1)-th
logit all exceed the bound; rows where only the k-th / (k+1)-th gap does are compared as a set, since two chosen
experts may be closer than fp32 resolves."""
import dataclasses

import pytest
import torch

from ps_amd import knobs
from ps_amd.models.transformer import LlamaBlock, LlamaConfig
from ps_amd.ops import moe as M
from ps_amd.ops import transformer as TR
from ps_amd.ops._ext import native

pytestmark = pytest.mark.gpu

shapes = pytest.mark.parametrize("T,D,E,k", [(T, D, E, k) for T in (1, 200, 1100) for D in (64, 192, 384)
                                             for E, k in ((4, 2), (8, 1), (72, 8), (128, 8))])
norms = pytest.mark.parametrize("norm", [True, False])


def _inputs(T, D, E):
    g = torch.Generator().manual_seed(1000 * T + 10 * D + E + 1)
    return torch.randn(T, D, generator=g).bfloat16().cuda(), (torch.randn(E, D, generator=g) / D ** 0.5).bfloat16().cuda()


@shapes
def test_selection_is_exact_ties_to_the_lower_id(T, D, E, k):
    g = torch.Generator().manual_seed(T + D + E)
    h = torch.randint(-2, 3, (T, D), generator=g).bfloat16().cuda()  # every logit exact in fp32, ties common
    w = torch.randint(-1, 2, (E, D), generator=g).bfloat16().cuda()
    idx, _, _ = M.router(h, w, k)
    z64 = h.double() @ w.double().t()
    assert torch.equal(idx, torch.sort(z64, dim=-1, descending=True, stable=True).indices[:, :k])


@shapes
@norms
def test_values_against_fp64(T, D, E, k, norm):
    h, w = _inputs(T, D, E)
    idx, wts, lse, logits, part = native().moe_router_fwd(h, w, k, norm)
    counts, _, (lb, zl, aux) = native().moe_router_finish(part, T, k, 0.5, 0.25)
    h64, w64 = h.double(), w.double()
    z64 = h64 @ w64.t()
    bound = D * 2.0 ** -23 * (h64.abs() @ w64.abs().t()).max().item()
    assert (logits.double() - z64).abs().max() <= bound
    _, rwts, rlb = M._router_ref(h64, w64, k, norm, 1.0, 0.0, idx=idx)
    _, _, rzl = M._router_ref(h64, w64, k, norm, 0.0, 1.0, idx=idx)
    for what, got, ref in (("wts", wts, rwts), ("lse", lse, torch.logsumexp(z64, -1)), ("lb", lb, rlb), ("zl", zl, rzl),
                           ("aux", aux, 0.5 * rlb + 0.25 * rzl)):
        err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
        print(f"router T={T} D={D} E={E} k={k} norm={norm} {what}: {err:.3e} (bound {4 * bound + 1e-6:.3e})")
        assert err <= 4 * bound + 1e-6, what
    assert torch.equal(counts.long(), torch.bincount(idx.reshape(-1), minlength=E))
    top = torch.sort(z64, dim=-1, descending=True, stable=True)
    clear = top.values[:, k - 1] - top.values[:, k] > bound  # rows whose k-th / (k+1)-th gap fp32 resolves
    assert (~clear).float().mean() < 0.02
    assert torch.equal(idx.sort(1).values[clear], top.indices[:, :k].sort(1).values[clear])
    ordered = (-top.values[:, :k + 1].diff(dim=1) > bound).all(1)  # every adjacent gap resolved: the order too
    assert torch.equal(idx[ordered], top.indices[:, :k][ordered])


@pytest.mark.parametrize("E,k", [(4, 2), (8, 1), (72, 8), (128, 8)])
def test_row_tile_64_gives_the_same_bits(E, k):
    T, D = 200, 384
    h, w = _inputs(T, D, E)
    a, b = (native().moe_router_fwd(h, w, k, True, tm) for tm in (32, 64))
    assert b[4].shape[0] == (T + 63) // 64 and all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))
    fa, fb = (native().moe_router_finish(p[4], T, k, 0.5, 0.25) for p in (a, b))
    assert torch.equal(fa[0], fb[0]) and (fa[2] - fb[2]).abs().max() <= 1e-5 * fa[2].abs().max()


@shapes
@norms
def test_gradients_within_2x_of_the_bf16_composition(T, D, E, k, norm):
    h, w = _inputs(T, D, E)
    dwts = torch.randn(T, k, generator=torch.Generator().manual_seed(E)).cuda()

    def grads(h, w, idx):
        h, w = h.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
        if idx is None:
            idx, wts, aux = M.router(h, w, k, norm, 0.5, 0.25)
        else:
            _, wts, aux = M._router_ref(h, w, k, norm, 0.5, 0.25, idx=idx)
        ((wts * dwts.to(wts.dtype)).sum() + 0.7 * aux).backward()
        return idx, h.grad, w.grad

    idx, *fused = grads(h, w, None)
    _, *ref = grads(h.double(), w.double(), idx)
    _, *comp = grads(h, w, idx)
    for what, f, c, r in zip(("dh", "dWr"), fused, comp, ref):
        assert f.dtype == torch.bfloat16 and f.shape == r.shape
        ef, ec = (((t.double() - r).abs().max() / r.abs().max()).item() for t in (f, c))
        print(f"router T={T} D={D} E={E} k={k} norm={norm} {what}: fused {ef:.3e} composition {ec:.3e} "
              f"ratio {ef / max(ec, 1e-300):.3f}")
        assert ef <= 2 * ec, what


def test_bitwise_repeatable_rows_independent_nan_row_routed():
    T, D, E, k = 200, 192, 72, 8
    h, w = _inputs(T, D, E)
    dwts = torch.randn(T, k, generator=torch.Generator().manual_seed(0)).cuda()

    def run(h, ac, zc):
        h, w_ = h.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
        idx, wts, aux = M.router(h, w_, k, True, ac, zc)
        ((wts * dwts).sum() + aux).backward()
        return idx, wts.detach(), aux.detach(), h.grad, w_.grad

    assert all(torch.equal(a, b) for a, b in zip(run(h, 0.5, 0.25), run(h, 0.5, 0.25)))
    keep = torch.arange(0, T, 7, device="cuda")
    h2 = -3 * h.flip(0)
    h2[keep] = h[keep]
    a, b = run(h, 0.0, 0.0), run(h2, 0.0, 0.0)
    assert all(torch.equal(a[i][keep], b[i][keep]) for i in (0, 1, 3)) and not torch.equal(a[1], b[1])
    h3 = h.clone()
    h3[3] = float("nan")
    idx = M.router(h3, w, k)[0].sort(1).values
    assert (idx >= 0).all() and (idx < E).all() and (idx.diff(dim=1) > 0).all()


def test_llama_block_takes_the_fused_router(monkeypatch):
    ran = []
    real = M._Router.apply
    monkeypatch.setattr(M._Router, "apply", lambda *a: ran.append(1) or real(*a))
    c = dataclasses.replace(LlamaConfig.tiny_moe(), moe_fused_router=True)
    torch.manual_seed(0)
    blk = LlamaBlock(c).cuda().bfloat16()
    x = torch.randn(2, 128, c.hidden, device="cuda").bfloat16()
    cs = TR.rope_table(128, c.hidden // c.heads, c.rope_theta, "cuda")
    _, on = blk(x, None, cs)
    assert ran == [1] and M.router.last_counts.sum() == 2 * 128 * c.moe_top_k
    monkeypatch.setenv(knobs.ENV, "moe_router")
    _, off = blk(x, None, cs)
    assert ran == [1] and on.shape == off.shape and torch.isfinite(off.float()).all()


def test_bindings_refuse_what_does_not_fit():
    n = native()
    z = lambda *s: torch.zeros(*s, device="cuda").bfloat16()  # noqa: E731
    for h, w, k in ((z(4, 64), z(129, 64), 2), (z(4, 64), z(4, 64), 5), (z(4, 32), z(4, 32), 2),
                    (z(4, 64).float(), z(4, 64), 2)):
        with pytest.raises(RuntimeError):
            n.moe_router_fwd(h, w, k, True)
    odd = torch.randn(4 * 64 + 1, device="cuda").bfloat16()[1:].view(4, 64)  # contiguous, 2 bytes off a 16-B boundary
    with pytest.raises(RuntimeError):
        n.moe_router_fwd(odd, z(4, 64), 2, True)
    assert not M.router_ok(odd, z(4, 64), 2) and M.router(odd, z(4, 64), 2)[0].shape == (4, 2)  # the composition
