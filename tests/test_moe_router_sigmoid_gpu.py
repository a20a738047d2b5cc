"""The sigmoid / bias / group-limited form of the fused MoE router (csrc/kernels/moe_router.hip,
``ops.moe.router(score="sigmoid")``) against ``_router_ref`` in fp64.

Shapes: T 1 (one row alone) and 200 (six row tiles and a partial one); D 64 (one K stage) and 192 (an odd number);
(E, k, n_group, topk_group) without groups below and at one column per lane, three groups of 24 (E no multiple of 32,
the third group straddles the lane / lane + 64 split) and eight groups of 16 at the full width.  With the fp32 logit
bound b = D 2^-23 max(|h| |Wr|^T), a score is off by at most eb = b / 4 + 1e-6 (the sigmoid's slope is at most 1/4;
1e-6 for its fp32 evaluation) and a group score by 2 eb: the choice is compared on the rows that these resolve."""
import dataclasses

import pytest
import torch

from ps_amd.models.transformer import LlamaBlock, LlamaConfig
from ps_amd.ops import moe as M
from ps_amd.ops import transformer as TR
from ps_amd.ops._ext import native

pytestmark = pytest.mark.gpu

SCALE = 2.5
shapes = pytest.mark.parametrize("T,D,E,k,ng,tg", [(T, D, *r) for T in (1, 200) for D in (64, 192)
                                                   for r in ((8, 2, 1, 1), (64, 6, 1, 1), (72, 8, 3, 2), (128, 8, 8, 4))])
norms = pytest.mark.parametrize("norm", [True, False])


def _inputs(T, D, E):
    g = torch.Generator().manual_seed(1000 * T + 10 * D + E + 1)
    h, w = torch.randn(T, D, generator=g).bfloat16().cuda(), (torch.randn(E, D, generator=g) / D ** 0.5).bfloat16().cuda()
    return h, w, (torch.rand(E, generator=g) * 0.2 - 0.1).cuda()


@shapes
@norms
def test_selection_and_values_against_fp64(T, D, E, k, ng, tg, norm):
    h, w, bias = _inputs(T, D, E)
    kw = dict(score="sigmoid", bias=bias, n_group=ng, topk_group=tg, scale=SCALE)
    idx, wts, lse, logits, part = native().moe_router_fwd(h, w, k, norm, 0, True, bias, ng, tg, SCALE)
    counts, _, (lb, zl, aux) = native().moe_router_finish(part, T, k, 0.5, 0.25)
    h64, w64 = h.double(), w.double()
    z64 = h64 @ w64.t()
    bound = D * 2.0 ** -23 * (h64.abs() @ w64.abs().t()).max().item()
    eb = bound / 4 + 1e-6
    assert (logits.double() - z64).abs().max() <= bound
    c = torch.sigmoid(z64) + bias.double()
    resolved = torch.ones(T, dtype=torch.bool, device="cuda")
    if ng > tg:
        per = c.view(T, ng, E // ng)
        gs = per.topk(2, dim=-1).values.sum(-1).sort(dim=-1, descending=True, stable=True)
        resolved = gs.values[:, tg - 1] - gs.values[:, tg] > 2 * eb
        drop = torch.ones(T, ng, dtype=torch.bool, device="cuda").scatter_(1, gs.indices[:, :tg], False)
        c = per.masked_fill(drop[:, :, None], float("-inf")).view(T, E)
    top = torch.sort(c, dim=-1, descending=True, stable=True)
    resolved &= top.values[:, k - 1] - top.values[:, k] > eb
    print(f"sigmoid router T={T} D={D} E={E} k={k} groups {ng}/{tg}: unresolved {(~resolved).float().mean().item():.4f}")
    assert (~resolved).float().mean() <= 0.03
    ridx = M._router_ref(h64, w64, k, norm, **kw)[0]
    assert torch.equal(ridx, top.indices[:, :k])  # the reference is what this test takes it for
    assert torch.equal(idx.sort(1).values[resolved], ridx.sort(1).values[resolved])
    ordered = resolved & (-top.values[:, :k + 1].diff(dim=1) > eb).all(1)
    assert torch.equal(idx[ordered], ridx[ordered])
    _, rwts, rlb = M._router_ref(h64, w64, k, norm, 1.0, 0.0, idx, **kw)
    _, _, rzl = M._router_ref(h64, w64, k, norm, 0.0, 1.0, idx, **kw)
    for what, got, ref in (("wts", wts, rwts), ("lse", lse, torch.logsumexp(z64, -1)), ("lb", lb, rlb), ("zl", zl, rzl),
                           ("aux", aux, 0.5 * rlb + 0.25 * rzl)):
        err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
        print(f"sigmoid router T={T} D={D} E={E} k={k} norm={norm} {what}: {err:.3e} (bound {4 * bound + 1e-6:.3e})")
        assert err <= 4 * bound + 1e-6, what
    assert torch.equal(counts.long(), torch.bincount(idx.reshape(-1), minlength=E))


@shapes
def test_exact_ties_go_to_the_lower_id(T, D, E, k, ng, tg):  # without bias or groups
    g = torch.Generator().manual_seed(T + D + E)
    h = torch.randint(-1, 2, (T, D), generator=g).bfloat16().cuda()
    # eight entries of +-1 a weight row: |z| <= 8, every logit an integer, the fp32 sigmoid still strictly monotone
    w = torch.zeros(E, D).scatter_(1, torch.rand(E, D, generator=g).argsort(1)[:, :8],
                                   torch.randint(0, 2, (E, 8), generator=g) * 2.0 - 1).bfloat16().cuda()
    z64 = h.double() @ w.double().t()
    assert torch.equal(M.router(h, w, k, score="sigmoid")[0],
                       torch.sort(z64, dim=-1, descending=True, stable=True).indices[:, :k])


@shapes
@norms
def test_gradients_within_2x_of_the_bf16_composition(T, D, E, k, ng, tg, norm):
    h, w, bias = _inputs(T, D, E)
    kw = dict(score="sigmoid", bias=bias, n_group=ng, topk_group=tg, scale=SCALE)
    dwts = torch.randn(T, k, generator=torch.Generator().manual_seed(E)).cuda()

    def grads(h, w, idx):
        h, w = h.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
        if idx is None:
            idx, wts, aux = M.router(h, w, k, norm, 0.5, 0.25, **kw)
        else:
            _, wts, aux = M._router_ref(h, w, k, norm, 0.5, 0.25, idx, **kw)
        ((wts * dwts.to(wts.dtype)).sum() + 0.7 * aux).backward()
        return idx, h.grad, w.grad

    idx, *fused = grads(h, w, None)
    _, *ref = grads(h.double(), w.double(), idx)
    _, *comp = grads(h, w, idx)
    for what, f, c, r in zip(("dh", "dWr"), fused, comp, ref):
        assert f.dtype == torch.bfloat16 and f.shape == r.shape
        ef, ec = (((t.double() - r).abs().max() / r.abs().max()).item() for t in (f, c))
        print(f"sigmoid router T={T} D={D} E={E} k={k} groups {ng}/{tg} norm={norm} {what}: fused {ef:.3e} "
              f"composition {ec:.3e} ratio {ef / max(ec, 1e-300):.3f}")
        assert ef <= 2 * ec, what


def test_bitwise_repeatable_rows_independent_nan_row_routed_defaults_unchanged():
    T, D, E, k = 200, 192, 72, 8
    h, w, bias = _inputs(T, D, E)
    kw = dict(score="sigmoid", bias=bias, n_group=3, topk_group=2, scale=SCALE)
    dwts = torch.randn(T, k, generator=torch.Generator().manual_seed(0)).cuda()

    def run(h, ac, zc, **kw):
        h, w_ = h.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
        idx, wts, aux = M.router(h, w_, k, True, ac, zc, **kw)
        ((wts * dwts).sum() + aux).backward()
        return idx, wts.detach(), aux.detach(), h.grad, w_.grad

    assert all(torch.equal(a, b) for a, b in zip(run(h, 0.5, 0.25, **kw), run(h, 0.5, 0.25, **kw)))
    keep = torch.arange(0, T, 7, device="cuda")
    h2 = -3 * h.flip(0)
    h2[keep] = h[keep]
    a, b = run(h, 0.0, 0.0, **kw), run(h2, 0.0, 0.0, **kw)
    assert all(torch.equal(a[i][keep], b[i][keep]) for i in (0, 1, 3)) and not torch.equal(a[1], b[1])
    h3 = h.clone()
    h3[3] = float("nan")
    idx = M.router(h3, w, k, **kw)[0].sort(1).values
    assert (idx >= 0).all() and (idx < E).all() and (idx.diff(dim=1) > 0).all()
    explicit = dict(score="softmax", bias=None, n_group=1, topk_group=1, scale=1.0)
    assert all(torch.equal(a, b) for a, b in zip(run(h, 0.5, 0.25), run(h, 0.5, 0.25, **explicit)))


def test_llama_block_routes_with_a_balanced_bias(monkeypatch):
    ran = []
    real = M._Router.apply
    monkeypatch.setattr(M._Router, "apply", lambda *a: ran.append(1) or real(*a))
    c = dataclasses.replace(LlamaConfig.tiny_moe(), moe_score="sigmoid", moe_bias_balance=True, moe_n_group=2,
                            moe_topk_group=1)
    torch.manual_seed(0)
    blk = LlamaBlock(c).cuda().bfloat16()
    assert "router_bias" in dict(blk.named_buffers())
    x = torch.randn(2, 128, c.hidden, device="cuda").bfloat16()
    blk(x, None, TR.rope_table(128, c.hidden // c.heads, c.rope_theta, "cuda"))
    n = blk.last_counts.float()
    assert ran == [1] and n.sum() == 2 * 128 * c.moe_top_k and (n != n.mean()).any()
    blk.update_router_bias(1e-2)
    assert (blk.router_bias[n < n.mean()] > 0).all() and (blk.router_bias[n > n.mean()] < 0).all()
    assert not hasattr(LlamaBlock(LlamaConfig.tiny_moe()), "router_bias")


def test_refusals():
    h, w, bias = _inputs(4, 64, 8)
    for k, kw in ((2, dict(score="sigmoid", n_group=3, topk_group=1)), (3, dict(score="sigmoid", n_group=4, topk_group=1)),
                  (2, dict(bias=bias)), (2, dict(score="sigmoid", bias=bias[:7]))):
        with pytest.raises(ValueError):
            M.router(h, w, k, **kw)
