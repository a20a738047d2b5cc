"""The attention oracles of tests/attn_oracle.py, checked without a GPU: the backward formulas
against fp64 autograd, the input builders against the regimes they claim to reach (measured on
the fp64 scores), and a demonstration that the ramped inputs and the row metric expose an online-
softmax defect that the flat inputs cannot."""
import pytest
import torch

from . import attn_oracle as ao


# ------------------------------------------------------------------ oracle backward == autograd
def _direct_flash(q, k, v):
    B, H, S, D = q.shape
    G = H // k.shape[1]
    sc = q @ k.repeat_interleave(G, 1).transpose(-1, -2) / D ** 0.5
    sc = sc.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    o = torch.softmax(sc, -1) @ v.repeat_interleave(G, 1)
    return o.transpose(1, 2).reshape(B, S, H * D), torch.logsumexp(sc, -1)


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("kind", ["flat", "rescale"])
def test_flash_oracle_backward_is_autograd(G, kind):
    q, k, v, dout = ao.flash_inputs(kind, 2, 2 * G, 2, 128, seed=3)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    ro, rl = _direct_flash(qd, kd, vd)
    out, lse = ao.flash_fwd(q, k, v)
    torch.testing.assert_close(out, ro.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lse, rl.detach(), rtol=1e-12, atol=1e-12)
    ro.backward(dout.double())
    for got, ref in zip(ao.flash_bwd(q, k, v, out, dout, lse), (qd.grad, kd.grad, vd.grad)):
        assert got.shape == ref.shape
        torch.testing.assert_close(got, ref, rtol=1e-10, atol=1e-10)


def _direct_short(qkv, heads, keep, p):
    b, s, _ = qkv.shape
    q, k, v = qkv.view(b, s, 3, heads, 64).permute(2, 0, 3, 1, 4)
    sc = q @ k.transpose(-1, -2) * 0.125
    pr = torch.softmax(sc, -1)
    if keep is not None:
        pr = pr * keep.view(b, heads, s, s).double() / (1 - ao.short_p_eff(p))
    return (pr @ v).transpose(1, 2).reshape(b, s, heads * 64), torch.logsumexp(sc, -1)


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_short_oracle_backward_is_autograd(S, p):
    B, H = 2, 3
    qkv, dout = ao.short_inputs(3.0, B, S, H, seed=S)
    keep = None
    if p > 0:
        keep = (torch.rand(B * H, S, S, generator=torch.Generator().manual_seed(1)) >= p).to(torch.uint8)
    x = qkv.double().requires_grad_()
    ro, rl = _direct_short(x, H, keep, p)
    out, lse = ao.short_fwd(qkv, H, keep, p)
    torch.testing.assert_close(out, ro.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lse, rl.detach(), rtol=1e-12, atol=1e-12)
    ro.backward(dout.double())
    got = ao.short_bwd(qkv, out, dout, lse, H, keep, p)
    torch.testing.assert_close(got, x.grad, rtol=1e-10, atol=1e-10)


def test_short_rkeep_is_the_launchers():
    assert ao.short_rkeep(0.0) == 1.0
    assert ao.short_rkeep(0.5) == 2.0
    assert ao.short_p_eff(0.1) == 6554 / 65536 and ao.short_rkeep(0.1) == 65536.0 / (65536 - 6554)


def test_rowerr_sees_one_bad_row_that_the_tensor_norm_hides():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(8, 512, 128, generator=g, dtype=torch.float64)
    ref[0, 0] = 0  # an exactly-zero reference row: the floor keeps the metric finite
    a = ref.clone()
    assert ao.rowerr(a, ref) == 0.0
    a[2, 255] *= 0.5
    assert ao.relerr(a, ref) < 1e-2 < 0.4 < ao.rowerr(a, ref) < 0.5
    a = ref.clone()
    a[0, 0] += 1e-3
    assert 0 < ao.rowerr(a, ref) < 0.1


# ------------------------------------------------------------------ builder preconditions
def _growth(kind):
    q, k, _, _ = ao.flash_inputs(kind, 1, 4, 2, 512, seed=0)
    return ao.flash_growth(q, k)


def test_growth_counts_every_row_and_tile_once():
    # rows 64 t .. S - 1 see tile t: sum over t = 1..7 of (512 - 64 t), times 4 heads
    assert _growth("flat").numel() == 4 * sum(512 - 64 * t for t in range(1, 8))


def test_rescale_inputs_grow_past_the_threshold():
    gr = _growth("rescale")
    assert (gr > ao.RESCALE).double().mean().item() >= 0.90


def test_deferred_inputs_grow_below_the_threshold():
    gr = _growth("deferred")
    assert ((gr > 0) & (gr <= ao.RESCALE)).double().mean().item() >= 0.90
    assert (gr > ao.RESCALE).double().mean().item() <= 0.01


def test_flat_inputs_never_reach_the_threshold():
    assert not bool((_growth("flat") > ao.RESCALE).any())


def test_descend_inputs_never_grow():
    assert not bool((_growth("descend") > 0).any())


@pytest.mark.parametrize("S", [32, 128])
def test_short_inputs_peaked_and_flat(S):
    qkv, _ = ao.short_inputs(3.0, 2, S, 4, seed=0)
    assert ao.short_row_max_prob(qkv, 4).median().item() >= 0.5
    qkv, _ = ao.short_inputs(0.8, 2, S, 4, seed=0)
    assert ao.short_row_max_prob(qkv, 4).median().item() <= 0.15


# ------------------------------------------------------------------ the new inputs have power
def _online_softmax(q, k, v, rescale_l):
    """Tile-by-tile online softmax with fa_fwd_kernel's deferred-max rule, in fp64: 64-key tiles,
    32-query waves, and l / o rescaled only when some row of the wave sees its tile max exceed the
    reference by more than 8 exp2 units.  rescale_l=False is the planted defect: o is rescaled,
    l is not."""
    B, H, S, D = q.shape
    G = H // k.shape[1]
    sc = ao.flash_scores(q, k) * ao.LOG2E  # exp2 units, future keys -inf
    vv = v.double().repeat_interleave(G, 1)
    out = torch.empty(B, H, S, D, dtype=torch.float64)
    lse = torch.empty(B, H, S, dtype=torch.float64)
    fired = 0
    for q0 in range(0, S, 32):
        rows = slice(q0, q0 + 32)
        m2 = torch.full((B, H, 32), float("-inf"), dtype=torch.float64)
        l = torch.zeros(B, H, 32, dtype=torch.float64)
        o = torch.zeros(B, H, 32, D, dtype=torch.float64)
        for kb in range(0, q0 + 32, ao.FLASH_TILE):
            st = sc[:, :, rows, kb:kb + ao.FLASH_TILE]
            mb = st.amax(-1)
            fire = ~(mb - m2 <= ao.RESCALE).all(-1)  # wave-wide, per (batch, head)
            mn = torch.where(fire[..., None], torch.maximum(m2, mb), m2)
            alpha = torch.exp2(m2 - mn)  # 1 where the wave did not fire
            fired += int((fire[..., None] & (alpha > 0) & (alpha < 1)).sum())
            if rescale_l:
                l = l * alpha
            o = o * alpha[..., None]
            m2 = mn
            p = torch.exp2(st - m2[..., None])
            l = l + p.sum(-1)
            o = o + p @ vv[:, :, kb:kb + ao.FLASH_TILE]
        out[:, :, rows] = o / l[..., None]
        lse[:, :, rows] = m2 / ao.LOG2E + torch.log(l)
    return out.transpose(1, 2).reshape(B, S, H * D), lse, fired


def _heads(out):
    return out.view(*out.shape[:2], -1, ao.FLASH_D)


@pytest.mark.parametrize("kind", list(ao.FLASH_KINDS))
def test_online_softmax_emulation_is_the_oracle(kind):
    """Without the defect the emulation equals the oracle on every input kind, so what the next
    two tests see is the defect and nothing else."""
    q, k, v, _ = ao.flash_inputs(kind, 1, 4, 2, 512, seed=0)
    ref, rl = ao.flash_fwd(q, k, v)
    out, lse, _ = _online_softmax(q, k, v, rescale_l=True)
    assert ao.rowerr(_heads(out), _heads(ref)) < 1e-12
    torch.testing.assert_close(lse, rl, rtol=1e-12, atol=1e-12)


def test_flat_inputs_cannot_see_an_unrescaled_l():
    q, k, v, _ = ao.flash_inputs("flat", 1, 4, 2, 512, seed=0)
    ref, _ = ao.flash_fwd(q, k, v)
    out, _, fired = _online_softmax(q, k, v, rescale_l=False)
    assert fired == 0  # the only rescale is the first one, alpha = exp2(-inf) = 0
    assert ao.relerr(out, ref) < 1e-12
    assert ao.rowerr(_heads(out), _heads(ref)) < 1e-12


@pytest.mark.parametrize("kind", ["rescale", "deferred"])
def test_ramped_inputs_see_an_unrescaled_l(kind):
    q, k, v, _ = ao.flash_inputs(kind, 1, 4, 2, 512, seed=0)
    ref, _ = ao.flash_fwd(q, k, v)
    yard, _ = ao.flash_fwd(q, k, v, rounded=True)
    out, _, fired = _online_softmax(q, k, v, rescale_l=False)
    assert fired > 0
    assert ao.rowerr(_heads(out), _heads(ref)) > 3 * ao.rowerr(_heads(yard), _heads(ref))
