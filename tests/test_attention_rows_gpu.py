"""Fused short-sequence attention (csrc/kernels/attention.hip) per row, on nearly flat (0.8 randn)
and peaked (3.0 randn) scores, with and without dropout and with seeds that use the high 32 bits:
every 64-wide row of out and of the q, k and v thirds of dqkv against the fp64 oracle of
tests/attn_oracle.py, bounded by three times the row error of the bf16 rounding yardstick on the
same inputs and keep mask.  The backward is fed the oracle's out and lse.  Then the dropout mask
itself: keep rates overall, per row and per column, independence of the two 16-bit halves of one
hash, reproducibility, and the fold of the seed's high half.

Observed on MI355X, rowerr(kernel) / rowerr(yardstick), min - max over the four shapes and both
seed kinds (the bound is 3); in brackets the yardstick's own rowerr:

    scale  p    out                     dq                             dk                      dv
    0.8    0.0  1.00 (0.0026 - 0.0034)  1.00 (0.0030 - 0.0036)         1.00 (0.0032 - 0.0035)  1.00 (0.0028 - 0.0033)
    0.8    0.1  1.00 (0.0027 - 0.0036)  1.00 (0.0027 - 0.0036)         1.00 (0.0028 - 0.0036)  1.00 (0.0030 - 0.0034)
    0.8    0.5  1.00 (0.0031 - 0.0033)  1.00 (0.0030 - 0.0042)         1.00 (0.0032 - 0.0037)  1.00 (0.0031 - 0.0033)
    3.0    0.0  1.00 (0.0030 - 0.0042)  1.00 (0.0030 - 0.0041)         1.00 (0.0033 - 0.0042)  1.00 (0.0027 - 0.0040)
    3.0    0.1  1.00 (0.0037 - 0.0043)  1.00 - 1.07 (0.0031 - 0.0043)  1.00 (0.0030 - 0.0041)  1.00 (0.0032 - 0.0043)
    3.0    0.5  1.00 (0.0027 - 0.0039)  1.00 (0.0033 - 0.0041)         1.00 (0.0037 - 0.0041)  1.00 (0.0032 - 0.0042)

The kernel rounds where the yardstick does (P after the normalisation and the dropout, dS, the
outputs) and accumulates in fp32 in between, so the two agree to the printed digits.
"""
import functools
import math

import pytest
import torch

from ps_amd.ops import native

from . import attn_oracle as ao

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 32, 1), (2, 64, 3), (3, 96, 5), (2, 128, 2)]
FACTOR = 3.0
HIGH = 7 << 40

CASES = [(shape, scale, p) for shape in SHAPES for scale in (0.8, 3.0) for p in (0.0, 0.1, 0.5)]


def _seed(i):
    return 12345 + (HIGH if i % 2 else 0)  # every other case: a seed above 2^32


def _id(case):
    i, ((B, S, H), scale, p) = case
    return f"{B}x{S}x{H}-s{scale}-p{p}-{'hi' if _seed(i) >> 32 else 'lo'}"


def _thirds(dqkv, heads):
    b, s, _ = dqkv.shape
    return dqkv.view(b, s, 3, heads, ao.SHORT_D).unbind(2)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs, keep mask, fp64 oracle and yardstick of one case, computed once and left unchanged."""
    (B, S, H), scale, p = CASES[i]
    seed = _seed(i)
    qkv, dout = ao.short_inputs(scale, B, S, H, seed=i)
    keep = native().attn_dropout_mask(qkv.to(DEV), B * H, S, p, seed).cpu() if p > 0 else None
    out, lse = ao.short_fwd(qkv, H, keep, p)
    yout, _ = ao.short_fwd(qkv, H, keep, p, rounded=True)
    out_in, lse_in = out.to(torch.bfloat16), lse.float()  # what attn_bwd is given
    grad = ao.short_bwd(qkv, out_in, dout, lse_in, H, keep, p)
    ygrad = ao.short_bwd(qkv, out_in, dout, lse_in, H, keep, p, rounded=True)
    return dict(qkv=qkv, dout=dout, H=H, p=p, seed=seed, out=out, lse=lse, yout=yout, out_in=out_in, lse_in=lse_in,
                grad=grad, ygrad=ygrad)


def _bound(name, tag, got, ref, yard):
    e, y = ao.rowerr(got, ref), ao.rowerr(yard, ref)
    print(f"RATIO short {tag} {name}: kernel {e:.5f} yardstick {y:.5f} ratio {e / y:.2f}")
    assert y > 0
    assert e <= FACTOR * y, (name, e, y)


@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=_id)
def test_attention_forward_rows(case):
    c = _case(case[0])
    H = c["H"]
    out, lse = native().attn_fwd(c["qkv"].to(DEV), H, c["p"], c["seed"])
    rows = lambda x: x.view(*x.shape[:2], H, ao.SHORT_D)  # noqa: E731
    _bound("out", _id(case), rows(out), rows(c["out"]), rows(c["yout"]))
    torch.testing.assert_close(lse.cpu(), c["lse"].float(), rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=_id)
def test_attention_backward_rows(case):
    c = _case(case[0])
    H = c["H"]
    dqkv = native().attn_bwd(c["qkv"].to(DEV), c["out_in"].to(DEV), c["dout"].to(DEV), c["lse_in"].to(DEV), H, c["p"],
                             c["seed"])
    assert dqkv.shape == c["grad"].shape
    for name, g, ref, yard in zip(("dq", "dk", "dv"), _thirds(dqkv, H), _thirds(c["grad"], H), _thirds(c["ygrad"], H)):
        _bound(name, _id(case), g, ref, yard)


# ------------------------------------------------------------------ the dropout mask itself
BH, MS = 8, 128
MASK_SEEDS = [2024, 99 + (5 << 40)]


def _mask(p, seed):
    like = torch.empty(1, device=DEV, dtype=torch.bfloat16)
    return native().attn_dropout_mask(like, BH, MS, p, seed).cpu()


def _within(rate, expect, n, what):
    sigma = math.sqrt(expect * (1 - expect) / n)
    worst = (rate - expect).abs().max().item()
    assert worst <= 6 * sigma, (what, worst, 6 * sigma)


@pytest.mark.parametrize("seed", MASK_SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_rates(p, seed):
    m = _mask(p, seed)
    assert m.shape == (BH, MS, MS) and m.dtype == torch.uint8 and bool((m <= 1).all())
    keep = m.double()
    pe = ao.short_p_eff(p)
    _within(keep.mean(), 1 - pe, keep.numel(), "mean")
    _within(keep.mean(-1), 1 - pe, MS, "rows")  # every (head, query)
    _within(keep.mean(-2), 1 - pe, MS, "columns")  # every (head, key)
    _within(keep.mean((0, 1)), 1 - pe, BH * MS, "key positions")
    _within(keep.mean((0, 2)), 1 - pe, BH * MS, "query positions")
    # the two 16-bit halves of one hash (keys 2j, 2j + 1) are independent draws
    both = ((m[..., 0::2] == 0) & (m[..., 1::2] == 0)).double()
    _within(both.mean(), pe * pe, both.numel(), "pairs")


@pytest.mark.parametrize("seed", MASK_SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_reproduces_and_folds_the_high_seed_half(p, seed):
    m = _mask(p, seed)
    assert torch.equal(m, _mask(p, seed))
    other = _mask(p, seed + 2 ** 32)
    # independent masks differ in 2 p (1 - p) of the elements; half of that is far outside chance
    assert (m != other).double().mean().item() >= p * (1 - p)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_forward_depends_on_the_high_seed_half(p):
    qkv, _ = ao.short_inputs(0.8, 2, 128, 2, seed=5)
    qkv = qkv.to(DEV)
    seed = MASK_SEEDS[0]
    out, lse = native().attn_fwd(qkv, 2, p, seed)
    again, _ = native().attn_fwd(qkv, 2, p, seed)
    other, lse2 = native().attn_fwd(qkv, 2, p, seed + 2 ** 32)
    assert torch.equal(out, again)
    assert torch.equal(lse, lse2)  # the softmax statistics do not see the mask
    changed = (out != other).any(-1).double().mean().item()
    assert changed > 0.99  # every row draws its own mask
