"""Causal GQA flash attention (csrc/kernels/flash_attn.hip) per row, on flat, ramped and descending
scores (tests/attn_oracle.py): every 128-wide row of out, dq, dk and dv against the fp64 oracle,
bounded by three times the row error of the bf16 rounding yardstick on the same inputs; lse with
the suite's bound; and bitwise invariance of a causal prefix (suffix for dk / dv) under changes to
the positions it must not see.  The backward is fed the oracle's out and lse, so a forward error
can neither mask nor cause a backward failure.

Observed on MI355X, rowerr(kernel) / rowerr(yardstick), min - max over the four shapes (the bound
is 3); in brackets the yardstick's own rowerr, the quantity the bound is a multiple of:

    kind      out                            dq                     dk                     dv
    flat      0.84 - 1.09 (0.0036 - 0.0040)  1.00 (0.0036 - 0.0039)  1.00 (0.0041 - 0.0056)  1.00 (0.0028 - 0.0033)
    deferred  0.96 - 1.05 (0.0036 - 0.0039)  1.00 (0.0039 - 0.0067)  1.00 (0.0044 - 0.0060)  1.00 (0.0030 - 0.0035)
    rescale   0.64 - 0.71 (0.0038 - 0.0041)  1.00 (0.0054 - 0.0248)  1.00 (0.0044 - 0.0057)  1.00 (0.0030 - 0.0037)
    descend   0.68 - 0.72 (0.0038 - 0.0042)  1.00 (0.0059 - 0.0290)  1.00 (0.0037 - 0.0068)  1.00 (0.0027 - 0.0036)

The gradients agree with the yardstick to the printed digits because the kernels round where it
does and accumulate in fp32 in between.  out differs because the kernel rounds P before the
division by l, the yardstick after it.  The yardstick's dq rises to 0.025 - 0.029 on the 12-unit
ramps at S = 512: that is the conditioning of dP - D there, the same for kernel and yardstick.
"""
import functools

import pytest
import torch

from ps_amd.ops import native

from . import attn_oracle as ao

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [
    (1, 4, 2, 512),  # 8-wave path, G = 2, plain block order
    (1, 2, 1, 384),  # 4-wave path, three query blocks
    (1, 8, 8, 256),  # 8 units: XCD-aware order, G = 1
    (3, 8, 8, 128),  # 24 units: three rounds of the XCD order, a single block per unit
]
KINDS = list(ao.FLASH_KINDS)
FACTOR = 3.0


def _heads(out):
    return out.view(*out.shape[:2], -1, ao.FLASH_D)


@functools.lru_cache(maxsize=None)
def _case(kind, shape):
    """Inputs, fp64 oracle and yardstick of one case, computed once and left unchanged."""
    q, k, v, dout = ao.flash_inputs(kind, *shape, seed=0)
    out, lse = ao.flash_fwd(q, k, v)
    yout, _ = ao.flash_fwd(q, k, v, rounded=True)
    out_in, lse_in = out.to(torch.bfloat16), lse.float()  # what fa_bwd is given
    grads = ao.flash_bwd(q, k, v, out_in, dout, lse_in)
    ygrads = ao.flash_bwd(q, k, v, out_in, dout, lse_in, rounded=True)
    return dict(q=q, k=k, v=v, dout=dout, out=out, lse=lse, yout=yout, out_in=out_in, lse_in=lse_in, grads=grads,
                ygrads=ygrads)


def _bound(name, kind, shape, got, ref, yard):
    e, y = ao.rowerr(got, ref), ao.rowerr(yard, ref)
    print(f"RATIO flash {kind} {shape} {name}: kernel {e:.5f} yardstick {y:.5f} ratio {e / y:.2f}")
    assert y > 0
    assert e <= FACTOR * y, (name, e, y)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flash_forward_rows(shape, kind):
    c = _case(kind, shape)
    out, lse = native().fa_fwd(*(c[n].to(DEV) for n in "qkv"))
    _bound("out", kind, shape, _heads(out), _heads(c["out"]), _heads(c["yout"]))
    torch.testing.assert_close(lse.cpu(), c["lse"].float(), rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flash_backward_rows(shape, kind):
    c = _case(kind, shape)
    got = native().fa_bwd(*(c[n].to(DEV) for n in ("q", "k", "v", "out_in", "dout", "lse_in")))
    for name, g, ref, yard in zip(("dq", "dk", "dv"), got, c["grads"], c["ygrads"]):
        assert g.shape == ref.shape
        _bound(name, kind, shape, g, ref, yard)
    if kind == "descend":
        # keys two or more tiles down the ramp get (numerically) no gradient: 2^-24 and less of
        # the first tile's.  The kernel must return them below the metric's floor term too.
        for name, g, ref in zip(("dk", "dv"), got[1:], c["grads"][1:]):
            n = ref.norm(dim=-1)
            rms = n.pow(2).mean().sqrt()
            zero = n <= 1e-6 * rms
            assert int(zero.sum()) >= (shape[3] - 128) * shape[0] * shape[2] // 2, name  # the case has such rows
            assert g.double().cpu().norm(dim=-1)[zero].max().item() < 0.05 * rms.item(), name


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _run(q, k, v, dout):
    out, lse = native().fa_fwd(q, k, v)
    return (out, lse) + tuple(native().fa_bwd(q, k, v, out, dout, lse))


@pytest.mark.parametrize("t", [32, 96, 160])
def test_flash_prefix_is_bitwise_blind_to_later_keys(t):
    """Rows < t of out, lse and dq do not change by one bit when k and v change at positions >= t."""
    q, k, v, dout = (x.to(DEV) for x in ao.flash_inputs("rescale", 1, 2, 1, 256, seed=1))
    g = torch.Generator().manual_seed(t)
    k2, v2 = k.clone(), v.clone()
    for x in (k2, v2):
        x[:, :, t:] = (8 * torch.randn(x[:, :, t:].shape, generator=g)).bfloat16().to(DEV)
    out, lse, dq, _, _ = _run(q, k, v, dout)
    out2, lse2, dq2, _, _ = _run(q, k2, v2, dout)
    assert not torch.equal(out[:, t:], out2[:, t:])  # the change is seen where it may be
    assert torch.equal(_bits(out[:, :t]), _bits(out2[:, :t]))
    assert torch.equal(_bits(lse[:, :, :t]), _bits(lse2[:, :, :t]))
    assert torch.equal(_bits(dq[:, :, :t]), _bits(dq2[:, :, :t]))


@pytest.mark.parametrize("t", [32, 96, 160])
def test_flash_suffix_grads_are_bitwise_blind_to_earlier_queries(t):
    """Rows >= t of dk and dv do not change by one bit when q, dout, out and lse change at
    positions < t."""
    q, k, v, dout = (x.to(DEV) for x in ao.flash_inputs("rescale", 1, 2, 1, 256, seed=2))
    out, lse = native().fa_fwd(q, k, v)
    g = torch.Generator().manual_seed(t)
    q2, dout2, out2, lse2 = q.clone(), dout.clone(), out.clone(), lse.clone()
    q2[:, :, :t] = (8 * torch.randn(q[:, :, :t].shape, generator=g)).bfloat16().to(DEV)
    dout2[:, :t] = (8 * torch.randn(dout[:, :t].shape, generator=g)).bfloat16().to(DEV)
    out2[:, :t] = (8 * torch.randn(out[:, :t].shape, generator=g)).bfloat16().to(DEV)
    lse2[:, :, :t] += 1.0
    _, dk, dv = native().fa_bwd(q, k, v, out, dout, lse)
    _, dk2, dv2 = native().fa_bwd(q2, k, v, out2, dout2, lse2)
    assert not torch.equal(dk[:, :, :t], dk2[:, :, :t])
    assert torch.equal(_bits(dk[:, :, t:]), _bits(dk2[:, :, t:]))
    assert torch.equal(_bits(dv[:, :, t:]), _bits(dv2[:, :, t:]))
