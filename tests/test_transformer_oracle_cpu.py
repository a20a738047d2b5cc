"""The transformer oracles of tests/transformer_oracle.py, checked without a GPU: the Philox keep
mask against the published Philox4x32-10 known answers, the unrounded oracles against fp64
autograd, and, on every input test_transformer_rows_gpu.py uses, the project's own fp32 CPU
compositions (ops/transformer.py: _rms_ref, F.layer_norm, F.silu(g) * u, _rope_ref; bf16 rounding
at the outputs) against the two bounds the GPU tests put on the kernels, so that the oracle, the
yardstick and the bounds are known to hold for a correct fp32 implementation."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ps_amd.ops import transformer as T

from . import transformer_oracle as to

FACTOR = 3.0


# ------------------------------------------------------------------ Philox
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(w[0]) for w in to.philox4x32(*ctr, *key))
    assert got == want, [hex(g) for g in got]


def test_philox_keep_indexes_counter_and_word():
    """Element i is word i % 4 of counter i // 4 under key (seed low, seed high); u01 = (w >> 8) 2^-24."""
    seed, p = 12345 + (7 << 40), 0.1
    keep = to.philox_keep(seed, 23, p)
    assert keep.shape == (23,) and keep.dtype == torch.bool
    for i in (0, 3, 4, 9, 22):
        w = to.philox4x32(i // 4, 0, 0, 0, seed & 0xFFFFFFFF, seed >> 32)[i % 4][0]
        assert bool(keep[i]) == bool(np.float32(int(w) >> 8) * np.float32(2.0 ** -24) >= np.float32(p))
    # a counter above 2^32 carries into the second counter word
    big = to.philox4x32(5, 1, 0, 0, 1, 2)
    assert [int(x[0]) for x in big] != [int(x[0]) for x in to.philox4x32(5, 0, 0, 0, 1, 2)]
    n = 1 << 16
    for pp in (0.1, 0.5):
        rate = to.philox_keep(seed, n, pp).double().mean().item()
        assert abs(rate - (1 - pp)) < 6 * (pp * (1 - pp) / n) ** 0.5
    assert (to.philox_keep(seed, n, 0.5) != to.philox_keep(seed & 0xFFFFFFFF, n, 0.5)).double().mean() > 0.25


# ------------------------------------------------------------------ oracle == fp64 autograd
def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("residual", [False, True])
def test_rms_oracle_is_autograd(residual):
    c = to.norm_inputs(9, 72, 1)
    x, r, w = (c[k].double().requires_grad_() for k in ("x", "r", "w"))
    s = x + r if residual else x
    rstd = torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + 1e-5)
    y = s * rstd * w
    os_, oy, orstd = to.rms_fwd(c["x"], c["r"] if residual else None, c["w"], 1e-5)
    _close(os_, s.detach())
    _close(oy, y.detach())
    _close(orstd, rstd.detach()[:, 0])
    ds = c["ds"] if residual else None
    torch.autograd.backward([y] + ([s] if residual else []), [c["dy"].double()] + ([ds.double()] if residual else []))
    dx, dw, mag, magw = to.rms_bwd(c["dy"], os_, c["w"], orstd, ds)
    _close(dx, x.grad)
    _close(dw, w.grad)
    assert bool((mag >= dx.abs() - 1e-12).all()) and bool((magw >= dw.abs() - 1e-12).all())


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_ln_oracle_is_autograd(p):
    c = to.norm_inputs(9, 72, 2, shift=3.0)
    keep = to.philox_keep(77, 9 * 72, p).view(9, 72) if p > 0 else None
    x, o, g, b = (c[k].double().requires_grad_() for k in ("x", "r", "w", "b"))
    s = x + (o * keep.double() / (1 - p) if p > 0 else o)
    y = F.layer_norm(s, (72,), g, b, 1e-12)
    os_ = to.ln_fwd(c["x"], c["r"], keep, p)
    oy, mean, rstd, magy = to.ln_from_s(os_, c["w"], c["b"], 1e-12)
    _close(os_, s.detach())
    _close(oy, y.detach())
    _close(mean, s.detach().mean(-1))
    y.backward(c["dy"].double())
    dx, do, dg, db, mags = to.ln_bwd(c["dy"], os_, c["w"], mean, rstd, keep, p)
    for got, ref in ((dx, x.grad), (do, o.grad), (dg, g.grad), (db, b.grad)):
        _close(got, ref)
    assert bool((magy >= oy.abs() - 1e-12).all()) and bool((mags["dx"] >= dx.abs() - 1e-9).all())


def test_swiglu_oracle_is_autograd():
    gu, dh = to.swiglu_inputs(5, 24, 3)
    x = gu.double().requires_grad_()
    g, u = x.chunk(2, dim=-1)
    h = F.silu(g) * u
    oh, _ = to.swiglu_fwd(gu)
    _close(oh, h.detach())
    h.backward(dh.double())
    dgu, mag = to.swiglu_bwd(dh, gu)
    _close(dgu, x.grad)
    assert bool((mag[:, :24] >= dgu[:, :24].abs() * (1 - 1e-12)).all())  # the dg half: a sum of two terms


def test_rope_oracle_is_autograd_and_rope_ref():
    B, S, H, KV, hd = 2, 7, 4, 2, 32
    qkv, gq, gk, gv, cs = to.rope_inputs(B, S, H, KV, hd, 4)
    x = qkv.double().requires_grad_()
    xt = x.transpose(1, 2)
    q, k, v = T._rope_ref(xt[:, :H], cs.double()), T._rope_ref(xt[:, H:H + KV], cs.double()), xt[:, H + KV:]
    oq, ok, ov, mq, _ = to.rope_fwd(qkv, cs, H, KV)
    for got, ref in ((oq, q), (ok, k), (ov, v)):
        _close(got, ref.detach())
    torch.autograd.backward([q, k, v], [gq.double(), gk.double(), gv.double()])
    dqkv, mag = to.rope_bwd(gq, gk, gv, cs)
    _close(dqkv, x.grad)
    assert mag.shape == dqkv.shape and bool((mq >= oq.abs() - 1e-12).all())


def test_rope_table64_is_rope_table():
    cs64, f = to.rope_table64(33, 32, 10.0)
    torch.testing.assert_close(T.rope_table(33, 32, 10.0, "cpu").double(), cs64, rtol=0, atol=2.0 ** -21 * 33)
    assert f.shape == (33, 16)


# ------------------------------------------------------------------ the metrics have power
def test_elemerr_sees_one_vector_and_allows_two_ulps():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(64, 4096, generator=g, dtype=torch.float64)
    assert to.elemerr(ref, ref) == (0, 0.0)
    a = ref.clone()
    a[17, 2048:2056] *= 1.05  # one 8-element vector of one row, 5 % off
    bad, worst = to.elemerr(a, ref)
    assert bad == 8 and worst > 3
    a = ref * (1 + 2.0 ** -7)
    assert to.elemerr(a, ref)[0] == 0
    # cancellation: a zero reference with a magnitude passes up to 2^-14 of it
    z = torch.zeros(4, dtype=torch.float64)
    assert to.elemerr(z + 2.0 ** -15, z, torch.ones(4))[0] == 0
    assert to.elemerr(z + 2.0 ** -13, z, torch.ones(4))[0] == 4
    assert to.elemerr(z + float("nan"), z, torch.ones(4))[0] == 4


# ------------------------------------------------------------------ the fp32 compositions stay inside the bounds
def _two_bounds(name, got, exact, yard, mag=None):
    e, y = to.rowerr(got, exact), to.rowerr(yard, exact)
    bad, worst = to.elemerr(got, yard, mag)
    print(f"CPU {name}: rowerr {e:.5f} yardstick {y:.5f} ratio {e / y if y else 0:.2f} elemerr bad {bad} worst {worst:.2f}")
    assert e <= FACTOR * y, (name, e, y)
    assert bad == 0, (name, bad, worst)


def _b(t):
    return t.detach().to(torch.bfloat16)


@pytest.mark.parametrize("R,D", to.NORM_SHAPES + to.RMS_ONLY_SHAPES)
@pytest.mark.parametrize("residual", [False, True])
def test_rms_fp32_composition_within_bounds(R, D, residual):
    c = to.norm_inputs(R, D, 1000 + R + D)
    r = c["r"] if residual else None
    s_e, y_e, _ = to.rms_fwd(c["x"], r, c["w"], to.RMS_EPS)
    s_y, y_y, rstd_y = to.rms_fwd(c["x"], r, c["w"], to.RMS_EPS, rounded=True)
    sf = (c["x"].float() + c["r"].float()).to(torch.bfloat16).float() if residual else c["x"].float()
    sf.requires_grad_()
    w = c["w"].clone().requires_grad_()
    y = T._rms_ref(sf, w, to.RMS_EPS)
    _two_bounds("rms y", _b(y), y_e, y_y)
    if residual:
        assert torch.equal(_b(sf).double(), s_y)
    ds = c["ds"] if residual else None
    s_in, rstd_in = s_y.to(torch.bfloat16), rstd_y.float()
    dx_e, _, _, _ = to.rms_bwd(c["dy"], s_in, c["w"], rstd_in, ds)
    dx_y, dw_y, mag, magw = to.rms_bwd(c["dy"], s_in, c["w"], rstd_in, ds, rounded=True)
    # autograd through _rms_ref differentiates the unrounded xhat; the kernel (and the oracle) reuse
    # the forward's bf16 xhat, which moves dx by up to 2^-9 |rstd xhat c| where g and xhat c cancel.
    # So the backward is modelled here in fp32 with the kernel's rounding points.
    rs, d = rstd_in[:, None], c["dy"].float()
    xh = (s_in.float() * rs).to(torch.bfloat16).float()
    g = d * c["w"]
    dx = rs * (g - xh * (g * xh).mean(-1, keepdim=True))
    if residual:
        dx = dx + ds.float()
    _two_bounds("rms dx", _b(dx), dx_e, dx_y, mag)
    dw = (d * xh).sum(0)
    assert bool(((dw.double() - dw_y).abs() <= to.U24 * (R + 3) * magw).all())  # any summation order


@pytest.mark.parametrize("R,D", to.NORM_SHAPES)
def test_ln_fp32_composition_within_bounds(R, D):
    c = to.norm_inputs(R, D, 2000 + R + D, shift=3.0)
    ps = [0.0] + ([0.1, 0.5] if (R, D) in to.DROP_SHAPES else [])
    for p in ps:
        keep = to.philox_keep(to.SEEDS[1], R * D, p).view(R, D) if p > 0 else None
        s_e = to.ln_fwd(c["x"], c["r"], keep, p)
        s_y = to.ln_fwd(c["x"], c["r"], keep, p, rounded=True)
        y_e, _, _, _ = to.ln_from_s(s_e, c["w"], c["b"], to.LN_EPS)
        y_y, mean_y, rstd_y, magy = to.ln_from_s(s_y, c["w"], c["b"], to.LN_EPS, rounded=True)
        sf = s_y.float().requires_grad_()
        y = F.layer_norm(sf, (D,), c["w"], c["b"], to.LN_EPS)
        _two_bounds(f"ln y p={p}", _b(y), y_e, y_y, magy)
        s_in = s_y.to(torch.bfloat16)
        dx_e, do_e, _, _, _ = to.ln_bwd(c["dy"], s_in, c["w"], mean_y.float(), rstd_y.float(), keep, p)
        dx_y, do_y, _, _, mags = to.ln_bwd(c["dy"], s_in, c["w"], mean_y.float(), rstd_y.float(), keep, p, rounded=True)
        y.backward(c["dy"].float())
        _two_bounds(f"ln dx p={p}", _b(sf.grad), dx_e, dx_y, mags["dx"])
        if p > 0:
            do = sf.grad * (keep.float() * torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))
            _two_bounds(f"ln do p={p}", _b(do), do_e, do_y, mags["do"])


@pytest.mark.parametrize("R,Fd", to.SWIGLU_SHAPES)
def test_swiglu_fp32_composition_within_bounds(R, Fd):
    gu, dh = to.swiglu_inputs(R, Fd, 3000 + R)
    h_e, _ = to.swiglu_fwd(gu)
    h_y, magh = to.swiglu_fwd(gu, rounded=True)
    x = gu.float().requires_grad_()
    g, u = x.chunk(2, dim=-1)
    h = F.silu(g) * u
    assert torch.isfinite(h).all()
    _two_bounds("swiglu h", _b(h), h_e, h_y, magh)
    d_e, _ = to.swiglu_bwd(dh, gu)
    d_y, magd = to.swiglu_bwd(dh, gu, rounded=True)
    h.backward(dh.float())
    assert torch.isfinite(x.grad).all()
    _two_bounds("swiglu dgu", _b(x.grad), d_e, d_y, magd)


@functools.lru_cache(maxsize=None)
def _rope_case(i):
    shape = (to.ROPE_SHAPES + [to.ROPE_TABLE_SHAPE])[i]
    return shape, to.rope_inputs(*shape, 4000 + i)


@pytest.mark.parametrize("i", range(len(to.ROPE_SHAPES) + 1))
def test_rope_fp32_composition_within_bounds(i):
    (B, S, H, KV, hd), (qkv, gq, gk, gv, cs) = _rope_case(i)
    if i == len(to.ROPE_SHAPES):
        cs = T.rope_table(S, hd, to.ROPE_TABLE_THETA, "cpu")
    x = qkv.float().requires_grad_()
    xt = x.transpose(1, 2)
    q, k, v = T._rope_ref(xt[:, :H], cs), T._rope_ref(xt[:, H:H + KV], cs), xt[:, H + KV:]
    q_e, k_e, v_e, _, _ = to.rope_fwd(qkv, cs, H, KV)
    q_y, k_y, _, mq, mk = to.rope_fwd(qkv, cs, H, KV, rounded=True)
    _two_bounds("rope q", _b(q), q_e, q_y, mq)
    _two_bounds("rope k", _b(k), k_e, k_y, mk)
    assert torch.equal(_b(v).double(), v_e)
    torch.autograd.backward([q, k, v], [gq.float(), gk.float(), gv.float()])
    d_e, _ = to.rope_bwd(gq, gk, gv, cs)
    d_y, mag = to.rope_bwd(gq, gk, gv, cs, rounded=True)
    _two_bounds("rope dqkv", _b(x.grad)[:, :, :H + KV], d_e[:, :, :H + KV], d_y[:, :, :H + KV], mag[:, :, :H + KV])
    assert torch.equal(_b(x.grad)[:, :, H + KV:].double(), d_e[:, :, H + KV:])
