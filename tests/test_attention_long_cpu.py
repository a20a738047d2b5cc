"""The inputs of test_attention_long_gpu.py, validated without a GPU (tests/attn_long_oracle.py): these
are conditions on the inputs, so that a pass of the GPU tests means what it says.

1. long_inputs does to the running max of a 128-key-chunked softmax what its kind says: over every shape of
   the GPU tests with more than one chunk, the per-row growth of the chunk max (chunk_growth, exp2 units)
   reaches g / 2 for the ascending kinds (flat 0, deferred 3, rescale 12), its median is at least g / 2
   where g > 0, and no row grows at all for descend (the first chunk sets the max).
2. every row error of the bf16 yardstick against the fp64 oracle is > 0 (the GPU bound is a multiple of it),
   for out, dq, dk and dv, on every shape and input of the key-length and packed-only cases at p = 0.1.
3. under the mask model no row of a p = 0.1 case loses all of its valid keys, except where L = 1 (a row of
   zeros would make its rowerr a statement about nothing).
4. the mask model keeps about 1 - p of the elements and changes with either half of the 64-bit seed; the
   GPU test compares it bit for bit with attn_dropout_mask.
"""
import functools

import pytest
import torch

from . import attn_long_oracle as alo
from . import attn_oracle as ao

HIGH = 7 << 40
SEED = 12345 + HIGH
P = 0.1
BATCHES = [("klen", b) for b in alo.PADDED] + [("packed", b) for b in alo.PACKED_ONLY]


def _bid(lb):
    layout, ((B, S, H), lens) = lb
    return f"{layout}-{B}x{S}x{H}-" + "_".join(map(str, lens))


@functools.lru_cache(maxsize=None)
def _keep(layout, i):
    (B, S, H), lens = BATCHES[i][1]
    return alo.keep_model(B * H, alo.max_len(lens) if layout == "packed" else S, P, SEED)


# ------------------------------------------------------------------ 1. the ramp
@pytest.mark.parametrize("kind", alo.KINDS)
@pytest.mark.parametrize("batch", alo.PACKED, ids=lambda b: "x".join(map(str, b[0])))
def test_long_inputs_move_the_running_max_as_their_kind_says(batch, kind):
    (B, S, H), _ = batch
    g, rev = ao.FLASH_KINDS[kind]
    qkv, _ = alo.long_inputs(kind, B, S, H, seed=7)
    gr = alo.chunk_growth(qkv, H)
    assert gr.numel() == B * H * S * ((S - 1) // alo.CHUNK)
    if gr.numel() == 0:
        return  # one chunk: nothing to grow
    print(f"GROWTH {B}x{S}x{H} {kind}: min {gr.min():.2f} median {gr.median():.2f} max {gr.max():.2f}")
    if rev:
        assert gr.max().item() <= 0
    else:
        assert gr.max().item() >= g / 2
        if g > 0:
            assert gr.median().item() >= g / 2


# ------------------------------------------------------------------ 2. the yardstick
@pytest.mark.parametrize("inp", alo.INPUTS, ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("lb", list(enumerate(BATCHES)), ids=lambda x: _bid(x[1]))
def test_every_yardstick_row_error_is_positive(lb, inp):
    i, (layout, batch) = lb
    H = batch[0][2]
    qkv, dout = alo.inputs(layout, batch, inp, seed=100 + i)
    r = alo.reference(layout, batch, qkv, dout, _keep(layout, i), P)
    assert 0 < ao.rowerr(alo.rows(r["yout"], H), alo.rows(r["out"], H)) < 0.1
    for y, ref in zip(alo.thirds(r["ygrad"], H), alo.thirds(r["grad"], H)):
        assert 0 < ao.rowerr(y, ref) < 0.1
    assert bool(torch.isfinite(r["lse"]).all())


# ------------------------------------------------------------------ 3. no row without a kept key
@pytest.mark.parametrize("lb", list(enumerate(BATCHES)), ids=lambda x: _bid(x[1]))
def test_no_row_loses_all_its_valid_keys(lb):
    i, (layout, ((B, S, H), lens)) = lb
    keep = _keep(layout, i)
    for b, L in enumerate(lens):
        if L == 1:
            continue
        nq = L if layout == "packed" else S
        left = keep[b * H:(b + 1) * H, :nq, :L].sum(-1)
        assert int(left.min()) > 0, (b, L)


# ------------------------------------------------------------------ 4. the mask model
def test_mask_model_rate_and_seed_halves():
    a = alo.keep_model(4, 160, P, SEED)
    assert a.shape == (4, 160, 160) and a.dtype == torch.uint8
    assert abs(a.float().mean().item() - (1 - ao.short_p_eff(P))) < 5e-3  # 102400 draws: sigma 9.4e-4
    assert not torch.equal(a, alo.keep_model(4, 160, P, SEED + 1))
    assert not torch.equal(a, alo.keep_model(4, 160, P, SEED + (1 << 32)))
    assert bool(alo.keep_model(2, 32, 0.0, SEED).all())
