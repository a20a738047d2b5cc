"""Per-head QK RMSNorm fused into RoPE + split (csrc/kernels/rope_norm.hip) against the same composition in
fp64 on the bf16 inputs.  The bound is relative to the bf16 torch composition (``_rope_norm_ref``): the fused
kernels round once where it rounds several times, so their maximum error, per tensor and per head row relative
to the row's magnitude, stays within 2x its error."""
import functools

import pytest
import torch

from ps_amd.ops import transformer as T
from ps_amd.ops._ext import native

pytestmark = pytest.mark.gpu

EPS = 1e-6
SHAPES = [(1, 3, 2, 1), (2, 130, 4, 2), (1, 257, 8, 8)]  # odd S, several grid-stride steps, GQA and MHA


@functools.lru_cache(maxsize=None)
def _case(hd, shape, wdtype):
    """Inputs, output gradients and the fp64 result (q, k, v, dqkv, dwq, dwk); read-only."""
    B, S, H, KV = shape
    g = torch.Generator().manual_seed(hd + S)
    qkv = 2 * torch.randn(B, S, H + 2 * KV, hd, generator=g)
    qkv[0, 0, 0] *= 1e-3  # a query row and a key row on which rstd matters
    qkv[-1, -1, H] *= 30
    qkv = qkv.bfloat16().cuda()
    wq, wk = ((0.5 + torch.rand(hd, generator=g)).to(wdtype).cuda() for _ in range(2))
    grads = tuple(torch.randn(B, h, S, hd, generator=g).bfloat16().cuda() for h in (H, KV, KV))
    cs = T.rope_table(S, hd, 500000.0, "cuda")
    ref = _run(T._rope_norm_ref, qkv.double(), cs, H, KV, wq.double(), wk.double(), grads)
    return qkv, cs, wq, wk, grads, ref


def _run(fn, qkv, cs, H, KV, wq, wk, grads):
    qkv, wq, wk = (t.detach().clone().requires_grad_() for t in (qkv, wq, wk))
    out = fn(qkv, cs, H, KV, wq, wk, EPS)
    torch.autograd.backward(out, [g.to(qkv.dtype) for g in grads])
    return tuple(out) + (qkv.grad, wq.grad, wk.grad), out[0].grad_fn


@pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16], ids=["w32", "w16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("hd", [64, 128])
def test_fused_within_2x_of_composition(hd, shape, wdtype):
    qkv, cs, wq, wk, grads, (ref, _) = _case(hd, shape, wdtype)
    _, _, H, KV = shape
    fused, fn = _run(T.rope_split, qkv, cs, H, KV, wq, wk, grads)
    assert "RopeNormSplit" in fn.name()  # the HIP path, not the composition
    comp, _ = _run(T._rope_norm_ref, qkv, cs, H, KV, wq, wk, grads)
    assert torch.equal(fused[2], qkv[:, :, H + KV:].transpose(1, 2))  # v: the input's v heads, transposed
    assert torch.equal(fused[3][:, :, H + KV:], grads[2].transpose(1, 2))  # and dv back into dqkv
    for name, f, c, r in zip(("q", "k", "v", "dqkv", "dwq", "dwk"), fused, comp, ref):
        assert f.dtype == c.dtype and f.shape == c.shape
        # "abs": the tensor's maximum error.  "row": every head row over its own fp64 maximum first, so that the
        # 1e-3 row, whose gradient is 1000 times the others', does not set the scale for all of dqkv
        for what, scale in (("abs", 1.0), ("row", r.abs().amax(-1, keepdim=True).clamp_min(1e-30))):
            ef, ec = (((t.double() - r).abs() / scale).max().item() for t in (f, c))
            print(f"qk_norm hd={hd} shape={shape} w={wdtype} {name} {what}: fused {ef:.3e} composition {ec:.3e} "
                  f"ratio {ef / max(ec, 1e-300):.3f}")
            assert ef <= 2 * ec, (name, what)


@pytest.mark.parametrize("hd", [64, 128])
def test_unit_weights_and_unit_rstd_give_rope_split(hd):
    """Rows of +-1 with eps = 0 have rstd = 1 exactly: with weights of ones the kernel is rope_split bitwise."""
    B, S, H, KV = SHAPES[0]
    g = torch.Generator().manual_seed(hd)
    qkv = (torch.randint(0, 2, (B, S, H + 2 * KV, hd), generator=g) * 2 - 1).bfloat16().cuda()
    cs = T.rope_table(S, hd, 500000.0, "cuda")
    ones = torch.ones(hd, device="cuda")
    for a, b in zip(T.rope_split(qkv, cs, H, KV, ones, ones, 0.0), T.rope_split(qkv, cs, H, KV)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("hd", [64, 128])
def test_weight_gradients_are_deterministic(hd):
    shape = SHAPES[1]
    qkv, cs, wq, wk, grads, _ = _case(hd, shape, torch.float32)
    a = native().rope_norm_split_bwd(*grads, qkv, cs, wq, wk, EPS)
    b = native().rope_norm_split_bwd(*grads, qkv, cs, wq, wk, EPS)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_head_dim_32_takes_the_composition():
    B, S, H, KV = SHAPES[1]
    g = torch.Generator().manual_seed(32)
    qkv = torch.randn(B, S, H + 2 * KV, 32, generator=g).bfloat16().cuda()
    wq, wk = ((0.5 + torch.rand(32, generator=g)).cuda() for _ in range(2))
    cs = T.rope_table(S, 32, 500000.0, "cuda")
    for a, b in zip(T.rope_split(qkv, cs, H, KV, wq, wk, EPS), T._rope_norm_ref(qkv, cs, H, KV, wq, wk, EPS)):
        assert torch.equal(a, b)
