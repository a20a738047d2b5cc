"""fp64 oracles, a bf16 yardstick, a replay of the launch plans and input builders for the implicit-GEMM
convolution kernels (csrc/kernels/convgemm.hip, conv_big.hip, conv_bwd_fused.hip).  Plain torch; imported
by test_conv_oracle_cpu.py and test_conv_rows_gpu.py.  bf16r, rowerr, elemerr, U24, REL and MAGREL are
transformer_oracle's, AMBIG is bn_oracle's.

The gather is written from convgemm.hip's header comment: output pixel m = (i, oh, ow) with tap (kh, kw)
and channel c reads input (i, oh s - p + kh, ow s - p + kw, c), zero outside the map, and the reduction
index is k = (kh ks + kw) C + c.  Every function takes the bf16 / fp32 tensors the kernel receives and
computes in fp64.

Where the bf16 roundings are (read from the kernels)
    staged A        a prologue's result is rounded to bf16 when it is staged (kProBnRelu:
                    relu(bf16(x sc + sh)); kProBnBwd: bf16(ca a + cb a2 + cc); kProBlockOut:
                    bf16(relu(a sc + sh + r))) -- in BOTH variants: it is the GEMM's bf16 operand, and for
                    the two-source prologues the stored `aout` itself.  `abits` are o > 0 of the value
                    before that rounding, which equals (aout > 0): rounding keeps a positive fp32 positive.
    c               the fp32 accumulator is rounded to bf16 when it goes to the LDS output tile (acc_to_lds),
                    BEFORE any epilogue runs.  So the residual epilogues (2, 4, 5 and the folds 6-9) add the
                    residual to the rounded accumulator in fp32 and round a SECOND time:
                    c = bf16(bf16(acc) + r); masks (3, and bits2 of the folds) zero the rounded value.
    statistics      taken on the final bf16 c (after residual and masks), in fp32: never rounded.
    dW, db          fp32 slabs, fixed-order fp32 reduce, dW rounded once at the end; db stays fp32.
    conv11_bwd_fused  dz3 = bf16(ca g + cb z3 + cc) staged in LDS (never stored), a2 = relu(bf16(z2 sc + sh))
                    staged, gy = bf16(acc) then masked, dW3 as dW.
The yardstick (rounded=True) rounds exactly there; the exact variant keeps the staged bf16 operands and
rounds nothing after them.  `mag` is sum_k |f(a)_k b_k| plus the absolute values of the residual terms
that the last expression adds; elemerr allows 2^-6 |yardstick| + 2^-14 mag.

Ambiguity sets (computed here from the inputs alone, capped at 1e-3 of a case's elements):
  (a) ReLU-mask elements with |z sc + sh| <= AMBIG (|z sc| + |sh|): either masked value is accepted;
  (b) staged prologue values whose fp64 value lies within 2^-22 (sum of |terms|) of a bf16 rounding
      boundary or of zero: ulp_bf16(a_k) |b_k| more tolerance on the outputs that element feeds.
The builders settle their inputs (one bf16 step away) so that both sets are empty or nearly so.

The second rounding of the residual epilogues has no term in the elementwise rule: where the residual
cancels the accumulator, one bf16 step of the intermediate bf16(acc) -- which fp32 accumulation order
may legitimately flip -- is many steps of the small sum.  The builders therefore give a residual the
sign of the exact accumulator and magnitude >= 0.25, so |c| >= |bf16(acc)| and two steps of c cover it.
"""
import functools
import math

import torch

from .bn_oracle import AMBIG, mask_bits, unpack_bits  # noqa: F401  (re-exported)
from .bn_oracle import apply as bn_apply
from .bn_oracle import bwd_apply as bn_bwd_apply
from .transformer_oracle import MAGREL, REL, U24, bf16_ulp, bf16r, elemerr, rowerr  # noqa: F401  (re-exported)

CAP = 1e-3  # largest share of a case's elements in an ambiguity set
PRO_NONE, PRO_BN_RELU, PRO_BN_BWD, PRO_BLOCK_OUT = 0, 1, 2, 3
# psamd::ConvFwdFamily, as the conv_gemm_family binding reports it
FAMILY = {"big": 0, "twosrc_glds": 1, "patch": 2, "tall": 3, "twosrc_reg": 4, "glds": 5, "reg": 6}


def geo(h, w, ks=1, stride=1, pad=0):
    """[H, W, OH, OW, ks, stride, pad], the bindings' geometry vector."""
    return [h, w, (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1, ks, stride, pad]


# ------------------------------------------------------------------------------------ gather
def src_rows(images, H, W, OH, OW, nh, nw, stride, pad):
    """src(m, tap): long [images OH OW, nh nw], the input pixel row (i H + ih) W + iw that output pixel
    m = (i, oh, ow) reads for tap (kh, kw) = (tap // nw, tap % nw), or -1 outside the map."""
    i = torch.arange(images).view(-1, 1, 1, 1, 1)
    oh = torch.arange(OH).view(1, -1, 1, 1, 1)
    ow = torch.arange(OW).view(1, 1, -1, 1, 1)
    ih = oh * stride - pad + torch.arange(nh).view(1, 1, 1, -1, 1)
    iw = ow * stride - pad + torch.arange(nw).view(1, 1, 1, 1, -1)
    ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
    idx = (i * H + ih) * W + iw
    return torch.where(ok, idx, torch.full_like(idx, -1)).reshape(images * OH * OW, nh * nw)


def gather(x, idx):
    """x [rows, C] -> A [M, taps C] with A[m, tap C + c] = x[src(m, tap), c], zero where src is -1."""
    C = x.shape[1]
    xz = torch.cat([x, torch.zeros(1, C, dtype=x.dtype)])
    return xz[idx.reshape(-1)].reshape(idx.shape[0], idx.shape[1] * C)


def gather_geo(x, g):
    H, W, OH, OW, ks, st, pd = g
    return gather(x, src_rows(x.shape[0] // (H * W), H, W, OH, OW, ks, ks, st, pd))


def mat3(w):
    """[N, C, 3, 3] -> [N, 9 C] with k = (kh 3 + kw) C + c."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def mat3_dgrad(w):
    """The stride-1 3x3 data gradient as a forward GEMM over dz: wd[c, (kh 3 + kw) N + n] = w[n, c, 2 - kh, 2 - kw]."""
    N, C = w.shape[:2]
    kh = torch.arange(3).view(1, 3, 1, 1)
    kw = torch.arange(3).view(1, 1, 3, 1)
    return w[torch.arange(N).view(1, 1, 1, N), torch.arange(C).view(C, 1, 1, 1), 2 - kh, 2 - kw].reshape(C, 9 * N)


PHASE_TAPS = {0: [1], 1: [2, 0]}  # input row 2 i + a takes dz rows i + d with kernel row PHASE_TAPS[a][d]


def phase_weight(w, a, b):
    """Phase (a, b) of the stride-2 3x3 data gradient: wp[c1, (dh nw + dw) C2 + c2] = w[c2, c1, kh(a, dh), kw(b, dw)]."""
    C2, C1 = w.shape[:2]
    kh = torch.tensor(PHASE_TAPS[a]).view(1, -1, 1, 1)
    kw = torch.tensor(PHASE_TAPS[b]).view(1, 1, -1, 1)
    return w[torch.arange(C2).view(1, 1, 1, C2), torch.arange(C1).view(C1, 1, 1, 1), kh, kw].reshape(C1, -1)


def phase_rows(images, H, W, a, b):
    """(src [M, nh nw] into the dz map H/2 x W/2, dst [M] rows of the H x W map) of phase (a, b): phase
    pixel (i, oh, ow) reads dz (oh + dh, ow + dw) and lands at (i, 2 oh + a, 2 ow + b)."""
    OH, OW = H // 2, W // 2
    src = src_rows(images, OH, OW, OH, OW, 1 + a, 1 + b, 1, 0)
    i = torch.arange(images).view(-1, 1, 1)
    dst = (i * H + 2 * torch.arange(OH).view(1, -1, 1) + a) * W + 2 * torch.arange(OW).view(1, 1, -1) + b
    return src, dst.reshape(-1)


def mm(a, bt, device=None, chunk=16384):
    """a [M, K] @ bt [K, N] in fp64, in row chunks, on `device` (None: where a is); the result on the CPU."""
    if device is None:
        return a.double() @ bt.double()
    btd = bt.double().to(device)
    return torch.cat([(a[i:i + chunk].double().to(device) @ btd).cpu() for i in range(0, a.shape[0], chunk)])


# ------------------------------------------------------------------------------------ prologues
def near_boundary(v, scale):
    """bool like v: the fp64 value v lies within 2^-22 scale of a bf16 rounding boundary or of zero."""
    r = bf16r(v)
    dist = 0.5 * bf16_ulp(v) - (v - r).abs()
    return (dist <= AMBIG * scale) | (v.abs() <= AMBIG * scale)


def stage_bn_relu(x, cf):
    """kProBnRelu: a = relu(bf16(x sc + sh)) -> (a fp64, amb (b) bool, the bf16 step at a)."""
    C = x.shape[1]
    cf = cf.double()
    t = x.double() * cf[:C]
    v = t + cf[C:]
    a = bf16r(v).clamp_min(0.0)
    return a, near_boundary(v, t.abs() + cf[C:].abs()), bf16_ulp(v)


def stage_block_out(a, r, cf, cf2=None):
    """kProBlockOut: relu(a sc + sh + r) or relu(a sc + sh + (r sc2 + sh2)) -> (exact, yardstick (the bf16
    aout), mag); the same arithmetic as bn_oracle.apply with act 1."""
    ye, mag = bn_apply(a, cf, r, cf2, 1, False)
    yy, _ = bn_apply(a, cf, r, cf2, 1, True)
    return ye, yy, mag


def stage_bn_bwd(a, a2, c3):
    """kProBnBwd: ca a + cb a2 + cc -> (exact, yardstick (the bf16 aout), mag)."""
    ye, mag = bn_bwd_apply(a, a2, c3, False)
    yy, _ = bn_bwd_apply(a, a2, c3, True)
    return ye, yy, mag


def mask_ambiguous(z, mc):
    """Set (a): |z sc + sh| <= AMBIG (|z sc| + |sh|)."""
    N = z.shape[-1]
    mc = mc.double()
    t = z.double() * mc[:N]
    return (t + mc[N:]).abs() <= AMBIG * (t.abs() + mc[N:].abs())


def settle_mask(z, mc):
    """z with every set-(a) element moved one bf16 step away from zero (as bn_oracle.settle)."""
    for _ in range(4):
        a = mask_ambiguous(z, mc)
        if not bool(a.any()):
            break
        z = torch.where(a, (z.view(torch.int16) + 1).view(torch.bfloat16), z)
    return z


def settle_stage(x, value_scale):
    """x (bf16) with every element whose staged value is in set (b) moved one bf16 step; value_scale(x) ->
    (v, scale).  Up to 4 passes; what remains is counted by the caller."""
    for _ in range(4):
        v, s = value_scale(x)
        a = near_boundary(v, s)
        if not bool(a.any()):
            break
        x = torch.where(a, (x.view(torch.int16) + 1).view(torch.bfloat16), x)
    return x


# ------------------------------------------------------------------------------------ epilogues
def s2_residual(t, images, OH, OW):
    """Epilogues 4 / 8: the (OH+1)/2 x (OW+1)/2 map t scattered to even (h, w) of the OH x OW map ->
    (rows [M, N] fp64, present bool [M, 1])."""
    N = t.shape[1]
    RH, RW = (OH + 1) // 2, (OW + 1) // 2
    full = torch.zeros(images, OH, OW, N, dtype=torch.float64)
    full[:, ::2, ::2] = t.double().view(images, RH, RW, N)
    here = torch.zeros(images, OH, OW, 1, dtype=torch.bool)
    here[:, ::2, ::2] = True
    return full.view(-1, N), here.view(-1, 1)


def epi_base(epi):
    return {6: 5, 7: 2, 8: 4, 9: 5}.get(epi, epi)


def epilogue(epi, acc, mag, t):
    """Epilogue `epi` on the exact accumulator acc [M, N] -> dict(exact, yard, mag, amb, alt).
    t: dict of the kernel's operands (aux, bits, aux2, bits2, mc, ... as the binding names them; for
    epilogues 4 / 8 also images, OH, OW).  on: epilogue 3's mask; amb / alt: set (a) and the yardstick with
    the mask flipped."""
    M, N = acc.shape
    base = epi_base(epi)
    c0 = bf16r(acc)  # acc_to_lds
    oe, oy, m = acc, c0, mag
    amb = alt = on = None
    if base in (2, 4, 5):
        if base == 4:
            r, _ = s2_residual(t["aux"], t["images"], t["OH"], t["OW"])
        else:
            r = t["aux"].double()
            if base == 5:
                r = r * unpack_bits(t["bits"], (M, N)).double()
        oe, oy, m = acc + r, bf16r(c0 + r), mag + r.abs()
    elif base == 3:
        mc = t["mc"].double()
        on = t["aux"].double() * mc[:N] + mc[N:] > 0
        amb = mask_ambiguous(t["aux"], t["mc"])
        oe, oy, alt = acc * on, c0 * on, c0 * ~on
    if epi >= 6:
        keep2 = unpack_bits(t["bits2"], (M, N)).double()
        oe, oy = oe * keep2, oy * keep2
    return dict(exact=oe, yard=oy, mag=m, amb=amb, alt=alt, on=on)


def sum_terms(epi, c, t):
    """The terms of the fp32 partial sums, from a stored output c [M, N]: one [M, N] fp64 tensor per slab.
    1: c - kshift, (c - kshift)^2;  3: g, g xhat(aux);  6-9: g, g xhat(aux2) (9: and g xhat2(aux3))."""
    cd = c.double()
    if epi == 1:
        d = cd - (t["kshift"].double() if t.get("kshift") is not None else 0.0)
        return [d, d * d]
    if epi == 3:
        return [cd, cd * ((t["aux"].double() - t["mean"].double()) * t["invstd"].double())]
    if epi >= 6:
        out = [cd, cd * ((t["aux2"].double() - t["mean"].double()) * t["invstd"].double())]
        if epi == 9:
            out.append(cd * ((t["aux3"].double() - t["mean2"].double()) * t["invstd2"].double()))
        return out
    return []


def block_sums(terms, block_of_row, G):
    """Per-block fp64 sums of the terms: (sums [slabs, G, N], abs sums [slabs, G, N]); block_of_row [M] long."""
    N = terms[0].shape[1]
    s = torch.zeros(len(terms), G, N, dtype=torch.float64)
    a = torch.zeros(len(terms), G, N, dtype=torch.float64)
    for i, x in enumerate(terms):
        s[i].index_add_(0, block_of_row, x)
        a[i].index_add_(0, block_of_row, x.abs())
    return s, a


def fwd_blocks(M, bm, gm):
    """Block (partial-sum row) of each output pixel: tile m // bm runs on block tile % gm."""
    return (torch.arange(M) // bm) % gm


# ------------------------------------------------------------------------------------ plan replay
def _cdiv(a, b):
    return -(-a // b)


def _patch_fwd_ok(g, C, N, pro):
    H, W, OH, OW, ks, st, pd = g
    if pro or ks != 3 or st != 1 or pd != 1 or OH != H or OW != W or C % 64 or OH * OW < 128 or N % 128:
        return False
    span = (OW - 1 + 128 + OW - 1) // OW
    plane = _cdiv((span + 4) * (W + 2) * 16, 1024) * 1024
    return 8 * plane <= 40960


def _big_ok(M, N, K, C, g, pro, epi):
    H, W, OH, OW, ks, st, pd = g
    src2 = {PRO_BLOCK_OUT: 1, PRO_BN_BWD: 2}.get(pro, 0)
    if ks != 1 or pd != 0 or C != K or N % 256 or K % 64 or K < 256:
        return False
    plain = epi in (0, 1, 3)
    if not plain and ((pro and src2 != 2) or src2 == 1):
        return False
    if pro:
        if st != 1 or (src2 == 2 and epi in (0, 1)) or (src2 == 1 and epi == 3):
            return False
    nblk = _cdiv(M, 256) * (N // 256)
    return nblk >= 256 and (nblk >= 1024 or K >= 1024)


def plan_fwd(M, N, C, g, pro=PRO_NONE, epi=0):
    """Replay of conv_fwd_plan_geo / conv_fwd_plan and launch_conv_fwd's ladder (convgemm.hip, conv_big.hip):
    family ('big' 256 x 256, 'twosrc_glds', 'twosrc_reg', 'patch', 'tall' 256 x 64, 'glds' LDS-DMA,
    'reg' register-staged), bm, bn, gm (blocks per channel tile = partial-sum rows), tiles, tpb (most tiles
    of one block), nk (64-deep stages) and L, the fp32 roundings on the longest addition chain of a
    partial sum: a thread adds NPASS = bm / (256 / (bn / 8)) rows per tile (big: 256 / (512 / 32) = 16),
    serially over its tpb tiles; then log2(64 / (bn / 8)) shuffle steps (big: 1) join the lanes of equal
    column group; then the waves' values are added ((a + b) + (c + d): 2; big: 8 in sequence); 3 roundings
    lie inside a term (z - mean, x invstd, x g)."""
    K = g[4] * g[4] * C
    nk = K // 64
    src2 = {PRO_BLOCK_OUT: 1, PRO_BN_BWD: 2}.get(pro, 0)
    mt128 = _cdiv(M, 128)

    def base(p):
        if not p and N == 64 and nk >= 8:
            return 256, 64, _cdiv(M, 256)
        bn = 128 if N % 128 == 0 else 64
        persist = nk <= 2 or (p and nk <= 4)
        return 128, bn, (max(1, min(mt128, 512 // (N // bn))) if persist else mt128)

    bn128 = 128 if N % 128 == 0 else 64
    if _big_ok(M, N, K, C, g, pro, epi):
        fam, bm, bn, gm = "big", 256, 256, _cdiv(M, 256)
    elif src2 and nk >= 4:
        fam, bm, bn, gm = "twosrc_glds", 128, bn128, mt128
    elif src2 == 1:
        _, _, gm = base(True)
        fam, bm, bn = "twosrc_reg", 128, 64
        if gm != mt128:
            gm = max(1, min(mt128, 512 // (N // 64)))
    elif _patch_fwd_ok(g, C, N, pro != 0):
        bm, bn, gm = 128, bn128, mt128
        fam = "patch" if epi in (0, 1, 3) else "glds"
    else:
        bm, bn, gm = base(pro != 0)
        if src2:
            fam = "twosrc_reg"
        elif bm == 256:
            fam = "tall"
        elif pro == PRO_NONE and gm == mt128 and nk > 2:
            fam = "glds"
        else:
            fam = "reg"
    tiles = _cdiv(M, bm)
    tpb = _cdiv(tiles, gm)
    if fam == "big":
        L = tpb * 16 + 1 + 8 + 3
    else:
        cpr = bn // 8
        L = tpb * (bm // (256 // cpr)) + int(math.log2(64 // cpr)) + 2 + 3
    return dict(family=fam, bm=bm, bn=bn, gm=gm, tiles=tiles, tpb=tpb, nk=nk, L=L)


def _fill_rounds(tiles, slots, cap):
    ns, best = 1, -1.0
    for rounds in (1, 2):
        cand = max(1, min(rounds * slots // tiles, cap))
        blocks = cand * tiles
        eff = blocks / (_cdiv(blocks, slots) * float(slots))
        if eff > best + 0.02:
            best, ns = eff, cand
    return ns


def _slab_groups(nsplit, E):
    return 0 if nsplit <= 16 or (E >= 1 << 18 and nsplit <= 64) else _cdiv(nsplit, 16)


def _wgrad_patch_ok(g, C, M, N, pro):
    H, W, OH, OW, ks, st, pd = g
    if pro or ks != 3 or pd != 1 or C % 64 or N % 64 or C > 128 or M % 112:
        return False
    if st == 1:
        return H == OH and W == OW and W in (56, 28) and OH % (112 // W) == 0
    return st == 2 and W == 56 and H % 2 == 0 and OH == H // 2 and OW == 28 and OH % 4 == 0


def _reduce_chain(n):
    """slab_reduce_kernel over n slabs: four interleaved accumulators, then (a0 + a1) + (a2 + a3)."""
    return _cdiv(n, 4) + 2


def plan_wgrad(M, N, K, C, g, pro=False):
    """Replay of wplan / pplan / patch_ok / fill_rounds / slab_groups (convgemm.hip): kind (0 the 64 / 128
    tiles, 1-4 the wide tiles, 5 the 3x3 patch kernel), tn x tk (the dW tile), tiles, nsplit (fp32 slabs),
    rows (pixels per split; patch: 112-pixel stages per split), groups (first-level reduce groups, 0 = one
    level), levels, and two chain lengths in fp32 roundings: L of a dW element -- the MFMA accumulator takes
    one 16-pixel step per instruction, ceil(pixels per split / 16) in sequence, 4 more inside a step's
    16-term sum, then the slab reduce (ceil(n / 4) + 2 over n slabs: four interleaved accumulators and
    their pairwise sum) once per level -- and L_db of the bias gradient: a thread of the db blocks adds
    32 / (512 / (tn / 8)) rows per 32-pixel stage over rows / 32 stages, then 512 / (tn / 8) values in
    sequence, then the slab reduce over nsplit."""
    if _wgrad_patch_ok(g, C, M, N, pro):
        kind, tn, tk = 5, 64, 64
        tiles = (N // 64) * (C // 64)
        stages = M // 112
        ns = _fill_rounds(tiles, 256, max(1, stages // 4))
        rows = _cdiv(stages, ns)
        nsplit = _cdiv(stages, rows)
        pix = rows * 112
    else:
        ks1 = K == C
        bno = 256 if N % 256 == 0 else 128
        bko = 256 if K % 256 == 0 else 128
        if bno == 128 and bko == 128 and K % 384 == 0:
            bko = 384
        if (not pro or ks1) and N % 128 == 0 and K % 128 == 0 and C % 8 == 0 and (bno == 256 or bko > 128):
            kind = (1 if bko == 256 else 2) if bno == 256 else (3 if bko == 256 else 4)
            tn, tk = bno, bko
            tiles = (N // bno) * (K // bko)
            chunks = _cdiv(M, 32)
            ns = _fill_rounds(tiles, 256, max(1, chunks // 8))
            rows = _cdiv(chunks, ns) * 32
        else:
            kind = 0
            tn, tk = (128 if N % 128 == 0 else 64), (128 if C % 128 == 0 else 64)
            tiles = (N // tn) * (K // tk)
            chunks = _cdiv(M, 64)
            ns = _fill_rounds(tiles, 512, max(1, chunks // 4))
            rows = _cdiv(chunks, ns) * 64
        nsplit = _cdiv(M, rows)
        pix = rows
    groups = _slab_groups(nsplit, N * K)
    red = _reduce_chain(16) + _reduce_chain(groups) if groups else _reduce_chain(nsplit)
    L = _cdiv(pix, 16) + 4 + red
    L_db = 0
    if 1 <= kind <= 4:
        dbr = 512 // (tn // 8)
        L_db = (rows // 32) * max(1, 32 // dbr) + dbr + _reduce_chain(nsplit)
    return dict(kind=kind, tn=tn, tk=tk, tiles=tiles, nsplit=nsplit, rows=rows, groups=groups,
                levels=2 if groups else 1, L=L, L_db=L_db)


def plan_fused(M):
    """conv11_bwd_fused (64 -> 256): blocks = min(tiles, 256), tile ti of block b is b + ti blocks; a thread
    adds 16 values per tile, then one shuffle step, then (a + b) + (c + d) over the pixel blocks."""
    tiles = _cdiv(M, 128)
    gm = max(1, min(tiles, 256))
    tpb = _cdiv(tiles, gm)
    return dict(gm=gm, tiles=tiles, tpb=tpb, L=16 * tpb + 1 + 2 + 3, groups=_cdiv(gm, 16) if gm > 16 else 0)


# ------------------------------------------------------------------------------------ builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _coef(n, g):
    """[scale | shift] fp32: scale in [0.5, 1.5], shift ~ 0.5 N(0, 1)."""
    return torch.cat([torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.5]).float()


def _bits(M, N, g, p):
    keep = torch.rand(M, N, generator=g) > p
    return mask_bits(keep.double())


def signed_residual(acc, g, rows=None):
    """bf16 residual with the sign of acc (+ where acc is 0) and |r| = 0.25 + |randn| (module docstring)."""
    shape = acc.shape if rows is None else (rows, acc.shape[1])
    mag = 0.25 + torch.randn(*shape, generator=g).abs()
    return mag, torch.where(acc >= 0, 1.0, -1.0)


@functools.lru_cache(maxsize=2)
def _base_fwd(images, H, W, ks, stride, pad, C, N, pro, dual, kind, seed, device):
    """The operands and the exact GEMM of a forward case, shared by every epilogue of the shape."""
    g = _gen(seed)
    gg = geo(H, W, ks, stride, pad)
    rows, K = images * H * W, ks * ks * C
    t = dict(geo=gg, images=images, OH=gg[2], OW=gg[3])
    x = torch.randn(rows, C, generator=g).bfloat16()
    if kind == "impulse":
        b = torch.zeros(N, K)
        b[torch.arange(N), (37 * torch.arange(N) + 11) % K] = 1.0
        t["kn"] = (37 * torch.arange(N) + 11) % K
    else:
        b = torch.randn(N, K, generator=g) * K ** -0.5
    t["b"] = b.bfloat16()
    amb_b = ulp = None
    if pro == PRO_BN_RELU:
        cf = _coef(C, g)
        cd = cf.double()
        x = settle_stage(x, lambda v: (v.double() * cd[:C] + cd[C:], (v.double() * cd[:C]).abs() + cd[C:].abs()))
        a, amb_b, ulp = stage_bn_relu(x, cf)
        t.update(pro=cf)
    elif pro == PRO_BLOCK_OUT:
        cf = _coef(C, g)
        r = torch.randn(rows, C, generator=g).bfloat16()
        cf2 = _coef(C, g) if dual else None
        ye, a, ymag = stage_block_out(x, r, cf, cf2)
        t.update(pro=cf, a2=r, pro2=cf2, aout_exact=ye, aout_yard=a, aout_mag=ymag)
    elif pro == PRO_BN_BWD:
        z = torch.randn(rows, C, generator=g).bfloat16()
        c3 = torch.cat([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3,
                        torch.randn(C, generator=g) * 0.1]).float()
        ye, a, ymag = stage_bn_bwd(x, z, c3)
        t.update(a2=z, bwd=c3, aout_exact=ye, aout_yard=a, aout_mag=ymag)
    else:
        a = None
    t["a"] = x
    # (no prologue: gather the bf16 rows first, so only the [M, K] operand exists in fp64)
    A = gather_geo(x, gg).double() if a is None else gather_geo(a, gg)
    t["A"] = A
    bt = t["b"].double().t()
    t["acc"] = mm(A, bt, device)
    t["mag"] = mm(A.abs(), bt.abs(), device)
    if amb_b is not None:
        t["share_b"] = float(amb_b.double().mean())
        t["extra"] = mm(gather_geo(amb_b.double() * ulp, gg), bt.abs(), device) if bool(amb_b.any()) else None
    return t


def fwd_inputs(case, device=None):
    """dict of a forward case's operands (CPU tensors named as conv_gemm's arguments), the staged and
    gathered A, the exact accumulator acc and mag, and the shares of the ambiguity sets."""
    images, H, W, ks, stride, pad, C, N, pro, epi = (case[k] for k in
                                                     ("images", "H", "W", "ks", "stride", "pad", "C", "N", "pro", "epi"))
    seed = 1000 + 7 * (images * H * W) + 3 * C + N + 11 * ks + stride + 13 * pro
    t = dict(_base_fwd(images, H, W, ks, stride, pad, C, N, pro, case.get("dual", False),
                       case.get("kind", "randn"), seed, device))
    M = t["acc"].shape[0]
    g = _gen(seed + 100 + epi)
    base = epi_base(epi)
    t.setdefault("share_b", 0.0)
    t["share_a"] = 0.0
    if epi == 1:
        t["kshift"] = (torch.randn(N, generator=g) * 0.1).float()
    if base in (2, 5):
        mag, sign = signed_residual(t["acc"], g)
        t["aux"] = (mag * sign).bfloat16()
    if base == 4:
        RH, RW = (t["OH"] + 1) // 2, (t["OW"] + 1) // 2
        even = t["acc"].view(images, t["OH"], t["OW"], N)[:, ::2, ::2].reshape(-1, N)
        mag, sign = signed_residual(even, g)
        assert mag.shape[0] == images * RH * RW
        t["aux"] = (mag * sign).bfloat16()
    if base == 5:
        t["bits"] = _bits(M, N, g, 0.5)
    if epi == 3:
        t["mc"] = _coef(N, g)
        t["aux"] = settle_mask(torch.randn(M, N, generator=g).bfloat16(), t["mc"])
        t["share_a"] = float(mask_ambiguous(t["aux"], t["mc"]).double().mean())
    if epi == 3 or epi >= 6:
        t["mean"] = (torch.randn(N, generator=g) * 0.1).float()
        t["invstd"] = (torch.rand(N, generator=g) + 0.5).float()
    if epi >= 6:
        t["aux2"] = torch.randn(M, N, generator=g).bfloat16()
        t["bits2"] = _bits(M, N, g, 0.4)
    if epi == 9:
        t["aux3"] = torch.randn(M, N, generator=g).bfloat16()
        t["mean2"] = (torch.randn(N, generator=g) * 0.1).float()
        t["invstd2"] = (torch.rand(N, generator=g) + 0.5).float()
    return t


def wgrad_oracle(dz, A, device=None, amb=None, ulp=None):
    """dW[n, k] = sum_m dz[m, n] A[m, k] -> dict(exact, yard, mag, extra); db = sum_m dz with its mag."""
    dzt = dz.double().t().contiguous()
    e = mm(dzt, A, device)
    out = dict(exact=e, yard=bf16r(e), mag=mm(dzt.abs(), A.abs(), device), extra=None,
               db=dz.double().sum(0), db_mag=dz.double().abs().sum(0))
    if amb is not None and bool(amb.any()):
        out["extra"] = mm(dzt.abs(), amb.double() * ulp, device)
    return out


def wgrad_inputs(case):
    """dict(dz [M, N], x [rows, C] bf16, geo, pro, A (staged, gathered), share_b, amb, ulp) of a
    weight-gradient case; kind 'impulse': dz has one nonzero, 1.0 at row (37 n + 11) mod M of column n."""
    images, H, W, ks, stride, pad, C, N = (case[k] for k in ("images", "H", "W", "ks", "stride", "pad", "C", "N"))
    gg = geo(H, W, ks, stride, pad)
    M = images * gg[2] * gg[3]
    g = _gen(2000 + 5 * M + C + 3 * N + ks + stride)
    x = torch.randn(images * H * W, C, generator=g).bfloat16()
    t = dict(geo=gg, M=M, pro=None, share_b=0.0, amb=None, ulp=None)
    if case.get("kind") == "impulse":
        dz = torch.zeros(M, N)
        t["mn"] = (37 * torch.arange(N) + 11) % M
        dz[t["mn"], torch.arange(N)] = 1.0
    else:
        dz = torch.randn(M, N, generator=g)
    a = x.double()
    if case.get("pro"):
        cf = _coef(C, g)
        cd = cf.double()
        x = settle_stage(x, lambda v: (v.double() * cd[:C] + cd[C:], (v.double() * cd[:C]).abs() + cd[C:].abs()))
        a, amb, ulp = stage_bn_relu(x, cf)
        t.update(pro=cf, share_b=float(amb.double().mean()), amb=gather_geo(amb.double(), gg) > 0,
                 ulp=gather_geo(ulp, gg))
    t.update(dz=dz.bfloat16(), x=x, A=gather_geo(a, gg))
    return t


def dgrad_s2_inputs(images, H, W, C1, C2, epi, seed):
    """dict(dz [images H/2 W/2, C2], w [C2, C1, 3, 3] bf16, and for epilogue 3 z1 / mc / mean / invstd)."""
    g = _gen(seed)
    t = dict(dz=torch.randn(images * (H // 2) * (W // 2), C2, generator=g).bfloat16(),
             w=(torch.randn(C2, C1, 3, 3, generator=g) * (9 * C1) ** -0.5).bfloat16(), share_a=0.0)
    if epi == 3:
        t["mc"] = _coef(C1, g)
        t["aux"] = settle_mask(torch.randn(images * H * W, C1, generator=g).bfloat16(), t["mc"])
        t["mean"] = (torch.randn(C1, generator=g) * 0.1).float()
        t["invstd"] = (torch.rand(C1, generator=g) + 0.5).float()
        t["share_a"] = float(mask_ambiguous(t["aux"], t["mc"]).double().mean())
    return t


def dgrad_s2_oracle(t, images, H, W, epi):
    """The four phases assembled: dict(exact, yard, mag, amb, alt [images H W, C1]) and block [images H W],
    the partial-sum row (phase gm + phase tile) that owns each dx row."""
    M = images * (H // 2) * (W // 2)
    C1 = t["w"].shape[1]
    gm = _cdiv(M, 128)
    acc = torch.zeros(images * H * W, C1, dtype=torch.float64)
    mag = torch.zeros_like(acc)
    block = torch.zeros(images * H * W, dtype=torch.long)
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        src, dst = phase_rows(images, H, W, a, b)
        A = gather(t["dz"].double(), src)
        wp = phase_weight(t["w"].double(), a, b).t()
        acc[dst] = A @ wp
        mag[dst] = A.abs() @ wp.abs()
        block[dst] = ph * gm + torch.arange(M) // 128
    out = epilogue(epi, acc, mag, t)
    out.update(block=block, G=4 * gm)
    return out


def fused_inputs(M, plain, seed):
    """conv11_bwd_fused (CI 64, CO 256): g, z3 [M, 256], z2 [M, 64] bf16, cbwd [768], wt [64, 256] bf16, and
    (not plain) cf2 [128], mean2, invstd2 [64].  g and z2 are settled against sets (b) and (a)."""
    CI, CO = 64, 256
    g = _gen(seed)
    t = dict(z3=torch.randn(M, CO, generator=g).bfloat16(),
             cbwd=torch.cat([torch.rand(CO, generator=g) + 0.5, torch.randn(CO, generator=g) * 0.3,
                             torch.randn(CO, generator=g) * 0.1]).float(),
             wt=(torch.randn(CI, CO, generator=g) * CO ** -0.5).bfloat16(),
             z2=torch.randn(M, CI, generator=g).bfloat16())
    c3, z3 = t["cbwd"].double(), t["z3"].double()

    def vs(v):
        t1, t2 = c3[:CO] * v.double(), c3[CO:2 * CO] * z3
        return t1 + t2 + c3[2 * CO:], t1.abs() + t2.abs() + c3[2 * CO:].abs()

    t["g"] = settle_stage(torch.randn(M, CO, generator=g).bfloat16(), vs)
    if not plain:
        t["cf2"] = _coef(CI, g)
        cd = t["cf2"].double()
        z2 = settle_mask(t["z2"], t["cf2"])
        t["z2"] = settle_stage(z2, lambda v: (v.double() * cd[:CI] + cd[CI:], (v.double() * cd[:CI]).abs() + cd[CI:].abs()))
        t["mean2"] = (torch.randn(CI, generator=g) * 0.1).float()
        t["invstd2"] = (torch.rand(CI, generator=g) + 0.5).float()
    return t


def fused_oracle(t, plain, device=None):
    """-> dict(dz3 (the staged bf16 value), gy / dw = dict(exact, yard, mag, extra), amb / alt of gy,
    share_a, share_b)."""
    CI, CO = 64, 256
    v, vmag = bn_bwd_apply(t["g"], t["z3"], t["cbwd"], False)
    dz3 = bf16r(v)
    amb3, ulp3 = near_boundary(v, vmag), bf16_ulp(v)
    wt = t["wt"].double()
    acc = mm(dz3, wt.t(), device)
    mag = mm(dz3.abs(), wt.t().abs(), device)
    e3 = amb3.double() * ulp3
    extra_gy = mm(e3, wt.t().abs(), device)
    share_a, n_b = 0.0, float(amb3.double().sum())
    if plain:
        a2, e2 = t["z2"].double(), None
        gy = dict(exact=acc, yard=bf16r(acc), mag=mag, extra=extra_gy, amb=None, alt=None)
    else:
        a2, amb2, ulp2 = stage_bn_relu(t["z2"], t["cf2"])
        e2 = amb2.double() * ulp2
        n_b += float(amb2.double().sum())
        gy = epilogue(3, acc, mag, dict(aux=t["z2"], mc=t["cf2"]))
        gy["extra"] = extra_gy
        share_a = float(gy["amb"].double().mean())
    dw = wgrad_oracle(dz3, a2, device)
    dw["extra"] = mm(e3.t().contiguous(), a2.abs(), device)
    if e2 is not None:
        dw["extra"] = dw["extra"] + mm(dz3.abs().t().contiguous(), e2, device)
    return dict(dz3=dz3, gy=gy, dw=dw, share_a=share_a, share_b=n_b / (dz3.numel() + a2.numel()))


def with_extra(mag, extra=None, L=None):
    """The mag to hand to elemerr so that its tolerance is 2^-6 |ref| + f mag + extra, f = 2^-14 or, with L,
    2^-24 L (the fallback for long reductions)."""
    m = mag if L is None else mag * (U24 * L / MAGREL)
    return m if extra is None else m + extra / MAGREL


# ------------------------------------------------------------------------------------ cases
def _c11(M, C, N, pro, epi, fam, tpb=1, images=None, H=None, W=None, **kw):
    images, H, W = (1, M, 1) if images is None else (images, H, W)
    assert images * H * W == M
    return dict(images=images, H=H, W=W, ks=1, stride=1, pad=0, C=C, N=N, pro=pro, epi=epi, family=fam, tpb=tpb, **kw)


def _c(images, H, W, ks, stride, C, N, pro, epi, fam, tpb=1, **kw):
    return dict(images=images, H=H, W=W, ks=ks, stride=stride, pad=ks // 2, C=C, N=N, pro=pro, epi=epi, family=fam,
                tpb=tpb, **kw)


def case_id(c):
    s = f"{c['images']}x{c['H']}x{c['W']}-k{c['ks']}s{c['stride']}-C{c['C']}-N{c['N']}-pro{c['pro']}-epi{c['epi']}"
    return s + ("-dual" if c.get("dual") else "") + ("-impulse" if c.get("kind") == "impulse" else "")


_MAPS = {1: (1, 1, 1), 127: (1, 127, 1), 129: (3, 43, 1), 300: (3, 10, 10), 255: (3, 17, 5), 257: (1, 257, 1),
         600: (6, 10, 10), 517: (11, 47, 1), 20000: (2, 100, 100), 40001: (1, 40001, 1), 65300: (1, 653, 100)}


def _m(M):
    return dict(zip(("images", "H", "W"), _MAPS[M]))


FWD_CASES = []
# register-staged 128 x {64, 128}, one tile per block
for _M in (1, 127, 129, 300):
    for _K in (64, 128):
        for _N in (64, 128, 192):
            FWD_CASES += [_c11(_M, _K, _N, 0, e, "reg", **_m(_M)) for e in range(10)]
            FWD_CASES += [_c11(_M, _K, _N, PRO_BN_RELU, e, "reg", **_m(_M)) for e in (0, 1)]
FWD_CASES += [_c(3, 13, 11, 1, 2, 128, 64, 0, e, "reg") for e in (0, 1)]
FWD_CASES += [_c11(300, 64, 128, 0, 0, "reg", kind="impulse", **_m(300))]
# persistent loop: 157 tiles over 64 blocks, 313 tiles over 128 blocks
FWD_CASES += [_c11(20000, 64, 1024, 0, e, "reg", 3, **_m(20000)) for e in (1, 3, 6, 9)]
FWD_CASES += [_c11(40001, 128, 512, 0, e, "reg", 3, **_m(40001)) for e in (1, 3, 6, 9)]
FWD_CASES += [_c11(20000, 64, 1024, PRO_BN_RELU, 1, "reg", 3, **_m(20000)),
              _c11(40001, 128, 512, PRO_BN_RELU, 1, "reg", 3, **_m(40001)),
              _c11(20000, 256, 1024, PRO_BN_RELU, 1, "reg", 3, **_m(20000)),
              _c11(40001, 256, 512, PRO_BN_RELU, 1, "reg", 3, **_m(40001)),
              _c11(20000, 128, 512, PRO_BLOCK_OUT, 1, "twosrc_reg", 3, **_m(20000))]
# LDS-DMA 128 x {64, 128}
for _K, _N in ((192, 128), (192, 192), (512, 128), (512, 192)):
    FWD_CASES += [_c11(300, _K, _N, 0, e, "glds", **_m(300)) for e in range(10)]
for _H, _W in ((9, 9), (7, 5)):
    for _s in (1, 2):
        FWD_CASES += [_c(3, _H, _W, 3, _s, 128, 128, 0, e, "glds") for e in (0, 1, 3)]
FWD_CASES += [_c(3, 9, 1, 3, 1, 128, 128, 0, 0, "glds"), _c(3, 2, 2, 3, 1, 128, 128, 0, 0, "glds"),
              _c(3, 9, 9, 3, 1, 128, 128, 0, 0, "glds", kind="impulse")]
# tall 256 x 64
for _M in (255, 257, 600):
    FWD_CASES += [_c11(_M, 512, 64, 0, e, "tall", **_m(_M)) for e in range(9)]
    FWD_CASES += [dict(_c(1, 1, 1, 3, 1, 64, 64, 0, e, "tall"), **_m(_M)) for e in range(9)]
# patch-staged 3x3
for _i, _H, _W in ((3, 12, 11), (3, 9, 15), (2, 28, 28)):
    for _C in (64, 128):
        for _N in (128, 256):
            FWD_CASES += [_c(_i, _H, _W, 3, 1, _C, _N, 0, e, "patch") for e in (0, 1, 3)]
    FWD_CASES += [_c(_i, _H, _W, 3, 1, 64, 128, 0, 0, "patch", kind="impulse")]
# two-source prologues
for _M in (129, 517):
    for _K in (64, 192, 256, 512):
        _f = "twosrc_reg" if _K < 256 else "twosrc_glds"
        for _e in (0, 1):
            FWD_CASES += [_c11(_M, _K, 128, PRO_BLOCK_OUT, _e, _f, dual=d, **_m(_M)) for d in (False, True)]
        FWD_CASES += [_c11(_M, _K, 128, PRO_BN_BWD, 3, _f, **_m(_M))]
# ... on 64-channel tiles (N = 64, 192): both prologues on the LDS-DMA variant (three stage buffers under the
# 128 x 68 output tile), kProBnBwd on the register-staged one (kProBlockOut always runs bn 64 there: above)
for _N in (64, 192):
    for _K in (64, 192, 256, 512):
        _f = "twosrc_reg" if _K < 256 else "twosrc_glds"
        FWD_CASES += [_c11(517, _K, _N, PRO_BN_BWD, 3, _f, **_m(517))]
        if _K >= 256:
            FWD_CASES += [_c11(517, _K, _N, PRO_BLOCK_OUT, e, _f, dual=d, **_m(517)) for e, d in ((0, False), (1, True))]
# kProBnRelu on a 3x3 (register-staged, !KS1): a padded tap must stay 0 AFTER the prologue
for _H, _W in ((7, 5), (9, 9)):
    for _C, _N in ((64, 64), (128, 128), (64, 192)):
        FWD_CASES += [_c(3, _H, _W, 3, 1, _C, _N, PRO_BN_RELU, e, "reg") for e in (0, 1)]
FWD_CASES += [_c(3, 9, 9, 3, 2, 64, 128, PRO_BN_RELU, 1, "reg")]
# conv_big at the eligibility floor: 256 blocks, the last tile partial
BIG_CASES = [_c11(65300, 1024, 256, 0, e, "big", **_m(65300)) for e in range(10)]
BIG_CASES += [_c11(65300, 1024, 256, PRO_BN_RELU, e, "big", **_m(65300)) for e in (0, 1)]
BIG_CASES += [_c11(65300, 1024, 256, PRO_BLOCK_OUT, e, "big", **_m(65300)) for e in (0, 1)]
BIG_CASES += [_c11(65300, 1024, 256, PRO_BN_BWD, e, "big", **_m(65300)) for e in range(2, 10)]
BIG_CASES += [dict(_c(1, 1305, 199, 1, 2, 1024, 256, 0, 0, "big"), pad=0)]

# (images, H, W, C1, C2): both channel tiles; 8 x 12: h != w (every phase has images H W / 4 pixels whatever the map)
DGRAD_S2_CASES = [(2, 6, 4, 64, 64), (2, 14, 10, 128, 128), (3, 8, 12, 64, 128), (3, 8, 12, 128, 64)]


def _w(images, H, W, ks, stride, C, N, pro, wkind, levels, **kw):
    return dict(images=images, H=H, W=W, ks=ks, stride=stride, pad=ks // 2, C=C, N=N, pro=pro, wkind=wkind,
                levels=levels, **kw)


WGRAD_CASES = []
for _N, _C in ((128, 128), (128, 64), (64, 128), (64, 64)):  # (tno, tko) = (2, 2), (2, 1), (1, 2), (1, 1)
    WGRAD_CASES += [_w(3, 10, 10, 1, 1, _C, _N, p, 0, 1) for p in (False, True)]
WGRAD_CASES += [_w(3, 9, 9, 3, 1, 64, 64, False, 0, 1), _w(3, 9, 9, 3, 1, 64, 64, True, 0, 1),
                _w(4, 14, 13, 1, 2, 64, 128, False, 0, 1),
                _w(1, 2000, 1, 1, 1, 64, 64, False, 0, 1),  # 8 slabs, one level
                _w(1, 6000, 1, 1, 1, 64, 64, False, 0, 2), _w(1, 6000, 1, 1, 1, 64, 64, True, 0, 2),  # 19 slabs
                _w(3, 10, 10, 1, 1, 64, 64, False, 0, 1, kind="impulse")]
# wide: kinds 1-4; LIN (1x1 stride 1) and not; PROL (pro, tk 128 / 256) and the fragment prologue (tk 384)
WGRAD_CASES += [_w(1, 777, 1, 1, 1, 256, 256, False, 1, 1), _w(1, 777, 1, 1, 1, 256, 256, True, 1, 1),
                _w(1, 777, 1, 1, 1, 128, 256, False, 2, 1), _w(1, 777, 1, 1, 1, 128, 256, True, 2, 1),
                _w(1, 777, 1, 1, 1, 256, 128, False, 3, 1), _w(1, 777, 1, 1, 1, 256, 128, True, 3, 1),
                _w(3, 9, 9, 3, 1, 128, 128, False, 4, 1), _w(3, 11, 11, 3, 2, 128, 128, False, 4, 1),
                _w(1, 777, 1, 1, 1, 384, 128, True, 4, 1), _w(1, 777, 1, 1, 1, 384, 128, False, 4, 1),
                _w(5, 11, 11, 1, 2, 256, 256, False, 1, 1),
                _w(5, 11, 11, 1, 2, 256, 256, True, 1, 1),   # PROL, not LIN
                _w(5, 11, 11, 1, 2, 384, 128, True, 4, 1),   # the fragment prologue (tk 384), not LIN
                _w(1, 5001, 1, 1, 1, 256, 256, False, 1, 2), _w(1, 5001, 1, 1, 1, 256, 256, True, 1, 2),
                _w(1, 5001, 1, 1, 1, 512, 512, False, 1, 1),  # 18 slabs of 2^18 elements: one level (the exception)
                _w(1, 777, 1, 1, 1, 256, 256, False, 1, 1, kind="impulse")]
# patch: <56, 1>, <28, 1>, <56, 2> at one image (M = 3136 / 784 / 784, multiples of 112)
WGRAD_CASES += [_w(1, 56, 56, 3, 1, 64, 64, False, 5, 1), _w(1, 28, 28, 3, 1, 128, 128, False, 5, 1),
                _w(1, 56, 56, 3, 2, 64, 128, False, 5, 1), _w(1, 56, 56, 3, 1, 64, 64, False, 5, 1, kind="impulse")]
# linear_wgrad_db (the wide kernel's DB variant): (M, N, K, levels)
DB_CASES = [(777, 256, 256, 1), (5001, 256, 128, 2), (777, 128, 256, 1), (777, 128, 384, 1)]  # kinds 1, 2, 3, 4


def db_inputs(M, N, K):
    """(dz [M, N], x [M, K]) bf16 randn of a linear_wgrad_db case (no prologue: no ambiguity set)."""
    g = _gen(M + N + K)
    return torch.randn(M, N, generator=g).bfloat16(), torch.randn(M, K, generator=g).bfloat16()


def wgrad_id(c):
    return (f"{c['images']}x{c['H']}x{c['W']}-k{c['ks']}s{c['stride']}-C{c['C']}-N{c['N']}-kind{c['wkind']}"
            + ("-pro" if c["pro"] else "") + ("-impulse" if c.get("kind") == "impulse" else ""))


# conv11_bwd_fused: M; 33000 -> 258 tiles over 256 blocks (blocks 0 and 1 run two tiles)
FUSED_MS = [1, 129, 300, 33000]
