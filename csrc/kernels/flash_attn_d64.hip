// Causal grouped-query flash attention at head dim 64 (Llama-3.2-1B: 32 query heads, 8 KV heads),
// S a multiple of 128, forward and backward on v_mfma_f32_32x32x16_bf16, without and with document
// bounds.  Semantics, layouts and properties are those of flash_attn.hip with 64 in place of 128: dK /
// dV summed over the GQA group in registers, no atomics and no partials (two calls are bitwise equal),
// deferred-rescale online softmax, XCD-aware block order, heaviest blocks first.  launch_fa_fwd /
// launch_fa_bwd dispatch here on the head dim.
//
// Against D = 128 a 64-key tile carries half the MFMA work (QK^T, PV and the four backward products)
// and the same softmax VALU work (exp2, max, sum, masks, bf16 packs), so per tile the fixed costs --
// barrier, votes, LDS latency -- weigh twice as much and the VALU stream, not the matrix pipe, sets the
// pace.  The halved rows (128 B: the RL = 64 swizzle) and accumulators are spent on that:
//
//   forward / dQ   LDS tiles of 128 keys in the same 64 KB: ONE barrier and one prefetch round per
//                  128 keys.  The softmax still runs per 64 keys (forward) and the backward per 32 keys,
//                  so a wave skips the future half of its diagonal tile and the masks stay on the
//                  slices that need them.  O^T / dQ^T take 32 accumulator registers instead of 64 and
//                  Q^T / dO^T 16 instead of 32; the 8-wave kernels stay at two waves per SIMD (155 - 171
//                  registers: capped at 128 for two blocks per compute unit they spill, and the kernels
//                  use no scratch), and the freed registers let the compiler keep all K / V fragments
//                  of a softmax block in flight at once.
//   dK / dV        stages of 128 queries (half the barriers per query); dK / dV take 64 accumulator
//                  registers instead of 128 and the resident K / V fragments half, so the kernel fits
//                  two waves per SIMD (two 128-key blocks per compute unit, 66 KB of LDS each) where
//                  D = 128 runs one.  The in-wave "every LDS read a phase ahead" order is kept; what it
//                  cannot hide in one wave, the second wave covers.
//
// This file is compiled with packed fp32 VALU operations off (ps_amd/_build.py): the softmax is
// written, and counted, as scalar-per-lane VALU work.
// Figures, and what was tried and dropped: profiles/flash_d64_probe.txt.
#include "psamd_flash.h"

namespace psamd {
namespace {

using namespace mfma;
using namespace flash;

constexpr int kD = 64;    // head dim
constexpr int kBK = 128;  // keys per forward / dQ LDS tile
constexpr int kSB = 64;   // keys per forward softmax block
constexpr int kBKB = 128; // keys per dK / dV block (4 waves x 32)
constexpr int kBQS = 128; // queries per dK / dV stage

// acc^T layout: lane column = the output row, register rows d = db*32 + (e & 3) + 8 (e >> 2) + 4 hl
__device__ __forceinline__ void store_t(const f32x16 (&acc)[2], uint16_t* row, float mul, int hl) {
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const u16x4 v = {f32_to_bf16(acc[db][4 * g] * mul), f32_to_bf16(acc[db][4 * g + 1] * mul),
                       f32_to_bf16(acc[db][4 * g + 2] * mul), f32_to_bf16(acc[db][4 * g + 3] * mul)};
      *reinterpret_cast<u16x4*>(row + db * 32 + 8 * g + 4 * hl) = v;
    }
}

// the bounds a forward / dQ lane works with, from its row ds of doc_start: lo of its own query qi;
// uniform: kb0, the first key tile of the block whose first query is qblk, and wlo0 / wlo1, the bounds of
// the first and last query of the wave that begins at q0.  Every bound is clamped to [0, query], so
// malformed bounds cannot move an address out of the tensors.
__device__ __forceinline__ void lower_bounds(const int* __restrict__ ds, int qi, int qblk, int q0, int& lo, int& kb0,
                                             int& wlo0, int& wlo1) {
  lo = clampi(ds[qi], 0, qi);
  kb0 = clampi(ds[qblk], 0, qblk) / kBK;
  wlo0 = __builtin_amdgcn_readfirstlane(clampi(ds[q0], 0, q0));
  wlo1 = __builtin_amdgcn_readfirstlane(clampi(ds[q0 + 31], 0, q0 + 31));
}

// K / V tiles of the forward and dQ kernels: 128 keys x 64, double-buffered, prefetched into registers
// two tiles ahead and written late (flash_attn.hip's scheme at twice the keys per barrier)
template <int NT>
struct KvTiles {
  static constexpr int CH = kBK * 8 / NT;  // 16-B chunks per thread per tensor per tile
  static_assert(CH >= 1 && kBK * 8 % NT == 0, "tile / block shape");
  u16x8 kr[CH], vr[CH];
  __device__ __forceinline__ void gload(const uint16_t* kp, const uint16_t* vp, int kb) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int id = threadIdx.x + i * NT, r = id >> 3, ch = id & 7;
      const int64_t o = static_cast<int64_t>(kb * kBK + r) * kD + ch * 8;
      kr[i] = *reinterpret_cast<const u16x8*>(kp + o);
      vr[i] = *reinterpret_cast<const u16x8*>(vp + o);
    }
  }
  __device__ __forceinline__ void swrite(uint16_t* K, uint16_t* V) const {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int id = threadIdx.x + i * NT, r = id >> 3, ch = id & 7;
      *reinterpret_cast<u16x8*>(K + off<64>(r, ch * 8)) = kr[i];
      *reinterpret_cast<u16x8*>(V + off<64>(r, ch * 8)) = vr[i];
    }
  }
};

// ------------------------------------------------------------------------------ forward
// NW waves x 32 queries share each 128-key K / V tile; per 64-key softmax block S^T = K Q^T is held
// with ONE query per lane column (flash_attn.hip's forward).  DOCS: query i sees doc_start[b, i] <= j <=
// i; the key loop starts at the tile of the block's first bound, a wave skips blocks that end before the
// bound of its first query, and blocks that begin before the bound of its last query are masked by select.
template <int NW, bool DOCS>
__global__ __launch_bounds__(NW * 64) void fa64_fwd_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
    uint16_t* __restrict__ out, float* __restrict__ lse, int S, int H, int KV, float scale,
    const int* __restrict__ doc_start) {
  constexpr int BQ = NW * 32, NT = NW * 64;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[2][kBK * kD];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[2][kBK * kD];
  const int G = H / KV, nqb = S / BQ;
  int unit, rr;
  xcd_unit(blockIdx.x, G * nqb, static_cast<int>(gridDim.x) / (G * nqb), unit, rr);
  const int b = unit / KV, kvh = unit % KV, qb = nqb - 1 - rr / G, h = kvh * G + rr % G;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hl = lane >> 5, c = lane & 31;
  const uint16_t* qp = q + static_cast<int64_t>(b * H + h) * S * kD;
  const uint16_t* kp = k + static_cast<int64_t>(b * KV + kvh) * S * kD;
  const uint16_t* vp = v + static_cast<int64_t>(b * KV + kvh) * S * kD;
  const int q0 = qb * BQ + w * 32, qi = q0 + c;
  const int nkb = (qb * BQ + BQ - 1) / kBK + 1;  // the last tile ends at or before S: S % 128 == 0
  const float k2 = scale * kLog2e;
  int lo = 0, kb0 = 0, wlo0 = 0, wlo1 = 0;
  if constexpr (DOCS) lower_bounds(doc_start + static_cast<int64_t>(b) * S, qi, qb * BQ, q0, lo, kb0, wlo0, wlo1);
  KvTiles<NT> t;
  t.gload(kp, vp, kb0);
  bf16x8_t qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8_t*>(qp + static_cast<int64_t>(qi) * kD + 16 * s + 8 * hl);
  t.swrite(Ks[kb0 & 1], Vs[kb0 & 1]);
  if (kb0 + 1 < nkb) t.gload(kp, vp, kb0 + 1);
  float m2 = -INFINITY, l = 0.f;  // reference max in exp2 units (scores * scale * log2 e)
  f32x16 o[2];
  zero(o[0]);
  zero(o[1]);
  for (int kb = kb0; kb < nkb; ++kb) {
    __syncthreads();  // tile kb is in LDS; every wave is done with tile kb - 1's buffer
    const uint16_t* K = Ks[kb & 1];
    const uint16_t* V = Vs[kb & 1];
#pragma unroll
    for (int sb = 0; sb < kBK / kSB; ++sb) {
      const int kk = kb * kBK + sb * kSB;
      // wave-uniform: skip blocks wholly in this wave's future (DOCS: or wholly before its documents)
      if (kk > q0 + 31) continue;
      if constexpr (DOCS) {
        if (kk + kSB - 1 < wlo0) continue;
      }
      f32x16 st[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        zero(st[ks]);
#pragma unroll
        for (int s = 0; s < 4; ++s) st[ks] = mma(frag<64>(K, sb * kSB + ks * 32 + c, 2 * s + hl), qf[s], st[ks]);
      }
      if (kk + kSB - 1 > q0) {  // the diagonal block: mask the future keys
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int key = kk + ks * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl;
            if (key > qi) st[ks][e] = -INFINITY;
          }
      }
      if constexpr (DOCS) {
        if (kk < wlo1) {  // the block begins before the last query's document: mask earlier documents
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int key = kk + ks * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl;
              if (key < lo) st[ks][e] = -INFINITY;
            }
        }
      }
      float mb = st[0][0];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int e = 0; e < 16; ++e) mb = fmaxf(mb, st[ks][e]);
      // plain: every processed block holds >= 1 visible key per query.  DOCS: a lane whose document
      // begins after the block sees none of it (mb = -inf, maybe m2 = -inf too) and passes through
      // unchanged: no vote for a rescale, alpha = 1, p = 0 -- by select
      mb = xhalf_max(mb) * k2;
      const bool vis = !DOCS || mb > -INFINITY;
      if (!__all(!vis || mb - m2 <= kRescale)) {
        // the vote only opens the branch: a lane moves its reference when its OWN max grew past the
        // threshold, so a row's bits do not depend on which rows (documents) share its wave
        const bool grow = vis && mb - m2 > kRescale;
        const float mn = grow ? mb : m2;
        const float alpha = grow ? fast_exp2(m2 - mn) : 1.f;
        l *= alpha;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
        m2 = mn;
      }
      const float mr = vis ? m2 : 0.f;  // exp2(-inf - 0) = 0 where m2 is still -inf
      float ls = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float p = fast_exp2(st[ks][e] * k2 - mr);
          st[ks][e] = p;
          ls += p;
        }
      l += xhalf_sum(ls);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8_t pb = acc_to_b(st[s >> 1], s, hl);
#pragma unroll
        for (int db = 0; db < 2; ++db) o[db] = mma(tfrag<64>(V, sb * 4 + s, db * 32, lane), pb, o[db]);
      }
    }
    if (kb + 1 < nkb) {
      t.swrite(Ks[(kb + 1) & 1], Vs[(kb + 1) & 1]);  // write-late: the loads had a whole tile to land
      if (kb + 2 < nkb) t.gload(kp, vp, kb + 2);     // in flight behind the next tile's math
    }
  }
  store_t(o, out + (static_cast<int64_t>(b) * S + qi) * H * kD + h * kD, 1.f / l, hl);
  if (hl == 0) lse[static_cast<int64_t>(b * H + h) * S + qi] = m2 * 0.6931471805599453f + __logf(l);
}

// ------------------------------------------------------------------------------ backward: dQ (+ D)
// The forward's structure with each 128-key tile taken as four 32-key slices, so S^T, dP^T and dS^T of
// only one slice are live.  It recomputes P^T from the forward's log-sum-exp, forms dS^T = P^T (dO V^T -
// D), accumulates dQ^T = K^T dS^T, and stores D = rowsum(dO * O).  DOCS: the forward's tile range and
// skips; masked P is set to 0 by select.
template <int NW, bool DOCS>
__global__ __launch_bounds__(NW * 64) void fa64_bwd_dq_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
    const uint16_t* __restrict__ o, const uint16_t* __restrict__ dout, const float* __restrict__ lse,
    float* __restrict__ dsum, uint16_t* __restrict__ dq, int S, int H, int KV, float scale,
    const int* __restrict__ doc_start) {
  constexpr int BQ = NW * 32, NT = NW * 64;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[2][kBK * kD];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[2][kBK * kD];
  const int G = H / KV, nqb = S / BQ;
  int unit, rr;
  xcd_unit(blockIdx.x, G * nqb, static_cast<int>(gridDim.x) / (G * nqb), unit, rr);
  const int b = unit / KV, kvh = unit % KV, qb = nqb - 1 - rr / G, h = kvh * G + rr % G;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hl = lane >> 5, c = lane & 31;
  const uint16_t* qp = q + static_cast<int64_t>(b * H + h) * S * kD;
  const uint16_t* kp = k + static_cast<int64_t>(b * KV + kvh) * S * kD;
  const uint16_t* vp = v + static_cast<int64_t>(b * KV + kvh) * S * kD;
  const int q0 = qb * BQ + w * 32, qi = q0 + c;
  const int nkb = (qb * BQ + BQ - 1) / kBK + 1;
  int lo = 0, kb0 = 0, wlo0 = 0, wlo1 = 0;
  if constexpr (DOCS) lower_bounds(doc_start + static_cast<int64_t>(b) * S, qi, qb * BQ, q0, lo, kb0, wlo0, wlo1);
  KvTiles<NT> t;
  t.gload(kp, vp, kb0);
  const int64_t orow = (static_cast<int64_t>(b) * S + qi) * H * kD + h * kD;
  bf16x8_t qf[4], df[4];
  float dd = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8_t*>(qp + static_cast<int64_t>(qi) * kD + 16 * s + 8 * hl);
    df[s] = *reinterpret_cast<const bf16x8_t*>(dout + orow + 16 * s + 8 * hl);
    const u16x8 ov = *reinterpret_cast<const u16x8*>(o + orow + 16 * s + 8 * hl);
    const u16x8 dv = __builtin_bit_cast(u16x8, df[s]);
#pragma unroll
    for (int e = 0; e < 8; ++e) dd += bf16_to_f32(ov[e]) * bf16_to_f32(dv[e]);
  }
  dd = xhalf_sum(dd);
  const int64_t li = static_cast<int64_t>(b * H + h) * S + qi;
  if (hl == 0) dsum[li] = dd;
  const float l2 = lse[li] * kLog2e, k2 = scale * kLog2e;
  t.swrite(Ks[kb0 & 1], Vs[kb0 & 1]);
  if (kb0 + 1 < nkb) t.gload(kp, vp, kb0 + 1);
  f32x16 acc[2];
  zero(acc[0]);
  zero(acc[1]);
  for (int kb = kb0; kb < nkb; ++kb) {
    __syncthreads();
    const uint16_t* K = Ks[kb & 1];
    const uint16_t* V = Vs[kb & 1];
#pragma unroll
    for (int ks = 0; ks < kBK / 32; ++ks) {
      const int kk0 = kb * kBK + ks * 32;
      if (kk0 > q0 + 31) continue;  // wave-uniform: this slice is wholly in the future
      if constexpr (DOCS) {
        if (kk0 + 31 < wlo0) continue;  // wave-uniform: wholly before this wave's documents
      }
      f32x16 st, dp;
      zero(st);
      zero(dp);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        st = mma(frag<64>(K, ks * 32 + c, 2 * s + hl), qf[s], st);
        dp = mma(frag<64>(V, ks * 32 + c, 2 * s + hl), df[s], dp);  // dP^T = V dO^T
      }
      if (DOCS && kk0 < wlo1) {  // wave-uniform: the slice begins before the last query's document
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float p = fast_exp2(st[e] * k2 - l2);
          const int key = kk0 + (e & 3) + 8 * (e >> 2) + 4 * hl;
          if (key > qi || key < lo) p = 0.f;
          st[e] = p * (dp[e] - dd);
        }
      } else if (kk0 + 31 > q0) {  // wave-uniform: only the diagonal slice needs the causal mask
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float p = fast_exp2(st[e] * k2 - l2);
          if (kk0 + (e & 3) + 8 * (e >> 2) + 4 * hl > qi) p = 0.f;
          st[e] = p * (dp[e] - dd);  // dS^T
        }
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) st[e] = fast_exp2(st[e] * k2 - l2) * (dp[e] - dd);
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8_t sb = acc_to_b(st, s2, hl);
#pragma unroll
        for (int db = 0; db < 2; ++db) acc[db] = mma(tfrag<64>(K, ks * 2 + s2, db * 32, lane), sb, acc[db]);
      }
    }
    if (kb + 1 < nkb) {
      t.swrite(Ks[(kb + 1) & 1], Vs[(kb + 1) & 1]);
      if (kb + 2 < nkb) t.gload(kp, vp, kb + 2);
    }
  }
  store_t(acc, dq + static_cast<int64_t>(b * H + h) * S * kD + static_cast<int64_t>(qi) * kD, scale, hl);
}

// ------------------------------------------------------------------------------ backward: dK / dV
// One block per (128-key block, KV head), 4 waves of 32 keys, ONE key per lane column: the block sweeps
// EVERY query head of its GQA group, so dK / dV of its keys accumulate over the group in registers and
// leave once, in bf16.  Query stages of 128 rows (Q, dO, L, D) arrive by LDS-DMA into a double buffer
// (one barrier per stage); per 32-query slice every LDS read is issued a phase ahead of the MFMAs that
// consume it, as in flash_attn.hip.  Two blocks share a compute unit (launch bounds), so each SIMD holds
// two waves.  Key blocks with the most queries (the first ones) run first.
// DOCS: key j is seen by queries j <= i < doc_end[b, j] (non-decreasing along the row).  The block's
// query stages end with the document of its last key, a wave skips the 32-query slices at or beyond the
// bound of its last key, and slices that reach the bound of its first key take the upper-bound mask (by
// select).  Every bound is clamped to [key + 1, S].
template <bool DOCS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void fa64_bwd_dkdv_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
    const uint16_t* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ dsum,
    uint16_t* __restrict__ dko, uint16_t* __restrict__ dvo, int S, int H, int KV, float scale,
    const int* __restrict__ doc_end) {
  __shared__ __attribute__((aligned(16))) uint16_t Qs[2][kBQS * kD];
  __shared__ __attribute__((aligned(16))) uint16_t dOs[2][kBQS * kD];
  __shared__ __attribute__((aligned(16))) float Ls[2][kBQS];
  __shared__ __attribute__((aligned(16))) float Ds[2][kBQS];
  const int G = H / KV, nkb = S / kBKB;
  int unit, kblk;
  xcd_unit(blockIdx.x, nkb, static_cast<int>(gridDim.x) / nkb, unit, kblk);
  const int b = unit / KV, kvh = unit % KV;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hl = lane >> 5, c = lane & 31;
  const uint16_t* kp = k + static_cast<int64_t>(b * KV + kvh) * S * kD;
  const uint16_t* vp = v + static_cast<int64_t>(b * KV + kvh) * S * kD;
  const int k0 = kblk * kBKB + w * 32, key = k0 + c;
  // stages: (q head g, query stage qs) for qs from this key block's own stage on
  // (DOCS: up to the stage that holds the end of the block's last key's document)
  int hi = S, nqs = S / kBQS, whi0 = S, whi1 = S;
  if constexpr (DOCS) {
    const int* de = doc_end + static_cast<int64_t>(b) * S;
    hi = clampi(de[key], key + 1, S);
    nqs = (clampi(de[kblk * kBKB + kBKB - 1], kblk * kBKB + kBKB, S) + kBQS - 1) / kBQS;
    whi0 = __builtin_amdgcn_readfirstlane(clampi(de[k0], k0 + 1, S));
    whi1 = __builtin_amdgcn_readfirstlane(clampi(de[k0 + 31], k0 + 32, S));
  }
  const int qs0 = kblk * kBKB / kBQS, per = nqs - qs0, nst = G * per;
  auto issue = [&](int st) {
    const int g = st / per, qs = qs0 + st % per, h = kvh * G + g, buf = st & 1;
    const int64_t li = static_cast<int64_t>(b * H + h) * S + qs * kBQS;
    dma_tile64(Qs[buf], q + li * kD, kD, kBQS, w, 4, lane);
    dma_tile64(dOs[buf], dout + (static_cast<int64_t>(b) * S + qs * kBQS) * H * kD + h * kD, static_cast<int64_t>(H) * kD,
               kBQS, w, 4, lane);
    // 128 L and 128 D values: one 64-lane instruction per wave
    const int o = (w & 1) * 64;
    if (w < 2) __builtin_amdgcn_global_load_lds((gptr_t*)(lse + li + o + lane), (lptr_t*)(Ls[buf] + o), 4, 0, 0);
    else __builtin_amdgcn_global_load_lds((gptr_t*)(dsum + li + o + lane), (lptr_t*)(Ds[buf] + o), 4, 0, 0);
  };
  issue(0);
  bf16x8_t kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = *reinterpret_cast<const bf16x8_t*>(kp + static_cast<int64_t>(key) * kD + 16 * s + 8 * hl);
    vf[s] = *reinterpret_cast<const bf16x8_t*>(vp + static_cast<int64_t>(key) * kD + 16 * s + 8 * hl);
  }
  const float k2 = scale * kLog2e;
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    zero(dk[db]);
    zero(dv[db]);
  }
  for (int st = 0; st < nst; ++st) {
    const int qbase = (qs0 + st % per) * kBQS, buf = st & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // stage st landed everywhere; stage st - 1's buffer is read out
    if (st + 1 < nst) issue(st + 1);
    const uint16_t* Q = Qs[buf];
    const uint16_t* dO = dOs[buf];
#pragma unroll 1
    for (int sl = 0; sl < kBQS / 32; ++sl) {
      const int qr0 = qbase + sl * 32;
      if (qr0 + 31 < k0) continue;  // wave-uniform: every query precedes every key of this wave
      if constexpr (DOCS) {
        if (qr0 >= whi1) continue;  // wave-uniform: every query is beyond this wave's documents
      }
      f32x4 lv[4], dv4[4];
      bf16x8_t qa[4], da[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        lv[g] = lds_f4(Ls[buf] + sl * 32 + 8 * g + 4 * hl);
        dv4[g] = lds_f4(Ds[buf] + sl * 32 + 8 * g + 4 * hl);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) qa[s] = frag_a<64>(Q, sl * 32 + c, 2 * s + hl);
#pragma unroll
      for (int s = 0; s < 4; ++s) da[s] = frag_a<64>(dO, sl * 32 + c, 2 * s + hl);
      lgkm_wait<4>();  // L / D and the Q fragments are in; the dO fragments land behind the S chain
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        tie4(lv[g]);
        tie4(dv4[g]);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) tie(qa[s]);
      f32x16 sa, dp;
      zero(sa);
      zero(dp);
#pragma unroll
      for (int s = 0; s < 4; ++s) sa = mma(qa[s], kf[s], sa);
      lgkm_wait<0>();
#pragma unroll
      for (int s = 0; s < 4; ++s) tie(da[s]);
#pragma unroll
      for (int s = 0; s < 4; ++s) dp = mma(da[s], vf[s], dp);
      bf16x8_t ta[2][2], tq[2][2];  // transposed dO / Q fragments: behind the dP chain, under the softmax
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          ta[s2][db] = tfrag_a<64>(dO, sl * 2 + s2, db * 32, lane);
          tq[s2][db] = tfrag_a<64>(Q, sl * 2 + s2, db * 32, lane);
        }
      if (DOCS && qr0 + 31 >= whi0) {  // wave-uniform: the slice reaches the end of the first key's document
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float p = fast_exp2(sa[e] * k2 - lv[e >> 2][e & 3] * kLog2e);
          const int qr = qr0 + (e & 3) + 8 * (e >> 2) + 4 * hl;
          if (key > qr || qr >= hi) p = 0.f;
          sa[e] = p;
          dp[e] = p * (dp[e] - dv4[e >> 2][e & 3]);
        }
      } else if (k0 + 31 > qr0) {  // wave-uniform: only slices on the diagonal need the causal mask
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float p = fast_exp2(sa[e] * k2 - lv[e >> 2][e & 3] * kLog2e);
          if (key > qr0 + (e & 3) + 8 * (e >> 2) + 4 * hl) p = 0.f;
          sa[e] = p;
          dp[e] = p * (dp[e] - dv4[e >> 2][e & 3]);  // dS
        }
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float p = fast_exp2(sa[e] * k2 - lv[e >> 2][e & 3] * kLog2e);
          sa[e] = p;
          dp[e] = p * (dp[e] - dv4[e >> 2][e & 3]);
        }
      }
      lgkm_wait<0>();
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          tie(ta[s2][db]);
          tie(tq[s2][db]);
        }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8_t pb = acc_to_b(sa, s2, hl), sb = acc_to_b(dp, s2, hl);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          dv[db] = mma(ta[s2][db], pb, dv[db]);
          dk[db] = mma(tq[s2][db], sb, dk[db]);
        }
      }
    }
  }
  // bf16 rows of this KV head: lane column = key, rows d -> 8-B pieces
  const int64_t row = (static_cast<int64_t>(b * KV + kvh) * S + key) * kD;
  store_t(dk, dko + row, scale, hl);
  store_t(dv, dvo + row, 1.f, hl);
}

}  // namespace

void launch_fa64_fwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, float* lse, int B, int S,
                     int H, int KV, float scale, hipStream_t s, const int* doc_start) {
  const bool w8 = S % 256 == 0;  // 256-query blocks (8 waves) where they tile the row, else 128 (4 waves)
  auto* kern = w8 ? (doc_start ? fa64_fwd_kernel<8, true> : fa64_fwd_kernel<8, false>)
                  : (doc_start ? fa64_fwd_kernel<4, true> : fa64_fwd_kernel<4, false>);
  hipLaunchKernelGGL(kern, dim3(S / (w8 ? 256 : 128) * H * B), dim3(w8 ? 512 : 256), 0, s, q, k, v, out, lse, S, H, KV,
                     scale, doc_start);
}

void launch_fa64_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* out, const uint16_t* dout,
                     const float* lse, float* dsum, uint16_t* dq, uint16_t* dk, uint16_t* dv, int B, int S, int H,
                     int KV, float scale, hipStream_t s, const int* doc_start, const int* doc_end) {
  const bool w8 = S % 256 == 0, docs = doc_start != nullptr;
  auto* kq = w8 ? (docs ? fa64_bwd_dq_kernel<8, true> : fa64_bwd_dq_kernel<8, false>)
                : (docs ? fa64_bwd_dq_kernel<4, true> : fa64_bwd_dq_kernel<4, false>);
  hipLaunchKernelGGL(kq, dim3(S / (w8 ? 256 : 128) * H * B), dim3(w8 ? 512 : 256), 0, s, q, k, v, out, dout, lse, dsum,
                     dq, S, H, KV, scale, doc_start);
  hipLaunchKernelGGL(docs ? fa64_bwd_dkdv_kernel<true> : fa64_bwd_dkdv_kernel<false>, dim3(S / kBKB * KV * B), dim3(256),
                     0, s, q, k, v, dout, lse, dsum, dk, dv, S, H, KV, scale, doc_end);
}

}  // namespace psamd
