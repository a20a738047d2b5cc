// Fused multi-head self-attention for BERT sequences beyond one tile (S <= 512, head dim 64): the
// 128-query x 128-key tile of attention.hip inside loops over 128-row blocks, the way flash_attn.hip
// runs Llama.  Same I/O (qkv [B, S, 3, H, 64] or packed [T, 3, H, 64]; out [B, S, H * 64] or [T, H * 64];
// lse [B * H, S] or packed [H, T]; dqkv like qkv), same dropout draw per element at the call's S
// (psamd_attn_dropout.h), same length rules.  Three kernels, deterministic, no atomics, no fp32
// partials in HBM:
//
//   forward  one workgroup per (128-query block, batch x head), 4 waves x 32 queries; Q fragments in
//            registers; loop over 128-key chunks staged into swizzled [128][64] LDS tiles.  A lane owns
//            ONE query column of S^T = K Q^T, so the running max, the running sum and the O^T
//            accumulators are per-lane: the online rescale is one scalar multiply per accumulator with
//            no cross-lane traffic, and it is done for every chunk (32 multiplies beside 64 exp2).
//            O^T is normalised by the row sum once, at the end; lse = m * scale + log(sum).
//   dQ       same grid; O / dO fragments, D = rowsum(dO * O) and lse of the lane's query loaded once;
//            per chunk P = exp2(score * k2 - lse * log2e), dP = dO V^T, dS = P * (dP - D); dS^T is
//            already the accumulator of a [key][query] block, so it becomes the B operand of
//            dQ^T += K^T dS^T by the register relayout the forward uses for P^T (no LDS round trip).
//   dK / dV  one workgroup per (128-key block, batch x head), wave w owns keys [32w, 32w + 32) of it;
//            loop over 128-query blocks: stage Q and dO, recompute P_drop and dS of the tile as
//            attn_bwd_kernel does and pass each through the [128][128] LDS tile T; dV^T and dK^T stay
//            in registers across the loop.
//
// One code path for the three layouts: a sequence is (row0, Lq, Lk) at run time --
//   dense        row0 = b * S,        Lq = S, Lk = S
//   key lengths  row0 = b * S,        Lq = S, Lk = clamp(klen[b], 1, S)
//   packed       row0 = clamped cu[b], Lq = Lk = L (pack_rows)
// Tiles are staged with zeros at rows at or beyond the bound, direct global loads of such rows clamp
// to the bound's last row, stores are guarded: nothing is read or written at or beyond row L of a
// packed sequence.  Key chunks and 32-key blocks wholly beyond Lk are skipped; the pad keys of the
// partly valid block are excluded by select (p = 0 exactly, dp = 0 whatever the V row holds); in the
// padded layout dK / dV rows >= Lk are stored as exact zeros (dqkv is not pre-zeroed).
#include "psamd_attn_dropout.h"
#include "psamd_device.h"
#include "psamd_launch.h"
#include "psamd_mfma.h"

namespace psamd {
namespace {

using namespace mfma;

constexpr int kD = 64;    // head dim
constexpr int kC = 128;   // rows of a query block / a key chunk
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kMasked = -3.0e38f;  // score of a pad key (the running max starts there too)

struct Seq {
  int64_t row0;  // first row of the sequence in qkv / out / dqkv
  int Lq, Lk;    // query and key bound
  int64_t lse0;  // index of query 0's lse
};
__device__ __forceinline__ Seq seq_of(int b, int h, int S, int H, int T, const int32_t* __restrict__ klen,
                                      const int32_t* __restrict__ cu) {
  if (cu) {
    const PackRows pr = pack_rows(cu, b, S, T);
    return {pr.row0, pr.L, pr.L, static_cast<int64_t>(h) * T + pr.row0};
  }
  const int Lk = klen ? min(max(klen[b], 1), S) : S;
  return {static_cast<int64_t>(b) * S, S, Lk, (static_cast<int64_t>(b) * H + h) * S};
}

// rows [0, nr[i]) of N 64-wide slices (row strides rs[i] elements) into [128][64] tiles, rows nr[i]..127
// zeroed (and not read from memory); 256 threads, every global load issued before any LDS store
template <int N>
__device__ __forceinline__ void stage(uint16_t* const (&T)[N], const uint16_t* const (&src)[N], const int64_t (&rs)[N],
                                      const int (&nr)[N]) {
  constexpr int PER = kC * 8 / 256;  // 16-B chunks per thread per tile
  u16x8 v[N][PER];
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int id = threadIdx.x + i * 256, r = id >> 3, ch = id & 7;
      v[n][i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (r < nr[n]) v[n][i] = *reinterpret_cast<const u16x8*>(src[n] + r * rs[n] + ch * 8);
    }
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int id = threadIdx.x + i * 256, r = id >> 3, ch = id & 7;
      *reinterpret_cast<u16x8*>(T[n] + off<64>(r, ch * 8)) = v[n][i];
    }
}

// the key of accumulator element e of the 32-key block that begins at k0, on lane half hl
__device__ __forceinline__ int key_of(int k0, int e, int hl) { return k0 + (e & 3) + 8 * (e >> 2) + 4 * hl; }

// acc^T (lane column = the output row, 4 consecutive d per 8-B piece) * mul -> one 64-wide row
__device__ __forceinline__ void store_row(const f32x16 (&acc)[2], uint16_t* row, float mul, int hl) {
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const u16x4 v = {f32_to_bf16(acc[db][4 * g] * mul), f32_to_bf16(acc[db][4 * g + 1] * mul),
                       f32_to_bf16(acc[db][4 * g + 2] * mul), f32_to_bf16(acc[db][4 * g + 3] * mul)};
      *reinterpret_cast<u16x4*>(row + db * 32 + 8 * g + 4 * hl) = v;
    }
}

// ------------------------------------------------------------------------------ forward
template <bool DROP>
__global__ __launch_bounds__(256) void attn_long_fwd_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out,
                                                            float* __restrict__ lse, int S, int H, float scale,
                                                            uint64_t seed, uint32_t thr, float rkeep,
                                                            const int32_t* __restrict__ klen,
                                                            const int32_t* __restrict__ cu, int T) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kC * kD];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[kC * kD];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H, qb0 = blockIdx.y * kC;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hl = lane >> 5, c = lane & 31;
  const Seq sq = seq_of(b, h, S, H, T, klen, cu);
  if (qb0 >= sq.Lq) return;  // a query block beyond L (packed): block-uniform, before any barrier
  const int Lq = sq.Lq, Lk = sq.Lk;
  const int64_t rs = 3LL * H * kD;
  const uint16_t* base = qkv + sq.row0 * rs + h * kD;
  const int q0 = qb0 + w * 32, q = q0 + c;
  const bool act = q0 < Lq;  // wave-uniform; an idle wave still stages and meets the barriers
  // Q^T as the B operand: lane holds Q[q][16 s + 8 hl + e]
  bf16x8_t qf[4];
  const int qr = min(q, Lq - 1);
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8_t*>(base + qr * rs + 16 * s + 8 * hl);
  const float k2 = scale * kLog2e;
  const uint32_t rowbase = (static_cast<uint32_t>(bh) * S + q) * S;
  float m = kMasked, sum = 0.f;  // running max (raw score units) and this lane half's part of the running sum
  f32x16 o[2];
  zero(o[0]);
  zero(o[1]);
  for (int k0 = 0; k0 < Lk; k0 += kC) {
    if (k0) __syncthreads();  // the previous chunk is read out
    {
      uint16_t* const tt[2] = {Ks, Vs};
      const uint16_t* const ss[2] = {base + H * kD + k0 * rs, base + 2 * H * kD + k0 * rs};
      const int64_t rr[2] = {rs, rs};
      const int nr[2] = {Lk - k0, Lk - k0};
      stage<2>(tt, ss, rr, nr);
    }
    __syncthreads();
    if (!act) continue;
    const int nkb = min(4, (Lk - k0 + 31) >> 5);  // >= 1
    const bool part = k0 + kC > Lk;               // the chunk holds pad keys
    f32x16 st[4];
    float mc = kMasked;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      zero(st[kb]);
      if (kb < nkb) {
#pragma unroll
        for (int s = 0; s < 4; ++s) st[kb] = mma(frag<64>(Ks, kb * 32 + c, 2 * s + hl), qf[s], st[kb]);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          // a pad key's score by select: out of the max, and its p = exp2(-huge) is 0 exactly
          if (part) st[kb][e] = key_of(k0 + kb * 32, e, hl) < Lk ? st[kb][e] : kMasked;
          mc = fmaxf(mc, st[kb][e]);
        }
      }
    }
    // online softmax: every processed chunk holds a valid key, so mn is a real score; the first
    // chunk's alpha is exp2(-huge) = 0 on accumulators that are zeros
    const float mn = fmaxf(m, xhalf_max(mc));
    const float alpha = fast_exp2((m - mn) * k2);
    m = mn;
    sum *= alpha;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        if (kb >= nkb) continue;  // a skipped block: its p are zeros already, no hash
        float p0 = fast_exp2((st[kb][e] - m) * k2), p1 = fast_exp2((st[kb][e + 1] - m) * k2);
        sum += p0 + p1;
        if constexpr (DROP) {  // keys key, key + 1 (key even): one hash
          const uint32_t hh = pair_hash(seed, (rowbase + key_of(k0 + kb * 32, e, hl)) >> 1);
          p0 = keep_lo(hh, thr) ? p0 * rkeep : 0.f;
          p1 = keep_hi(hh, thr) ? p1 * rkeep : 0.f;
        }
        st[kb][e] = p0;
        st[kb][e + 1] = p1;
      }
    // O^T[d][q] += sum_key V^T[d][key] P^T[key][q]
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (s < 2 * nkb) {
        const bf16x8_t pb = acc_to_b(st[s >> 1], s, hl);
#pragma unroll
        for (int db = 0; db < 2; ++db) o[db] = mma(tfrag<64>(Vs, s, db * 32, lane), pb, o[db]);
      }
    }
  }
  if (!act) return;
  sum = xhalf_sum(sum);
  if (q >= Lq) return;  // a lane on a clamped row: it stores nothing
  if (hl == 0) lse[sq.lse0 + q] = m * scale + __logf(sum);
  store_row(o, out + (sq.row0 + q) * H * kD + h * kD, 1.f / sum, hl);
}

// ------------------------------------------------------------------------------ dQ
template <bool DROP>
__global__ __launch_bounds__(256) void attn_long_dq_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o,
                                                           const uint16_t* __restrict__ dout,
                                                           const float* __restrict__ lse, uint16_t* __restrict__ dqkv,
                                                           int S, int H, float scale, uint64_t seed, uint32_t thr,
                                                           float rkeep, const int32_t* __restrict__ klen,
                                                           const int32_t* __restrict__ cu, int T) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kC * kD];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[kC * kD];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H, qb0 = blockIdx.y * kC;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hl = lane >> 5, c = lane & 31;
  const Seq sq = seq_of(b, h, S, H, T, klen, cu);
  if (qb0 >= sq.Lq) return;  // block-uniform, before any barrier
  const int Lq = sq.Lq, Lk = sq.Lk;
  const int64_t rs = 3LL * H * kD, ors = static_cast<int64_t>(H) * kD;
  const uint16_t* base = qkv + sq.row0 * rs + h * kD;
  const int q0 = qb0 + w * 32, q = q0 + c;
  const bool act = q0 < Lq;
  const int qr = min(q, Lq - 1);
  // Q^T and dO^T as B operands (lane holds row q, columns 16 s + 8 hl + e), and the same columns of O:
  // D = rowsum(dO * O) is this half's 32 columns plus the other half's
  bf16x8_t qf[4], of[4];
  float dd = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8_t*>(base + qr * rs + 16 * s + 8 * hl);
    of[s] = *reinterpret_cast<const bf16x8_t*>(dout + (sq.row0 + qr) * ors + h * kD + 16 * s + 8 * hl);
    const u16x8 ov = *reinterpret_cast<const u16x8*>(o + (sq.row0 + qr) * ors + h * kD + 16 * s + 8 * hl);
#pragma unroll
    for (int e = 0; e < 8; ++e) dd += bf16_to_f32(static_cast<uint16_t>(of[s][e])) * bf16_to_f32(ov[e]);
  }
  dd = xhalf_sum(dd);
  const float l2 = lse[sq.lse0 + qr] * kLog2e, k2 = scale * kLog2e;
  const uint32_t rowbase = (static_cast<uint32_t>(bh) * S + q) * S;
  f32x16 acc[2];
  zero(acc[0]);
  zero(acc[1]);
  for (int k0 = 0; k0 < Lk; k0 += kC) {
    if (k0) __syncthreads();
    {
      uint16_t* const tt[2] = {Ks, Vs};
      const uint16_t* const ss[2] = {base + H * kD + k0 * rs, base + 2 * H * kD + k0 * rs};
      const int64_t rr[2] = {rs, rs};
      const int nr[2] = {Lk - k0, Lk - k0};
      stage<2>(tt, ss, rr, nr);
    }
    __syncthreads();
    if (!act) continue;
    const int nkb = min(4, (Lk - k0 + 31) >> 5);
    const bool part = k0 + kC > Lk;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      if (kb >= nkb) continue;
      // S^T = K Q^T and dP^T = V dO^T of this 32-key block
      f32x16 pt, ds;
      zero(pt);
      zero(ds);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        pt = mma(frag<64>(Ks, kb * 32 + c, 2 * s + hl), qf[s], pt);
        ds = mma(frag<64>(Vs, kb * 32 + c, 2 * s + hl), of[s], ds);
      }
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        const int key = key_of(k0 + kb * 32, e, hl);
        uint32_t hh = 0;
        if constexpr (DROP) hh = pair_hash(seed, (rowbase + key) >> 1);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          // pad keys: p = exp2(-huge) = 0 exactly, and dp = 0 whatever the V row holds
          const bool ok = !part || key + u < Lk;
          const float p = fast_exp2((ok ? pt[e + u] : kMasked) * k2 - l2);
          float dp = ok ? ds[e + u] : 0.f;
          if constexpr (DROP) {
            const bool kp = u ? keep_hi(hh, thr) : keep_lo(hh, thr);
            dp = kp ? dp * rkeep : 0.f;
          }
          ds[e + u] = p * (dp - dd);
        }
      }
      // dQ^T[d][q] += sum_key K^T[d][key] dS^T[key][q]
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int s = 2 * kb + s2;
        const bf16x8_t sb = acc_to_b(ds, s, hl);
#pragma unroll
        for (int db = 0; db < 2; ++db) acc[db] = mma(tfrag<64>(Ks, s, db * 32, lane), sb, acc[db]);
      }
    }
  }
  if (q >= Lq) return;
  store_row(acc, dqkv + (sq.row0 + q) * rs + h * kD, scale, hl);
}

// ------------------------------------------------------------------------------ dK / dV
template <bool DROP>
__global__ __launch_bounds__(256) void attn_long_dkv_kernel(const uint16_t* __restrict__ qkv,
                                                            const uint16_t* __restrict__ o,
                                                            const uint16_t* __restrict__ dout,
                                                            const float* __restrict__ lse, uint16_t* __restrict__ dqkv,
                                                            int S, int H, float scale, uint64_t seed, uint32_t thr,
                                                            float rkeep, const int32_t* __restrict__ klen,
                                                            const int32_t* __restrict__ cu, int T_) {
  __shared__ __attribute__((aligned(16))) uint16_t Qs[kC * kD];
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kC * kD];
  __shared__ __attribute__((aligned(16))) uint16_t dOs[kC * kD];
  __shared__ __attribute__((aligned(16))) uint16_t T[kC * kC];  // [query][key]: P_drop, then dS
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H, kb0 = blockIdx.y * kC;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hl = lane >> 5, c = lane & 31;
  const Seq sq = seq_of(b, h, S, H, T_, klen, cu);
  const int Lq = sq.Lq, Lk = sq.Lk;
  const int KB = cu ? Lk : S;  // the key rows that exist
  if (kb0 >= KB) return;       // a key block beyond L (packed): block-uniform, before any barrier
  const int64_t rs = 3LL * H * kD, ors = static_cast<int64_t>(H) * kD;
  const uint16_t* base = qkv + sq.row0 * rs + h * kD;
  const uint16_t* obase = o + sq.row0 * ors + h * kD;
  const uint16_t* dobase = dout + sq.row0 * ors + h * kD;
  const int kw = w * 32, key = kb0 + kw + c;  // wave w owns keys [kb0 + kw, kb0 + kw + 32)
  uint16_t* krow = dqkv + (sq.row0 + key) * rs + h * kD;
  const bool kact = kb0 + kw < Lk;  // wave-uniform
  if (!kact && key < KB) {  // a fully padded key wave (padded layout): dK = dV = 0, dqkv is not pre-zeroed
#pragma unroll
    for (int t = 1; t < 3; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<u16x4*>(krow + t * H * kD + 8 * j + 4 * hl) = u16x4{0, 0, 0, 0};
  }
  if (kb0 >= Lk) return;  // the whole block is padding: block-uniform, before any barrier
  const int nkb = min(4, (Lk - kb0 + 31) >> 5);
  const bool part = kb0 + kC > Lk;
  const float k2 = scale * kLog2e;
  f32x16 dv[2], dk[2];
  zero(dv[0]);
  zero(dv[1]);
  zero(dk[0]);
  zero(dk[1]);
  for (int qb0 = 0; qb0 < Lq; qb0 += kC) {
    const int ql = kw + c, q = qb0 + ql;  // wave w owns queries [qb0 + kw, qb0 + kw + 32) of the tile
    const bool act = qb0 + kw < Lq;       // wave-uniform
    const bool live = q < Lq;
    // this lane's O / dO row halves and the row's log-sum-exp, before the staging
    const int qq = min(q, Lq - 1);
    u16x8 orow[4], drow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      orow[j] = *reinterpret_cast<const u16x8*>(obase + static_cast<int64_t>(qq) * ors + 32 * hl + 8 * j);
      drow[j] = *reinterpret_cast<const u16x8*>(dobase + static_cast<int64_t>(qq) * ors + 32 * hl + 8 * j);
    }
    const float l2 = lse[sq.lse0 + qq] * kLog2e;
    if (qb0) __syncthreads();  // the previous tile step has read Qs, dOs and T out
    if (qb0 == 0) {
      uint16_t* const tt[3] = {Qs, Ks, dOs};
      const uint16_t* const ss[3] = {base, base + H * kD + kb0 * rs, dobase};
      const int64_t rr[3] = {rs, rs, ors};
      const int nr[3] = {Lq, Lk - kb0, Lq};
      stage<3>(tt, ss, rr, nr);
    } else {
      uint16_t* const tt[2] = {Qs, dOs};
      const uint16_t* const ss[2] = {base + qb0 * rs, dobase + qb0 * ors};
      const int64_t rr[2] = {rs, ors};
      const int nr[2] = {Lq - qb0, Lq - qb0};
      stage<2>(tt, ss, rr, nr);
    }
    __syncthreads();
    float dd = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) dd += bf16_to_f32(orow[j][e]) * bf16_to_f32(drow[j][e]);
    dd = xhalf_sum(dd);
    f32x16 pt[4], ds[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      zero(pt[kb]);
      zero(ds[kb]);
    }
    if (act) {
      // S^T = K Q^T and dP^T = V dO^T for this wave's 32 queries
      bf16x8_t qf[4], of[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        qf[s] = frag<64>(Qs, ql, 2 * s + hl);
        of[s] = frag<64>(dOs, ql, 2 * s + hl);
      }
      const uint32_t rowbase = (static_cast<uint32_t>(bh) * S + q) * S;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        if (kb >= nkb) continue;  // a skipped block: pt and ds stay zeros, no hash
        // row Lk is not this sequence's key: clamped, its values are selected away below
        const int vr = min(kb0 + kb * 32 + c, Lk - 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          pt[kb] = mma(frag<64>(Ks, kb * 32 + c, 2 * s + hl), qf[s], pt[kb]);
          const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(base + 2 * H * kD + vr * rs + 16 * s + 8 * hl);
          ds[kb] = mma(vf, of[s], ds[kb]);
        }
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const int k = key_of(kb0 + kb * 32, e, hl);
          uint32_t hh = 0;
          if constexpr (DROP) hh = pair_hash(seed, (rowbase + k) >> 1);
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            // pad keys: p = exp2(-huge) = 0 exactly, and dp = 0 whatever the V row holds
            const bool ok = !part || k + u < Lk;
            const float p = fast_exp2((ok ? pt[kb][e + u] : kMasked) * k2 - l2);
            float dp = ok ? ds[kb][e + u] : 0.f;
            float pd = p;
            if constexpr (DROP) {
              const bool kp = u ? keep_hi(hh, thr) : keep_lo(hh, thr);
              pd = kp ? p * rkeep : 0.f;
              dp = kp ? dp * rkeep : 0.f;
            }
            ds[kb][e + u] = p * (dp - dd);
            pt[kb][e + u] = pd;
          }
        }
      }
    }
    // -> T[query][key]: a lane's 4 consecutive keys of its query row per 8-B store; the row of a query at
    // or beyond Lq (an idle wave's, or a lane that computed on the clamped row) is zeros
    auto put = [&](const f32x16 (&v)[4]) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const u16x4 x = live ? u16x4{f32_to_bf16(v[kb][4 * g]), f32_to_bf16(v[kb][4 * g + 1]),
                                       f32_to_bf16(v[kb][4 * g + 2]), f32_to_bf16(v[kb][4 * g + 3])}
                               : u16x4{0, 0, 0, 0};
          *reinterpret_cast<u16x4*>(T + off<128>(ql, kb * 32 + 8 * g + 4 * hl)) = x;
        }
    };
    const int nqs = min(8, (Lq - qb0 + 15) >> 4);  // 16-query steps that hold a query
    put(pt);
    __syncthreads();
    if (kact) {
      // dV^T[d][key] += sum_q dO^T[d][q] P_drop[q][key]
      for (int s = 0; s < nqs; ++s) {
        const bf16x8_t pb = tfrag<128>(T, s, kw, lane);
#pragma unroll
        for (int db = 0; db < 2; ++db) dv[db] = mma(tfrag<64>(dOs, s, db * 32, lane), pb, dv[db]);
      }
    }
    __syncthreads();  // P_drop read out
    put(ds);
    __syncthreads();
    if (kact) {
      // dK^T[d][key] += sum_q Q^T[d][q] dS[q][key]
      for (int s = 0; s < nqs; ++s) {
        const bf16x8_t sb = tfrag<128>(T, s, kw, lane);
#pragma unroll
        for (int db = 0; db < 2; ++db) dk[db] = mma(tfrag<64>(Qs, s, db * 32, lane), sb, dk[db]);
      }
    }
  }
  if (!kact || key >= KB) return;  // (packed: there is no row L to store)
  store_row(dv, krow + 2 * H * kD, 1.f, hl);
  store_row(dk, krow + H * kD, scale, hl);
}

struct Drop {
  uint32_t thr;
  float rkeep;
};
Drop drop_of(float p) {
  const uint32_t thr = static_cast<uint32_t>(static_cast<double>(p) * 65536.0 + 0.5);
  return {thr, thr > 0 ? static_cast<float>(65536.0 / (65536.0 - thr)) : 1.f};  // 1 / (1 - p_eff)
}

}  // namespace

// klen / cu as launch_attn_fwd; S % 32 == 0, 32 <= S <= 512
void launch_attn_long_fwd(const uint16_t* qkv, uint16_t* out, float* lse, int B, int S, int H, float scale, float p,
                          uint64_t seed, hipStream_t s, const int32_t* klen, const int32_t* cu, int T) {
  const Drop d = drop_of(p);
  const dim3 grid(B * H, (S + kC - 1) / kC);
  auto* k = p > 0.f ? attn_long_fwd_kernel<true> : attn_long_fwd_kernel<false>;
  hipLaunchKernelGGL(k, grid, dim3(256), 0, s, qkv, out, lse, S, H, scale, seed, d.thr, d.rkeep, klen, cu, T);
}

void launch_attn_long_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse,
                          uint16_t* dqkv, int B, int S, int H, float scale, float p, uint64_t seed, hipStream_t s,
                          const int32_t* klen, const int32_t* cu, int T) {
  const Drop d = drop_of(p);
  const dim3 grid(B * H, (S + kC - 1) / kC);
  auto* kq = p > 0.f ? attn_long_dq_kernel<true> : attn_long_dq_kernel<false>;
  auto* kk = p > 0.f ? attn_long_dkv_kernel<true> : attn_long_dkv_kernel<false>;
  hipLaunchKernelGGL(kq, grid, dim3(256), 0, s, qkv, out, dout, lse, dqkv, S, H, scale, seed, d.thr, d.rkeep, klen, cu,
                     T);
  hipLaunchKernelGGL(kk, grid, dim3(256), 0, s, qkv, out, dout, lse, dqkv, S, H, scale, seed, d.thr, d.rkeep, klen, cu,
                     T);
}

}  // namespace psamd
