// Mixture-of-experts router: a skinny bf16 MFMA GEMM whose epilogue finishes the routing, the fold of its loss
// statistics, and the softmax / top-k / auxiliary-loss gradient.
//
//   moe_router_fwd     z = h Wr^T (h [T, D], Wr [E, D], E <= 128) in fp32, never rounded; per row: lse, the k experts
//                      of largest z in descending order (a tie goes to the lower id), their probabilities
//                      (renormalised over the k when asked), the fp32 logits for the backward; per block: how often
//                      each expert was chosen, the sum of each expert's probability and the sum of lse^2 over the
//                      block's rows -- one row [counts E | psum E | lse^2] of `part`.
//   moe_router_finish  one block: the partial rows folded in a fixed order (sixteen runs of consecutive rows, each in
//                      index order, then the sixteen sums in order) -> counts [E] (int32), psum [E],
//                      lb = E sum_e (counts_e / (T k)) (psum_e / T), zl = sum lse^2 / T, aux = aux_coef lb + z_coef zl.
//   moe_router_bwd     one wave per row: dz = p (g - <p, g>) + daux z_coef (2 lse / T) p, where g holds the top-k
//                      weights' gradient on the chosen columns (through the renormalisation when it was applied)
//                      plus daux aux_coef E f_e / T on every column; one rounding to bf16.
//   sigmoid form       (DeepSeek-V3 style) the forward's SIG epilogue and moe_router_sigmoid_bwd: scores sigmoid(z), the
//                      k experts of largest score + bias inside the topk_group best of n_group expert groups (group
//                      score: its two largest score + bias summed), weights the unbiased scores (renormalised when
//                      asked) times a scale; psum sums score / row sum of scores.  Same partial rows, same finish.
//
// Forward design.  The problem streams h once from HBM; Wr (at most 1 MB) stays in every XCD's L2, so the block
// order is the plain walk along the rows.  A block owns TM token rows (32 or 64) and ALL columns, padded inside the
// kernel to EP = 32 NB (weight rows >= E and token rows >= T are staged as zeros without a load).  256 threads =
// 4 waves that share the K stage of 64: wave w multiplies the 16-wide k step w of every stage for the whole
// TM x EP tile ((TM / 32) x NB v_mfma_f32_32x32x16_bf16, weights as "A": a lane ends with 4-column groups of one
// token row), so every operand fragment is read from LDS once per block.  Operands move global -> registers into
// the double-buffered chunk-swizzled LDS stages of psamd_gemm_tile.h's kernels, but FOUR stages ahead (a register
// ring): a stage holds few MFMAs per wave and 16384 tokens make two blocks per CU, so there is little else to hide a
// stage's loads behind (measured: 2 to 8 % less time than one stage ahead, profiles/moe_router_probe.txt).  After the K loop
// the stages are free: the four waves' fp32 partial tiles are added into a [TM][EP + 4] fp32 tile on top of them,
// wave 0 first, then 1, 2, 3 -- a fixed order.  Then each wave takes whole rows, a lane holding columns lane and
// lane + 64: row max and sum-exp by cross-lane reduce, the top-k as k rounds of a max-reduce over
// (ordered value bits, ~column) 64-bit keys with the winner retired.  Columns >= E take part in nothing.
// No atomics anywhere: every output element has one writer and every sum a fixed order, so two calls are bitwise
// equal, and a row's results do not depend on the other rows.
#include "psamd_device.h"
#include "psamd_gemm_tile.h"
#include "psamd_launch.h"
#include "psamd_mfma.h"

namespace psamd {
namespace {

using namespace mfma;
using tile::kNT;
using tile::kTK;
using tile::load_row8;

constexpr int kFoldLd = 4 * 64 + 1;  // a wave's partials: counts of columns lane, lane + 64; psums likewise; lse^2
constexpr int kFinishNT = 1024;      // threads of the finish block
constexpr int kRouterAhead = 4;      // K stages a thread keeps in flight in registers
static_assert(kRouterAhead % 2 == 0, "the LDS buffer of a stage is its ring position's parity");

// float -> bits whose unsigned order is the float order, every NaN on top (torch.sort's order), -0 as +0
__device__ __forceinline__ uint32_t ordered_bits(float z) {
  if (z != z) return 0xffffffffu;
  if (z == 0.f) z = 0.f;
  const uint32_t b = __float_as_uint(z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ float sigmoid(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), off, kWave);
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), off, kWave);
    const unsigned long long o = (static_cast<unsigned long long>(hi) << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

template <int TM, int NB>
struct RouterTile {
  static constexpr int EP = 32 * NB, MB = TM / 32, LD = EP + 4;
  static constexpr int kA = TM * kTK, kB = EP * kTK;  // elements of one operand stage
  static constexpr int kOpBytes = 2 * (kA + kB) * 2, kTileBytes = TM * LD * 4;
  static constexpr int kBytes = kOpBytes > kTileBytes ? kOpBytes : kTileBytes;
  static_assert(4 * kFoldLd * 4 <= kBytes, "the waves' partials lie on top of the tile");
};

// ------------------------------------------------------------------------------------------ forward
// SIG: the sigmoid epilogue (scores sigmoid(z), selection on score + bias, group-limited, weights times `scale`);
// the softmax instantiations read none of bias, n_group, topk_group and scale.
template <int TM, int NB, bool SIG>
__global__ __launch_bounds__(kNT) void moe_router_fwd_kernel(const uint16_t* __restrict__ h, const uint16_t* __restrict__ w,
                                                             int T, int E, int D, int k, int norm,
                                                             int64_t* __restrict__ idx, float* __restrict__ wts,
                                                             float* __restrict__ lse, float* __restrict__ logits,
                                                             float* __restrict__ part, const float* __restrict__ bias,
                                                             int n_group, int topk_group, float scale) {
  using RT = RouterTile<TM, NB>;
  constexpr int MB = RT::MB, LD = RT::LD, kA = RT::kA, kB = RT::kB;
  __shared__ __attribute__((aligned(16))) unsigned char raw[RT::kBytes];  // As[2] | Bs[2]; then the fp32 tile
  uint16_t* As = reinterpret_cast<uint16_t*>(raw);
  uint16_t* Bs = As + 2 * kA;
  float* L = reinterpret_cast<float*>(raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * TM;

  // both operands: thread = 16-B chunk ca of stage rows ra + 32 i
  const int ca = tid & 7, ra = tid >> 3;
  int tok[MB], wrow[NB];
#pragma unroll
  for (int i = 0; i < MB; ++i) tok[i] = r0 + ra + 32 * i < T ? r0 + ra + 32 * i : -1;
#pragma unroll
  for (int j = 0; j < NB; ++j) wrow[j] = ra + 32 * j < E ? ra + 32 * j : -1;
  struct Stage {
    u16x8 a[MB], b[NB];
  };
  Stage ring[kRouterAhead];  // stage kt travels in ring[kt % kRouterAhead]
  auto load = [&](Stage& s, int kt) {
    const int k0 = kt * kTK + ca * 8;
#pragma unroll
    for (int i = 0; i < MB; ++i) s.a[i] = load_row8(h, D, tok[i], k0, true);
#pragma unroll
    for (int j = 0; j < NB; ++j) s.b[j] = load_row8(w, D, wrow[j], k0, true);
  };
  auto store = [&](const Stage& s, int buf) {
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      const int r = ra + 32 * i;
      *reinterpret_cast<u16x8*>(As + buf * kA + r * 64 + ((ca ^ sw<64>(r)) << 3)) = s.a[i];
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int r = ra + 32 * j;
      *reinterpret_cast<u16x8*>(Bs + buf * kB + r * 64 + ((ca ^ sw<64>(r)) << 3)) = s.b[j];
    }
  };

  f32x16 acc[MB][NB];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) zero(acc[i][j]);

  const int nk = D / kTK, ch = 2 * wave + (lane >> 5);  // this wave's k step of every stage
#pragma unroll
  for (int p = 0; p < kRouterAhead; ++p)
    if (p < nk) load(ring[p], p);
  store(ring[0], 0);
  if (kRouterAhead < nk) load(ring[0], kRouterAhead);
  __syncthreads();
  // unrolled by the ring's length, so that every ring index is a constant and the ring stays in registers
  for (int kt0 = 0; kt0 < nk; kt0 += kRouterAhead) {
#pragma unroll
    for (int p = 0; p < kRouterAhead; ++p) {
      const int kt = kt0 + p, buf = p & 1;
      if (kt < nk) {  // block-uniform
        bf16x8_t af[MB], bf[NB];
#pragma unroll
        for (int i = 0; i < MB; ++i) af[i] = frag<64>(As + buf * kA, 32 * i + (lane & 31), ch);
#pragma unroll
        for (int j = 0; j < NB; ++j) bf[j] = frag<64>(Bs + buf * kB, 32 * j + (lane & 31), ch);
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
          for (int j = 0; j < NB; ++j) acc[i][j] = mma(bf[j], af[i], acc[i][j]);  // C^T blocks: lane = one token row
        if (kt + 1 < nk) {  // the next stage lands in LDS; its registers fetch the stage a ring's length further on
          Stage& s = ring[(p + 1) % kRouterAhead];
          store(s, buf ^ 1);
          if (kt + 1 + kRouterAhead < nk) load(s, kt + 1 + kRouterAhead);
        }
        __syncthreads();
      }
    }
  }

  // the four k-step partials -> one fp32 tile, wave 0 first: L[row][col], a lane's 4 consecutive columns as 16 B
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            f32x4* p = reinterpret_cast<f32x4*>(L + (32 * i + (lane & 31)) * LD + 32 * j + 8 * q4 + 4 * (lane >> 5));
            const f32x16& a = acc[i][j];
            f32x4 v = {a[4 * q4], a[4 * q4 + 1], a[4 * q4 + 2], a[4 * q4 + 3]};
            if (wv) v += *p;
            *p = v;
          }
    }
    __syncthreads();
  }

  // rows wave, wave + 4, ...: a lane holds columns lane and lane + 64
  const bool v0 = lane < E, v1 = lane + 64 < E;
  float cnt0 = 0.f, cnt1 = 0.f, ps0 = 0.f, ps1 = 0.f, zsq = 0.f;
  if constexpr (SIG) {
    const int G = E / n_group;                 // a group: G consecutive columns
    const bool grouped = n_group > topk_group;  // otherwise every group is kept: no group step
    const float bi0 = v0 && bias ? bias[lane] : 0.f, bi1 = v1 && bias ? bias[lane + 64] : 0.f;
    const int grp0 = lane / G, grp1 = (lane + 64) / G;
    for (int r = wave; r < TM; r += 4) {
      const int t = r0 + r;
      if (t >= T) break;  // wave-uniform
      float* Lr = L + r * LD;
      const float z0 = v0 ? Lr[lane] : -INFINITY, z1 = v1 ? Lr[lane + 64] : -INFINITY;
      const float m = wave_max(fmaxf(z0, z1));
      const float l = m + logf(wave_sum((v0 ? expf(z0 - m) : 0.f) + (v1 ? expf(z1 - m) : 0.f)));
      const float s0 = v0 ? sigmoid(z0) : 0.f, s1 = v1 ? sigmoid(z1) : 0.f;
      const float ssum = wave_sum(s0 + s1);
      const float c0 = s0 + bi0, c1 = s1 + bi1;  // the selection scores
      unsigned long long key0 = v0 ? (static_cast<unsigned long long>(ordered_bits(c0)) << 32) | static_cast<uint32_t>(~lane) : 0ull;
      unsigned long long key1 = v1 ? (static_cast<unsigned long long>(ordered_bits(c1)) << 32) | static_cast<uint32_t>(~(lane + 64)) : 0ull;
      if (grouped) {  // block-uniform
        // The row of the tile is this wave's alone and its logits are in registers: it takes the selection scores,
        // and lane g < n_group walks group g's run of them (any G, a run may straddle the lane / lane + 64 split)
        // for the two largest.  A wave's LDS operations complete in order: the walk sees the row's stores.
        if (v0) Lr[lane] = c0;
        if (v1) Lr[lane + 64] = c1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        unsigned long long gkey = 0ull;
        if (lane < n_group) {
          const float* cg = Lr + lane * G;  // columns lane G .. lane G + G - 1 < E
          float m1 = -INFINITY, m2 = -INFINITY;  // a NaN enters neither
#pragma unroll 4
          for (int i = 0; i < G; ++i) {
            const float c = cg[i];
            m2 = c > m1 ? m1 : (c > m2 ? c : m2);
            m1 = c > m1 ? c : m1;
          }
          gkey = (static_cast<unsigned long long>(ordered_bits(G > 1 ? m1 + m2 : m1)) << 32) | static_cast<uint32_t>(~lane);
        }
        uint32_t keep = 0u;  // bit g: group g is among the topk_group of largest score, a tie to the lower id
        for (int j = 0; j < topk_group; ++j) {
          const unsigned long long best = wave_max_u64(gkey);
          keep |= 1u << (~static_cast<uint32_t>(best) & 31u);
          if (gkey == best) gkey = 0ull;
        }
        if (v0 && !((keep >> grp0) & 1u)) key0 = 0ull;  // a dropped group's columns: key 0, like pad columns
        if (v1 && !((keep >> grp1) & 1u)) key1 = 0ull;
      }
      int my_e = 0;
      float my_s = 0.f, sel = 0.f;
      for (int j = 0; j < k; ++j) {
        const unsigned long long best = wave_max_u64(key0 > key1 ? key0 : key1);
        const int e = static_cast<int>(~static_cast<uint32_t>(best)) & 127;
        const float se = __shfl((e >> 6) ? s1 : s0, e & 63, kWave);  // the unbiased score, from its owner
        if (lane == j) {
          my_e = e;
          my_s = se;
        }
        sel += se;  // j ascending, on every lane
        if (key0 == best) {
          key0 = 0ull;
          cnt0 += 1.f;
        }
        if (key1 == best) {
          key1 = 0ull;
          cnt1 += 1.f;
        }
      }
      if (lane < k) {
        idx[static_cast<int64_t>(t) * k + lane] = my_e;
        wts[static_cast<int64_t>(t) * k + lane] = (norm ? my_s / sel : my_s) * scale;
      }
      if (lane == 0) lse[t] = l;
      if (v0) logits[static_cast<int64_t>(t) * E + lane] = z0;
      if (v1) logits[static_cast<int64_t>(t) * E + lane + 64] = z1;
      ps0 += s0 / ssum;  // DeepSeek-V3's normalised scores take the probabilities' place in the balance loss
      ps1 += s1 / ssum;
      zsq += l * l;
    }
  } else {
    for (int r = wave; r < TM; r += 4) {
      const int t = r0 + r;
      if (t >= T) break;  // wave-uniform
      const float z0 = v0 ? L[r * LD + lane] : -INFINITY, z1 = v1 ? L[r * LD + lane + 64] : -INFINITY;
      const float m = wave_max(fmaxf(z0, z1));
      const float s = wave_sum((v0 ? expf(z0 - m) : 0.f) + (v1 ? expf(z1 - m) : 0.f));
      const float l = m + logf(s);
      const float p0 = v0 ? expf(z0 - l) : 0.f, p1 = v1 ? expf(z1 - l) : 0.f;
      // a retired or pad column: key 0, below every live key (ordered bits of a live column >= 0x007fffff)
      unsigned long long key0 = v0 ? (static_cast<unsigned long long>(ordered_bits(z0)) << 32) | static_cast<uint32_t>(~lane) : 0ull;
      unsigned long long key1 = v1 ? (static_cast<unsigned long long>(ordered_bits(z1)) << 32) | static_cast<uint32_t>(~(lane + 64)) : 0ull;
      int my_e = 0;
      float my_p = 0.f, sel = 0.f;
      for (int j = 0; j < k; ++j) {
        const unsigned long long best = wave_max_u64(key0 > key1 ? key0 : key1);
        const int e = static_cast<int>(~static_cast<uint32_t>(best)) & 127;
        const float pe = expf(from_ordered_bits(static_cast<uint32_t>(best >> 32)) - l);  // the owner's p, bit for bit
        if (lane == j) {
          my_e = e;
          my_p = pe;
        }
        sel += pe;  // j ascending, on every lane
        if (key0 == best) {
          key0 = 0ull;
          cnt0 += 1.f;
        }
        if (key1 == best) {
          key1 = 0ull;
          cnt1 += 1.f;
        }
      }
      if (lane < k) {
        idx[static_cast<int64_t>(t) * k + lane] = my_e;
        wts[static_cast<int64_t>(t) * k + lane] = norm ? my_p / sel : my_p;
      }
      if (lane == 0) lse[t] = l;
      if (v0) logits[static_cast<int64_t>(t) * E + lane] = z0;
      if (v1) logits[static_cast<int64_t>(t) * E + lane + 64] = z1;
      ps0 += p0;
      ps1 += p1;
      zsq += l * l;
    }
  }
  __syncthreads();  // the tile is read: the waves' partials go on top of it

  float* F = reinterpret_cast<float*>(raw);
  F[wave * kFoldLd + lane] = cnt0;
  F[wave * kFoldLd + 64 + lane] = cnt1;
  F[wave * kFoldLd + 128 + lane] = ps0;
  F[wave * kFoldLd + 192 + lane] = ps1;
  if (lane == 0) F[wave * kFoldLd + 256] = zsq;
  __syncthreads();
  float* prow = part + static_cast<int64_t>(blockIdx.x) * (2 * E + 1);
  if (tid < E) {
    prow[tid] = ((F[tid] + F[kFoldLd + tid]) + F[2 * kFoldLd + tid]) + F[3 * kFoldLd + tid];
    prow[E + tid] = ((F[128 + tid] + F[kFoldLd + 128 + tid]) + F[2 * kFoldLd + 128 + tid]) + F[3 * kFoldLd + 128 + tid];
  }
  if (tid == 0) prow[2 * E] = ((F[256] + F[kFoldLd + 256]) + F[2 * kFoldLd + 256]) + F[3 * kFoldLd + 256];
}

// ------------------------------------------------------------------------------------------ finish
// One block of 16 waves over part [nblk, 2 E + 1].  Wave s sums the s-th sixteenth of the partial rows in index
// order, a lane holding columns lane + 64 q (one thread walking all rows alone is a chain of nblk dependent loads:
// 56 us at 512 rows, profiles/moe_router_probe.txt); then one thread per column adds the 16 sums in wave order.
// Counts are summed as integers.
__global__ __launch_bounds__(kFinishNT) void moe_router_finish_kernel(const float* __restrict__ part, int nblk, int T,
                                                                      int E, int k, float aux_coef, float z_coef,
                                                                      int* __restrict__ counts, float* __restrict__ psum,
                                                                      float* __restrict__ stats) {
  constexpr int kSeg = kFinishNT / 64;
  __shared__ float seg[kSeg][2 * kMoeMaxExperts];  // count columns as integer bits
  __shared__ float col[2 * kMoeMaxExperts];
  __shared__ float red[kSeg];
  const int tid = threadIdx.x, lane = tid & 63, sg = tid >> 6, S = 2 * E + 1;
  const int per = (nblk + kSeg - 1) / kSeg, b0 = sg * per, b1 = min(nblk, b0 + per);
  float fa[4] = {0.f, 0.f, 0.f, 0.f};
  int ia[4] = {0, 0, 0, 0};
#pragma unroll 4
  for (int b = b0; b < b1; ++b) {
    const float* row = part + static_cast<int64_t>(b) * S;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = lane + 64 * q;
      const float v = c < 2 * E ? row[c] : 0.f;
      fa[q] += v;
      ia[q] += static_cast<int>(v);  // a count column: exact, <= 64 a block
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) seg[sg][lane + 64 * q] = lane + 64 * q < E ? __int_as_float(ia[q]) : fa[q];
  __syncthreads();
  if (tid < E) {
    int c = 0;
    for (int s = 0; s < kSeg; ++s) c += __float_as_int(seg[s][tid]);
    counts[tid] = c;
    col[tid] = static_cast<float>(c);
  } else if (tid < 2 * E) {
    float s = 0.f;
    for (int i = 0; i < kSeg; ++i) s += seg[i][tid];
    psum[tid - E] = s;
    col[tid] = s;
  }
  __syncthreads();
  const float fp = block_sum(tid < E ? col[tid] * col[E + tid] : 0.f, red);
  float z = 0.f;
  for (int b = tid; b < nblk; b += kFinishNT) z += part[static_cast<int64_t>(b) * S + 2 * E];
  const float zs = block_sum(z, red);
  if (tid == 0) {
    const float lb = static_cast<float>(E) * fp / (static_cast<float>(T) * static_cast<float>(k)) / static_cast<float>(T);
    const float zl = zs / static_cast<float>(T);
    stats[0] = lb;
    stats[1] = zl;
    stats[2] = aux_coef * lb + z_coef * zl;
  }
}

// ------------------------------------------------------------------------------------------ backward
__global__ __launch_bounds__(kNT) void moe_router_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ lse,
                                                             const int64_t* __restrict__ idx, const float* __restrict__ wts,
                                                             const float* __restrict__ dwts, const float* __restrict__ daux,
                                                             const int* __restrict__ counts, int T, int E, int k, int norm,
                                                             float aux_coef, float z_coef, uint16_t* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const bool v0 = lane < E, v1 = lane + 64 < E;
  const float da = daux[0], fT = static_cast<float>(T);
  // the balance term of a column: daux aux_coef E f_e / T with f_e = counts_e / (T k)
  const float bal = da * aux_coef * static_cast<float>(E) / (fT * static_cast<float>(k)) / fT;
  const float b0 = v0 ? bal * static_cast<float>(counts[lane]) : 0.f;
  const float b1 = v1 ? bal * static_cast<float>(counts[lane + 64]) : 0.f;
  const float zc = da * z_coef * 2.f / fT;
  const int64_t nw = static_cast<int64_t>(gridDim.x) * (kNT / 64);
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * (kNT / 64) + (threadIdx.x >> 6); t < T; t += nw) {
    const float* zr = logits + t * E;
    const float l = lse[t];
    const float p0 = v0 ? expf(zr[lane] - l) : 0.f, p1 = v1 ? expf(zr[lane + 64] - l) : 0.f;
    int e = -1;  // lane j < k: slot j of the row
    float dw = 0.f, wj = 0.f, pj = 0.f;
    if (lane < k) {
      const int64_t ev = idx[t * k + lane];
      e = (ev >= 0 && ev < E) ? static_cast<int>(ev) : -1;  // an id off [0, E) never becomes an index
      dw = dwts[t * k + lane];
      wj = wts[t * k + lane];
      if (e >= 0) pj = expf(zr[e] - l);
    }
    float gs = dw;
    if (norm) {  // wts = p_sel / s: d p_sel = (dwts - <dwts, wts>) / s
      const float dot = wave_sum(dw * wj), s = wave_sum(pj);
      gs = (dw - dot) / s;
    }
    float g0 = b0, g1 = b1;
    for (int j = 0; j < k; ++j) {
      const int ej = __shfl(e, j, kWave);
      const float gj = __shfl(gs, j, kWave);
      if (ej >= 0 && lane == (ej & 63)) {
        if (ej >> 6) g1 += gj;
        else g0 += gj;
      }
    }
    const float inner = wave_sum(p0 * g0 + p1 * g1);
    if (v0) dz[t * E + lane] = f32_to_bf16(p0 * (g0 - inner) + zc * l * p0);
    if (v1) dz[t * E + lane + 64] = f32_to_bf16(p1 * (g1 - inner) + zc * l * p1);
  }
}

// The sigmoid form, one wave per row.  s = sigmoid(z), S = sum_e s_e, n = s / S and p = softmax(z) are recomputed
// from the saved logits and lse; g_j, the gradient of s on the chosen slot j, is dwts_j scale (through the
// renormalisation: (dwts_j scale - <dwts, wts>) / sum s_sel); b_e = daux aux_coef E f_e / T acts through n:
// ds_e = g_e + (b_e - <n, b>) / S, dz_e = ds_e s_e (1 - s_e) + daux z_coef (2 lse / T) p_e; one rounding to bf16.
__global__ __launch_bounds__(kNT) void moe_router_sigmoid_bwd_kernel(
    const float* __restrict__ logits, const float* __restrict__ lse, const int64_t* __restrict__ idx,
    const float* __restrict__ wts, const float* __restrict__ dwts, const float* __restrict__ daux,
    const int* __restrict__ counts, int T, int E, int k, int norm, float aux_coef, float z_coef, float scale,
    uint16_t* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const bool v0 = lane < E, v1 = lane + 64 < E;
  const float da = daux[0], fT = static_cast<float>(T);
  const float bal = da * aux_coef * static_cast<float>(E) / (fT * static_cast<float>(k)) / fT;
  const float b0 = v0 ? bal * static_cast<float>(counts[lane]) : 0.f;
  const float b1 = v1 ? bal * static_cast<float>(counts[lane + 64]) : 0.f;
  const float zc = da * z_coef * 2.f / fT;
  const int64_t nw = static_cast<int64_t>(gridDim.x) * (kNT / 64);
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * (kNT / 64) + (threadIdx.x >> 6); t < T; t += nw) {
    const float* zr = logits + t * E;
    const float l = lse[t];
    const float z0 = v0 ? zr[lane] : 0.f, z1 = v1 ? zr[lane + 64] : 0.f;
    const float p0 = v0 ? expf(z0 - l) : 0.f, p1 = v1 ? expf(z1 - l) : 0.f;
    const float s0 = v0 ? sigmoid(z0) : 0.f, s1 = v1 ? sigmoid(z1) : 0.f;
    const float ssum = wave_sum(s0 + s1);
    int e = -1;  // lane j < k: slot j of the row
    float dw = 0.f, wj = 0.f, sj = 0.f;
    if (lane < k) {
      const int64_t ev = idx[t * k + lane];
      e = (ev >= 0 && ev < E) ? static_cast<int>(ev) : -1;  // an id off [0, E) never becomes an index
      dw = dwts[t * k + lane];
      wj = wts[t * k + lane];
      if (e >= 0) sj = sigmoid(zr[e]);
    }
    float gs = dw * scale;
    if (norm) {  // wts = scale s_sel / sum s_sel
      const float dot = wave_sum(dw * wj), sel = wave_sum(sj);
      gs = (dw * scale - dot) / sel;
    }
    float g0 = 0.f, g1 = 0.f;
    for (int j = 0; j < k; ++j) {
      const int ej = __shfl(e, j, kWave);
      const float gj = __shfl(gs, j, kWave);
      if (ej >= 0 && lane == (ej & 63)) {
        if (ej >> 6) g1 += gj;
        else g0 += gj;
      }
    }
    const float nb = wave_sum(s0 * b0 + s1 * b1) / ssum;  // <n, b>
    const float ds0 = g0 + (b0 - nb) / ssum, ds1 = g1 + (b1 - nb) / ssum;
    if (v0) dz[t * E + lane] = f32_to_bf16(ds0 * s0 * (1.f - s0) + zc * l * p0);
    if (v1) dz[t * E + lane + 64] = f32_to_bf16(ds1 * s1 * (1.f - s1) + zc * l * p1);
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------ launches
// The row tile when the caller leaves it open: 32.  At 16384 tokens it took 0.69 to 0.91 of the 64-row tile's time
// on all three probed shapes (profiles/moe_router_probe.txt): twice the blocks, and two to three of them on a CU.
// The 64-row tile stays selectable so that the probe can repeat that comparison; the op never asks for it.
static int router_row_tile(int row_tile) { return row_tile > 0 ? row_tile : 32; }

int moe_router_blocks(int T, int row_tile) {
  const int tm = router_row_tile(row_tile);
  return (T + tm - 1) / tm;
}

void launch_moe_router_fwd(const uint16_t* h, const uint16_t* w, int T, int E, int D, int k, bool norm, int row_tile,
                           int64_t* idx, float* wts, float* lse, float* logits, float* part, bool sigmoid,
                           const float* bias, int n_group, int topk_group, float scale, hipStream_t st) {
  const int tm = router_row_tile(row_tile), nb = (E + 31) / 32;
  const dim3 grid(moe_router_blocks(T, row_tile)), block(kNT);
#define PSAMD_ROUTER(TMV, NBV, SIGV)                                                                               \
  hipLaunchKernelGGL((moe_router_fwd_kernel<TMV, NBV, SIGV>), grid, block, 0, st, h, w, T, E, D, k, norm ? 1 : 0, idx, \
                     wts, lse, logits, part, bias, n_group, topk_group, scale)
#define PSAMD_ROUTER_NB(TMV, SIGV)             \
  switch (nb) {                                \
    case 1: PSAMD_ROUTER(TMV, 1, SIGV); break; \
    case 2: PSAMD_ROUTER(TMV, 2, SIGV); break; \
    case 3: PSAMD_ROUTER(TMV, 3, SIGV); break; \
    default: PSAMD_ROUTER(TMV, 4, SIGV); break; \
  }
  if (sigmoid) {  // the 32-row tile only: the 64-row tile is the softmax probe's comparison
    PSAMD_ROUTER_NB(32, true)
  } else if (tm == 64) {
    PSAMD_ROUTER_NB(64, false)
  } else {
    PSAMD_ROUTER_NB(32, false)
  }
#undef PSAMD_ROUTER_NB
#undef PSAMD_ROUTER
}

void launch_moe_router_finish(const float* part, int nblk, int T, int E, int k, float aux_coef, float z_coef, int* counts,
                              float* psum, float* stats, hipStream_t st) {
  hipLaunchKernelGGL(moe_router_finish_kernel, dim3(1), dim3(kFinishNT), 0, st, part, nblk, T, E, k, aux_coef, z_coef, counts,
                     psum, stats);
}

void launch_moe_router_bwd(const float* logits, const float* lse, const int64_t* idx, const float* wts, const float* dwts,
                           const float* daux, const int* counts, int T, int E, int k, bool norm, float aux_coef,
                           float z_coef, bool sigmoid, float scale, uint16_t* dz, hipStream_t st) {
  if (sigmoid) {
    hipLaunchKernelGGL(moe_router_sigmoid_bwd_kernel, dim3(stream_grid(static_cast<int64_t>(T) * 64, kNT)), dim3(kNT), 0,
                       st, logits, lse, idx, wts, dwts, daux, counts, T, E, k, norm ? 1 : 0, aux_coef, z_coef, scale, dz);
    return;
  }
  hipLaunchKernelGGL(moe_router_bwd_kernel, dim3(stream_grid(static_cast<int64_t>(T) * 64, kNT)), dim3(kNT), 0, st,
                     logits, lse, idx, wts, dwts, daux, counts, T, E, k, norm ? 1 : 0, aux_coef, z_coef, dz);
}

}  // namespace psamd
