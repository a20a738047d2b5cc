// Per-head QK RMSNorm fused into RoPE + head split + transpose (Qwen3 / OLMo-2 / Gemma-3 style blocks):
//
//   rope_norm_split   q, k = RoPE(RMSNorm_head(q | k) * w),  v copied
//
// qkv: [B, S, NH, hd] bf16 with NH = H + 2 KV (the fused QKV GEMM output); cs: [S, hd/2, 2] fp32 (cos, sin);
// wq, wk: [hd] (WT = float or bf16), one weight for all query heads and one for all key heads.
// q: [B, H, S, hd], k / v: [B, KV, S, hd].  Per head row x of the first H + KV heads
//   xhat = x * rsqrt(mean(x^2) + eps),  y = xhat * w,  (y1, y2) -> (y1 c - y2 s, y2 c + y1 s)
// in fp32 with one rounding to bf16 at the store; nothing is saved for backward (rstd is recomputed there).
//
// Work split.  A lane owns 8 dims of the first half of a head row and their 8 rotation partners (the lane
// layout of rope_split), so a head row is hd / 16 adjacent lanes (8 at hd 128, 4 at hd 64) and its sums are
// 3 or 2 DPP steps inside that group: no LDS and no barrier on the row path.  A 256-thread block holds
// UB = 4096 / hd head rows per step; the grid is a multiple of NH / gcd(NH, UB) blocks, which makes the
// grid stride (gridDim.x * UB head rows) a multiple of NH: a lane keeps its head index -- its role (q, k or
// v), its output tensor and its 16 weight values -- for the whole loop and only its token advances.  That is
// what lets the backward keep the weight gradient of its 16 columns in registers across all its rows.
//
// Weight gradients are deterministic (no atomics): after the loop a block puts its lanes' register sums into
// an LDS tile [UB, hd], 2 hd threads add the head rows of equal role in slot order and write one fp32 partial
// row [2, hd] per block; colsum2 (transformer.hip) sums the partial rows in two fixed-order launches.
#include "psamd_device.h"
#include "psamd_launch.h"

namespace psamd {

namespace {
constexpr int kT = 256;

template <int CTRL>
__device__ __forceinline__ float dpp_read(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// Sum over the aligned group of LANES (4 or 8) adjacent lanes that holds one head row; every lane of the
// group gets the same bits (each step adds the same two values in both lanes of a pair).  Sources stay
// inside the group, and a group is active or idle as a whole.
template <int LANES>
__device__ __forceinline__ float head_sum(float v) {
  v += dpp_read<0xB1>(v);                            // quad_perm [1, 0, 3, 2]: lane ^ 1
  v += dpp_read<0x4E>(v);                            // quad_perm [2, 3, 0, 1]: lane ^ 2
  if constexpr (LANES == 8) v += dpp_read<0x141>(v);  // row_half_mirror: the other quad of the 8 (quads are uniform by now)
  return v;
}

// What a lane keeps for the whole grid-stride loop.
template <int HD>
struct Lane {
  static constexpr int HV = HD / 16;  // lanes per head row
  static constexpr int UB = kT / HV;  // head rows per block and step
  int c;      // first of the lane's 8 dims in the first half; partners at HD / 2 + c
  int hh;     // head index in qkv's NH
  int role;   // 0 q, 1 k, 2 v
  int hr, HR;  // head index in, and head count of, the role's own tensor
  int dt;     // the lane's token minus the block's first token
  int tb0, tstep;

  __device__ __forceinline__ Lane(int H, int KV) {
    const int NH = H + 2 * KV, slot = threadIdx.x / HV, base = blockIdx.x * UB;
    c = (threadIdx.x % HV) * 8;
    hh = (base + slot) % NH;
    role = hh < H ? 0 : hh < H + KV ? 1 : 2;
    hr = role == 0 ? hh : role == 1 ? hh - H : hh - H - KV;
    HR = role == 0 ? H : KV;
    tb0 = base / NH;
    dt = (base + slot) / NH - tb0;
    tstep = gridDim.x * UB / NH;  // exact: the launcher's grid makes gridDim.x * UB a multiple of NH
  }
};

template <typename WT>
__device__ __forceinline__ void lane_weights(const WT* wq, const WT* wk, int role, int c, int half, float (&w1)[8],
                                             float (&w2)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) w1[j] = w2[j] = 1.f;
  if (role < 2) {
    const WT* w = role == 0 ? wq : wk;
    load8(w, c, w1);
    load8(w, half + c, w2);
  }
}
}  // namespace

// T = B * S tokens.  The loop bound is uniform over the block (tb: the block's first token of the step), so
// every lane reaches the DPP sums; a lane past the last token loads and stores nothing.
template <int HD, typename WT>
__global__ __launch_bounds__(kT) void rope_norm_split_fwd_kernel(const uint16_t* __restrict__ qkv,
                                                                 const float* __restrict__ cs,
                                                                 const WT* __restrict__ wq, const WT* __restrict__ wk,
                                                                 uint16_t* __restrict__ q, uint16_t* __restrict__ k,
                                                                 uint16_t* __restrict__ v, int T, int S, int H, int KV,
                                                                 float eps) {
  constexpr int HALF = HD / 2;
  const Lane<HD> ln(H, KV);
  const int NH = H + 2 * KV;
  float w1[8], w2[8];
  lane_weights(wq, wk, ln.role, ln.c, HALF, w1, w2);
  uint16_t* const out = ln.role == 0 ? q : ln.role == 1 ? k : v;
  for (int tb = ln.tb0; tb < T; tb += ln.tstep) {
    const int t = tb + ln.dt;
    const bool act = t < T;
    const int b = t / S, s = t - b * S;
    float x1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, x2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) {
      const uint16_t* src = qkv + (static_cast<int64_t>(t) * NH + ln.hh) * HD;
      load8(src, ln.c, x1);
      load8(src, HALF + ln.c, x2);
    }
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += x1[j] * x1[j] + x2[j] * x2[j];
    const float rs = rsqrtf(head_sum<Lane<HD>::HV>(ss) * (1.f / HD) + eps);
    if (act) {
      if (ln.role < 2) {
        float c0[8], c1[8];  // (cos, sin) of the lane's dims 0..3 and 4..7
        const float* cp = cs + (static_cast<int64_t>(s) * HALF + ln.c) * 2;
        load8(cp, 0, c0);
        load8(cp, 8, c1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float co = j < 4 ? c0[2 * j] : c1[2 * j - 8], si = j < 4 ? c0[2 * j + 1] : c1[2 * j - 7];
          const float a = x1[j] * rs * w1[j], bb = x2[j] * rs * w2[j];
          x1[j] = a * co - bb * si;
          x2[j] = bb * co + a * si;
        }
      }
      uint16_t* dst = out + ((static_cast<int64_t>(b) * ln.HR + ln.hr) * S + s) * HD;
      store8(dst, ln.c, x1);
      store8(dst, HALF + ln.c, x2);
    }
  }
}

// dx = rstd * (g * w - xhat * mean(g * w * xhat)) with g = RoPE^T(dy); dw += g * xhat; dv copied.
// part: [gridDim.x, 2, HD] fp32, the block's (dwq | dwk) partial row.
template <int HD, typename WT>
__global__ __launch_bounds__(kT) void rope_norm_split_bwd_kernel(const uint16_t* __restrict__ dq,
                                                                 const uint16_t* __restrict__ dk,
                                                                 const uint16_t* __restrict__ dv,
                                                                 const uint16_t* __restrict__ qkv,
                                                                 const float* __restrict__ cs,
                                                                 const WT* __restrict__ wq, const WT* __restrict__ wk,
                                                                 uint16_t* __restrict__ dqkv, float* __restrict__ part,
                                                                 int T, int S, int H, int KV, float eps) {
  constexpr int HALF = HD / 2, UB = Lane<HD>::UB;
  const Lane<HD> ln(H, KV);
  const int NH = H + 2 * KV;
  float w1[8], w2[8];
  lane_weights(wq, wk, ln.role, ln.c, HALF, w1, w2);
  const uint16_t* const in = ln.role == 0 ? dq : ln.role == 1 ? dk : dv;
  float a1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int tb = ln.tb0; tb < T; tb += ln.tstep) {
    const int t = tb + ln.dt;
    const bool act = t < T;
    const bool qk = act && ln.role < 2;
    const int b = t / S, s = t - b * S;
    const int64_t xo = (static_cast<int64_t>(t) * NH + ln.hh) * HD;
    float g1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, g2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float x1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, x2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) {
      const uint16_t* src = in + ((static_cast<int64_t>(b) * ln.HR + ln.hr) * S + s) * HD;
      load8(src, ln.c, g1);
      load8(src, HALF + ln.c, g2);
    }
    if (qk) {
      load8(qkv + xo, ln.c, x1);
      load8(qkv + xo, HALF + ln.c, x2);
      float c0[8], c1[8];
      const float* cp = cs + (static_cast<int64_t>(s) * HALF + ln.c) * 2;
      load8(cp, 0, c0);
      load8(cp, 8, c1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {  // transpose of the rotation
        const float co = j < 4 ? c0[2 * j] : c1[2 * j - 8], si = j < 4 ? c0[2 * j + 1] : c1[2 * j - 7];
        const float a = g1[j], bb = g2[j];
        g1[j] = a * co + bb * si;
        g2[j] = bb * co - a * si;
      }
    }
    // both row sums at once: sum x^2 and sum g w x (mean(g w xhat) = rstd * the latter / HD)
    float ss = 0.f, m = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ss += x1[j] * x1[j] + x2[j] * x2[j];
      m += g1[j] * w1[j] * x1[j] + g2[j] * w2[j] * x2[j];
    }
    ss = head_sum<Lane<HD>::HV>(ss);
    m = head_sum<Lane<HD>::HV>(m);
    const float rs = rsqrtf(ss * (1.f / HD) + eps);
    const float cm = m * rs * (1.f / HD);
    if (qk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float h1 = x1[j] * rs, h2 = x2[j] * rs;
        a1[j] += g1[j] * h1;
        a2[j] += g2[j] * h2;
        g1[j] = rs * (g1[j] * w1[j] - h1 * cm);
        g2[j] = rs * (g2[j] * w2[j] - h2 * cm);
      }
    }
    if (act) {
      store8(dqkv + xo, ln.c, g1);
      store8(dqkv + xo, HALF + ln.c, g2);
    }
  }
  // the block's partial row: head rows of equal role added in slot order
  __shared__ __attribute__((aligned(16))) float tile[UB * HD];
  const int slot = threadIdx.x / Lane<HD>::HV;
  store8(tile, slot * HD + ln.c, a1);
  store8(tile, slot * HD + HALF + ln.c, a2);
  __syncthreads();
  if (threadIdx.x < 2 * HD) {
    const int r = threadIdx.x / HD, col = threadIdx.x % HD;
    int hj = (blockIdx.x * UB) % NH;  // head index of slot 0
    float sum = 0.f;
    for (int j = 0; j < UB; ++j) {
      const int rj = hj < H ? 0 : hj < H + KV ? 1 : 2;
      if (rj == r) sum += tile[j * HD + col];
      hj = hj + 1 == NH ? 0 : hj + 1;
    }
    part[static_cast<int64_t>(blockIdx.x) * 2 * HD + threadIdx.x] = sum;
  }
}

// ------------------------------------------------------------------------------ launchers
namespace {
int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }

// Blocks for T tokens of NH heads: two steps per block where there is that much work, at most `cap`, and
// a multiple of NH / gcd(NH, UB) so that the grid stride is a whole number of tokens.
int rope_norm_grid(int64_t T, int NH, int hd, int cap) {
  const int UB = kT / (hd / 16), period = NH / gcd(NH, UB);
  const int64_t steps = (T * NH + UB - 1) / UB, want = (steps + 1) / 2;
  if (want >= cap) return cap / period > 0 ? cap / period * period : period;
  return static_cast<int>((want + period - 1) / period) * period;
}
constexpr int kFwdCap = 2048, kBwdCap = 1024;  // bwd: one partial row per block for colsum2 to sum
}  // namespace

void launch_rope_norm_split_fwd(const uint16_t* qkv, const float* cs, const void* wq, const void* wk, bool w_bf16,
                                uint16_t* q, uint16_t* k, uint16_t* v, int B, int S, int H, int KV, int hd, float eps,
                                hipStream_t st) {
  const int T = B * S, NH = H + 2 * KV;
  if (T <= 0 || NH <= 0) return;
  const int g = rope_norm_grid(T, NH, hd, kFwdCap);
#define PSAMD_RN_F(HDV, WTV)                                                                                    \
  hipLaunchKernelGGL((rope_norm_split_fwd_kernel<HDV, WTV>), dim3(g), dim3(kT), 0, st, qkv, cs,                  \
                     static_cast<const WTV*>(wq), static_cast<const WTV*>(wk), q, k, v, T, S, H, KV, eps)
  if (hd == 128) {
    if (w_bf16) PSAMD_RN_F(128, uint16_t); else PSAMD_RN_F(128, float);
  } else {
    if (w_bf16) PSAMD_RN_F(64, uint16_t); else PSAMD_RN_F(64, float);
  }
#undef PSAMD_RN_F
}

int rope_norm_bwd_parts(int B, int S, int H, int KV, int hd) {
  return rope_norm_grid(static_cast<int64_t>(B) * S, H + 2 * KV, hd, kBwdCap) + 32;  // + colsum scratch rows
}

void launch_rope_norm_split_bwd(const uint16_t* dq, const uint16_t* dk, const uint16_t* dv, const uint16_t* qkv,
                                const float* cs, const void* wq, const void* wk, bool w_bf16, uint16_t* dqkv,
                                float* part, float* dw, int B, int S, int H, int KV, int hd, float eps,
                                hipStream_t st) {
  const int T = B * S, NH = H + 2 * KV;
  if (T <= 0 || NH <= 0) return;
  const int g = rope_norm_grid(T, NH, hd, kBwdCap);
#define PSAMD_RN_B(HDV, WTV)                                                                                    \
  hipLaunchKernelGGL((rope_norm_split_bwd_kernel<HDV, WTV>), dim3(g), dim3(kT), 0, st, dq, dk, dv, qkv, cs,      \
                     static_cast<const WTV*>(wq), static_cast<const WTV*>(wk), dqkv, part, T, S, H, KV, eps)
  if (hd == 128) {
    if (w_bf16) PSAMD_RN_B(128, uint16_t); else PSAMD_RN_B(128, float);
  } else {
    if (w_bf16) PSAMD_RN_B(64, uint16_t); else PSAMD_RN_B(64, float);
  }
#undef PSAMD_RN_B
  colsum2(part, g, 2 * hd, part + static_cast<int64_t>(g) * 2 * hd, dw, st);  // dw: [2, hd] = dwq | dwk
}

}  // namespace psamd
