// What the causal GQA flash attention kernels of both head dims share (flash_attn.hip: D = 128,
// flash_attn_d64.hip: D = 64): constants of the softmax, the XCD-aware block order, the clamp of
// document bounds, and the asm LDS helpers of the dK / dV kernels.
#pragma once
#include "psamd_launch.h"
#include "psamd_mfma.h"

namespace psamd {
namespace flash {

constexpr float kLog2e = 1.4426950408889634f;

// The forward's online softmax keeps a deferred reference max: it rescales only when the running
// max grows by more than 2^8 in exp2 units, so O and l are exact against that reference and P
// stays <= 256.
constexpr float kRescale = 8.f;

// XCD-aware 1-D block order.  The hardware deals consecutive block ids round-robin over the 8
// XCDs, each with its own L2; a "unit" is every block that reads one (batch, KV head)'s K / V
// (forward, dQ) or Q / dO (dK / dV), so each XCD is given whole units -- block L runs on XCD
// L mod 8 and takes the (L / 8) mod per -th item of unit (L mod 8) + 8 ((L / 8) / per).  Needs
// units % 8 == 0 (else plain order).  Items run heaviest first within a unit.
__device__ __forceinline__ void xcd_unit(int L, int per, int units, int& unit, int& r) {
  if ((units & 7) == 0) {
    const int x = L & 7, j = L >> 3;
    unit = x + 8 * (j / per);
    r = j % per;
  } else {
    unit = L / per;
    r = L % per;
  }
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

template <int N>
__device__ __forceinline__ void lgkm_wait() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ f32x4 lds_f4(const float* p) {
  f32x4 v;
  asm volatile("ds_read_b128 %0, %1"
               : "=v"(v)
               : "v"(mfma::lds_addr(reinterpret_cast<const uint16_t*>(p)))
               : "memory");
  return v;
}
__device__ __forceinline__ void tie4(f32x4& v) { asm volatile("" : "+v"(v)); }

}  // namespace flash

// the D = 64 kernels (flash_attn_d64.hip); launch_fa_fwd / launch_fa_bwd dispatch to them
void launch_fa64_fwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, float* lse, int B, int S,
                     int H, int KV, float scale, hipStream_t s, const int* doc_start);
void launch_fa64_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* out, const uint16_t* dout,
                     const float* lse, float* dsum, uint16_t* dq, uint16_t* dk, uint16_t* dv, int B, int S, int H,
                     int KV, float scale, hipStream_t s, const int* doc_start, const int* doc_end);

}  // namespace psamd
