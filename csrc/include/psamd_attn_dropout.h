// What the two fused BERT attention families (attention.hip: S <= 128; attention_long.hip: S <= 512)
// must agree on bit for bit: the dropout hash of an attention probability and the clamp of a packed
// sequence into its tensor.  Both include it from here, so neither can drift.
#pragma once
#include "psamd_device.h"

namespace psamd {
namespace {

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// one 32-bit hash per PAIR of elements (2j, 2j + 1): a 16-bit draw each, kept if >= p * 2^16.
// The 64-bit seed folds into one 32-bit key (uniform: scalar ALU), so a pair costs ONE avalanche
// finalizer (bijective in the pair index): the dropout hash had been the largest VALU item of the
// fused attention kernels (two finalizers per pair, ~85 VALU per MFMA in the forward).
__device__ __forceinline__ uint32_t pair_hash(uint64_t seed, uint32_t pair) {
  const uint32_t k = static_cast<uint32_t>(seed) ^ (static_cast<uint32_t>(seed >> 32) * 0x9E3779B9u);
  return mix32(pair ^ k);
}
__device__ __forceinline__ bool keep_lo(uint32_t h, uint32_t thr) { return (h & 0xffffu) >= thr; }
__device__ __forceinline__ bool keep_hi(uint32_t h, uint32_t thr) { return (h >> 16) >= thr; }

// Packed batches: sequence b's rows start at cu[b], L = cu[b + 1] - cu[b].  L is clamped into
// [0, min(S, T)] and the base into [0, T - L], so no cu can leave the T rows of the tensors.
struct PackRows {
  int64_t row0;
  int L;
};
__device__ __forceinline__ PackRows pack_rows(const int32_t* __restrict__ cu, int b, int S, int T) {
  const int c0 = cu[b], c1 = cu[b + 1];
  const int64_t d = static_cast<int64_t>(c1) - c0;
  const int L = static_cast<int>(min(max(d, int64_t{0}), static_cast<int64_t>(min(S, T))));
  return {static_cast<int64_t>(min(max(c0, 0), T - L)), L};
}

}  // namespace
}  // namespace psamd
