// The 128 x 128 x 64 bf16 MFMA tile shared by the row-tile GEMM kernels (moe.hip, lm_head.hip): sizes, zero-filled
// 16-B operand loads, the accumulator -> LDS -> global epilogue of the swapped-operand layout, and the block order
// that keeps 8 x 8 tile groups on one XCD.  The main loops themselves live with their kernels.
#pragma once
#include "psamd_device.h"
#include "psamd_mfma.h"

namespace psamd {
namespace tile {

constexpr int kTM = 128;           // rows per tile
constexpr int kTN = 128;           // columns per tile
constexpr int kTK = 64;            // reduction per stage
constexpr int kNT = 256;           // threads
constexpr int kCLd = kTN + 8;      // epilogue tile row length (272 B: 16-B aligned, rows on shifted banks)
constexpr int kStage = kTM * kTK;  // elements of one operand stage (either layout)
static_assert(kTM * kCLd <= 4 * kStage, "the epilogue tile lies on top of the two double-buffered operand tiles");

__device__ __forceinline__ u16x8 zero8() { return u16x8{0, 0, 0, 0, 0, 0, 0, 0}; }

// 8 elements at column col of row tok (row length ld); zeros, without a load, for tok < 0 or !col_ok
__device__ __forceinline__ u16x8 load_row8(const uint16_t* __restrict__ src, int64_t ld, int tok, int col, bool col_ok) {
  return (tok >= 0 && col_ok) ? *reinterpret_cast<const u16x8*>(src + static_cast<int64_t>(tok) * ld + col) : zero8();
}

// accumulators (lane: 4 consecutive columns 8 q4 + 4 (l >> 5) + {0..3} of row l & 31, per 32 x 32 block) -> Cs
__device__ __forceinline__ void acc_to_lds(uint16_t* Cs, const mfma::f32x16 (&acc)[2][2], int wr, int wc, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const mfma::f32x16& a = acc[i][j];
        uint2 v;
        v.x = pk_bf16(a[4 * q4], a[4 * q4 + 1]);
        v.y = pk_bf16(a[4 * q4 + 2], a[4 * q4 + 3]);
        *reinterpret_cast<uint2*>(Cs + (wr + 32 * i + (lane & 31)) * kCLd + wc + 32 * j + 8 * q4 + 4 * (lane >> 5)) = v;
      }
}

// Cs -> C rows [0, rows) x columns [0, cols) of the tile at c (row length ldc): 16 B per lane
__device__ __forceinline__ void lds_to_c(const uint16_t* Cs, uint16_t* __restrict__ c, int64_t ldc, int rows, int cols) {
  const int ch = (threadIdx.x & 15) * 8;
#pragma unroll
  for (int i = 0; i < kTM / 16; ++i) {
    const int r = (threadIdx.x >> 4) + 16 * i;
    if (r < rows && ch < cols)
      *reinterpret_cast<u16x8*>(c + static_cast<int64_t>(r) * ldc + ch) = *reinterpret_cast<const u16x8*>(Cs + r * kCLd + ch);
  }
}

// logical position of block b in the XCD-dealt order, then its place in the 8 x 8 groups: g = group, (u, v) in it
__device__ __forceinline__ void xcd_group(int b, int total, int& g, int& u, int& v) {
  const int L = (b & 7) * (total >> 3) + (b >> 3);
  g = L >> 6;
  u = L & 7;
  v = (L >> 3) & 7;
}

// blocks of a grid walked in 8 x 8 groups over n_a x n_b tiles
inline int group_grid(int n_a, int n_b) { return ((n_a + 7) / 8) * ((n_b + 7) / 8) * 64; }

}  // namespace tile
}  // namespace psamd
