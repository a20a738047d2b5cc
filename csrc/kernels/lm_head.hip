// LM-head loss without the logits: loss = CE(h W^T, labels) with no [T, V] tensor in memory in either direction.
//
//   lm_head_fwd     a block owns one 128-row tile of h [T, D] and one of NS splits of the vocabulary, and walks the
//                   128-column tiles of its split.  After each tile's K loop a lane folds the 32 fp32 logits it holds
//                   of each of its two rows into that row's running (max, sum-exp) pair -- one rescale per tile --,
//                   and the one lane that holds column labels[row] writes that logit to zlab[row].  At the end of the
//                   split every lane half of every column wave writes its pair: part [2, 4 NS, T].
//   lm_head_finish  per row: the 4 NS pairs combined in index order -> lse[T]; loss_row = lse - zlab (0 for a row
//                   that is not scored: label == ignore or outside [0, V)).
//   lm_head_dz      the softmax gradient of one vocabulary chunk [v0, v0 + C), recomputing the logits:
//                   dz = (exp(z - lse[row]) - [col == label]) * go / count, one rounding to bf16, through the LDS
//                   epilogue tile into a scratch [T, C] as 16-B row pieces.  A row tile without a scored row skips
//                   its K loop and stores zeros.
//
// The main loop is the NT form of moe.hip's: 256 threads, a 128 x 128 tile, K stages of 64, 2 x 2
// v_mfma_f32_32x32x16_bf16 per wave, operands one stage ahead in registers into a double-buffered swizzled LDS
// tile, direct frag<64> reads of both.  Rows >= T and weight rows past the end are staged as zeros without a load.
// The stages of consecutive vocabulary tiles form one sequence, so the prefetch runs across tile boundaries.  The
// MFMA operands are swapped (weights as "A"): a lane ends with, for each of two output rows, 32 columns
// (wn + 32 j + (q & 3) + 8 (q >> 2) + 4 (lane >> 5)), and the softmax work needs no cross-lane traffic in the loop.
// No atomics; every output element has one writer; the logits stay fp32 in the forward.
// Block order: the 8 x 8 walk of psamd_gemm_tile.h over (row tiles, splits) in the forward and (row tiles, column
// tiles) in dz: the 64 blocks side by side on an XCD read 8 + 8 operand slabs per stage from its L2.
#include "psamd_device.h"
#include "psamd_gemm_tile.h"
#include "psamd_launch.h"
#include "psamd_mfma.h"

namespace psamd {
namespace {

using namespace mfma;
using namespace tile;

// the label of a scored row, -1 otherwise (xent.hip's rule; rows >= T are not scored)
__device__ __forceinline__ int scored_label(const int64_t* __restrict__ lab, int row, int T, int V, int64_t ignore) {
  if (row >= T) return -1;
  const int64_t y = lab[row];
  return (y == ignore || y < 0 || y >= V) ? -1 : static_cast<int>(y);
}

// acc += h[r0 .. r0 + 128) . w[n0 .. n0 + 128)^T for the column tiles vt0 <= vt < vt1 of w [Vr, D] (n0 = 128 vt);
// tile_done(n0) runs after the last K stage of every tile, with the tile's logits in acc, and leaves acc as the
// next tile is to find it.  Ends behind a barrier: smem is free.
template <class TileDone>
__device__ __forceinline__ void tile_loop(const uint16_t* __restrict__ h, const uint16_t* __restrict__ w, int T, int Vr,
                                          int D, int r0, int vt0, int vt1, uint16_t* smem, f32x16 (&acc)[2][2],
                                          TileDone&& tile_done) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  uint16_t* As = smem;
  uint16_t* Bs = smem + 2 * kStage;
  // both operands: thread = 16-B chunk ca of tile rows ra + 32 i
  const int ca = tid & 7, ra = tid >> 3;
  int tok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) tok[i] = r0 + ra + 32 * i < T ? r0 + ra + 32 * i : -1;
  const int nk = D / kTK, total = (vt1 - vt0) * nk;
  if (total <= 0) return;
  u16x8 va[4], vb[4];
  int lvt = vt0, lkt = 0;  // the stage the next load() fetches
  auto load = [&]() {
    const int k0 = lkt * kTK + ca * 8, n0 = lvt * kTN;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      va[i] = load_row8(h, D, tok[i], k0, true);
      vb[i] = load_row8(w, D, n0 + ra + 32 * i < Vr ? n0 + ra + 32 * i : -1, k0, true);
    }
    if (++lkt == nk) {
      lkt = 0;
      ++lvt;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = ra + 32 * i, o = buf * kStage + r * 64 + ((ca ^ sw<64>(r)) << 3);
      *reinterpret_cast<u16x8*>(As + o) = va[i];
      *reinterpret_cast<u16x8*>(Bs + o) = vb[i];
    }
  };
  load();
  store(0);
  __syncthreads();
  int kt = 0, vt = vt0;  // the stage being multiplied
  for (int it = 0; it < total; ++it) {
    const int buf = it & 1;
    if (it + 1 < total) load();
    const uint16_t* A = As + buf * kStage;
    const uint16_t* B = Bs + buf * kStage;
#pragma unroll
    for (int s = 0; s < kTK / 16; ++s) {
      bf16x8_t af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = frag<64>(A, wm + 32 * i + (lane & 31), 2 * s + (lane >> 5));
        bf[i] = frag<64>(B, wn + 32 * i + (lane & 31), 2 * s + (lane >> 5));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mma(bf[j], af[i], acc[i][j]);  // C^T blocks: lane = one output row
    }
    if (it + 1 < total) store(buf ^ 1);
    if (++kt == nk) {
      tile_done(vt * kTN);
      kt = 0;
      ++vt;
    }
    __syncthreads();
  }
}

// column (within the 128-column tile) of accumulator element q of column block j
__device__ __forceinline__ int acc_col(int wn, int j, int q, int lane) {
  return wn + 32 * j + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
}

// ------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(kNT, 2) void lm_head_fwd_kernel(const uint16_t* __restrict__ h, const uint16_t* __restrict__ w,
                                                          const int64_t* __restrict__ lab, int64_t ignore, int T, int V,
                                                          int D, int ns, int tps, float* __restrict__ part,
                                                          float* __restrict__ zlab) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[4 * kStage];  // As[2] | Bs[2]
  const int n_rt = (T + kTM - 1) / kTM, n_vt = (V + kTN - 1) / kTN, RG = (n_rt + 7) >> 3;
  int g, u, v;
  xcd_group(blockIdx.x, gridDim.x, g, u, v);
  const int rt = (g % RG) * 8 + u, sp = (g / RG) * 8 + v;
  if (rt >= n_rt || sp >= ns) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, r0 = rt * kTM;
  int row[2], y[2];
  float m[2], s[2], zl[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    row[i] = r0 + wm + 32 * i + (lane & 31);
    y[i] = scored_label(lab, row[i], T, V, ignore);
    m[i] = -INFINITY;
    s[i] = 0.f;
    zl[i] = 0.f;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) zero(acc[i][j]);

  auto fold = [&](int n0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float lm = -INFINITY;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int c = n0 + acc_col(wn, j, q, lane);
          const float z = c < V ? acc[i][j][q] : -INFINITY;  // columns past the vocabulary: excluded by select
          acc[i][j][q] = z;
          lm = fmaxf(lm, z);
          zl[i] = c == y[i] ? z : zl[i];
        }
      if (lm > -INFINITY) {  // this lane holds a column of the vocabulary in this tile
        if (lm > m[i]) {     // one rescale per tile
          s[i] *= __expf(m[i] - lm);
          m[i] = lm;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 16; ++q) s[i] += __expf(acc[i][j][q] - m[i]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) zero(acc[i][j]);
    }
  };
  const int vt0 = sp * tps, vt1 = min(vt0 + tps, n_vt);
  tile_loop(h, w, T, V, D, r0, vt0, vt1, smem, acc, fold);

  // part [2][4 ns][T]: the maxima, then the sums
  const int p = sp * 4 + (wave & 1) * 2 + (lane >> 5);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (row[i] >= T) continue;
    part[static_cast<int64_t>(p) * T + row[i]] = m[i];
    part[static_cast<int64_t>(4 * ns + p) * T + row[i]] = s[i];
    // the label's column is one of this lane's in a tile of this split: one lane of one block per scored row
    const int d = (y[i] & (kTN - 1)) - wn - 4 * (lane >> 5);
    if (y[i] >= vt0 * kTN && y[i] < vt1 * kTN && d >= 0 && d < 64 && !(d & 4)) zlab[row[i]] = zl[i];
  }
}

__global__ __launch_bounds__(kNT) void lm_head_finish_kernel(const float* __restrict__ part,
                                                             const float* __restrict__ zlab,
                                                             const int64_t* __restrict__ lab, int64_t ignore, int T,
                                                             int V, int np, float* __restrict__ lse,
                                                             float* __restrict__ loss_row) {
  const int r = blockIdx.x * kNT + threadIdx.x;
  if (r >= T) return;
  float M = -INFINITY, S = 0.f;
  for (int p = 0; p < np; ++p) {  // index order; a pair without a column has m = -inf, s = 0
    const float m2 = part[static_cast<int64_t>(p) * T + r], s2 = part[static_cast<int64_t>(np + p) * T + r];
    if (m2 == -INFINITY) continue;
    const float mn = fmaxf(M, m2);
    S = S * __expf(M - mn) + s2 * __expf(m2 - mn);
    M = mn;
  }
  const float l = M + __logf(S);
  lse[r] = l;
  loss_row[r] = scored_label(lab, r, T, V, ignore) >= 0 ? l - zlab[r] : 0.f;
}

// ------------------------------------------------------------------------------------------ softmax gradient of a chunk
// w: the chunk's first weight row; C: its columns; v0: its first vocabulary index; dz [T, C]
__global__ __launch_bounds__(kNT) void lm_head_dz_kernel(const uint16_t* __restrict__ h, const uint16_t* __restrict__ w,
                                                         const int64_t* __restrict__ lab, int64_t ignore,
                                                         const float* __restrict__ lse, const float* __restrict__ go,
                                                         const float* __restrict__ count, int T, int V, int D, int v0,
                                                         int C, int n_rt, int n_ct, uint16_t* __restrict__ dz) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[4 * kStage];  // As[2] | Bs[2]; the epilogue tile on top
  const int RG = (n_rt + 7) >> 3;
  int g, u, v;
  xcd_group(blockIdx.x, gridDim.x, g, u, v);
  const int rt = (g % RG) * 8 + u, ct = (g / RG) * 8 + v;
  if (rt >= n_rt || ct >= n_ct) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, r0 = rt * kTM, c0 = ct * kTN;
  const float kk = go[0] / fmaxf(count[0], 1.f);
  int y[2];
  float k[2], l[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = r0 + wm + 32 * i + (lane & 31);
    y[i] = scored_label(lab, row, T, V, ignore);
    k[i] = y[i] >= 0 ? kk : 0.f;
    l[i] = row < T ? lse[row] : 0.f;
  }
  const bool any = __syncthreads_or(y[0] >= 0 || y[1] >= 0);  // a scored row in this row tile
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) zero(acc[i][j]);
  tile_loop(h, w, T, C, D, r0, ct, any ? ct + 1 : ct, smem, acc, [](int) {});
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int c = v0 + c0 + acc_col(wn, j, q, lane);
        const float p = __expf(acc[i][j][q] - l[i]) - (c == y[i] ? 1.f : 0.f);
        acc[i][j][q] = y[i] >= 0 ? p * k[i] : 0.f;  // a row that is not scored: exact zeros
      }
  acc_to_lds(smem, acc, wm, wn, lane);
  __syncthreads();
  lds_to_c(smem, dz + static_cast<int64_t>(r0) * C + c0, C, T - r0, C - c0);
}

}  // namespace

// ------------------------------------------------------------------------------------------ launches
int lm_head_splits(int T, int V, int ns) {
  const int n_rt = (T + kTM - 1) / kTM, n_vt = (V + kTN - 1) / kTN;
  // automatic: two rounds of the 512 blocks that 256 CUs hold (64 KB of LDS each), splits in whole groups of 8
  if (ns <= 0) ns = (((2 * 512 + n_rt - 1) / n_rt) + 7) / 8 * 8;
  ns = ns < n_vt ? ns : n_vt;
  const int tps = (n_vt + ns - 1) / ns;
  return (n_vt + tps - 1) / tps;  // no empty split
}

void launch_lm_head_fwd(const uint16_t* h, const uint16_t* w, const int64_t* lab, int64_t ignore, int T, int V, int D,
                        int ns, float* part, float* zlab, float* lse, float* loss_row, hipStream_t st) {
  const int n_rt = (T + kTM - 1) / kTM, n_vt = (V + kTN - 1) / kTN, tps = (n_vt + ns - 1) / ns;
  hipLaunchKernelGGL(lm_head_fwd_kernel, dim3(group_grid(n_rt, ns)), dim3(kNT), 0, st, h, w, lab, ignore, T, V, D, ns,
                     tps, part, zlab);
  hipLaunchKernelGGL(lm_head_finish_kernel, dim3((T + kNT - 1) / kNT), dim3(kNT), 0, st, part, zlab, lab, ignore, T, V,
                     4 * ns, lse, loss_row);
}

void launch_lm_head_dz(const uint16_t* h, const uint16_t* w, const int64_t* lab, int64_t ignore, const float* lse,
                       const float* go, const float* count, int T, int V, int D, int v0, int C, uint16_t* dz,
                       hipStream_t st) {
  const int n_rt = (T + kTM - 1) / kTM, n_ct = (C + kTN - 1) / kTN;
  hipLaunchKernelGGL(lm_head_dz_kernel, dim3(group_grid(n_rt, n_ct)), dim3(kNT), 0, st, h,
                     w + static_cast<int64_t>(v0) * D, lab, ignore, lse, go, count, T, V, D, v0, C, n_rt, n_ct, dz);
}

}  // namespace psamd
