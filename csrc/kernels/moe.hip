// Mixture-of-experts FFN: routing plan, grouped bf16 MFMA GEMMs over the routed rows, combine.
//
//   moe_plan      stable counting sort of the T * k (token, slot) pairs by expert; every expert's segment of
//                 the permuted row space starts at a multiple of the 128-row GEMM tile, so no row tile holds
//                 two experts.  Three launches, no atomics, no host sync: per-chunk histograms, one scan
//                 block, scatter.  row_token / row_slot [R_cap] (-1 on pad rows), slot_row [T, k] (-1 for an
//                 id outside [0, E)), tile_expert [R_cap / 128] (-1 on unused tiles), counts / seg [E].
//   moe_gemm      C[rows of tile] = A'[rows] . op(W[tile_expert[tile]]): NT (W [E, N, K], the forward GEMMs)
//                 or NN (W [E, K, N], the data gradients: the weight's reduction index is its slow one and
//                 its fragments are read transposed).  A' row r is src[row_token[r]] (GATHER; a pad row is
//                 staged as zeros without a load), optionally times wts[row_slot[r]] (SCALE, one bf16
//                 rounding of the product: dY = wts * dout).
//   moe_wgrad     dW[e][n, c] = sum over the rows r of expert e of G'[r, n] A'[r, c], in row order; either
//                 operand may be the gathered (and scaled) one.  An expert without rows gets exact zeros.
//   moe_combine   out[t] = sum_j wts[t, j] Y[slot_row[t, j]] in fp32, j ascending, one rounding (without
//                 wts: the plain sum that folds dX_perm into dx);  moe_combine_bwd: dwts[t, j] = <Y[row], dout[t]>.
//
// GEMM design.  256 threads = 4 waves, C tile 128 x 128, reduction 64 per stage, each wave a 64 x 64 quadrant
// = 2 x 2 v_mfma_f32_32x32x16_bf16 blocks (64 accumulator registers).  Operands move global -> registers one
// stage ahead (16 B per lane per access) and land in a double-buffered, chunk-swizzled LDS tile after the
// current stage's MFMAs (one barrier per stage): [row][k] tiles of 128-B rows are read as direct 16-B
// fragments, [k][col] tiles of 256-B rows as ds_read_b64_tr_b16 fragments (psamd_mfma.h).  The MFMA operands
// are swapped (weights as "A", activations as "B"), so a lane ends with 4 consecutive output columns of one
// output row: the accumulators go to LDS as 8-B bf16 quads and leave as full 16-B row pieces.
// Block order: ids are dealt round-robin over the 8 XCDs, so XCD x takes the x-th eighth of the logical
// order, and the logical order walks 8 x 8 groups (8 row tiles of -- mostly -- one expert x 8 column tiles):
// the 64 blocks an XCD runs side by side read 8 + 8 operand slabs per stage from its L2, not 64 + 64.  The
// weight gradient's groups go expert-fastest, so every XCD's share holds all experts however skewed the routing.
#include "psamd_device.h"
#include "psamd_gemm_tile.h"
#include "psamd_launch.h"
#include "psamd_mfma.h"

namespace psamd {
namespace {

using namespace mfma;
using namespace tile;  // the 128 x 128 x 64 tile, its epilogue and block order (psamd_gemm_tile.h)

constexpr int kChunk = 1024;    // (token, slot) pairs per plan block
static_assert(kTM == kMoeRowTile, "row tile");

// ------------------------------------------------------------------------------------------ plan
__device__ __forceinline__ int load_id(const void* idx, bool is64, int64_t p, int E) {
  const int64_t v = is64 ? static_cast<const int64_t*>(idx)[p] : static_cast<const int32_t*>(idx)[p];
  return (v >= 0 && v < E) ? static_cast<int>(v) : -1;  // an id off [0, E) never becomes an index
}

// hist[b][e] = pairs of chunk b on expert e; also presets the row maps to -1 (pad rows)
__global__ __launch_bounds__(kNT) void moe_count_kernel(const void* __restrict__ idx, bool is64, int n, int E,
                                                        int* __restrict__ hist, int* __restrict__ row_token,
                                                        int* __restrict__ row_slot, int r_cap) {
  __shared__ int ids[kChunk];
  const int base = blockIdx.x * kChunk, m = min(kChunk, n - base);
  for (int i = threadIdx.x; i < m; i += kNT) ids[i] = load_id(idx, is64, base + i, E);
  for (int r = blockIdx.x * kNT + threadIdx.x; r < r_cap; r += gridDim.x * kNT) {
    row_token[r] = -1;
    row_slot[r] = -1;
  }
  __syncthreads();
  const int e = threadIdx.x;
  if (e < E) {
    int c = 0;
    for (int i = 0; i < m; ++i) c += ids[i] == e;
    hist[blockIdx.x * E + e] = c;
  }
}

// one block: hist -> exclusive offsets of every chunk within its expert, counts, tile-aligned segment starts,
// the expert of every row tile
__global__ __launch_bounds__(kNT) void moe_scan_kernel(int* __restrict__ hist, int nb, int E, int* __restrict__ counts,
                                                       int* __restrict__ seg, int* __restrict__ tile_expert,
                                                       int n_tiles) {
  __shared__ int cnt[kMoeMaxExperts];
  __shared__ int start[kMoeMaxExperts + 1];  // in tiles
  const int e = threadIdx.x;
  if (e < E) {
    int run = 0;
    for (int b = 0; b < nb; ++b) {
      const int c = hist[b * E + e];
      hist[b * E + e] = run;
      run += c;
    }
    cnt[e] = run;
    counts[e] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < E; ++i) {
      start[i] = s;
      s += (cnt[i] + kTM - 1) / kTM;
    }
    start[E] = s;
  }
  __syncthreads();
  if (e < E) seg[e] = start[e] * kTM;
  for (int t = threadIdx.x; t < n_tiles; t += kNT) {
    int ex = -1;
    for (int i = 0; i < E; ++i) ex = (t >= start[i] && t < start[i + 1]) ? i : ex;
    tile_expert[t] = ex;
  }
}

// pair p of chunk b on expert e -> row seg[e] + (pairs of e in earlier chunks) + (pairs of e earlier in b)
__global__ __launch_bounds__(kNT) void moe_scatter_kernel(const void* __restrict__ idx, bool is64, int n, int E, int k,
                                                          const int* __restrict__ boff, const int* __restrict__ seg,
                                                          int* __restrict__ row_token, int* __restrict__ row_slot,
                                                          int* __restrict__ slot_row) {
  __shared__ int ids[kChunk];
  __shared__ int rank[kChunk];
  const int base = blockIdx.x * kChunk, m = min(kChunk, n - base);
  for (int i = threadIdx.x; i < m; i += kNT) ids[i] = load_id(idx, is64, base + i, E);
  __syncthreads();
  const int e = threadIdx.x;
  if (e < E) {  // every rank[i] has one writer: the thread of ids[i]
    int c = 0;
    for (int i = 0; i < m; ++i)
      if (ids[i] == e) rank[i] = c++;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += kNT) {
    const int x = ids[i], p = base + i;
    int row = -1;
    if (x >= 0) {
      row = seg[x] + boff[blockIdx.x * E + x] + rank[i];
      row_token[row] = p / k;
      row_slot[row] = p;
    }
    slot_row[p] = row;
  }
}

// ------------------------------------------------------------------------------------------ staging
// One thread's row of a gathered / scaled operand: the source row (-1: zeros) and its factor.
struct RowSrc {
  int tok;
  float scl;
};

template <bool GATHER, bool SCALE>
__device__ __forceinline__ RowSrc row_src(int r, bool in, const int* __restrict__ row_token,
                                          const int* __restrict__ row_slot, const float* __restrict__ wts) {
  RowSrc s{-1, 1.f};
  if (!in) return s;
  if constexpr (GATHER) {
    s.tok = row_token[r];
    if constexpr (SCALE) {
      if (s.tok >= 0) s.scl = wts[row_slot[r]];
    }
  } else {
    s.tok = r;
  }
  return s;
}

template <bool SCALE>
__device__ __forceinline__ u16x8 scaled(u16x8 v, float s) {
  if constexpr (!SCALE) return v;
  const u32x4_t w = __builtin_bit_cast(u32x4_t, v);
  u32x4_t o;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = pk_bf16(s * __uint_as_float(w[i] << 16), s * __uint_as_float(w[i] & 0xffff0000u));
  return __builtin_bit_cast(u16x8, o);
}

// ------------------------------------------------------------------------------------------ row-tile GEMM
template <bool NN, bool GATHER, bool SCALE>
__global__ __launch_bounds__(kNT) void moe_gemm_kernel(const uint16_t* __restrict__ a, const int* __restrict__ row_token,
                                                       const int* __restrict__ row_slot, const float* __restrict__ wts,
                                                       const uint16_t* __restrict__ w, const int* __restrict__ tile_expert,
                                                       uint16_t* __restrict__ c, int N, int K, int n_rt, int n_nt) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[4 * kStage];  // As[2] | Bs[2]; the epilogue tile on top
  static_assert(kTM * kCLd <= 4 * kStage, "epilogue tile");
  const int RG = (n_rt + 7) >> 3;
  int g, u, v;
  xcd_group(blockIdx.x, gridDim.x, g, u, v);
  const int rt = (g % RG) * 8 + u, nt = (g / RG) * 8 + v;
  if (rt >= n_rt || nt >= n_nt) return;
  const int e = tile_expert[rt];
  if (e < 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int r0 = rt * kTM, n0 = nt * kTN;
  const uint16_t* we = w + static_cast<int64_t>(e) * N * K;
  uint16_t* As = smem;
  uint16_t* Bs = smem + 2 * kStage;

  // A: thread = 16-B chunk ca of rows ra + 32 i
  const int ca = tid & 7, ra = tid >> 3;
  RowSrc rs[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rs[i] = row_src<GATHER, SCALE>(r0 + ra + 32 * i, true, row_token, row_slot, wts);
  // B: NT rows n0 + ra + 32 i of [N, K], chunk ca; NN rows k0 + rb + 16 i of [K, N], chunk cb of 16
  const int cb = tid & 15, rb = tid >> 4;
  u16x8 va[4], vb[4];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      va[i] = load_row8(a, K, rs[i].tok, k0 + ca * 8, true);
      if constexpr (NN) vb[i] = load_row8(we, N, k0 + rb + 16 * i, n0 + cb * 8, n0 + cb * 8 < N);
      else vb[i] = load_row8(we, K, n0 + ra + 32 * i < N ? n0 + ra + 32 * i : -1, k0 + ca * 8, true);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = ra + 32 * i;
      *reinterpret_cast<u16x8*>(As + buf * kStage + r * 64 + ((ca ^ sw<64>(r)) << 3)) = scaled<SCALE>(va[i], rs[i].scl);
      if constexpr (NN) {
        const int kr = rb + 16 * i;
        *reinterpret_cast<u16x8*>(Bs + buf * kStage + kr * 128 + ((cb ^ sw<128>(kr)) << 3)) = vb[i];
      } else {
        *reinterpret_cast<u16x8*>(Bs + buf * kStage + r * 64 + ((ca ^ sw<64>(r)) << 3)) = vb[i];
      }
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) zero(acc[i][j]);

  const int nk = K / kTK;
  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load((kt + 1) * kTK);
    const uint16_t* A = As + buf * kStage;
    const uint16_t* B = Bs + buf * kStage;
#pragma unroll
    for (int s = 0; s < kTK / 16; ++s) {
      bf16x8_t af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = frag<64>(A, wm + 32 * i + (lane & 31), 2 * s + (lane >> 5));
        if constexpr (NN) bf[i] = tfrag<128>(B, s, wn + 32 * i, lane);
        else bf[i] = frag<64>(B, wn + 32 * i + (lane & 31), 2 * s + (lane >> 5));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mma(bf[j], af[i], acc[i][j]);  // C^T blocks: lane = one output row
    }
    if (kt + 1 < nk) store(buf ^ 1);
    __syncthreads();
  }
  acc_to_lds(smem, acc, wm, wn, lane);
  __syncthreads();
  lds_to_c(smem, c + static_cast<int64_t>(r0) * N + n0, N, kTM, N - n0);
}

// ------------------------------------------------------------------------------------------ grouped weight gradient
// dW[e][n, c] = sum_r G'[r, n] A'[r, c] over rows [seg[e], seg[e] + counts[e]) (stages of 64 rows; the rows past
// the count inside the expert's last tile are pad rows: zeros in a plain operand, staged as zeros in a gathered one).
// GSRC: which operand is gathered (0 none, 1 G', 2 A').
template <int GSRC, bool SCALE>
__global__ __launch_bounds__(kNT) void moe_wgrad_kernel(const uint16_t* __restrict__ gmat, const uint16_t* __restrict__ amat,
                                                        const int* __restrict__ row_token, const int* __restrict__ row_slot,
                                                        const float* __restrict__ wts, const int* __restrict__ seg,
                                                        const int* __restrict__ counts, uint16_t* __restrict__ dw, int Nn,
                                                        int Cc, int n_nt, int n_ct) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[4 * kStage];  // Gs[2] | As[2]; the epilogue tile on top
  const int NG = (n_nt + 7) >> 3, CG = (n_ct + 7) >> 3;
  int g, u, v;
  xcd_group(blockIdx.x, gridDim.x, g, u, v);
  const int E = gridDim.x / (NG * CG * 64);
  const int e = g % E, ge = g / E;  // experts fastest: every XCD's share of the order holds all of them, however skewed
  const int nt = (ge % NG) * 8 + u, ct = (ge / NG) * 8 + v;
  if (nt >= n_nt || ct >= n_ct) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = (wave >> 1) * 64, wc = (wave & 1) * 64;
  const int n0 = nt * kTN, c0 = ct * kTN;
  const int rbeg = seg[e], cnt = counts[e], nk = (cnt + kTK - 1) / kTK, rend = rbeg + nk * kTK;
  uint16_t* Gs = smem;
  uint16_t* As = smem + 2 * kStage;

  // both operands: thread = 16-B chunk cb (of 16) of stage rows rb + 16 i
  const int cb = tid & 15, rb = tid >> 4;
  const bool g_ok = n0 + cb * 8 < Nn, a_ok = c0 + cb * 8 < Cc;
  RowSrc cur[4], nxt[4];  // the gathered operand's rows of the stage being loaded / the one after
  u16x8 vg[4], va[4];
  auto rows = [&](RowSrc (&rs)[4], int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = rbeg + k0 + rb + 16 * i;
      rs[i] = row_src<(GSRC != 0), SCALE>(r, r < rend, row_token, row_slot, wts);
    }
  };
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = rbeg + k0 + rb + 16 * i;
      vg[i] = load_row8(gmat, Nn, GSRC == 1 ? cur[i].tok : r, n0 + cb * 8, g_ok);
      va[i] = load_row8(amat, Cc, GSRC == 2 ? cur[i].tok : r, c0 + cb * 8, a_ok);
      if constexpr (GSRC == 1) vg[i] = scaled<SCALE>(vg[i], cur[i].scl);
      if constexpr (GSRC == 2) va[i] = scaled<SCALE>(va[i], cur[i].scl);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kr = rb + 16 * i, o = buf * kStage + kr * 128 + ((cb ^ sw<128>(kr)) << 3);
      *reinterpret_cast<u16x8*>(Gs + o) = vg[i];
      *reinterpret_cast<u16x8*>(As + o) = va[i];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) zero(acc[i][j]);

  if (nk > 0) {
    rows(cur, 0);
    load(0);
    rows(nxt, kTK);
    store(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) {
#pragma unroll
      for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
      load((kt + 1) * kTK);
      rows(nxt, (kt + 2) * kTK);  // row maps two stages ahead: the data loads never wait for them
    }
    const uint16_t* G = Gs + buf * kStage;
    const uint16_t* A = As + buf * kStage;
#pragma unroll
    for (int s = 0; s < kTK / 16; ++s) {
      bf16x8_t gf[2], af[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        gf[i] = tfrag<128>(G, s, wn + 32 * i, lane);
        af[i] = tfrag<128>(A, s, wc + 32 * i, lane);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mma(af[j], gf[i], acc[i][j]);  // lane = one dW row n
    }
    if (kt + 1 < nk) store(buf ^ 1);
    __syncthreads();
  }
  acc_to_lds(smem, acc, wn, wc, lane);
  __syncthreads();
  lds_to_c(smem, dw + (static_cast<int64_t>(e) * Nn + n0) * Cc + c0, Cc, Nn - n0, Cc - c0);
}

// ------------------------------------------------------------------------------------------ combine
// out[t] = sum_j wts[t, j] Y[slot_row[t, j]] (wts null: factor 1); fp32, j ascending, one rounding
__global__ __launch_bounds__(kNT) void moe_combine_kernel(const uint16_t* __restrict__ y, const int* __restrict__ slot_row,
                                                          const float* __restrict__ wts, uint16_t* __restrict__ out,
                                                          int64_t T, int k, int D) {
  const int dc = D / 8;
  const int64_t total = T * dc;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kNT + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * kNT) {
    const int64_t t = i / dc;
    const int col = static_cast<int>(i % dc) * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
      const int row = slot_row[t * k + j];
      if (row < 0) continue;
      const float wj = wts ? wts[t * k + j] : 1.f;
      float v[8];
      load8(y, static_cast<int64_t>(row) * D + col, v);
#pragma unroll
      for (int x = 0; x < 8; ++x) acc[x] = fmaf(wj, v[x], acc[x]);
    }
    store8(out, t * D + col, acc);
  }
}

// dwts[t, j] = <Y[slot_row[t, j]], dout[t]>: one wave per token, lanes stride the row, fixed-order wave sum
__global__ __launch_bounds__(kNT) void moe_combine_bwd_kernel(const uint16_t* __restrict__ y,
                                                              const int* __restrict__ slot_row,
                                                              const uint16_t* __restrict__ dout, float* __restrict__ dwts,
                                                              int64_t T, int k, int D) {
  const int lane = threadIdx.x & 63, dc = D / 8;
  const int64_t nw = static_cast<int64_t>(gridDim.x) * (kNT / 64);
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * (kNT / 64) + (threadIdx.x >> 6); t < T; t += nw) {
    for (int j = 0; j < k; ++j) {
      const int row = slot_row[t * k + j];  // wave-uniform
      float s = 0.f;
      if (row >= 0) {
        for (int ch = lane; ch < dc; ch += 64) {
          float a[8], b[8];
          load8(y, static_cast<int64_t>(row) * D + ch * 8, a);
          load8(dout, t * D + ch * 8, b);
#pragma unroll
          for (int x = 0; x < 8; ++x) s = fmaf(a[x], b[x], s);
        }
      }
      s = wave_sum(s);
      if (lane == 0) dwts[t * k + j] = s;
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------ launches
int moe_plan_chunks(int64_t n) { return static_cast<int>((n + kChunk - 1) / kChunk); }

void launch_moe_plan(const void* idx, bool idx_i64, int64_t T, int k, int E, int* hist, int* row_token, int* row_slot,
                     int* slot_row, int* tile_expert, int* counts, int* seg, hipStream_t st) {
  const int n = static_cast<int>(T * k), nb = moe_plan_chunks(n), n_tiles = moe_row_tiles(T, k, E);
  hipLaunchKernelGGL(moe_count_kernel, dim3(nb), dim3(kNT), 0, st, idx, idx_i64, n, E, hist, row_token, row_slot,
                     n_tiles * kTM);
  hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(kNT), 0, st, hist, nb, E, counts, seg, tile_expert, n_tiles);
  hipLaunchKernelGGL(moe_scatter_kernel, dim3(nb), dim3(kNT), 0, st, idx, idx_i64, n, E, k, hist, seg, row_token,
                     row_slot, slot_row);
}

void launch_moe_gemm(const uint16_t* a, const int* row_token, const int* row_slot, const float* wts, const uint16_t* w,
                     const int* tile_expert, uint16_t* c, int n_tiles, int N, int K, bool nn, hipStream_t st) {
  const int n_nt = (N + kTN - 1) / kTN;
  const dim3 grid(group_grid(n_tiles, n_nt)), block(kNT);
#define PSAMD_MOE_GEMM(NNV, GV, SV)                                                                                  \
  hipLaunchKernelGGL((moe_gemm_kernel<NNV, GV, SV>), grid, block, 0, st, a, row_token, row_slot, wts, w, tile_expert, \
                     c, N, K, n_tiles, n_nt)
  const bool gather = row_token != nullptr, scale = gather && wts != nullptr;
  if (nn) {
    if (scale) PSAMD_MOE_GEMM(true, true, true);
    else if (gather) PSAMD_MOE_GEMM(true, true, false);
    else PSAMD_MOE_GEMM(true, false, false);
  } else {
    if (scale) PSAMD_MOE_GEMM(false, true, true);
    else if (gather) PSAMD_MOE_GEMM(false, true, false);
    else PSAMD_MOE_GEMM(false, false, false);
  }
#undef PSAMD_MOE_GEMM
}

void launch_moe_wgrad(const uint16_t* g, const uint16_t* a, int gathered, const int* row_token, const int* row_slot,
                      const float* wts, const int* seg, const int* counts, uint16_t* dw, int E, int Nn, int Cc,
                      hipStream_t st) {
  const int n_nt = (Nn + kTN - 1) / kTN, n_ct = (Cc + kTN - 1) / kTN;
  const dim3 grid(E * group_grid(n_nt, n_ct)), block(kNT);
#define PSAMD_MOE_WGRAD(GS, SV)                                                                                     \
  hipLaunchKernelGGL((moe_wgrad_kernel<GS, SV>), grid, block, 0, st, g, a, row_token, row_slot, wts, seg, counts, dw, \
                     Nn, Cc, n_nt, n_ct)
  const bool scale = gathered != 0 && wts != nullptr;
  if (gathered == 1) {
    if (scale) PSAMD_MOE_WGRAD(1, true);
    else PSAMD_MOE_WGRAD(1, false);
  } else if (gathered == 2) {
    if (scale) PSAMD_MOE_WGRAD(2, true);
    else PSAMD_MOE_WGRAD(2, false);
  } else {
    PSAMD_MOE_WGRAD(0, false);
  }
#undef PSAMD_MOE_WGRAD
}

void launch_moe_combine(const uint16_t* y, const int* slot_row, const float* wts, uint16_t* out, int64_t T, int k, int D,
                        hipStream_t st) {
  hipLaunchKernelGGL(moe_combine_kernel, dim3(stream_grid(T * (D / 8), kNT)), dim3(kNT), 0, st, y, slot_row, wts, out, T,
                     k, D);
}

void launch_moe_combine_bwd(const uint16_t* y, const int* slot_row, const uint16_t* dout, float* dwts, int64_t T, int k,
                            int D, hipStream_t st) {
  hipLaunchKernelGGL(moe_combine_bwd_kernel, dim3(stream_grid(T * 64, kNT)), dim3(kNT), 0, st, y, slot_row, dout, dwts,
                     T, k, D);
}

}  // namespace psamd
