// Multi-hot embedding bags: pooled lookups over the pulled unique rows of a sparse table.
//
// A one-hot lookup gathers rows[inv[k]] per looked-up position (gather_rows) and reduces the
// output gradient per unique row (segment_reduce_rows).  A multi-hot field holds a list of ids
// (a bag) and its vector is the sum, mean or weighted sum of their rows; composing that from
// the one-hot kernels writes and re-reads an [nnz, dim] tensor forward and another backward.
// The two kernels here never materialise it:
//
//  bag_pool_fwd  out[g] = s_g * sum_{j in [bag_off[g], bag_off[g+1])} w[j] * rows[inv[j]]
//  bag_pool_bwd  drows[u] = sum_{j in [seg_off[u], seg_off[u+1])} w[p] * s_{g(p)} * dout[g(p)],
//                p = perm[j], g(p) = bag_of[p]
//
// s_g = 1 / max(1, len_g) in mean mode, else 1; w is optional.  Both follow
// segment_reduce_rows (sparse.hip): for dim = 4 * 2^lg <= 256 and 16-B aligned bases 2^lg lanes
// own one bag / segment, each lane one 16-B load per row, four independent row loads in flight,
// the running sum in registers; any other dim or alignment takes one wave per bag / segment.
// No atomics, no LDS; the result is bitwise reproducible.  Summation order: j ascending, groups
// of four added as (t0 + t1) + (t2 + t3) onto the running sum, then the tail one by one (the
// generic kernels add one by one).  An empty bag / segment stores zeros and loads no row.
#include "psamd_device.h"
#include "psamd_launch.h"

namespace psamd {

__device__ __forceinline__ float bag_scale(const int64_t* __restrict__ bag_off, int64_t g) {
  const int64_t len = bag_off[g + 1] - bag_off[g];
  return 1.f / static_cast<float>(len > 0 ? len : 1);
}

// ---------------------------------------------------------------------------------- forward
template <typename O, bool W>
__global__ __launch_bounds__(256) void bag_pool_fwd_kernel(const float* __restrict__ rows,
                                                           const int64_t* __restrict__ inv,
                                                           const int64_t* __restrict__ bag_off,
                                                           const float* __restrict__ w, int64_t nbags, int dim,
                                                           O* __restrict__ out, int mean) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t g = wave; g < nbags; g += nwaves) {
    const int64_t b = bag_off[g], e = bag_off[g + 1];
    const float s = mean ? 1.f / static_cast<float>(e - b > 0 ? e - b : 1) : 1.f;
    for (int c = lane; c < dim; c += 64) {
      float acc = 0.f;
      for (int64_t j = b; j < e; ++j) {
        const float v = rows[inv[j] * dim + c];
        acc += W ? w[j] * v : v;
      }
      Elem<O>::store(out + g * dim, c, mean ? acc * s : acc);
    }
  }
}

template <typename O, bool W>
__global__ __launch_bounds__(256) void bag_pool_fwd_vec_kernel(const float* __restrict__ rows,
                                                               const int64_t* __restrict__ inv,
                                                               const int64_t* __restrict__ bag_off,
                                                               const float* __restrict__ w, int64_t nbags, int dim,
                                                               int lg, O* __restrict__ out, int mean) {
  const int lane = threadIdx.x & 63;
  const int sub = lane >> lg;
  const int c = (lane & ((1 << lg) - 1)) * 4;
  const int per_wave = 64 >> lg;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t gb = wave * per_wave; gb < nbags; gb += nwaves * per_wave) {
    const int64_t g = gb + sub;
    if (g >= nbags) continue;
    const int64_t b = bag_off[g], e = bag_off[g + 1];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int64_t j = b;
    // 4 independent row loads in flight: a long bag is a latency chain otherwise
    for (; j + 4 <= e; j += 4) {
      const int64_t i0 = inv[j], i1 = inv[j + 1], i2 = inv[j + 2], i3 = inv[j + 3];
      f32x4 v0 = load4(rows, i0 * dim + c), v1 = load4(rows, i1 * dim + c);
      f32x4 v2 = load4(rows, i2 * dim + c), v3 = load4(rows, i3 * dim + c);
      if (W) {
        v0 *= w[j]; v1 *= w[j + 1]; v2 *= w[j + 2]; v3 *= w[j + 3];
      }
      acc += (v0 + v1) + (v2 + v3);
    }
    for (; j < e; ++j) {
      f32x4 v = load4(rows, inv[j] * dim + c);
      if (W) v *= w[j];
      acc += v;
    }
    if (mean) acc *= 1.f / static_cast<float>(e - b > 0 ? e - b : 1);
    store4(out, g * dim + c, acc);
  }
}

static int bag_lg(int dim) {
  if (dim % 4 != 0 || dim > 256) return -1;
  const int l = dim / 4;
  if ((l & (l - 1)) != 0) return -1;
  int lg = 0;
  while ((1 << lg) < l) ++lg;
  return lg;
}

int launch_bag_pool_fwd(const float* rows, const int64_t* inv, const int64_t* bag_off, const float* w,
                        int64_t nbags, int dim, void* out, int odtype, int mean, hipStream_t s) {
  const int lg = bag_lg(dim);
  const int oalign = odtype == 1 ? 7 : 15;  // one lane stores 4 elements
  const bool vec = lg >= 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & oalign) == 0;
  if (nbags <= 0) return vec ? 1 : 0;
  if (vec) {
    const int grid = stream_grid(((nbags << lg) + 63) / 64 * 64, 256);
#define PSAMD_BF(O, W)                                                                                           \
  hipLaunchKernelGGL((bag_pool_fwd_vec_kernel<O, W>), dim3(grid), dim3(256), 0, s, rows, inv, bag_off, w, nbags, \
                     dim, lg, static_cast<O*>(out), mean);
    if (odtype == 1 && w) PSAMD_BF(uint16_t, true)
    else if (odtype == 1) PSAMD_BF(uint16_t, false)
    else if (w) PSAMD_BF(float, true)
    else PSAMD_BF(float, false)
#undef PSAMD_BF
    return 1;
  }
  const int grid = stream_grid(nbags * 64, 256);
#define PSAMD_BG(O, W)                                                                                       \
  hipLaunchKernelGGL((bag_pool_fwd_kernel<O, W>), dim3(grid), dim3(256), 0, s, rows, inv, bag_off, w, nbags, \
                     dim, static_cast<O*>(out), mean);
  if (odtype == 1 && w) PSAMD_BG(uint16_t, true)
  else if (odtype == 1) PSAMD_BG(uint16_t, false)
  else if (w) PSAMD_BG(float, true)
  else PSAMD_BG(float, false)
#undef PSAMD_BG
  return 0;
}

// --------------------------------------------------------------------------------- backward
// SC: the terms carry a scale (weights and / or mean); without one the kernel is the segment sum
// of dout rows read through bag_of[perm[j]], bit for bit segment_reduce_rows on the expanded rows
__device__ __forceinline__ float bag_term_scale(const int64_t* __restrict__ bag_off, const float* __restrict__ w,
                                                int64_t p, int64_t g, int mean) {
  float sc = w ? w[p] : 1.f;
  if (mean) sc *= bag_scale(bag_off, g);
  return sc;
}

template <typename S, bool SC>
__global__ __launch_bounds__(256) void bag_pool_bwd_kernel(const S* __restrict__ dout,
                                                           const int64_t* __restrict__ perm,
                                                           const int64_t* __restrict__ seg_off,
                                                           const int64_t* __restrict__ bag_of,
                                                           const int64_t* __restrict__ bag_off,
                                                           const float* __restrict__ w, int64_t nseg, int dim,
                                                           float* __restrict__ drows, int mean) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t u = wave; u < nseg; u += nwaves) {
    const int64_t b = seg_off[u], e = seg_off[u + 1];
    for (int c = lane; c < dim; c += 64) {
      float acc = 0.f;
      for (int64_t j = b; j < e; ++j) {
        const int64_t p = perm[j];
        const int64_t g = bag_of[p];
        const float v = Elem<S>::load(dout + g * dim, c);
        acc += SC ? bag_term_scale(bag_off, w, p, g, mean) * v : v;
      }
      drows[u * dim + c] = acc;
    }
  }
}

template <typename S, bool SC>
__global__ __launch_bounds__(256) void bag_pool_bwd_vec_kernel(const S* __restrict__ dout,
                                                               const int64_t* __restrict__ perm,
                                                               const int64_t* __restrict__ seg_off,
                                                               const int64_t* __restrict__ bag_of,
                                                               const int64_t* __restrict__ bag_off,
                                                               const float* __restrict__ w, int64_t nseg, int dim,
                                                               int lg, float* __restrict__ drows, int mean) {
  const int lane = threadIdx.x & 63;
  const int sub = lane >> lg;
  const int c = (lane & ((1 << lg) - 1)) * 4;
  const int per_wave = 64 >> lg;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t ub = wave * per_wave; ub < nseg; ub += nwaves * per_wave) {
    const int64_t u = ub + sub;
    if (u >= nseg) continue;
    const int64_t b = seg_off[u], e = seg_off[u + 1];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int64_t j = b;
    // 4 independent chains perm -> bag_of -> dout row in flight: a hot id is a latency chain otherwise
    for (; j + 4 <= e; j += 4) {
      const int64_t p0 = perm[j], p1 = perm[j + 1], p2 = perm[j + 2], p3 = perm[j + 3];
      const int64_t g0 = bag_of[p0], g1 = bag_of[p1], g2 = bag_of[p2], g3 = bag_of[p3];
      f32x4 v0 = load4(dout, g0 * dim + c), v1 = load4(dout, g1 * dim + c);
      f32x4 v2 = load4(dout, g2 * dim + c), v3 = load4(dout, g3 * dim + c);
      if (SC) {
        v0 *= bag_term_scale(bag_off, w, p0, g0, mean);
        v1 *= bag_term_scale(bag_off, w, p1, g1, mean);
        v2 *= bag_term_scale(bag_off, w, p2, g2, mean);
        v3 *= bag_term_scale(bag_off, w, p3, g3, mean);
      }
      acc += (v0 + v1) + (v2 + v3);
    }
    for (; j < e; ++j) {
      const int64_t p = perm[j];
      const int64_t g = bag_of[p];
      f32x4 v = load4(dout, g * dim + c);
      if (SC) v *= bag_term_scale(bag_off, w, p, g, mean);
      acc += v;
    }
    store4(drows, u * dim + c, acc);
  }
}

int launch_bag_pool_bwd(const void* dout, int ddtype, const int64_t* perm, const int64_t* seg_off,
                        const int64_t* bag_of, const int64_t* bag_off, const float* w, int64_t nseg, int dim,
                        float* drows, int mean, hipStream_t s) {
  const int lg = bag_lg(dim);
  const int dalign = ddtype == 1 ? 7 : 15;  // one lane loads 4 elements
  const bool vec = lg >= 0 && (reinterpret_cast<uintptr_t>(dout) & dalign) == 0 &&
                   (reinterpret_cast<uintptr_t>(drows) & 15) == 0;
  if (nseg <= 0) return vec ? 1 : 0;
  const bool sc = w != nullptr || mean != 0;
  if (vec) {
    const int grid = stream_grid(((nseg << lg) + 63) / 64 * 64, 256);
#define PSAMD_BB(S, SC)                                                                                    \
  hipLaunchKernelGGL((bag_pool_bwd_vec_kernel<S, SC>), dim3(grid), dim3(256), 0, s,                        \
                     static_cast<const S*>(dout), perm, seg_off, bag_of, bag_off, w, nseg, dim, lg, drows, \
                     mean);
    if (ddtype == 1 && sc) PSAMD_BB(uint16_t, true)
    else if (ddtype == 1) PSAMD_BB(uint16_t, false)
    else if (sc) PSAMD_BB(float, true)
    else PSAMD_BB(float, false)
#undef PSAMD_BB
    return 1;
  }
  const int grid = stream_grid(nseg * 64, 256);
#define PSAMD_BH(S, SC)                                                                                          \
  hipLaunchKernelGGL((bag_pool_bwd_kernel<S, SC>), dim3(grid), dim3(256), 0, s, static_cast<const S*>(dout),     \
                     perm, seg_off, bag_of, bag_off, w, nseg, dim, drows, mean);
  if (ddtype == 1 && sc) PSAMD_BH(uint16_t, true)
  else if (ddtype == 1) PSAMD_BH(uint16_t, false)
  else if (sc) PSAMD_BH(float, true)
  else PSAMD_BH(float, false)
#undef PSAMD_BH
  return 0;
}

}  // namespace psamd
