// Host-side launcher declarations for the ps_amd HIP kernels.
//
// The kernels live in csrc/kernels/*.hip (compiled by hipcc for gfx950 only); the torch
// bindings in csrc/bindings.cpp validate tensors and call these launchers on the current
// HIP stream.  Keeping this header free of torch lets the kernel TUs build in seconds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdexcept>
#include <string>

#include "psamd_opt_hyper.h"

namespace psamd {

// ---------------------------------------------------------------- optim.hip
struct FusedOptArgs {
  int kind;  // 0 sgd, 1 adam, 2 adagrad, 3 ftrl
  float* w;  // fp32 master shard (in/out)
  float* st0;  // momentum / adam m / adagrad h / ftrl z (nullable for plain sgd)
  float* st1;  // adam v / ftrl n (nullable)
  const void* g;  // gradient, bf16 (g_bf16) or fp32
  int g_bf16;
  void* wout;  // optional weight copy-out (pull buffer), bf16 (wout_bf16) or fp32
  int wout_bf16;
  int64_t n;
  OptHyper h;
  const float* gscale_ptr;  // optional device multiplier of the gradient (global-norm clip factor)
};
void launch_fused_opt(const FusedOptArgs& a, hipStream_t s);

// Multi-source gradient of the xGMI plane (optim.hip): element q of the gradient is the sum over
// s < nsrc, in order, of source s's value at chunk element off + q -- read from g[s] (bf16 when
// the FusedOptArgs say g_bf16, else fp32), or decoded from 1-bit words[s] / scales[s] (onebit;
// word q >> 6, scale q / kOnebitChunk, pointers at chunk element 0).
constexpr int kPlaneMaxSrc = 16;
struct MultiGrad {
  const void* g[kPlaneMaxSrc];
  const uint64_t* words[kPlaneMaxSrc];
  const float* scales[kPlaneMaxSrc];
  int nsrc;
  int onebit;
  int64_t off;
};
// fused optimizer over a segment (a.w / st / wout at the segment's first element; a.g unused)
void launch_fused_opt_multi(const FusedOptArgs& a, const MultiGrad& m, hipStream_t s);
// reduce only: out[0, n) fp32 = the multi-source gradient of the segment
void launch_reduce_multi(const MultiGrad& m, int g_bf16, int64_t n, float* out, hipStream_t s);

// ---------------------------------------------------------------- plane.hip
// up to kPlaneMaxSrc (src -> dst) copies issued as one launch (16-B aligned, sizes in bytes)
struct PlaneCopies {
  const void* src[kPlaneMaxSrc];
  void* dst[kPlaneMaxSrc];
  int64_t nbytes[kPlaneMaxSrc];
  int nseg;
};
// every segment ``nbytes`` long
void launch_plane_gather(const PlaneCopies& c, int64_t nbytes, hipStream_t s);
// one-node row exchange (sparse.hip, parallel/row_plane.py): every rank's arena pointers
struct RowPeers {
  const int64_t* skeys[kPlaneMaxSrc];  // unique keys sorted by owner
  const int64_t* meta[kPlaneMaxSrc];   // [2W]: offset of owner o's segment, then its count
  float* rows[kPlaneMaxSrc];           // [cap, dim] rows for skeys (written by the owners)
  const float* grads[kPlaneMaxSrc];    // [cap, dim] pushed gradient rows for skeys
  int W;
};
// worker <-> owner mailboxes of the asynchronous row tables: owner o's piece of a worker's
// owner-sorted buffer is [meta[o], meta[o] + meta[W + o]); cnt[o] (nullable) receives the count
struct PeerSegs {
  void* ptr[kPlaneMaxSrc];
  int64_t* cnt[kPlaneMaxSrc];
  int W;
};
void launch_segs_peers(bool to_peers, const void* local, int esize, const int64_t* meta, const PeerSegs& P,
                       int64_t width, int64_t cap, hipStream_t s);
void launch_keys_to_rows(const int64_t* keys, int64_t n, int64_t base, int64_t* rows, hipStream_t s);
void launch_system_acquire(hipStream_t s);
void launch_row_plane_recv(const RowPeers& P, int me, int64_t cap, int64_t* rkeys, int64_t* pmeta, hipStream_t s);
void launch_row_plane_send(const float* table, const int64_t* rslots, const int64_t* pmeta, const RowPeers& P,
                           int64_t cap, int dim, hipStream_t s);
void launch_row_plane_accum(const RowPeers& P, const int64_t* rslots, const int64_t* pmeta, float* acc, int32_t* tflag,
                            int32_t tag, int64_t* touched, int32_t* tcount, int64_t cap, int dim, hipStream_t s);
// segment sizes from c.nbytes
void launch_plane_copy(const PlaneCopies& c, hipStream_t s);
// total = sum_r *(float*)c.src[r] (rank order); factor = min(1, max_norm / (sqrt(total) + 1e-6))
void launch_plane_clip_factor(const PlaneCopies& c, float max_norm, float* total, float* factor, hipStream_t s);
void launch_plane_fill(float* p, int64_t n, float v, hipStream_t s);

struct SparseOptArgs {
  int kind;
  float* table;  // [rows_total, dim] owner-local fp32 table
  float* st0;
  float* st1;
  const int64_t* rows;  // [nrows] owner-local rows: unique (perm null) or sorted with repeats
  const int64_t* perm;  // nullable: grad row of sorted entry j is perm[j] (runs are summed)
  const void* grad;     // [nrows, dim]
  int g_bf16;
  int64_t nrows;
  int dim;
  int rowwise;  // adagrad: one accumulator per row
  int skip_zero;  // FTRL: skip a row whose first gradient element is 0 (reference)
  OptHyper h;
  const int32_t* ncount = nullptr;  // nullable device count: only rows [0, min(nrows, *ncount)) are live
};
void launch_sparse_opt(const SparseOptArgs& a, hipStream_t s);

// ---------------------------------------------------------------- reduce.hip
// dtype codes: 0 = fp32, 1 = bf16
void launch_sumsq_partial(const void* x, int dtype, int64_t n, float* partial, int nblocks, hipStream_t s);
void launch_sumsq_finish(const float* partial, int nblocks, float* out, int accumulate, hipStream_t s);
void launch_clip_factor(const float* sumsq, float max_norm, float* factor, hipStream_t s);
void launch_cast(const void* x, int xdtype, void* y, int ydtype, int64_t n, float scale, hipStream_t s);
void launch_axpy(float a, const void* x, int xdtype, void* y, int ydtype, int64_t n, hipStream_t s);
void launch_reduce_n(const void* x, int xdtype, int k, int64_t n, void* y, int ydtype, float scale, hipStream_t s);
void launch_lerp(const float* w0, const float* w, float sc, void* out, int odtype, int64_t n, hipStream_t s);
int sumsq_blocks(int64_t n);

// ---------------------------------------------------------------- compress.hip
// 1-bit sign compression with per-chunk scale and error feedback (K26).
constexpr int kOnebitChunk = 1024;
// mom (nullable, err's dtype): 1-bit Adam -- compress the worker momentum beta1 m + (1 - beta1) g
void launch_onebit_pack(const void* g, int gdtype, void* err, int edtype, int64_t n, uint64_t* words, float* scales,
                        hipStream_t s, void* mom = nullptr, float beta1 = 0.f);
void launch_onebit_momentum(const void* g, int gdtype, void* mom, int mdtype, int64_t n, float beta1, hipStream_t s);
void launch_onebit_unpack_reduce(const uint64_t* words, const float* scales, int nworkers, int64_t n,
                                 int64_t words_stride, int64_t scales_stride, void* out, int odtype, float mult,
                                 int accumulate, hipStream_t s);

// ---------------------------------------------------------------- bags.hip
// -> the path taken: 0 generic (one wave per bag / segment), 1 vector (2^lg lanes, 16-B loads)
int launch_bag_pool_fwd(const float* rows, const int64_t* inv, const int64_t* bag_off, const float* w,
                        int64_t nbags, int dim, void* out, int odtype, int mean, hipStream_t s);
int launch_bag_pool_bwd(const void* dout, int ddtype, const int64_t* perm, const int64_t* seg_off,
                        const int64_t* bag_of, const int64_t* bag_off, const float* w, int64_t nseg, int dim,
                        float* drows, int mean, hipStream_t s);

// ---------------------------------------------------------------- sparse.hip
void launch_gather_rows(const void* table, int tdtype, const int64_t* rows, int64_t nrows, int dim, void* out,
                        int odtype, int64_t out_ld, int64_t out_off, int act, hipStream_t s);
void launch_segment_reduce_rows(const void* src, int sdtype, const int64_t* perm, const int64_t* seg_off,
                                int64_t nseg, int dim, void* out, int odtype, int mean, hipStream_t s);
void launch_scatter_add_rows(const void* src, int sdtype, const int64_t* rows, int64_t nrows, int dim, float* table,
                             hipStream_t s);
void launch_embedding_bag_fwd(const float* table, const int64_t* ids, int64_t batch, int fields, int dim,
                              void* out, int odtype, int64_t out_ld, int64_t out_off, int act, hipStream_t s);
void launch_sparse_lr_fwd(const float* w, const int64_t* ids, int64_t batch, int fields, int64_t hash_size,
                          const float* bias, float* out, hipStream_t s);
void launch_lazy_init_rows(float* table, const int64_t* rows, const int64_t* keys, int64_t nrows, int dim,
                           uint8_t* init_flags, uint64_t seed, int64_t row_base, float lo, float hi, hipStream_t s);
void launch_unique_runs(const int64_t* srt, const int64_t* uidx, int64_t n, int64_t mask, int64_t* ukeys,
                        int64_t* seg, hipStream_t s);
void launch_hash_slots(int64_t* hkeys, int64_t capacity, const int64_t* ids, int64_t n, int64_t* out, int insert,
                       int32_t* status, hipStream_t s);
// rehash of a map-mode shard into a larger one (keys, rows, flags, up to kRehashMaxState optimizer
// states: st_full[i] = 1 for [cap, dim], 0 for row-wise [cap]); new_* pre-filled (-1 keys, zeros);
// remap[old_cap] receives the new slot of every old position (-1 = was empty).  lg is the launcher's.
constexpr int kRehashMaxState = 4;
struct RehashArgs {
  const int64_t* old_hkeys;
  int64_t old_cap;
  int64_t* new_hkeys;
  int64_t new_cap;  // power of two
  const float* old_table;
  float* new_table;
  int dim;
  const uint8_t* old_flags;
  uint8_t* new_flags;
  const float* old_st[kRehashMaxState];
  float* new_st[kRehashMaxState];
  int st_full[kRehashMaxState];
  int nstate;
  int64_t* remap;
  int lg;
  // compact_rows only (the filtered form): a position moves iff its key is live and
  // old_stamp >= cutoff; counters = {rows placed, rows evicted} (added to); status is set when a
  // survivor finds the target full
  const int32_t* old_stamp;
  int32_t* new_stamp;
  int32_t cutoff;
  int64_t* counters;
  int32_t* status;
};
void launch_rehash_rows(const RehashArgs& a, hipStream_t s);
// the same pass with the filter: new_cap is any power of two, smaller than old_cap included
void launch_compact_rows(const RehashArgs& a, hipStream_t s);
// hash_slots with insert that also writes stamp[slot] = now; with table != nullptr a key found
// with stamp < cutoff has its slot reset to a fresh one's state (row, flag, states zero)
struct StampRebirth {
  float* table;
  uint8_t* flags;
  float* st[kRehashMaxState];
  int st_full[kRehashMaxState];
  int nstate;
  int dim;
};
void launch_hash_slots_stamp(int64_t* hkeys, int64_t capacity, const int64_t* ids, int64_t n, int64_t* out,
                             int32_t* stamp, int32_t now, int32_t cutoff, const StampRebirth& r, int32_t* status,
                             hipStream_t s);

// ---------------------------------------------------------------- fc.hip
// fused FC backward: dW = (act'(y) * dy)^T x (+ db = column sums), dX = (act'(y) * dy) W;
// dtype 0 fp32 / 1 bf16 for every operand; dw / db / dx nullable
void launch_fc_bwd(const void* dy, const void* y, const void* x, const void* w, void* dw, float* db, void* dx,
                   int dtype, int M, int N, int K, int act, float* ws, hipStream_t s);
// fp32 workspace (floats) of the split-reduction dW path, 0 = unsplit
int64_t fc_bwd_ws_floats(int M, int N, int K);
void launch_fc_fwd_f32(const float* x, const float* w, const float* b, float* y, int M, int N, int K, int act,
                       hipStream_t s);

// ---------------------------------------------------------------- ref_ops.hip
void launch_softmax_temp_fwd(const float* x, float* y, int64_t rows, int cols, float inv_temp, float clamp_lo,
                             float clamp_hi, hipStream_t s);
void launch_softmax_temp_bwd(const float* p, const float* dy, float* dx, int64_t rows, int cols, float scale,
                             hipStream_t s);
void launch_softmax_xent(const float* p, const int64_t* labels, int64_t rows, int cols, float* loss,
                         float* grad, hipStream_t s);
void launch_bce(const float* p, const float* y, int64_t n, float* loss, float* grad, hipStream_t s);
void launch_maxpool2d_fwd(const void* x, int dtype, int64_t nc, int h, int w, int k, int stride, int pad,
                          void* y, int32_t* argmax, int oh, int ow, hipStream_t s);
void launch_maxpool2d_bwd(const void* dy, int dtype, const int32_t* argmax, int64_t nc, int h, int w, int oh,
                          int ow, int k, int stride, int pad, void* dx, hipStream_t s);
void launch_im2col(const float* x, int64_t n, int c, int h, int w, int k, int stride, int pad, int oh, int ow,
                   float* col, hipStream_t s);
void launch_col2im(const float* col, int64_t n, int c, int h, int w, int k, int stride, int pad, int oh, int ow,
                   float* x, hipStream_t s);
void launch_dropout_fwd(const void* x, int dtype, void* y, int64_t n, float p_drop, uint64_t seed,
                        uint64_t offset, hipStream_t s);
void launch_dropout_bwd(const void* dy, int dtype, void* dx, int64_t n, float p_drop, uint64_t seed,
                        uint64_t offset, hipStream_t s);
void launch_uniform_init(float* w, int64_t n, uint64_t seed, uint64_t offset, float lo, float hi, hipStream_t s);

// ---------------------------------------------------------------- bn_act.hip
// NHWC BatchNorm (+residual) + activation; x/y/dy/dx/res bf16 [R, C]; params/stats fp32 [C].
struct BnFwdArgs {
  const uint16_t* x;
  const uint16_t* res;  // nullable
  uint16_t* y;
  const float* gamma;   // nullable (affine=False)
  const float* beta;
  float* rmean;         // nullable (no running stats)
  float* rvar;
  float* mean;          // [C] saved for backward
  float* invstd;        // [C]
  float* scale;         // [C] scratch
  float* shift;         // [C] scratch
  float* ws;            // [2, G, C] partials
  int64_t R;
  int C;
  int G;
  int act;
  int training;
  float eps, momentum;
};
void launch_bn_fwd(const BnFwdArgs& a, hipStream_t s);

void launch_maxpool_nhwc_fwd(const uint16_t* x, const float* coef, uint16_t* y, uint8_t* idx, int N, int H, int W,
                             int C, int OH, int OW, int k, int s, int p, hipStream_t st);
void launch_maxpool_nhwc_bwd(const uint16_t* dy, const uint8_t* idx, uint16_t* dx, int N, int H, int W, int C, int OH,
                             int OW, int k, int s, int p, hipStream_t st);
// stem backward: maxpool 3x3/2/1 scatter fused into the BN(+ReLU) backward of its input z
// (mc = the forward's [scale | shift]); ws: [2 G C + 3 C] fp32, G = pool_bn_bwd_blocks(...);
// dz == nullptr: the statistics pass only (dgamma, dbeta and the coefficients at ws + 2 G C)
int pool_bn_bwd_blocks(int64_t N, int H, int W, int C);
void launch_pool_bn_bwd(const uint16_t* dy, const uint8_t* idx, const uint16_t* z, const float* mc, const float* mean,
                        const float* invstd, const float* gamma, float* ws, int G, float* dgamma, float* dbeta,
                        uint16_t* dz, int N, int H, int W, int C, int OH, int OW, hipStream_t st);

// ---------------------------------------------------------------- stem.hip (ResNet 7x7/2 stem, MFMA)
// x: [N, H, W, cin] bf16, cin 3 or 4 (channel 3 meets zero weights); wp: [64][224] packed
// bf16 (k' = kh*32 + kw*4 + c); z: [N, OH, OW, 64] bf16; OW <= 128.
// kshift/part optional: per-block BN partial sums of z about kshift -> part[2][blocks][64]
void launch_stem_conv_fwd(const uint16_t* x, int cin, const uint16_t* wp, uint16_t* z, int N, int H, int W, int OH,
                          int OW, const float* kshift, float* part, hipStream_t s);
int stem_fwd_blocks(int N);
int stem_wrw_blocks(int N, int OH);
// Tall [G][C] partial pairs: rows S = partials_fold_rows(G) (0: no fold needed) of a first-level
// fixed-order sum into op/oq [S][C]
int partials_fold_rows(int G);
void launch_partials_fold(const float* p, const float* q, int G, int C, float* op, float* oq, hipStream_t s);
// BN finalize from producer-fused partial sums ps/pq: [G][C] of sum(x - k), sum((x - k)^2)
void launch_bn_finalize_sums(const float* ps, const float* pq, const float* kshift, int G, int C, int64_t R,
                             float eps, float momentum, const float* gamma, const float* beta, float* rmean,
                             float* rvar, float* mean, float* invstd, float* scale, float* shift, hipStream_t s);
// ws: (stem_wrw_blocks + 32) * 64 * 224 floats; dwp: [64][224] fp32 packed weight gradient
// pool_dy != nullptr: FUSED -- dz is z (the stem BN's input) and each dz row is computed in the
// kernel from the pooled gradient pool_dy / pool_idx ([N, OH/2, OW/2, 64]), mc ([2 * 64] scale |
// shift) and coef ([3 * 64] bn backward ca | cb | cc; pool.hip launch_pool_bn_bwd with dz null)
void launch_stem_conv_wrw(const uint16_t* x, int cin, const uint16_t* dz, float* ws, float* dwp, int N, int H, int W,
                          int OH, int OW, hipStream_t s, const uint16_t* pool_dy = nullptr,
                          const uint8_t* pool_idx = nullptr, const float* mc = nullptr, const float* coef = nullptr);

// ---------------------------------------------------------------- transformer.hip (row / elementwise)
void launch_rmsnorm_fwd(const uint16_t* x, const uint16_t* r, const void* w, bool w_bf16, uint16_t* s, uint16_t* y,
                        float* rstd, int R, int D, float eps, hipStream_t st);
int rmsnorm_bwd_parts(int R);
void launch_rmsnorm_bwd(const uint16_t* dy, const uint16_t* s, const void* w, bool w_bf16, const float* rstd,
                        const uint16_t* ds_in, uint16_t* dx, float* wpart, float* dw, int R, int D, hipStream_t st);
void launch_layernorm_fwd(const uint16_t* x, const uint16_t* o, const void* gamma, const void* beta, bool w_bf16,
                          uint16_t* s, uint16_t* y, float* mean, float* rstd, int R, int D, float eps, float p,
                          uint64_t seed, hipStream_t st);
int layernorm_bwd_parts(int R);
void launch_layernorm_bwd(const uint16_t* dy, const uint16_t* s, const void* gamma, bool w_bf16, const float* mean,
                          const float* rstd, uint16_t* dx, uint16_t* dout, float* part, float* dgamma, float* dbeta,
                          int R, int D, float p, uint64_t seed, hipStream_t st);
void launch_swiglu_fwd(const uint16_t* gu, uint16_t* h, int64_t R, int F, hipStream_t st);
void launch_swiglu_bwd(const uint16_t* dh, const uint16_t* gu, uint16_t* dgu, int64_t R, int F, hipStream_t st);
void launch_rope_split_fwd(const uint16_t* qkv, const float* cs, uint16_t* q, uint16_t* k, uint16_t* v, int B, int S,
                           int H, int KV, int hd, hipStream_t st);
void launch_rope_split_bwd(const uint16_t* dq, const uint16_t* dk, const uint16_t* dv, const float* cs,
                           uint16_t* dqkv, int B, int S, int H, int KV, int hd, hipStream_t st);

struct BnBwdArgs {
  const uint16_t* dy;
  const uint16_t* y;          // nullable when mask_coef is given (relu, no residual)
  const float* mask_coef;     // nullable: forward [scale | shift], relu mask recomputed from x
  const uint16_t* x;
  const float* gamma;
  const float* mean;
  const float* invstd;
  float* dgamma;  // nullable
  float* dbeta;   // nullable
  uint16_t* dx;
  uint16_t* dres;  // nullable: gradient of the fused residual input (= dz)
  const uint8_t* mbits;  // nullable: ReLU mask bits of the forward output (1 bit / element)
  float* ws;       // [2, G, C] partials + [3, C] coefficients
  int64_t R;
  int C;
  int G;
  int act;
};
void launch_bn_bwd(const BnBwdArgs& a, hipStream_t s);
int bn_red_blocks(int64_t R, int C);

// ---------------------------------------------------------------- dense.hip (MFMA)
// C[M,N] (+)= act(alpha * A[M,K] . B[N,K]^T + bias[N]); A, B bf16 K-contiguous; C bf16 or fp32.
// act: 0 none, 1 relu, 2 leaky relu(0.01), 3 reference clipped sigmoid (0.001 + 0.998*sigmoid)
void launch_gemm_nt_bf16(const uint16_t* a, int64_t lda, const uint16_t* b, int64_t ldb, void* c, int c_f32,
                         int64_t ldc, int M, int N, int K, float alpha, int accumulate, const float* bias, int act,
                         hipStream_t s);
void launch_act_bwd(const uint16_t* dy, const uint16_t* y, uint16_t* dz, int64_t n, int act, hipStream_t s);
// DLRM dot interaction: out [B, D + n(n-1)/2] = [x | triu(z z^T)], z = [x; e[b]] (n = T+1 <= 32, D % 32 == 0)
void launch_dlrm_interact_fwd(const uint16_t* x, const uint16_t* e, uint16_t* out, int B, int T, int D,
                              hipStream_t s);
void launch_dlrm_interact_bwd(const uint16_t* x, const uint16_t* e, const uint16_t* dout, uint16_t* dx, uint16_t* de,
                              int B, int T, int D, hipStream_t s);

// ---------------------------------------------------------------- convgemm.hip (MFMA implicit-GEMM convs)
// NHWC conv geometry of the A operand: input map H x W x C, output map OH x OW, square kernel
// ks with stride / pad.  Reduction index k = (kh * ks + kw) * C + c (channels_last weight order).
struct ConvGeo {
  int H, W, OH, OW, C, ks, stride, pad;
  int ksw;             // taps along the width (0: = ks, square kernel)
  int RH, RW, ra, rb;  // RH > 0: output pixel (i, oh, ow) lands at row (i, 2 oh + ra, 2 ow + rb) of an
                       // RH x RW map (one phase of a stride-2 data gradient); 0: rows in order
};
// n / d for 0 <= n < 2^31 as (umulhi(n, mul) + n) >> shift (d fixed per launch): the wide
// weight-gradient kernel decodes pixel indices with it instead of two integer divisions per DMA
// instruction per stage.
struct FastDiv {
  uint32_t mul, shift;
};
inline FastDiv make_fastdiv(uint32_t d) {
  uint32_t sh = 0;
  while (sh < 32 && (uint64_t(1) << sh) < d) ++sh;
  const uint64_t one = 1;
  return FastDiv{static_cast<uint32_t>(((one << 32) * ((one << sh) - d)) / d + 1), sh};
}
// conv_gemm's contract: which epilogue runs on the output tile, which prologue on the A rows.
// The values are the binding's ``epi`` integers and the kernels' EPI / PRO template arguments.
enum ConvEpi : int {
  kEpiStore = 0,            // c = the GEMM result
  kEpiStats = 1,            // + BN partial sums of c about kshift -> part
  kEpiAdd = 2,              // + residual rows aux
  kEpiMaskSums = 3,         // ReLU mask of the BN (mc, input z = aux) + its backward sums (mean, invstd) -> part
  kEpiAddS2 = 4,            // + residual aux of the (OH+1)/2 x (OW+1)/2 map at even (h, w)
  kEpiAddMasked = 5,        // + aux * relu'(forward output), the mask from bits
  // the fold epilogues: a base epilogue + the previous block's bn3 backward reduce (aux2, bits2,
  // mean, invstd) -- the output is masked by bits2 and its sums go to part
  kEpiFoldAddMasked = 6,    // kEpiAddMasked + fold
  kEpiFoldAdd = 7,          // kEpiAdd + fold
  kEpiFoldAddS2 = 8,        // kEpiAddS2 + fold
  kEpiFoldAddMaskedDs = 9,  // kEpiFoldAddMasked + the previous block's downsample-BN sum (aux3, mean2,
                            // invstd2) as a third slab of part
  kEpiCount = 10
};
enum ConvPro : int {
  kProNone = 0,
  kProBnRelu = 1,    // A := relu(A * scale + shift) while staging (pro)
  kProBnBwd = 2,     // A := bf16(ca * a + cb * a2 + cc), also stored to aout (bwd, a2)
  kProBlockOut = 3   // A := relu(a * sc + sh + r), r = a2 or a2 * sc2 + sh2; -> aout, abits (pro, a2, pro2)
};
// the launch's two-source prologue, as the tile plans see it
enum ConvSrc2 : int { kSrc2None = 0, kSrc2BlockOut = 1, kSrc2BnBwd = 2 };

// The one decode of an epilogue number.
constexpr bool epi_valid(int64_t e) { return e >= kEpiStore && e < kEpiCount; }
constexpr bool epi_folds_ds(int e) { return e == kEpiFoldAddMaskedDs; }
constexpr bool epi_folds(int e) {
  return e == kEpiFoldAddMasked || e == kEpiFoldAdd || e == kEpiFoldAddS2 || epi_folds_ds(e);
}
constexpr int epi_base(int e) {  // the epilogue a fold epilogue extends (itself for the others)
  return e == kEpiFoldAddMasked || epi_folds_ds(e) ? kEpiAddMasked
         : e == kEpiFoldAdd                        ? kEpiAdd
         : e == kEpiFoldAddS2                      ? kEpiAddS2
                                                   : e;
}
constexpr bool epi_writes_sums(int e) { return e == kEpiStats || e == kEpiMaskSums || epi_folds(e); }
constexpr int epi_sum_slabs(int e) { return epi_folds_ds(e) ? 3 : 2; }  // part is [slabs][gm][N]
constexpr bool epi_reads_aux(int e) { return e != kEpiStore && e != kEpiStats; }
constexpr bool epi_needs_bits(int e) { return epi_base(e) == kEpiAddMasked; }
constexpr bool epi_needs_aux2(int e) { return epi_folds(e); }  // aux2, bits2, mean, invstd
constexpr bool epi_needs_aux3(int e) { return epi_folds_ds(e); }  // aux3, mean2, invstd2
constexpr bool epi_is_fwd(int e) { return e == kEpiStore || e == kEpiStats; }
// Whether any kernel pairs this prologue with this epilogue: the forward prologues feed the
// forward epilogues, the BN-backward prologue a data-gradient epilogue (the 128-pixel tiles only
// kEpiMaskSums: conv_fwd_runs).
constexpr bool conv_pro_epi_exists(int pro, int epi) {
  return epi_valid(epi) && (pro == kProNone || ((pro == kProBnRelu || pro == kProBlockOut) && epi_is_fwd(epi)) ||
                            (pro == kProBnBwd && !epi_is_fwd(epi)));
}
constexpr int pro_src2(int pro) {
  return pro == kProBlockOut ? kSrc2BlockOut : pro == kProBnBwd ? kSrc2BnBwd : kSrc2None;
}
// Launch ladders.  `switch (epi) { PSAMD_EPIS_X(L, args) default: conv_no_kernel(pro, epi); }`
// runs L(args, E) for the epilogues E that set X lists and throws for every other: the lists are
// the kernel instantiations of the launchers.  (kEpiStore comes last in each: the order the
// kernels have had in the code object.)
#define PSAMD_EPI_CASE(L, E, ...) \
  case E: L(__VA_ARGS__, E); break;
#define PSAMD_EPIS_FWD(L, ...) PSAMD_EPI_CASE(L, kEpiStats, __VA_ARGS__) PSAMD_EPI_CASE(L, kEpiStore, __VA_ARGS__)
#define PSAMD_EPIS_ADD(L, ...) /* the residual / fold epilogues every tile has */                                  \
  PSAMD_EPI_CASE(L, kEpiAddS2, __VA_ARGS__) PSAMD_EPI_CASE(L, kEpiAddMasked, __VA_ARGS__)                          \
  PSAMD_EPI_CASE(L, kEpiFoldAddMasked, __VA_ARGS__) PSAMD_EPI_CASE(L, kEpiFoldAdd, __VA_ARGS__)                    \
  PSAMD_EPI_CASE(L, kEpiFoldAddS2, __VA_ARGS__)
#define PSAMD_EPIS_NO_DS(L, ...) /* all but kEpiFoldAddMaskedDs */                                                 \
  PSAMD_EPI_CASE(L, kEpiStats, __VA_ARGS__) PSAMD_EPI_CASE(L, kEpiAdd, __VA_ARGS__)                                \
  PSAMD_EPI_CASE(L, kEpiMaskSums, __VA_ARGS__) PSAMD_EPIS_ADD(L, __VA_ARGS__) PSAMD_EPI_CASE(L, kEpiStore, __VA_ARGS__)
#define PSAMD_EPIS_ALL(L, ...)                                                                                     \
  PSAMD_EPI_CASE(L, kEpiStats, __VA_ARGS__) PSAMD_EPI_CASE(L, kEpiAdd, __VA_ARGS__)                                \
  PSAMD_EPI_CASE(L, kEpiMaskSums, __VA_ARGS__) PSAMD_EPIS_ADD(L, __VA_ARGS__)                                      \
  PSAMD_EPI_CASE(L, kEpiFoldAddMaskedDs, __VA_ARGS__) PSAMD_EPI_CASE(L, kEpiStore, __VA_ARGS__)
#define PSAMD_EPIS_DGRAD(L, ...) /* all but the forward ones (the BN-backward prologue on the 256 x 256 tiles) */  \
  PSAMD_EPI_CASE(L, kEpiAdd, __VA_ARGS__) PSAMD_EPIS_ADD(L, __VA_ARGS__)                                           \
  PSAMD_EPI_CASE(L, kEpiFoldAddMaskedDs, __VA_ARGS__) PSAMD_EPI_CASE(L, kEpiMaskSums, __VA_ARGS__)
[[noreturn]] inline void conv_no_kernel(int pro, int epi) {
  throw std::invalid_argument("conv_gemm: no kernel for prologue " + std::to_string(pro) + " with epilogue " +
                              std::to_string(epi) + " on this tile");
}

struct ConvGemmArgs {
  const uint16_t* a;    // [images, H, W, C] bf16
  const uint16_t* b;    // [N, K] bf16, K = ks * ks * C
  uint16_t* c;          // [M, N] bf16, M = images * OH * OW
  int M, N, K;
  ConvGeo g;
  const float* pro;     // [scale | shift] (2C): A := relu(A * scale + shift) while staging; nullable
  int epi;              // ConvEpi
  const uint16_t* aux;  // epi_reads_aux: residual rows; kEpiMaskSums: BN input z [M, N]
  const uint8_t* bits;  // epi_needs_bits: ReLU mask bits of aux's elements
  const uint16_t* aux2; // epi_needs_aux2: previous block's bn3 input z3 [M, N]
  const uint8_t* bits2; // epi_needs_aux2: ReLU mask bits of the previous block's output (= this input)
  const float* kshift;  // kEpiStats: shift of the partial sums [N] (nullable = 0)
  const float* mc;      // kEpiMaskSums: [scale | shift] (2N) of that BN (ReLU mask)
  const float* mean;    // kEpiMaskSums / epi_needs_aux2: [N]
  const float* invstd;  // kEpiMaskSums / epi_needs_aux2: [N]
  float* part;          // epi_writes_sums: [epi_sum_slabs][conv_fwd_plan(M, N, K, pro).gm][N] block partial sums
  const uint16_t* aux3; // epi_needs_aux3: the previous block's downsample-BN input zd [M, N]
  const float* mean2;   // epi_needs_aux3: [N] that BN's batch mean / inverse std
  const float* invstd2;
  // kProBnBwd (1x1; excludes pro): the previous BN's data gradient from its output gradient a and
  // input a2 (coefficients bwd = [ca | cb | cc], 3C); the A tile is also stored to aout [M, C] (by
  // the channel-tile-0 blocks)
  const uint16_t* a2;   // [M, C] BN input; nullable
  const float* bwd;     // [3C]
  uint16_t* aout;       // [M, C]
  // kProBlockOut (1x1 forward; pro and a2 set, bwd null): pro = [sc | sh] of bn3, r = a2 (identity)
  // or a2 * sc2 + sh2 (pro2 = the downsample BN's [sc2 | sh2]); the block output goes to aout, its
  // ReLU bits to abits [M C / 8]
  const float* pro2;    // [2C]; nullable
  uint8_t* abits;
  FastDiv fd_ohw, fd_ow;  // set by launch_conv_fwd (OH * OW, OW)
  int pgm;                // rows per partial slab (0: the launch's gm); several GEMMs share one part
  uint64_t* tbuf = nullptr;  // conv_big only, diagnostics: 8 wall-clock stamps per block (nullable)
};
// the prologue a launch runs, from the pointers that are set (the binding checks the rest)
inline int conv_pro(const ConvGemmArgs& a) {
  return a.bwd != nullptr ? kProBnBwd : a.pro == nullptr ? kProNone : a.a2 != nullptr ? kProBlockOut : kProBnRelu;
}
inline int conv_src2(const ConvGemmArgs& a) { return pro_src2(conv_pro(a)); }
struct ConvFwdPlan {
  int bm, bn, gm;       // tile pixels / channels, pixel-tile groups (partial-sum rows)
};
ConvFwdPlan conv_fwd_plan(int M, int N, int K, bool pro, int epi = 0);
// conv_big.hip: 256 x 256 tiles, one 512-thread block per CU, for deep-K 1x1 GEMMs (every epilogue);
// conv_fwd_plan_geo / launch_conv_fwd route there when conv_big_tn is not 0 (gm = conv_big_gm(M))
// the channel tile conv_big runs for this GEMM: 256, 0 = not eligible
int conv_big_tn(int M, int N, int K, bool pro, const ConvGeo& g, int src2, int epi);
int conv_big_gm(int M);
// whether launch_conv_big instantiates this (ConvPro, ConvEpi)
bool conv_big_runs(int pro, int epi);
void launch_conv_big(const ConvGemmArgs& a, hipStream_t s);
// the four stride-2 data-gradient phase GEMMs (no prologue, LDS-DMA staging, 128-pixel tiles) in
// one launch; phase i's partials go to rows [sum gm(<i), ..) of a part with pgm = sum of gm
void launch_conv_dgrad_phases(const ConvGemmArgs* ph, hipStream_t s);
bool conv_dgrad_phases_runs(int epi);  // kEpiStore or kEpiMaskSums
int conv_dgrad_phase_gm(int M);
// the plan launch_conv_fwd uses for this geometry (the 3x3 patch-staged tiles where they apply)
// src2: the launch's two-source prologue (ConvSrc2)
ConvFwdPlan conv_fwd_plan_geo(int M, int N, int K, bool pro, const ConvGeo& g, int src2 = 0, int epi = 0);
// whether the tile family of plan pl instantiates this (ConvPro, ConvEpi): launch_conv_fwd throws
// std::invalid_argument where it does not, and the binding checks before it launches
bool conv_fwd_runs(const ConvFwdPlan& pl, int pro, int epi);
void launch_conv_fwd(const ConvGemmArgs& a, hipStream_t s);
// the kernel family launch_conv_fwd runs for plan pl (its ladder branches on this value only)
enum ConvFwdFamily : int {
  kFamBig = 0,         // conv_big.hip, 256 x 256 tiles
  kFamTwosrcGlds = 1,  // two-source prologue, LDS-DMA staging
  kFamPatch = 2,       // 3x3 patch-staged tiles
  kFamTall = 3,        // 256 x 64 tiles, LDS-DMA staging
  kFamTwosrcReg = 4,   // two-source prologue, register staging
  kFamGlds = 5,        // no prologue, LDS-DMA staging, one tile per block
  kFamReg = 6          // register staging (persistent grid where the plan says so)
};
int conv_fwd_family(const ConvFwdPlan& pl, int M, int N, int K, const ConvGeo& g, int pro, int epi);
// two-source prologues with K >= 64 x this run on the LDS-DMA variant (convgemm.hip;
// profiles/r4_twosrc_probe.txt: LDS-DMA ahead at every K >= 256)
constexpr int kTwosrcGldsMinNk = 4;
// whether launch_conv_wgrad runs the 3x3 patch kernel for this weight gradient (convgemm.hip)
bool conv_wgrad_patch_ok(const ConvGeo& g, int M, int N, bool pro);
// Backward layouts of many conv weights in one launch: jobs = device array of
// {src, dst, kind (0 1x1 transpose, 1 3x3 flip-transpose, 2 3x3 stride-2 phases), A, B} (32 B each)
void launch_weight_prep(const void* jobs, int njobs, int max_blocks, hipStream_t s);

// Fused backward of a bottleneck's last 1x1 conv (conv3: CI -> CO channels) with bn3's backward
// in its prologue (conv_bwd_fused.hip): per 128-pixel tile, dz3 = bf16(ca g + cb z3 + cc) is built
// in LDS one 64-channel stage at a time and feeds BOTH GEMMs -- the data gradient
// gy = dz3 W3 (bn2's ReLU mask + backward sums in the epilogue, the conv_gemm kEpiMaskSums contract) and
// the weight gradient dW3 += dz3^T relu(bn2(z2)) (per-block fp32 slabs, fixed-order reduce) --
// so dz3 never reaches HBM and z2 is read once for both.
struct Conv11BwdArgs {
  const uint16_t* g;      // [M, CO] gradient at bn3's output (already ReLU-masked)
  const uint16_t* z3;     // [M, CO] bn3 input
  const float* cbwd;      // [3 CO] ca | cb | cc (bn3 backward coefficients)
  const uint16_t* wt;     // [CI, CO] conv3 weight transposed
  const uint16_t* z2;     // [M, CI] bn2 input (conv3's input before bn2 + ReLU)
  const float* cf2;       // [2 CI] bn2 scale | shift; nullptr: PLAIN (downsample: z2 used as is,
                          // gy unmasked, no part) -- the 64 -> 256 kernel only
  const float* mean2;     // [CI]
  const float* invstd2;   // [CI]
  uint16_t* gy;           // [M, CI] masked data gradient (bn2's output gradient)
  float* part;            // [2][gm][CI] bn2 backward partial sums
  float* ws;              // conv11_bwd_ws(M, CI, CO) floats: dW slabs (+ reduce scratch)
  uint16_t* dw;           // [CO, CI] bf16 conv3 weight gradient
  int M;
};
bool conv11_bwd_fused_ok(int CI, int CO);
bool conv11_bwd_plain_ok(int CI, int CO);
bool conv11_bwd_built(int CI, int CO);  // launchable (conv11_bwd_fused_ok: also chosen by default)
int conv11_bwd_blocks(int M, int CI, int CO);
int64_t conv11_bwd_ws(int M, int CI, int CO);
void launch_conv11_bwd_fused(const Conv11BwdArgs& a, int CI, int CO, hipStream_t s);

struct ConvWgradArgs {
  const uint16_t* dz;   // [M, N] output gradient rows
  const uint16_t* x;    // [images, H, W, C] input map
  int M, N, K;          // K = ks * ks * C
  ConvGeo g;
  const float* pro;     // [scale | shift] (2C) applied to x while staging; nullable
  float* ws;            // conv_wgrad_ws(M, N, K, C) floats
  uint16_t* dw;         // [N, K] bf16
  float* db;            // nullable: [N] fp32 column sums of dz (a Linear's bias gradient; wide plan only)
  float* dbws;          // [conv_wgrad_splits(...)][N] fp32 scratch when db is set
  FastDiv fd_ohw, fd_ow;  // set by launch_conv_wgrad (OH * OW, OW)
};
int conv_wgrad_splits(int M, int N, int K, int C, bool pro);
// The plan launch_conv_wgrad picks (no db): kind 0 conv_wgrad_kernel, 1-4 the wide tiles (256 x 256,
// 256 x 128, 128 x 256, 128 x 384), 5 the 3x3 patch kernel; the dW tile tn x tk (output channels x
// reduction columns), tiles, pixel splits (= fp32 slabs), pixels per split (patch: 112-pixel stages per
// split) and the first-level slab-reduce groups (0: one reduce level)
struct ConvWgradPlan {
  int kind, tn, tk, tiles, nsplit, rows, groups;
};
ConvWgradPlan conv_wgrad_plan(int M, int N, int K, const ConvGeo& g, bool pro, bool db = false);
// workspace of launch_conv_wgrad for this geometry (the 3x3 patch kernel's plan where it applies)
int64_t conv_wgrad_ws_geo(int M, int N, int K, const ConvGeo& g, bool pro);
bool conv_wgrad_is_wide(int M, int N, int K, int C, bool pro);
int64_t conv_wgrad_ws(int M, int N, int K, int C, bool pro);
// Fused short-sequence attention (attention.hip): qkv [B, S, 3, H, 64] bf16 (Linear layout),
// out [B, S, H * 64], lse [B, H, S] fp32; S % 32 == 0, S <= 128; dropout p on the probabilities.
// klen (nullable, device, [B]): right-padded batch -- keys >= clamp(klen[b], 1, S) of sequence b take
// no part in the softmax (a key-padding mask), dk / dv rows there are zeros; nullptr: no padding.
// cu (nullable, device, [B + 1], not together with klen): packed batch -- the tensors hold the T valid
// tokens only, qkv [T, 3, H, 64], out [T, H * 64], lse [H, T]; sequence b is rows [cu[b], cu[b + 1]), and
// S is the bound the kernels run with (>= every length, S % 32 == 0, S <= 128; the S of the dropout
// indices).  The kernels clamp what cu says into the T rows.
void launch_attn_fwd(const uint16_t* qkv, uint16_t* out, float* lse, int B, int S, int H, float scale, float p,
                     uint64_t seed, hipStream_t s, const int32_t* klen = nullptr, const int32_t* cu = nullptr,
                     int T = 0);
void launch_attn_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, uint16_t* dqkv,
                     int B, int S, int H, float scale, float p, uint64_t seed, hipStream_t s,
                     const int32_t* klen = nullptr, const int32_t* cu = nullptr, int T = 0);
void launch_attn_dropout_mask(uint8_t* mask, int64_t n, float p, uint64_t seed, hipStream_t s);
// The same attention beyond one tile (attention_long.hip): S % 32 == 0, 32 <= S <= 512, online softmax
// over 128-key chunks.  Arguments, layouts, length rules and the dropout draw of every element are those
// of launch_attn_fwd / launch_attn_bwd at the same S; the results agree to rounding, not bitwise.  The
// backward runs its dQ and its dK / dV kernel on s, in that order.
void launch_attn_long_fwd(const uint16_t* qkv, uint16_t* out, float* lse, int B, int S, int H, float scale, float p,
                          uint64_t seed, hipStream_t s, const int32_t* klen = nullptr, const int32_t* cu = nullptr,
                          int T = 0);
void launch_attn_long_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse,
                          uint16_t* dqkv, int B, int S, int H, float scale, float p, uint64_t seed, hipStream_t s,
                          const int32_t* klen = nullptr, const int32_t* cu = nullptr, int T = 0);
// Causal GQA flash attention (flash_attn.hip): q [B, H, S, 128], k / v [B, KV, S, 128] bf16,
// out [B, S, H * 128], lse / dsum [B, H, S] fp32; S % 128 == 0
// Fused softmax cross-entropy over bf16 logits [R, V] (xent.hip): forward lse / per-row loss,
// backward dx = (softmax - onehot) * go / count (go, count: device scalars); ignored rows -> 0
void launch_xent_fwd(const uint16_t* x, const int64_t* lab, int64_t R, int V, int64_t ignore, float* lse, float* loss,
                     hipStream_t s);
void launch_xent_bwd(const uint16_t* x, const int64_t* lab, const float* lse, int64_t R, int V, int64_t ignore,
                     const float* go, const float* count, uint16_t* dx, hipStream_t s);
void launch_fa_fwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, float* lse, int B, int S,
                   int H, int KV, float scale, hipStream_t s, const int* doc_start = nullptr);
// packed documents (flash_attn.hip): doc_start / doc_end (nullable, device, int32 [B, S], non-decreasing
// along S): query i of row b sees keys doc_start[b, i] <= j <= i, key j is seen by queries
// j <= i < doc_end[b, j]; the kernels clamp every bound into the row.  The backward takes both or neither
void launch_fa_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* out, const uint16_t* dout,
                   const float* lse, float* dsum, uint16_t* dq, uint16_t* dk, uint16_t* dv, int B, int S, int H,
                   int KV, float scale, hipStream_t s, const int* doc_start = nullptr, const int* doc_end = nullptr);
void launch_conv_wgrad(const ConvWgradArgs& a, hipStream_t s);
// BN helpers for the fused bottleneck (bn_act.hip): y = act(x*scale + shift [+ res [* rscale + rshift]])
// mbits (nullable): also write the ReLU mask of y, 1 bit per element
void launch_bn_apply_coef(const uint16_t* x, const uint16_t* res, const float* coef, const float* rcoef, uint16_t* y,
                          uint8_t* mbits, int64_t R, int C, int act, hipStream_t s);
// BN backward from producer partial sums pd/px [G][C] (g = already-masked output gradient)
void launch_bn_bwd_partials(const float* pd, const float* px, int G, const uint16_t* g, const uint16_t* x,
                            const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                            float* coef, uint16_t* dx, int64_t R, int C, hipStream_t s);

}  // namespace psamd
