// Exact cosine similarity over an item table (include/recoder_index.h, librecoder_index.so).
//
//   rk_ix_normalize    one wave per row: sum of squares in a fixed order, then x / ||x||
//   rk_ix_scores       out = Qn . En[lo:hi]^T on v_mfma_f32_32x32x2_f32, K never split: every
//                      output is the k-ascending fmaf chain from +0 (the f32-input MFMA is
//                      bitwise that chain), whatever its tile, batch position or strip
//   rk_ix_pool_scores  the SimilarityRecommender's aggregate over a user's history, the same
//                      chain per dot product, one thread per (user, pool item)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/recoder_index.h"
#include "side_error.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------ normalize
// 4 rows per workgroup, one wave each.  Lane l sums x[k]^2 over k = l, l + 64, ... ascending, then
// an xor butterfly: a + b == b + a bitwise, so every lane ends with the same total, and the order
// depends on h alone (never on the row's position).
__global__ __launch_bounds__(256) void ix_normalize_kernel(const float *X, int rows, int h, int ldx,
                                                           float *Y, int ldy) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float *x = X + (int64_t)r * ldx;
  float *y = Y + (int64_t)r * ldy;
  float ss = 0.f;
  for (int k = lane; k < h; k += 64) ss = fmaf(x[k], x[k], ss);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  if (ss > 0.f) {
    const float nrm = sqrtf(ss);
    for (int k = lane; k < h; k += 64) y[k] = x[k] / nrm;
  } else {
    for (int k = lane; k < h; k += 64) y[k] = 0.f;
  }
}

// --------------------------------------------------------------------- scores
// Workgroup tile BM queries x BN items, 4 waves as WM (queries) x 4/WM (items), each wave MT x NT
// tiles of 32 x 32.  K in steps of BK through LDS ([row][k], pitch BK + 1: the 32 rows a wave reads
// per k fall in distinct banks), the next K tile prefetched into registers during the MFMAs.  The
// K tail is zero in LDS and the last tile runs only ceil(rem / 2) k-pairs: a padded (0 * 0) term
// leaves the chain's value unchanged, and the accumulator is never -0 (it starts at +0).
constexpr int BK = 32, PITCH = BK + 1;

template <int WM, int MT, int NT>
__global__ __launch_bounds__(256) void ix_scores_kernel(const float *__restrict__ Qn, int Q, int ldq,
                                                        const float *__restrict__ En, int lde, int h,
                                                        int lo, int S, float *__restrict__ out, int ldo) {
  constexpr int WN = 4 / WM;
  constexpr int BM = WM * MT * 32, BN = WN * NT * 32;
  constexpr int LA = BM * BK / 256, LB = BN * BK / 256;
  __shared__ float sA[BM * PITCH];
  __shared__ float sB[BN * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w % WM, wn = w / WM;
  const int q0 = blockIdx.y * BM, c0 = blockIdx.x * BN;

  float ra[LA], rb[LB];
  auto load = [&](int k0) {
#pragma unroll
    for (int e = 0; e < LA; ++e) {
      const int idx = e * 256 + tid, r = idx / BK, k = k0 + idx % BK, q = q0 + r;
      ra[e] = (q < Q && k < h) ? Qn[(int64_t)q * ldq + k] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < LB; ++e) {
      const int idx = e * 256 + tid, r = idx / BK, k = k0 + idx % BK, c = c0 + r;
      rb[e] = (c < S && k < h) ? En[(int64_t)(lo + c) * lde + k] : 0.f;
    }
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  load(0);
  for (int k0 = 0; k0 < h; k0 += BK) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < LA; ++e) {
      const int idx = e * 256 + tid;
      sA[(idx / BK) * PITCH + idx % BK] = ra[e];
    }
#pragma unroll
    for (int e = 0; e < LB; ++e) {
      const int idx = e * 256 + tid;
      sB[(idx / BK) * PITCH + idx % BK] = rb[e];
    }
    __syncthreads();
    if (k0 + BK < h) load(k0 + BK);
    const int pairs = (min(BK, h - k0) + 1) >> 1;
    const float *pa = sA + (wm * MT * 32 + (lane & 31)) * PITCH + (lane >> 5);
    const float *pb = sB + (wn * NT * 32 + (lane & 31)) * PITCH + (lane >> 5);
    for (int s = 0; s < pairs; ++s) {
      float a[MT], b[NT];
#pragma unroll
      for (int i = 0; i < MT; ++i) a[i] = pa[i * 32 * PITCH + 2 * s];
#pragma unroll
      for (int j = 0; j < NT; ++j) b[j] = pb[j * 32 * PITCH + 2 * s];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  // C/D map of the 32x32 forms: column = lane & 31 (the item), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int c = c0 + (wn * NT + j) * 32 + (lane & 31);
      if (c >= S) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = q0 + (wm * MT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (q < Q) out[(int64_t)q * ldo + c] = acc[i][j][r];
      }
    }
}

// ---------------------------------------------------------------- pool scores
// One workgroup per (user, 256 pool items), one thread per pool item.  The history goes through
// LDS T rows at a time; each thread keeps T chains (one per history row) so that its pool row is
// read once per T history items.  The T similarities are then added in history order.
__device__ __forceinline__ float ix_pow(float x, float scale, int iscale) {
  if (iscale < 0) return powf(x, scale);
  float p = 1.f;
  for (int i = 0; i < iscale; ++i) p *= x;
  return p;
}

template <int T>
__global__ __launch_bounds__(256) void ix_pool_scores_kernel(const float *__restrict__ En, int lde, int h,
                                                             const int64_t *__restrict__ hist_ptr,
                                                             const int64_t *__restrict__ hist_idx,
                                                             const int64_t *__restrict__ pool_idx,
                                                             const int64_t *__restrict__ pool_cnt, int pool_ld,
                                                             float scale, int iscale, float *__restrict__ out) {
  extern __shared__ float sh[];          // [T][h]
  const int u = blockIdx.y, tid = threadIdx.x;
  const int j = blockIdx.x * 256 + tid;
  const int64_t cnt = pool_cnt[u];
  float *orow = out + (int64_t)u * pool_ld;
  if ((int64_t)blockIdx.x * 256 >= cnt) {                 // (workgroup-uniform) padding only
    if (j < pool_ld) orow[j] = -INFINITY;
    return;
  }
  const bool active = j < cnt;
  const float *prow = En + (active ? pool_idx[(int64_t)u * pool_ld + j] : 0) * (int64_t)lde;
  const int64_t hb = hist_ptr[u], he = hist_ptr[u + 1];
  float total = 0.f;
  for (int64_t t0 = hb; t0 < he; t0 += T) {
    const int nt = (int)min((int64_t)T, he - t0);
    __syncthreads();
    for (int e = tid; e < nt * h; e += 256) {
      const int i = e / h, k = e - i * h;
      sh[e] = En[hist_idx[t0 + i] * (int64_t)lde + k];
    }
    __syncthreads();
    if (!active) continue;
    float d[T];
#pragma unroll
    for (int i = 0; i < T; ++i) d[i] = 0.f;
    for (int k = 0; k < h; ++k) {
      const float p = prow[k];
#pragma unroll
      for (int i = 0; i < T; ++i)
        if (i < nt) d[i] = fmaf(p, sh[i * h + k], d[i]);
    }
#pragma unroll
    for (int i = 0; i < T; ++i)
      if (i < nt) total += ix_pow((d[i] + 1.f) * 0.5f, scale, iscale);
  }
  if (j < pool_ld) orow[j] = active ? total : -INFINITY;
}

constexpr int POOL_T = 8;
constexpr int POOL_LDS_MAX = 64 * 1024;

}  // namespace

extern "C" int rk_ix_version(void) { return 100; }
extern "C" const char *rk_ix_last_error(void) { return g_rk_side_err; }

extern "C" int rk_ix_normalize(const float *X, int32_t rows, int32_t h, int32_t ldx, float *Y, int32_t ldy,
                               void *stream) {
  RK_SIDE_REQUIRE(rows >= 0 && h >= 1 && ldx >= h && ldy >= h, "rows >= 0, h >= 1, ldx >= h, ldy >= h");
  RK_SIDE_REQUIRE(X != Y || ldx == ldy, "in place needs ldx == ldy");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(ix_normalize_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, X, rows, h,
                     ldx, Y, ldy);
  RK_SIDE_CHECK_LAUNCH("ix_normalize");
  return 0;
}

extern "C" int rk_ix_scores(const float *Qn, int32_t Q, int32_t ldq, const float *En, int32_t lde, int32_t h,
                            int32_t lo, int32_t hi, float *out, int32_t ldo, void *stream) {
  RK_SIDE_REQUIRE(Q >= 0 && h >= 1 && ldq >= h && lde >= h, "Q >= 0, h >= 1, ldq >= h, lde >= h");
  RK_SIDE_REQUIRE(lo >= 0 && hi >= lo && ldo >= hi - lo, "0 <= lo <= hi, ldo >= hi - lo");
  const int S = hi - lo;
  if (Q == 0 || S == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (Q <= 32) {               // one query tile: 32 queries x 256 items per workgroup
    hipLaunchKernelGGL((ix_scores_kernel<1, 1, 2>), dim3((S + 255) / 256, 1), dim3(256), 0, st, Qn, Q, ldq, En,
                       lde, h, lo, S, out, ldo);
  } else {                     // 128 x 128
    RK_SIDE_REQUIRE((Q + 127) / 128 <= 65535, "Q too large for one call");
    hipLaunchKernelGGL((ix_scores_kernel<2, 2, 2>), dim3((S + 127) / 128, (Q + 127) / 128), dim3(256), 0, st, Qn,
                       Q, ldq, En, lde, h, lo, S, out, ldo);
  }
  RK_SIDE_CHECK_LAUNCH("ix_scores");
  return 0;
}

extern "C" int rk_ix_pool_scores(const float *En, int32_t lde, int32_t h, const int64_t *hist_ptr,
                                 const int64_t *hist_idx, int32_t U, const int64_t *pool_idx,
                                 const int64_t *pool_cnt, int32_t pool_ld, float scale, float *out, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && lde >= h && U >= 0 && pool_ld >= 0, "h >= 1, lde >= h, U >= 0, pool_ld >= 0");
  RK_SIDE_REQUIRE(U <= 65535, "at most 65535 users per call");
  RK_SIDE_REQUIRE(!isnan(scale), "scale is NaN");
  if (U == 0 || pool_ld == 0) return 0;
  const int iscale = (scale >= 0.f && scale <= 64.f && scale == floorf(scale)) ? (int)scale : -1;
  const dim3 grid((pool_ld + 255) / 256, U);
  hipStream_t st = (hipStream_t)stream;
  if ((size_t)POOL_T * h * sizeof(float) <= POOL_LDS_MAX) {
    hipLaunchKernelGGL(ix_pool_scores_kernel<POOL_T>, grid, dim3(256), POOL_T * h * sizeof(float), st, En, lde, h,
                       hist_ptr, hist_idx, pool_idx, pool_cnt, pool_ld, scale, iscale, out);
  } else {
    RK_SIDE_REQUIRE((size_t)h * sizeof(float) <= POOL_LDS_MAX, "h > 16384");
    hipLaunchKernelGGL(ix_pool_scores_kernel<1>, grid, dim3(256), h * sizeof(float), st, En, lde, h, hist_ptr,
                       hist_idx, pool_idx, pool_cnt, pool_ld, scale, iscale, out);
  }
  RK_SIDE_CHECK_LAUNCH("ix_pool_scores");
  return 0;
}
