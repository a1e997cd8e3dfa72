#pragma once
#include "common.h"

namespace {

// --------------------------------------------------------------------- fold-in
// rk_als_foldin: the user-side normal equations of one history, solved exactly by Cholesky.  A group of TPR
// threads owns a row (256 / TPR rows a workgroup); every barrier below is reached by the whole workgroup with
// the same trip counts (the entry loop runs to the longest of the workgroup's rows, the others' extra chunks
// are empty), and nothing a group computes reads another group's LDS, so a row's bits depend on nothing else.
//
//   A      lower triangle only, packed: (k, l), l <= k, at k (k + 1) / 2 + l.  While the entries are taken it
//          lives in registers: thread t owns the TB x TB tile (bi, bj), bj <= bi, number t of the tiles in
//          row-major order, so that every element's chain over the entries stays in one lane
//   stage  FI_CHUNK item rows of the history at a time, zero past h up to the tile edge hp
//   r      thread k < h owns r_k, z_k and x_k in a register; zs hands the solved component to the others
//   dg     L[j][j]; the packed diagonal keeps the pivot, which nothing reads again
//
// LDS floats a group: FI_CHUNK hp + 2 hp + 3 FI_CHUNK + h (h + 1) / 2, rounded up to 4.  h = 128: 41.4 KiB, one
// row a workgroup, three workgroups a CU; h = 64: 12.8 KiB x 4 rows; h = 32: 4.5 KiB x 4 rows.
constexpr int FI_MAX_H = 128;
constexpr int FI_CHUNK = 16;

__host__ __device__ constexpr int fi_tri(int i) { return i * (i + 1) / 2; }

int fi_group_floats(int h, int tb) {
  const int hp = (h + tb - 1) / tb * tb;
  return (FI_CHUNK * hp + 2 * hp + 3 * FI_CHUNK + fi_tri(h) + 3) & ~3;
}

// the LDS of one group, in the order above
struct FiLds {
  float *stage, *zs, *dg, *sa, *scoef;
  int *scol;
  float *Ls;
};

__device__ __forceinline__ FiLds fi_lds_of(float *base, int hp) {
  FiLds L;
  L.stage = base;
  L.zs = L.stage + FI_CHUNK * hp;
  L.dg = L.zs + hp;
  L.sa = L.dg + hp;
  L.scoef = L.sa + FI_CHUNK;
  L.scol = (int *)(L.scoef + FI_CHUNK);
  L.Ls = (float *)(L.scol + FI_CHUNK);
  return L;
}

// coef_e of an entry with value val and item bias b; a = its confidence weight a_e
__device__ __forceinline__ float fi_coef(float val, float alpha, float b, float &a) {
#pragma clang fp contract(off)
  a = val > 0.f ? alpha : 0.f;
  return (1.f + a) * val - a * b;                   // (two products and a difference, each rounded)
}

// A_u of the group's row formed and factorised into Ls / dg, r = the right-hand side  sum_e coef_e y_e - v  in
// thread t < h; returns true where the row is not live or a pivot was not positive.  rk_als_foldin and rk_als_explain
// (explain.h) both stand on this one statement of the system.
template <int TPR, int TB>
__device__ __forceinline__ bool fi_form_factor(const FiLds &L, const int64_t *__restrict__ indptr,
                                               const int32_t *__restrict__ indices, const float *__restrict__ data,
                                               int rows, const float *__restrict__ Y, int ldy, int h,
                                               const float *__restrict__ G, const float *__restrict__ v,
                                               const float *__restrict__ bias, float alpha, int g, int t, float &r,
                                               bool &live, int64_t &e0, int &n) {
#pragma clang fp contract(off)                    // every fused operation below is written as fmaf
  constexpr int R = 256 / TPR;
  constexpr int TX = TPR == 256 ? 16 : 8, TY = TPR / TX;
  const int nb = (h + TB - 1) / TB, hp = nb * TB;
  float *stage = L.stage, *dg = L.dg, *sa = L.sa, *scoef = L.scoef, *Ls = L.Ls;
  int *scol = L.scol;

  const int64_t row0 = (int64_t)blockIdx.x * R, row = row0 + g;
  live = row < rows;
  e0 = 0;
  n = 0;
  int nmax = 0;
  if (live) {
    e0 = indptr[row];
    n = (int)(indptr[row + 1] - e0);
  }
#pragma unroll
  for (int q = 0; q < R; ++q)
    if (row0 + q < rows) nmax = max(nmax, (int)(indptr[row0 + q + 1] - indptr[row0 + q]));

  int bi = 0, bj = t;                               // tile t of the lower triangle's tiles, row-major
  while (bj > bi) {
    bj -= bi + 1;
    ++bi;
  }
  const bool tile = live && bi < nb;
  float acc[TB][TB];                                // (an element past h or above the diagonal is never stored:
#pragma unroll                                      //  it starts from the nearest one that is, read without a branch)
  for (int a = 0; a < TB; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      const int k = min(bi * TB + a, h - 1), l = min(bj * TB + b, k);
      acc[a][b] = tile ? G[k * h + l] : 0.f;
    }
  r = (live && t < h) ? -v[t] : 0.f;

  for (int c0 = 0; c0 < nmax; c0 += FI_CHUNK) {
    const int cnt = min(FI_CHUNK, n - c0);          // (<= 0: this row has no entry left)
    if (t < FI_CHUNK) {
      float a = 0.f, cf = 0.f;
      int col = 0;
      if (t < cnt) {
        const int64_t e = e0 + c0 + t;
        col = indices[e];
        cf = fi_coef(entry_value(data, e), alpha, bias ? bias[col] : 0.f, a);
      }
      sa[t] = a;
      scoef[t] = cf;
      scol[t] = col;
    }
    __syncthreads();
    for (int idx = t; idx < FI_CHUNK * hp; idx += TPR) {
      const int e = idx / hp, k = idx - e * hp;
      stage[idx] = (e < cnt && k < h) ? Y[(int64_t)scol[e] * ldy + k] : 0.f;
    }
    __syncthreads();
    if (t < h)
      for (int e = 0; e < cnt; ++e) r = fmaf(scoef[e], stage[e * hp + t], r);
    if (tile)
      for (int e = 0; e < cnt; ++e) {
        const float a = sa[e];
        if (a == 0.f) continue;
        float yk[TB], yl[TB];
#pragma unroll
        for (int q = 0; q < TB; q += 4) {
          const float4 pk = *(const float4 *)(stage + e * hp + bi * TB + q);
          const float4 pl = *(const float4 *)(stage + e * hp + bj * TB + q);
          yk[q] = pk.x, yk[q + 1] = pk.y, yk[q + 2] = pk.z, yk[q + 3] = pk.w;
          yl[q] = pl.x, yl[q + 1] = pl.y, yl[q + 2] = pl.z, yl[q + 3] = pl.w;
        }
#pragma unroll
        for (int p = 0; p < TB; ++p) {
          const float ay = a * yk[p];
#pragma unroll
          for (int b = 0; b < TB; ++b) acc[p][b] = fmaf(ay, yl[b], acc[p][b]);
        }
      }
    __syncthreads();
  }
  if (tile) {
#pragma unroll
    for (int a = 0; a < TB; ++a)
#pragma unroll
      for (int b = 0; b < TB; ++b) {
        const int k = bi * TB + a, l = bj * TB + b;
        if (k < h && l <= k) Ls[fi_tri(k) + l] = acc[a][b];
      }
  }
  __syncthreads();

  // Cholesky, right-looking: column j scaled by its pivot's root, then the trailing triangle takes
  // fmaf(-L[i][j], L[l][j], .): every element meets its k in ascending order
  const int tx = t % TX, ty = t / TX;
  bool bad = !live;
  for (int j = 0; j < h; ++j) {
    float ljj = 0.f;
    if (!bad) {
      const float d = Ls[fi_tri(j) + j];
      if (!(d > 0.f)) bad = true;                   // (the same value in every thread of the group)
      ljj = sqrtf(d);
    }
    if (!bad) {
      if (t == 0) dg[j] = ljj;
      for (int i = j + 1 + t; i < h; i += TPR) Ls[fi_tri(i) + j] = Ls[fi_tri(i) + j] / ljj;
    }
    __syncthreads();
    if (!bad) {
      for (int i = j + 1 + ty; i < h; i += TY) {
        const float nl = -Ls[fi_tri(i) + j];
        float *Ai = Ls + fi_tri(i);
        for (int l = j + 1 + tx; l <= i; l += TX) Ai[l] = fmaf(nl, Ls[fi_tri(l) + j], Ai[l]);
      }
    }
    __syncthreads();
  }
  return bad;
}

// L z = r by columns, k ascending; then L^T x = z by columns, k descending: thread t < h comes in with r_t and leaves
// with x_t, and zs holds all of x behind the last barrier.  Every thread of the workgroup reaches every barrier.
__device__ __forceinline__ void fi_solve(const FiLds &L, int h, int t, bool bad, float &r) {
#pragma clang fp contract(off)
  float *zs = L.zs;
  const float *dg = L.dg, *Ls = L.Ls;
  for (int k = 0; k < h; ++k) {
    if (!bad && t == k) {
      r = r / dg[k];
      zs[k] = r;
    }
    __syncthreads();
    if (!bad && t > k && t < h) r = fmaf(-Ls[fi_tri(t) + k], zs[k], r);
  }
  for (int k = h - 1; k >= 0; --k) {
    if (!bad && t == k) {
      r = r / dg[k];
      zs[k] = r;
    }
    __syncthreads();
    if (!bad && t < k) r = fmaf(-Ls[fi_tri(k) + t], zs[k], r);
  }
}

template <int TPR, int TB>
__global__ __launch_bounds__(256) void als_foldin_kernel(const int64_t *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices,
                                                         const float *__restrict__ data, int rows,
                                                         const float *__restrict__ Y, int ldy, int h,
                                                         const float *__restrict__ G, const float *__restrict__ v,
                                                         const float *__restrict__ bias, float alpha,
                                                         float *__restrict__ X, int ldx,
                                                         int32_t *__restrict__ status, int gfloats) {
  extern __shared__ __attribute__((aligned(16))) float fi_lds[];
  const int g = threadIdx.x / TPR, t = threadIdx.x % TPR;
  const int hp = (h + TB - 1) / TB * TB;
  const FiLds L = fi_lds_of(fi_lds + (int64_t)g * gfloats, hp);
  const int64_t row = (int64_t)blockIdx.x * (256 / TPR) + g;
  float r;
  bool live;
  int64_t e0;
  int n;
  const bool bad = fi_form_factor<TPR, TB>(L, indptr, indices, data, rows, Y, ldy, h, G, v, bias, alpha, g, t, r, live,
                                           e0, n);
  fi_solve(L, h, t, bad, r);
  if (live) {
    if (t < h) X[row * ldx + t] = bad ? 0.f : r;
    if (t == 0) status[row] = bad ? 1 : 0;
  }
}

}  // namespace

extern "C" int rk_als_foldin_max_h(void) { return FI_MAX_H; }

extern "C" int rk_als_foldin(const int64_t *indptr, const int32_t *indices, const float *data, int32_t rows,
                             const float *Y, int32_t ldy, int32_t h, const float *G, const float *v,
                             const float *bias, float alpha, float *X, int32_t ldx, int32_t *status, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= FI_MAX_H && ldy >= h && ldx >= h, "1 <= h <= 128, ldy >= h, ldx >= h");
  RK_SIDE_REQUIRE(rows >= 0, "rows >= 0");
  RK_SIDE_REQUIRE(alpha >= 0.f && alpha <= FLT_MAX, "alpha must be finite and >= 0");
  if (rows == 0) return 0;
  RK_SIDE_REQUIRE(indptr && indices && Y && G && v && X && status, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto kernel, int tpr, int tb) {
    const int per = 256 / tpr, gfloats = fi_group_floats(h, tb);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(256),
                       (size_t)per * gfloats * sizeof(float), st, indptr, indices, data, rows, Y, ldy, h, G, v, bias,
                       alpha, X, ldx, status, gfloats);
  };
  if (h <= 32) launch(als_foldin_kernel<64, 4>, 64, 4);
  else if (h <= 64) launch(als_foldin_kernel<64, 8>, 64, 8);
  else launch(als_foldin_kernel<256, 8>, 256, 8);
  RK_SIDE_CHECK_LAUNCH("als_foldin");
  return 0;
}
