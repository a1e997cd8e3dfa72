#pragma once
#include "common.h"

namespace {

// ---------------------------------------------------------------------- iALS++
// Block-subspace implicit ALS (Rendle, Krichene, Zhang & Koren 2021): one block of k <= 128 coordinates of a row is
// solved exactly against a per-entry prediction cache.  include/recoder_als.h states the arithmetic; the kernels:
//
//   ials_predict_kernel         a wave per 8 stored entries: the entries' rows by a binary search of indptr (lanes
//                               0..7), then the wave's dot chain per entry
//   ials_block_kernel           rk_als_foldin's shape on a k x k system: the packed lower triangle in register tiles
//                               while the entries are taken (IA_CHUNK gathered slices of k floats in LDS at a time), a
//                               right-looking Cholesky and both triangular solves in LDS, then the row's cache entries
//                               by lane groups of 16.  TPR threads a part, NP parts a row, R rows a workgroup: a row
//                               below RK_ALS_IALS_LONG_ROW entries has one part (R = 256 / TPR rows a workgroup), a
//                               longer one is cut into NP contiguous parts over one workgroup of 512 threads, the
//                               parts' triangles and right-hand sides added in ascending part order
//   ials_panel_part_kernel      F[:, pi]^T F over fixed row chunks, 64 x 64 output tiles through LDS, 4 x 4 a thread;
//   ials_panel_reduce_kernel    the chunks added in ascending order
//   ials_objective_part_kernel  the four sums of L in float64 over a fixed hand-out; ials_objective_sum_kernel adds
//                               the partials in ascending order
//
// LDS floats a row of the block kernel: NP (IA_CHUNK kp + 2 IA_CHUNK) + NP kp + 2 kp + k (k + 1) / 2, kp = k rounded up
// to the tile edge.  k = 128: 50.5 KiB (long rows, NP = 2), 41.4 KiB (short); k = 64: 12.9 KiB x 4 rows (short), 43.6
// KiB (long, NP = 8).  Every workgroup stays below 64 KiB.
constexpr int IA_MAX_H = 2048;
constexpr int IA_MAX_K = 128;
constexpr int IA_CHUNK = 16;
constexpr int IA_LONG_ROW = RK_ALS_IALS_LONG_ROW;
constexpr int IA_PANEL_CHUNKS = 64;
constexpr int IA_OBJ_BLOCKS = 256;

__host__ __device__ constexpr int ia_tri(int i) { return i * (i + 1) / 2; }

int ia_row_floats(int k, int tb, int np) {
  const int kp = (k + tb - 1) / tb * tb;
  return (np * (IA_CHUNK * kp + 2 * IA_CHUNK) + np * kp + 2 * kp + ia_tri(k) + 3) & ~3;
}

__global__ __launch_bounds__(256) void ials_predict_kernel(const int64_t *__restrict__ indptr,
                                                           const int32_t *__restrict__ indices, int rows, int64_t nnz,
                                                           const float *__restrict__ X, int ldx,
                                                           const float *__restrict__ Y, int ldy, int h,
                                                           float *__restrict__ c) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t eb = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8;
  if (eb >= nnz) return;
  const int64_t e = eb + (lane & 7) < nnz ? eb + (lane & 7) : nnz - 1;
  int lo = 0, hi = rows;                            // the last row r with indptr[r] <= e (indptr[rows] = nnz > e)
  while (hi - lo > 1) {
    const int mid = (int)(((int64_t)lo + hi) >> 1);
    if (indptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  const int myrow = lo, mycol = indices[e];
  const int cnt = nnz - eb < 8 ? (int)(nnz - eb) : 8;
#pragma unroll 2
  for (int q = 0; q < cnt; ++q) {
    const int64_t r = __shfl(myrow, q, 64), col = __shfl(mycol, q, 64);
    float s = 0.f;
    for (int k = lane; k < h; k += 64) s = fmaf(X[r * ldx + k], Y[col * ldy + k], s);
    s = wave_sum(s);
    if (lane == 0) c[eb + q] = s;
  }
}

template <int TPR, int TB, int NP, int R, bool LONG>
__global__ __launch_bounds__(TPR *NP *R) void ials_block_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const int64_t *__restrict__ perm,
    const int32_t *__restrict__ long_rows, int row_lo, int row_hi, const float *__restrict__ F, int ldf,
    float *__restrict__ X, int ldx, int h,
    const float *__restrict__ P, int ldp, const float *__restrict__ lam, float alpha0, int p0, int k,
    float *__restrict__ cache, int32_t *__restrict__ status, int gfloats) {
#pragma clang fp contract(off)                    // every fused operation below is written as fmaf
  extern __shared__ __attribute__((aligned(16))) float ia_lds[];
  constexpr int TT = TPR * NP;                      // the threads of a row
  constexpr int TX = TT >= 256 ? 16 : 8, TY = TT / TX;
  const int g = threadIdx.x / TT, tt = threadIdx.x % TT, p = tt / TPR, t = tt % TPR;
  const int nb = (k + TB - 1) / TB, kp = nb * TB;
  float *base = ia_lds + (int64_t)g * gfloats;
  float *stage = base + p * (IA_CHUNK * kp + 2 * IA_CHUNK);
  float *scoef = stage + IA_CHUNK * kp;
  int *scol = (int *)(scoef + IA_CHUNK);
  float *gs = base + NP * (IA_CHUNK * kp + 2 * IA_CHUNK);
  float *zs = gs + NP * kp;
  float *dg = zs + kp;
  float *Ls = dg + kp;

  // (the long kernel with a list: workgroup b takes the list's row b, and leaves when it lies outside the range)
  const int64_t row0 = (LONG && long_rows) ? (int64_t)long_rows[blockIdx.x] : (int64_t)row_lo + (int64_t)blockIdx.x * R;
  const int64_t row = row0 + g;
  bool live = row >= row_lo && row < row_hi;
  int64_t e0 = 0;
  int n = 0;
  if (live) {
    e0 = indptr[row];
    n = (int)(indptr[row + 1] - e0);
    if ((n >= IA_LONG_ROW) != LONG) live = false, n = 0;
  }
  if (LONG && !live) return;                        // (R == 1: the whole workgroup leaves)
  int nmax = 0;                                     // the longest part of the workgroup: every barrier's trip count
  if (LONG) {
#pragma unroll
    for (int q = 0; q < NP; ++q) nmax = max(nmax, (int)((int64_t)(q + 1) * n / NP - (int64_t)q * n / NP));
  } else {
#pragma unroll
    for (int q = 0; q < R; ++q)
      if (row0 + q < row_hi) {
        const int nq = (int)(indptr[row0 + q + 1] - indptr[row0 + q]);
        if (nq < IA_LONG_ROW) nmax = max(nmax, nq);
      }
  }
  const int ps = (int)((int64_t)p * n / NP), cntp = (int)((int64_t)(p + 1) * n / NP) - ps;

  int bi = 0, bj = t;                               // tile t of the lower triangle's tiles, row-major
  while (bj > bi) {
    bj -= bi + 1;
    ++bi;
  }
  const bool tile = live && bi < nb;
  float acc[TB][TB];
#pragma unroll
  for (int a = 0; a < TB; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b) acc[a][b] = 0.f;
  float gp = 0.f;

  for (int c0 = 0; c0 < nmax; c0 += IA_CHUNK) {
    const int cnt = min(IA_CHUNK, cntp - c0);       // (<= 0: this part has no entry left)
    if (t < IA_CHUNK) {
      float cf = 0.f;
      int col = 0;
      if (t < cnt) {
        const int64_t e = e0 + ps + c0 + t;
        col = indices[e];
        cf = cache[perm ? perm[e] : e] - 1.f;
      }
      scoef[t] = cf;
      scol[t] = col;
    }
    __syncthreads();
    for (int idx = t; idx < IA_CHUNK * kp; idx += TPR) {
      const int e = idx / kp, kk = idx - e * kp;
      stage[idx] = (e < cnt && kk < k) ? F[(int64_t)scol[e] * ldf + p0 + kk] : 0.f;
    }
    __syncthreads();
    if (t < k)
      for (int e = 0; e < cnt; ++e) gp = fmaf(scoef[e], stage[e * kp + t], gp);
    if (tile)
      for (int e = 0; e < cnt; ++e) {
        float yk[TB], yl[TB];
#pragma unroll
        for (int q = 0; q < TB; q += 4) {
          const float4 pk = *(const float4 *)(stage + e * kp + bi * TB + q);
          const float4 pl = *(const float4 *)(stage + e * kp + bj * TB + q);
          yk[q] = pk.x, yk[q + 1] = pk.y, yk[q + 2] = pk.z, yk[q + 3] = pk.w;
          yl[q] = pl.x, yl[q + 1] = pl.y, yl[q + 2] = pl.z, yl[q + 3] = pl.w;
        }
#pragma unroll
        for (int a = 0; a < TB; ++a)
#pragma unroll
          for (int b = 0; b < TB; ++b) acc[a][b] = fmaf(yk[a], yl[b], acc[a][b]);
      }
    __syncthreads();
  }

  // A = alpha0 P[:, pi] + lam I, then the parts' triangles in ascending part order
  const float lamu = live ? lam[row] : 0.f;
  if (t < k) gs[p * kp + t] = gp;
  if (live)
    for (int idx = tt; idx < k * k; idx += TT) {
      const int j = idx / k, l = idx - j * k;
      if (l <= j) Ls[ia_tri(j) + l] = fmaf(alpha0, P[(int64_t)j * ldp + p0 + l], j == l ? lamu : 0.f);
    }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    if (p == q && tile) {
#pragma unroll
      for (int a = 0; a < TB; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b) {
          const int kk = bi * TB + a, l = bj * TB + b;
          if (kk < k && l <= kk) Ls[ia_tri(kk) + l] += acc[a][b];
        }
    }
    __syncthreads();
  }
  // g: the dense term alpha0 P[j, :] . x as one chain over the columns, then lam x_j, then the parts' sparse sums
  float r = 0.f;
  if (live && tt < k) {
    const float *Pj = P + (int64_t)tt * ldp;
    const float *xr = X + row * ldx;
    float d = 0.f;
#pragma unroll 8
    for (int c = 0; c < h; ++c) d = fmaf(Pj[c], xr[c], d);
    r = fmaf(lamu, xr[p0 + tt], alpha0 * d);
#pragma unroll
    for (int q = 0; q < NP; ++q) r += gs[q * kp + tt];
  }

  // Cholesky, right-looking: column j scaled by its pivot's root, then the trailing triangle takes
  // fmaf(-L[i][j], L[l][j], .): every element meets its columns in ascending order
  const int tx = tt % TX, ty = tt / TX;
  bool bad = !live;
  for (int j = 0; j < k; ++j) {
    float ljj = 0.f;
    if (!bad) {
      const float d = Ls[ia_tri(j) + j];
      if (!(d > 0.f)) bad = true;                   // (the same value in every thread of the row)
      ljj = sqrtf(d);
    }
    if (!bad) {
      if (tt == 0) dg[j] = ljj;
      for (int i = j + 1 + tt; i < k; i += TT) Ls[ia_tri(i) + j] = Ls[ia_tri(i) + j] / ljj;
    }
    __syncthreads();
    if (!bad) {
      for (int i = j + 1 + ty; i < k; i += TY) {
        const float nl = -Ls[ia_tri(i) + j];
        float *Ai = Ls + ia_tri(i);
        for (int l = j + 1 + tx; l <= i; l += TX) Ai[l] = fmaf(nl, Ls[ia_tri(l) + j], Ai[l]);
      }
    }
    __syncthreads();
  }
  // L z = g by columns ascending; then L^T delta = z by columns descending: zs ends as delta
  for (int j = 0; j < k; ++j) {
    if (!bad && tt == j) {
      r = r / dg[j];
      zs[j] = r;
    }
    __syncthreads();
    if (!bad && tt > j && tt < k) r = fmaf(-Ls[ia_tri(tt) + j], zs[j], r);
  }
  for (int j = k - 1; j >= 0; --j) {
    if (!bad && tt == j) {
      r = r / dg[j];
      zs[j] = r;
    }
    __syncthreads();
    if (!bad && tt < j) r = fmaf(-Ls[ia_tri(j) + tt], zs[j], r);
  }
  if (!live) return;
  if (bad) {                                        // (left as it is, and counted)
    if (tt == 0) atomicAdd(status, 1);
    return;
  }
  if (tt < k) X[row * ldx + p0 + tt] = X[row * ldx + p0 + tt] - r;
  // the row's cache entries: a group of 16 lanes an entry, lane l the elements l + 16 q in ascending q, a butterfly
  const int sub = tt >> 4, l16 = tt & 15;
  for (int i = sub; i < n; i += TT / 16) {
    const int64_t e = e0 + i;
    const float *y = F + (int64_t)indices[e] * ldf + p0;
    float s = 0.f;
    for (int kk = l16; kk < k; kk += 16) s = fmaf(zs[kk], y[kk], s);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
    if (l16 == 0) {
      const int64_t pos = perm ? perm[e] : e;
      cache[pos] = cache[pos] - s;
    }
  }
}

// F[:, p0 : p0 + k]^T F over the rows [z cr, (z + 1) cr) of chunk z: part[z, j, c], rows ascending
__global__ __launch_bounds__(256) void ials_panel_part_kernel(const float *__restrict__ F, int rows, int ldf, int h,
                                                              int p0, int k, int cr, float *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float As[16][64], Bs[16][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int c0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
  const int64_t r0 = (int64_t)blockIdx.z * cr, r1 = r0 + cr < rows ? r0 + cr : (int64_t)rows;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int64_t rb = r0; rb < r1; rb += 16) {
    for (int i = tid; i < 16 * 64; i += 256) {
      const int rr = i >> 6, cc = i & 63;
      const int64_t row = rb + rr;
      As[rr][cc] = (row < r1 && j0 + cc < k) ? F[row * ldf + p0 + j0 + cc] : 0.f;
      Bs[rr][cc] = (row < r1 && c0 + cc < h) ? F[row * ldf + c0 + cc] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const float4 a4 = *(const float4 *)&As[rr][ty * 4], b4 = *(const float4 *)&Bs[rr][tx * 4];
      const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int jj = j0 + ty * 4 + i, cc = c0 + tx * 4 + j;
      if (jj < k && cc < h) part[((int64_t)blockIdx.z * k + jj) * h + cc] = acc[i][j];
    }
}

__global__ __launch_bounds__(256) void ials_panel_reduce_kernel(const float *__restrict__ part, int nch, int k, int h,
                                                                float *__restrict__ P, int ldp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)k * h) return;
  float s = 0.f;
  for (int z = 0; z < nch; ++z) s += part[(int64_t)z * k * h + i];
  P[(i / h) * ldp + i % h] = s;
}

__device__ __forceinline__ double ia_wave_sum(double s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// term 0: sum (c - 1)^2 over the cache; 1: sum Gx Gy; 2, 3: sum_r reg_r |T_r|^2 over the users, the items.  Element
// (row) b 256 + t + 65536 j goes to thread t of block b in ascending j (a row: to wave w of block b, rows b 4 + w +
// 1024 j, its lanes over the columns and a butterfly); the block's 256 threads by a halving tree
__global__ __launch_bounds__(256) void ials_objective_part_kernel(const float *__restrict__ cache, int64_t nnz,
                                                                  const float *__restrict__ Gx,
                                                                  const float *__restrict__ Gy, int h,
                                                                  const float *__restrict__ X, int ldx, int n_users,
                                                                  const float *__restrict__ lam,
                                                                  const float *__restrict__ Y, int ldy, int n_items,
                                                                  const float *__restrict__ mu,
                                                                  double *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double sh[256];
  const int term = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  if (term == 0) {
    for (int64_t i = (int64_t)b * 256 + tid; i < nnz; i += 256 * IA_OBJ_BLOCKS) {
      const double d = (double)cache[i] - 1.0;
      s += d * d;
    }
  } else if (term == 1) {
    for (int64_t i = (int64_t)b * 256 + tid; i < (int64_t)h * h; i += 256 * IA_OBJ_BLOCKS)
      s += (double)Gx[i] * (double)Gy[i];
  } else {
    const float *T = term == 2 ? X : Y, *reg = term == 2 ? lam : mu;
    const int ld = term == 2 ? ldx : ldy, rows = term == 2 ? n_users : n_items;
    const int lane = tid & 63;
    for (int64_t r = (int64_t)b * 4 + (tid >> 6); r < rows; r += 4 * IA_OBJ_BLOCKS) {
      double q = 0.0;
      for (int c = lane; c < h; c += 64) {
        const double v = (double)T[r * ld + c];
        q += v * v;
      }
      q = ia_wave_sum(q);
      if (lane == 0) s += (double)reg[r] * q;
    }
  }
  sh[tid] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) sh[tid] += sh[tid + off];
    __syncthreads();
  }
  if (tid == 0) part[term * IA_OBJ_BLOCKS + b] = sh[0];
}

__global__ __launch_bounds__(64) void ials_objective_sum_kernel(const double *__restrict__ part, float alpha0,
                                                                double *__restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double tot[4];
  if (threadIdx.x < 4) {
    double s = 0.0;
    for (int b = 0; b < IA_OBJ_BLOCKS; ++b) s += part[threadIdx.x * IA_OBJ_BLOCKS + b];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((tot[0] + (double)alpha0 * tot[1]) + tot[2]) + tot[3];
}

struct IaPanelPlan {
  int nch, cr;
};

// the chunks of the panel's rows, fixed by `rows` alone
IaPanelPlan ia_panel_plan(int rows) {
  IaPanelPlan p;
  p.nch = std::max(1, std::min(IA_PANEL_CHUNKS, (rows + 1023) / 1024));
  p.cr = std::max(16, ((rows + p.nch - 1) / p.nch + 15) / 16 * 16);
  return p;
}

}  // namespace

extern "C" int rk_als_ials_max_h(void) { return IA_MAX_H; }
extern "C" int rk_als_ials_max_block(void) { return IA_MAX_K; }

extern "C" int rk_als_ials_predict(const int64_t *indptr, const int32_t *indices, int32_t rows, int64_t nnz,
                                   const float *X, int32_t ldx, const float *Y, int32_t ldy, int32_t h, float *c,
                                   void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= IA_MAX_H && ldx >= h && ldy >= h, "1 <= h <= 2048, ldx >= h, ldy >= h");
  RK_SIDE_REQUIRE(rows >= 0 && nnz >= 0, "rows >= 0, nnz >= 0");
  if (nnz == 0) return 0;
  RK_SIDE_REQUIRE(rows >= 1 && indptr && indices && X && Y && c, "null pointer");
  const int64_t blocks = (nnz + 31) / 32;
  RK_SIDE_REQUIRE(blocks <= 0x7fffffff, "nnz too large");
  hipLaunchKernelGGL(ials_predict_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, indptr, indices,
                     rows, nnz, X, ldx, Y, ldy, h, c);
  RK_SIDE_CHECK_LAUNCH("ials_predict");
  return 0;
}

extern "C" int rk_als_ials_block(const int64_t *indptr, const int32_t *indices, const int64_t *perm, int32_t row_lo,
                                 int32_t row_hi, const int32_t *long_rows, int32_t n_long, const float *F, int32_t ldf,
                                 float *X, int32_t ldx, int32_t h, const float *P, int32_t ldp, const float *reg,
                                 float alpha0, int32_t p0, int32_t k, float *cache, int32_t *status, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= IA_MAX_H && ldf >= h && ldx >= h && ldp >= h,
                  "1 <= h <= 2048, ldf >= h, ldx >= h, ldp >= h");
  RK_SIDE_REQUIRE(k >= 1 && k <= IA_MAX_K && p0 >= 0 && p0 <= h - k, "1 <= k <= 128, 0 <= p0 <= h - k");
  RK_SIDE_REQUIRE(row_lo >= 0 && row_hi >= row_lo, "0 <= row_lo <= row_hi");
  RK_SIDE_REQUIRE(n_long >= 0 && (n_long == 0 || long_rows), "n_long >= 0, long_rows set when n_long > 0");
  RK_SIDE_REQUIRE(alpha0 >= 0.f && alpha0 <= FLT_MAX, "alpha0 must be finite and >= 0");
  const int rows = row_hi - row_lo;
  if (rows == 0) return 0;
  RK_SIDE_REQUIRE(indptr && indices && F && X && P && reg && cache && status, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  // the short rows: `per` rows a workgroup over the range; the long rows (np > 1): a workgroup a row of the caller's
  // list, or of the whole range when there is no list (long_rows NULL)
  auto launch = [&](auto kernel, int per, int threads, int tb, int np) {
    const int gfloats = ia_row_floats(k, tb, np);
    const int grid = (np > 1 && long_rows) ? n_long : (rows + per - 1) / per;
    if (grid == 0) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), (size_t)per * gfloats * sizeof(float), st, indptr,
                       indices, perm, np > 1 ? long_rows : nullptr, row_lo, row_hi, F, ldf, X, ldx, h, P, ldp, reg,
                       alpha0, p0, k, cache, status, gfloats);
  };
  if (k <= 32) {
    launch(ials_block_kernel<64, 4, 1, 4, false>, 4, 256, 4, 1);
    launch(ials_block_kernel<64, 4, 8, 1, true>, 1, 512, 4, 8);
  } else if (k <= 64) {
    launch(ials_block_kernel<64, 8, 1, 4, false>, 4, 256, 8, 1);
    launch(ials_block_kernel<64, 8, 8, 1, true>, 1, 512, 8, 8);
  } else {
    launch(ials_block_kernel<256, 8, 1, 1, false>, 1, 256, 8, 1);
    launch(ials_block_kernel<256, 8, 2, 1, true>, 1, 512, 8, 2);
  }
  RK_SIDE_CHECK_LAUNCH("ials_block");
  return 0;
}

extern "C" int64_t rk_als_ials_panel_workspace_bytes(int32_t rows, int32_t h, int32_t k) {
  if (rows < 0 || h < 1 || h > IA_MAX_H || k < 1 || k > IA_MAX_K || k > h) return -2;
  return (int64_t)ia_panel_plan(rows).nch * k * h * (int64_t)sizeof(float);
}

extern "C" int rk_als_ials_gram_panel(const float *F, int32_t rows, int32_t ldf, int32_t h, int32_t p0, int32_t k,
                                      float *P, int32_t ldp, void *ws, int64_t ws_bytes, void *stream) {
  RK_SIDE_REQUIRE(rows >= 0 && h >= 1 && h <= IA_MAX_H && ldf >= h && ldp >= h,
                  "rows >= 0, 1 <= h <= 2048, ldf >= h, ldp >= h");
  RK_SIDE_REQUIRE(k >= 1 && k <= IA_MAX_K && p0 >= 0 && p0 <= h - k, "1 <= k <= 128, 0 <= p0 <= h - k");
  RK_SIDE_REQUIRE(P && (rows == 0 || F), "P (and F when rows > 0) must be set");
  RK_SIDE_REQUIRE(ws && ws_bytes >= rk_als_ials_panel_workspace_bytes(rows, h, k), "workspace too small");
  const IaPanelPlan p = ia_panel_plan(rows);
  const int nch = rows == 0 ? 0 : (rows + p.cr - 1) / p.cr;      // (<= p.nch)
  hipStream_t st = (hipStream_t)stream;
  if (nch)
    hipLaunchKernelGGL(ials_panel_part_kernel, dim3((unsigned)((h + 63) / 64), (unsigned)((k + 63) / 64), (unsigned)nch),
                       dim3(256), 0, st, F, rows, ldf, h, p0, k, p.cr, (float *)ws);
  hipLaunchKernelGGL(ials_panel_reduce_kernel, dim3((unsigned)(((int64_t)k * h + 255) / 256)), dim3(256), 0, st,
                     (const float *)ws, nch, k, h, P, ldp);
  RK_SIDE_CHECK_LAUNCH("ials_gram_panel");
  return 0;
}

extern "C" int64_t rk_als_ials_objective_workspace_bytes(void) {
  return (int64_t)4 * IA_OBJ_BLOCKS * (int64_t)sizeof(double);
}

extern "C" int rk_als_ials_objective(const float *cache, int64_t nnz, const float *Gx, const float *Gy, int32_t h,
                                     const float *X, int32_t ldx, int32_t n_users, const float *lam, const float *Y,
                                     int32_t ldy, int32_t n_items, const float *mu, float alpha0, void *ws,
                                     int64_t ws_bytes, double *out, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= IA_MAX_H && ldx >= h && ldy >= h, "1 <= h <= 2048, ldx >= h, ldy >= h");
  RK_SIDE_REQUIRE(nnz >= 0 && n_users >= 0 && n_items >= 0, "nnz, n_users, n_items >= 0");
  RK_SIDE_REQUIRE(alpha0 >= 0.f && alpha0 <= FLT_MAX, "alpha0 must be finite and >= 0");
  RK_SIDE_REQUIRE(Gx && Gy && out && (nnz == 0 || cache) && (n_users == 0 || (X && lam)) &&
                      (n_items == 0 || (Y && mu)),
                  "null pointer");
  RK_SIDE_REQUIRE(ws && ws_bytes >= rk_als_ials_objective_workspace_bytes(), "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ials_objective_part_kernel, dim3(IA_OBJ_BLOCKS, 4), dim3(256), 0, st, cache, nnz, Gx, Gy, h, X,
                     ldx, n_users, lam, Y, ldy, n_items, mu, (double *)ws);
  hipLaunchKernelGGL(ials_objective_sum_kernel, dim3(1), dim3(64), 0, st, (const double *)ws, alpha0, out);
  RK_SIDE_CHECK_LAUNCH("ials_objective");
  return 0;
}
