#pragma once
#include "common.h"

namespace {

// ----------------------------------------------------------------------- gram
// Row chunks: a function of rows alone (never of the device or the launch), so G is bitwise
// repeatable.  At most GR_MAX_CHUNKS partial [h, h] images in the workspace.
constexpr int GR_MAX_CHUNKS = 64;
constexpr int GR_MIN_CHUNK = 512;

struct GramPlan {
  int nch, chunk, ntile, npairs;
};

GramPlan gram_plan(int rows, int h) {
  GramPlan p;
  p.nch = rows <= 0 ? 1 : (int)std::min<int64_t>(GR_MAX_CHUNKS, ((int64_t)rows + GR_MIN_CHUNK - 1) / GR_MIN_CHUNK);
  int64_t c = rows <= 0 ? 0 : ((int64_t)rows + p.nch - 1) / p.nch;
  p.chunk = (int)((c + 1) & ~(int64_t)1);           // even: k-pairs never straddle two chunks
  p.ntile = (h + 31) / 32;
  p.npairs = p.ntile * (p.ntile + 1) / 2;
  return p;
}

// One wave per (upper tile pair I <= J, chunk).  Lane l holds A[m = l & 31][k = l >> 5] =
// F[r + (l >> 5)][32 I + m] and B[k][n = l & 31] = F[r + (l >> 5)][32 J + n]; rows past the chunk
// and columns past h are 0 (a 0 * 0 term leaves the chain's value as it is).  Diagonal pairs also
// take v's chain for their 32 columns: lane halves over the even / odd rows, added at the end.
constexpr int GR_UNROLL = 8;

__global__ __launch_bounds__(64) void als_gram_partial_kernel(const float *__restrict__ F, int rows, int h,
                                                              int ldf, const float *__restrict__ w, int chunk,
                                                              int ntile, float *__restrict__ P,
                                                              float *__restrict__ Pv) {
  const int lane = threadIdx.x, c = blockIdx.y;
  int pi = blockIdx.x, I = 0;
  while (pi >= ntile - I) {
    pi -= ntile - I;
    ++I;
  }
  const int J = I + pi;
  const int i = I * 32 + (lane & 31), j = J * 32 + (lane & 31), kh = lane >> 5;
  const int64_t r0 = (int64_t)c * chunk, r1 = std::min<int64_t>(rows, r0 + chunk);
  const bool diag = I == J;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  float vacc = 0.f;
  for (int64_t r = r0; r < r1; r += 2 * GR_UNROLL) {
    float a[GR_UNROLL], b[GR_UNROLL], ww[GR_UNROLL];
#pragma unroll
    for (int u = 0; u < GR_UNROLL; ++u) {
      const int64_t rr = r + 2 * u + kh;
      const bool ok = rr < r1;
      a[u] = (ok && i < h) ? F[rr * ldf + i] : 0.f;
      b[u] = (ok && j < h) ? F[rr * ldf + j] : 0.f;
      ww[u] = ok ? (w ? w[rr] : 1.f) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < GR_UNROLL; ++u) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
      if (diag) vacc = fmaf(ww[u], b[u], vacc);
    }
  }
  // C/D map of the 32x32 forms: column n = lane & 31, row m = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
  float *Pc = P + (int64_t)c * h * h;
  if (j < h) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int m = I * 32 + (q & 3) + 8 * (q >> 2) + 4 * kh;
      if (m < h) Pc[(int64_t)m * h + j] = acc[q];
    }
  }
  if (diag) {
    const float vs = vacc + __shfl_xor(vacc, 32, 64);      // (even rows) + (odd rows), either lane
    if (lane < 32 && j < h) Pv[(int64_t)c * h + j] = vs;
  }
}

// G[i][j] = G[j][i] = sum over chunks (ascending) of the partial at (min, max) (+ reg on the diagonal)
__global__ __launch_bounds__(256) void als_gram_reduce_kernel(const float *__restrict__ P,
                                                              const float *__restrict__ Pv, int nch, int h,
                                                              float reg, float *__restrict__ G,
                                                              float *__restrict__ v) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t hh = (int64_t)h * h;
  if (e < hh) {
    const int i = (int)(e / h), j = (int)(e % h);
    const int a = min(i, j), b = max(i, j);
    float s = 0.f;
    for (int c = 0; c < nch; ++c) s += P[c * hh + (int64_t)a * h + b];
    if (i == j) s += reg;
    G[e] = s;
  } else if (e < hh + h) {
    const int j = (int)(e - hh);
    float s = 0.f;
    for (int c = 0; c < nch; ++c) s += Pv[(int64_t)c * h + j];
    v[j] = s;
  }
}

// ---------------------------------------------------------------------- solve
// Lane l owns dimensions k = l + 64 t (t < NT); every dot product is a per-lane chain over t then an
// xor butterfly (a + b == b + a bitwise: every lane ends with the same value, so every branch on it is
// wave-uniform).  LDS per workgroup (4 waves, one row each): [G if G_LDS][wave 0: stash][wave 1] ...
constexpr int SOLVE_LDS = 64 * 1024;     // two workgroups (8 waves) per CU
constexpr int G_LDS_MAX = 32 * 1024;     // G goes to LDS up to h = 90
constexpr int SOLVE_UNROLL = 4;
// Rows of LONG_ROW_MIN or more entries (popular items) go to a workgroup of LONG_WAVES waves: one wave per
// row would serialise a 100 000-entry row behind the whole grid
constexpr int LONG_ROW_MIN = 512;
constexpr int LONG_WAVES = 16;

// q = G p, one f32 chain per output over j ascending; p[j] comes from lane j & 63 of register j >> 6
template <int NT>
__device__ __forceinline__ void gemv(const float *Gs, int h, int lane, const float (&p)[NT], float (&q)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) q[t] = 0.f;
#pragma unroll
  for (int t2 = 0; t2 < NT; ++t2) {
    const int jn = min(64, h - 64 * t2);
    if (jn <= 0) break;
    const float *row = Gs + (int64_t)(64 * t2) * h;
    for (int l = 0; l < jn; ++l) {
      const float pj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p[t2]), l));
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int k = lane + 64 * t;
        if (k < h) q[t] = fmaf(row[k], pj, q[t]);
      }
      row += h;
    }
  }
}

__device__ __forceinline__ float entry_value(const float *data, int64_t e) { return data ? data[e] : 1.f; }

template <int NT, bool G_LDS>
__global__ __launch_bounds__(256) void als_solve_kernel(const int64_t *__restrict__ indptr,
                                                        const int32_t *__restrict__ indices,
                                                        const float *__restrict__ data, int row_lo, int row_hi,
                                                        const float *__restrict__ F, int ldf, int h,
                                                        const float *__restrict__ G, const float *__restrict__ v,
                                                        const float *__restrict__ col_bias,
                                                        const float *__restrict__ row_bias, float alpha,
                                                        int cg_steps, float *__restrict__ X, int ldx,
                                                        int stash_rows) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (G_LDS) {
    for (int e = threadIdx.x; e < h * h; e += 256) lds[e] = G[e];
    __syncthreads();
  }
  const int row = row_lo + blockIdx.x * 4 + wv;
  if (row >= row_hi) return;                      // (no barrier after this point)
  const float *Gs = G_LDS ? lds : G;
  float *stash = lds + (G_LDS ? h * h : 0) + (int64_t)wv * stash_rows * h;

  const int64_t e0 = indptr[row];
  const int n = (int)(indptr[row + 1] - e0);
  if (n >= LONG_ROW_MIN) return;                      // (als_solve_long_kernel's row)
  const bool stashed = n <= stash_rows;
  const float rb = row_bias ? row_bias[row] : 0.f;
  const float rs_scale = row_bias ? rb : 1.f;     // user side: -F^T b; item side: -b_i F^T 1
  float *xrow = X + (int64_t)row * ldx;

  float x[NT], r[NT], p[NT], q[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int k = lane + 64 * t;
    x[t] = k < h ? xrow[k] : 0.f;
    r[t] = k < h ? -(rs_scale * v[k]) : 0.f;
  }
  // q = A x0 (dense part first, then the row's entries in order); r = rhs, gathered in the same pass
  gemv<NT>(Gs, h, lane, x, q);
  for (int j0 = 0; j0 < n; j0 += SOLVE_UNROLL) {
    float f[SOLVE_UNROLL][NT], a[SOLVE_UNROLL], coef[SOLVE_UNROLL];
#pragma unroll
    for (int u = 0; u < SOLVE_UNROLL; ++u) {
      const int j = j0 + u;
      const bool ok = j < n;
      const int64_t col = ok ? indices[e0 + j] : 0;
      const float val = ok ? entry_value(data, e0 + j) : 0.f;
      a[u] = val > 0.f ? alpha : 0.f;
      const float bsel = col_bias ? (ok ? col_bias[col] : 0.f) : rb;
      coef[u] = ok ? (1.f + a[u]) * val - a[u] * bsel : 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int k = lane + 64 * t;
        f[u][t] = (ok && k < h) ? F[col * ldf + k] : 0.f;
      }
    }
    if (stashed) {
#pragma unroll
      for (int u = 0; u < SOLVE_UNROLL; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int k = lane + 64 * t;
          if (j0 + u < n && k < h) stash[(int64_t)(j0 + u) * h + k] = f[u][t];
        }
    }
    float d[SOLVE_UNROLL];
#pragma unroll
    for (int u = 0; u < SOLVE_UNROLL; ++u) d[u] = a[u] != 0.f ? wave_dot<NT>(f[u], x) : 0.f;
#pragma unroll
    for (int u = 0; u < SOLVE_UNROLL; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        r[t] = fmaf(coef[u], f[u][t], r[t]);
        if (a[u] != 0.f) q[t] = fmaf(a[u] * d[u], f[u][t], q[t]);
      }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    r[t] -= q[t];
    p[t] = r[t];
  }
  float rs = wave_dot<NT>(r, r);

  for (int s = 0; s < cg_steps && rs > 0.f; ++s) {
    gemv<NT>(Gs, h, lane, p, q);
    if (alpha != 0.f) {
      for (int j0 = 0; j0 < n; j0 += SOLVE_UNROLL) {
        float f[SOLVE_UNROLL][NT], a[SOLVE_UNROLL];
#pragma unroll
        for (int u = 0; u < SOLVE_UNROLL; ++u) {
          const int j = j0 + u;
          const bool ok = j < n;
          a[u] = (ok && entry_value(data, e0 + j) > 0.f) ? alpha : 0.f;
          const int64_t col = (a[u] != 0.f && !stashed) ? indices[e0 + j] : 0;
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const int k = lane + 64 * t;
            f[u][t] = 0.f;
            if (a[u] != 0.f && k < h) f[u][t] = stashed ? stash[(int64_t)j * h + k] : F[col * ldf + k];
          }
        }
        float d[SOLVE_UNROLL];
#pragma unroll
        for (int u = 0; u < SOLVE_UNROLL; ++u) d[u] = a[u] != 0.f ? wave_dot<NT>(f[u], p) : 0.f;
#pragma unroll
        for (int u = 0; u < SOLVE_UNROLL; ++u)
          if (a[u] != 0.f) {
#pragma unroll
            for (int t = 0; t < NT; ++t) q[t] = fmaf(a[u] * d[u], f[u][t], q[t]);
          }
      }
    }
    const float pq = wave_dot<NT>(p, q);
    if (!(pq > 0.f)) break;                      // (G singular at reg = 0, or a non-finite row)
    const float al = rs / pq;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      x[t] = fmaf(al, p[t], x[t]);
      r[t] = fmaf(-al, q[t], r[t]);
    }
    const float rsn = wave_dot<NT>(r, r);
    const float beta = rsn / rs;
#pragma unroll
    for (int t = 0; t < NT; ++t) p[t] = fmaf(beta, p[t], r[t]);
    rs = rsn;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int k = lane + 64 * t;
    if (k < h) xrow[k] = x[t];
  }
}

// Long rows: every wave of the workgroup carries the whole CG state (x, r, p identical in all of them)
// and computes G . p itself; the row's entries are cut into LONG_WAVES contiguous pieces, one per wave,
// and the pieces' sparse sums are added in wave order through LDS.  The factor rows stream from memory.
template <int NT>
__device__ __forceinline__ void long_combine(float *red, int wv, int lane, int h, const float (&part)[NT],
                                             float (&acc)[NT]) {
  __syncthreads();                                // (the previous combine's reads are done)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int k = lane + 64 * t;
    if (k < h) red[wv * MAX_H + k] = part[t];
  }
  __syncthreads();
  for (int w = 0; w < LONG_WAVES; ++w)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int k = lane + 64 * t;
      if (k < h) acc[t] += red[w * MAX_H + k];
    }
}

template <int NT>
__global__ __launch_bounds__(1024) void als_solve_long_kernel(const int64_t *__restrict__ indptr,
                                                              const int32_t *__restrict__ indices,
                                                              const float *__restrict__ data, int row_lo,
                                                              const float *__restrict__ F, int ldf, int h,
                                                              const float *__restrict__ G,
                                                              const float *__restrict__ v,
                                                              const float *__restrict__ col_bias,
                                                              const float *__restrict__ row_bias, float alpha,
                                                              int cg_steps, float *__restrict__ X, int ldx) {
  __shared__ float red[LONG_WAVES * MAX_H];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = row_lo + blockIdx.x;
  const int64_t e0 = indptr[row];
  const int n = (int)(indptr[row + 1] - e0);
  if (n < LONG_ROW_MIN) return;                       // (workgroup-uniform: no barrier has run yet)
  const int piece = (n + LONG_WAVES - 1) / LONG_WAVES;
  const int jb = min(n, wv * piece), je = min(n, jb + piece);
  const float rb = row_bias ? row_bias[row] : 0.f;
  const float rs_scale = row_bias ? rb : 1.f;
  float *xrow = X + (int64_t)row * ldx;

  float x[NT], r[NT], p[NT], q[NT], rp[NT], qp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int k = lane + 64 * t;
    x[t] = k < h ? xrow[k] : 0.f;
    r[t] = k < h ? -(rs_scale * v[k]) : 0.f;
    rp[t] = qp[t] = 0.f;
  }
  gemv<NT>(G, h, lane, x, q);
  for (int j0 = jb; j0 < je; j0 += SOLVE_UNROLL) {
    float f[SOLVE_UNROLL][NT], a[SOLVE_UNROLL], coef[SOLVE_UNROLL];
#pragma unroll
    for (int u = 0; u < SOLVE_UNROLL; ++u) {
      const int j = j0 + u;
      const bool ok = j < je;
      const int64_t col = ok ? indices[e0 + j] : 0;
      const float val = ok ? entry_value(data, e0 + j) : 0.f;
      a[u] = val > 0.f ? alpha : 0.f;
      const float bsel = col_bias ? (ok ? col_bias[col] : 0.f) : rb;
      coef[u] = ok ? (1.f + a[u]) * val - a[u] * bsel : 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int k = lane + 64 * t;
        f[u][t] = (ok && k < h) ? F[col * ldf + k] : 0.f;
      }
    }
    float d[SOLVE_UNROLL];
#pragma unroll
    for (int u = 0; u < SOLVE_UNROLL; ++u) d[u] = a[u] != 0.f ? wave_dot<NT>(f[u], x) : 0.f;
#pragma unroll
    for (int u = 0; u < SOLVE_UNROLL; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        rp[t] = fmaf(coef[u], f[u][t], rp[t]);
        if (a[u] != 0.f) qp[t] = fmaf(a[u] * d[u], f[u][t], qp[t]);
      }
  }
  long_combine<NT>(red, wv, lane, h, rp, r);
  long_combine<NT>(red, wv, lane, h, qp, q);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    r[t] -= q[t];
    p[t] = r[t];
  }
  float rs = wave_dot<NT>(r, r);

  for (int s = 0; s < cg_steps && rs > 0.f; ++s) {
    gemv<NT>(G, h, lane, p, q);
    if (alpha != 0.f) {
#pragma unroll
      for (int t = 0; t < NT; ++t) qp[t] = 0.f;
      for (int j0 = jb; j0 < je; j0 += SOLVE_UNROLL) {
        float f[SOLVE_UNROLL][NT], a[SOLVE_UNROLL];
#pragma unroll
        for (int u = 0; u < SOLVE_UNROLL; ++u) {
          const int j = j0 + u;
          a[u] = (j < je && entry_value(data, e0 + j) > 0.f) ? alpha : 0.f;
          const int64_t col = a[u] != 0.f ? indices[e0 + j] : 0;
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const int k = lane + 64 * t;
            f[u][t] = (a[u] != 0.f && k < h) ? F[col * ldf + k] : 0.f;
          }
        }
        float d[SOLVE_UNROLL];
#pragma unroll
        for (int u = 0; u < SOLVE_UNROLL; ++u) d[u] = a[u] != 0.f ? wave_dot<NT>(f[u], p) : 0.f;
#pragma unroll
        for (int u = 0; u < SOLVE_UNROLL; ++u)
          if (a[u] != 0.f) {
#pragma unroll
            for (int t = 0; t < NT; ++t) qp[t] = fmaf(a[u] * d[u], f[u][t], qp[t]);
          }
      }
      long_combine<NT>(red, wv, lane, h, qp, q);
    }
    const float pq = wave_dot<NT>(p, q);
    if (!(pq > 0.f)) break;                      // (the same value in every wave: a uniform exit)
    const float al = rs / pq;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      x[t] = fmaf(al, p[t], x[t]);
      r[t] = fmaf(-al, q[t], r[t]);
    }
    const float rsn = wave_dot<NT>(r, r);
    const float beta = rsn / rs;
#pragma unroll
    for (int t = 0; t < NT; ++t) p[t] = fmaf(beta, p[t], r[t]);
    rs = rsn;
  }
  if (wv == 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int k = lane + 64 * t;
      if (k < h) xrow[k] = x[t];
    }
  }
}

// ------------------------------------------------------------------ objective
// One wave per user row: sum over its entries of w (r - s)^2 - s^2 in float64, s = (x_u . y_i chain) + b_i
template <int NT>
__global__ __launch_bounds__(256) void als_objective_rows_kernel(const int64_t *__restrict__ indptr,
                                                                 const int32_t *__restrict__ indices,
                                                                 const float *__restrict__ data, int rows,
                                                                 const float *__restrict__ X, int ldx,
                                                                 const float *__restrict__ Y, int ldy, int h,
                                                                 const float *__restrict__ bias, float alpha,
                                                                 double *__restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float x[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int k = lane + 64 * t;
    x[t] = k < h ? X[(int64_t)row * ldx + k] : 0.f;
  }
  const int64_t e0 = indptr[row], e1 = indptr[row + 1];
  double acc = 0.0;
  for (int64_t e = e0; e < e1; e += SOLVE_UNROLL) {
    float f[SOLVE_UNROLL][NT];
#pragma unroll
    for (int u = 0; u < SOLVE_UNROLL; ++u) {
      const bool ok = e + u < e1;
      const int64_t col = ok ? indices[e + u] : 0;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int k = lane + 64 * t;
        f[u][t] = (ok && k < h) ? Y[col * ldy + k] : 0.f;
      }
    }
    float d[SOLVE_UNROLL];
#pragma unroll
    for (int u = 0; u < SOLVE_UNROLL; ++u) d[u] = wave_dot<NT>(f[u], x);
#pragma unroll
    for (int u = 0; u < SOLVE_UNROLL; ++u) {
      if (e + u >= e1) break;
      const float val = entry_value(data, e + u);
      const double s = (double)(d[u] + (bias ? bias[indices[e + u]] : 0.f));
      const double wt = 1.0 + (val > 0.f ? (double)alpha : 0.0);
      const double err = (double)val - s;
      acc += wt * err * err - s * s;
    }
  }
  if (lane == 0) part[row] = acc;
}

// One workgroup: thread t adds part[t], part[t + 256], ... and its share of the Gram terms, then a
// fixed tree.  tr(X^T X Y^T Y) = sum_ij (Gx - reg I)_ij (Gy - reg I)_ij (both symmetric).
__global__ __launch_bounds__(256) void als_objective_final_kernel(const double *__restrict__ part, int rows,
                                                                  int cols, int h, const float *__restrict__ bias,
                                                                  float reg, const float *__restrict__ Gx,
                                                                  const float *__restrict__ Gy,
                                                                  const float *__restrict__ sx,
                                                                  const float *__restrict__ cy,
                                                                  double *__restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int r = tid; r < rows; r += 256) s += part[r];
  const int64_t hh = (int64_t)h * h;
  const double lam = (double)reg;
  for (int64_t e = tid; e < hh; e += 256) {
    const bool dg = (e / h) == (e % h);
    const double gx = (double)Gx[e] - (dg ? lam : 0.0), gy = (double)Gy[e] - (dg ? lam : 0.0);
    s += gx * gy;
    if (dg) s += lam * (gx + gy);
  }
  if (bias) {
    double bb = 0.0;
    for (int c = tid; c < cols; c += 256) bb += (double)bias[c] * (double)bias[c];
    s += (double)rows * bb;
    for (int k = tid; k < h; k += 256) s += 2.0 * (double)sx[k] * (double)cy[k];
  }
  red[tid] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) out[0] = red[0];
}

}  // namespace

extern "C" int64_t rk_als_gram_workspace_bytes(int32_t rows, int32_t h) {
  if (rows < 0 || h < 1 || h > MAX_H) return -2;
  const GramPlan p = gram_plan(rows, h);
  return (int64_t)p.nch * ((int64_t)h * h + h) * (int64_t)sizeof(float);
}

extern "C" int rk_als_gram(const float *F, int32_t rows, int32_t h, int32_t ldf, const float *w, float reg,
                           float *G, float *v, void *ws, int64_t ws_bytes, void *stream) {
  RK_SIDE_REQUIRE(rows >= 0 && h >= 1 && h <= MAX_H && ldf >= h, "rows >= 0, 1 <= h <= 512, ldf >= h");
  RK_SIDE_REQUIRE(G && v && (rows == 0 || F), "G, v (and F when rows > 0) must be set");
  RK_SIDE_REQUIRE(ws_bytes >= rk_als_gram_workspace_bytes(rows, h) && ws, "workspace too small");
  const GramPlan p = gram_plan(rows, h);
  float *P = (float *)ws;
  float *Pv = P + (int64_t)p.nch * h * h;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(als_gram_partial_kernel, dim3(p.npairs, p.nch), dim3(64), 0, st, F, rows, h, ldf, w, p.chunk,
                     p.ntile, P, Pv);
  RK_SIDE_CHECK_LAUNCH("als_gram_partial");
  const int64_t n = (int64_t)h * h + h;
  hipLaunchKernelGGL(als_gram_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, Pv, p.nch, h,
                     reg, G, v);
  RK_SIDE_CHECK_LAUNCH("als_gram_reduce");
  return 0;
}

extern "C" int rk_als_solve(const int64_t *indptr, const int32_t *indices, const float *data, int32_t row_lo,
                            int32_t row_hi, const float *F, int32_t ldf, int32_t h, const float *G, const float *v,
                            const float *col_bias, const float *row_bias, float alpha, int32_t cg_steps, float *X,
                            int32_t ldx, int32_t flags, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldf >= h && ldx >= h, "1 <= h <= 512, ldf >= h, ldx >= h");
  RK_SIDE_REQUIRE(row_lo >= 0 && row_hi >= row_lo, "0 <= row_lo <= row_hi");
  RK_SIDE_REQUIRE(cg_steps >= 1, "cg_steps >= 1");
  RK_SIDE_REQUIRE(!(col_bias && row_bias), "at most one of col_bias / row_bias");
  RK_SIDE_REQUIRE((flags & ~(RK_ALS_FORCE_STREAM | RK_ALS_G_GLOBAL)) == 0, "unknown flags");
  if (row_hi == row_lo) return 0;
  RK_SIDE_REQUIRE(indptr && indices && F && G && v && X, "null pointer");
  const bool g_lds = !(flags & RK_ALS_G_GLOBAL) && (int64_t)h * h * 4 <= G_LDS_MAX;
  const int64_t g_floats = g_lds ? (int64_t)h * h : 0;
  int stash_rows = (int)((SOLVE_LDS / 4 - g_floats) / 4 / h);
  if (flags & RK_ALS_FORCE_STREAM) stash_rows = 0;
  const size_t lds = (size_t)(g_floats + 4 * (int64_t)stash_rows * h) * sizeof(float);
  const dim3 grid((unsigned)((row_hi - row_lo + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  dispatch_nt(h, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    hipLaunchKernelGGL(als_solve_long_kernel<NT>, dim3((unsigned)(row_hi - row_lo)), dim3(64 * LONG_WAVES), 0, st,
                       indptr, indices, data, row_lo, F, ldf, h, G, v, col_bias, row_bias, alpha, cg_steps, X, ldx);
    auto short_rows = g_lds ? als_solve_kernel<NT, true> : als_solve_kernel<NT, false>;
    hipLaunchKernelGGL(short_rows, grid, dim3(256), lds, st, indptr, indices, data, row_lo, row_hi, F, ldf, h, G, v,
                       col_bias, row_bias, alpha, cg_steps, X, ldx, stash_rows);
  });
  RK_SIDE_CHECK_LAUNCH("als_solve");
  return 0;
}

extern "C" int64_t rk_als_objective_workspace_bytes(int32_t rows) {
  if (rows < 0) return -2;
  return (int64_t)std::max(rows, 1) * (int64_t)sizeof(double);
}

extern "C" int rk_als_objective(const int64_t *indptr, const int32_t *indices, const float *data, int32_t rows,
                                int32_t cols, const float *X, int32_t ldx, const float *Y, int32_t ldy, int32_t h,
                                const float *bias, float alpha, float reg, const float *Gx, const float *Gy,
                                const float *sx, const float *cy, void *ws, int64_t ws_bytes, double *out,
                                void *stream) {
  RK_SIDE_REQUIRE(rows >= 0 && cols >= 0 && h >= 1 && h <= MAX_H && ldx >= h && ldy >= h,
              "rows, cols >= 0, 1 <= h <= 512, ldx, ldy >= h");
  RK_SIDE_REQUIRE(Gx && Gy && out && (!bias || (sx && cy)), "null pointer");
  RK_SIDE_REQUIRE(ws && ws_bytes >= rk_als_objective_workspace_bytes(rows), "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double *part = (double *)ws;
  if (rows > 0) {
    RK_SIDE_REQUIRE(indptr && indices && X && Y, "null pointer");
    const dim3 grid((unsigned)((rows + 3) / 4));
    dispatch_nt(h, [&](auto nt) {
      hipLaunchKernelGGL(als_objective_rows_kernel<decltype(nt)::value>, grid, dim3(256), 0, st, indptr, indices, data,
                         rows, X, ldx, Y, ldy, h, bias, alpha, part);
    });
    RK_SIDE_CHECK_LAUNCH("als_objective_rows");
  }
  hipLaunchKernelGGL(als_objective_final_kernel, dim3(1), dim3(256), 0, st, part, rows, cols, h, bias, reg, Gx, Gy,
                     sx, cy, out);
  RK_SIDE_CHECK_LAUNCH("als_objective_final");
  return 0;
}
