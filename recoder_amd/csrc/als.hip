// Implicit-feedback ALS (include/recoder_als.h, librecoder_als.so).
//
//   rk_als_gram       G = F^T F + reg I and v = F^T w: split-K over fixed row chunks, each chunk one
//                     k-ascending chain on v_mfma_f32_32x32x2_f32 (upper tile pairs only), then the
//                     chunks added in ascending order and mirrored: bitwise symmetric, no atomics
//   rk_als_solve      one wave per row: the row's factor rows gathered once into LDS (or streamed
//                     when they do not fit), cg_steps CG steps warm-started from the row's value;
//                     G . p from LDS (small h) or from memory (L2).  Rows of >= 512 entries: one
//                     workgroup of 16 waves each, the entries split between the waves
//   rk_als_objective  the sparse part of L, one wave per row, per-row float64 partials; one
//                     workgroup adds them and the Gram terms in a fixed order
//
// BPR pairwise ranking for the same model (rk_als_bpr_*): one synchronous mini-batch SGD step is
//   rk_als_bpr_sample  one thread per slot: a stored entry and a rejected-until-unseen negative, from
//                      a counter hash of (seed, step, slot, draw); integer arithmetic only
//   rk_als_bpr_grad    one wave per triple: x, g = sigma(-x), softplus(-x), and the staging rows
//                      D[t] = q_i - q_j, P[t] = p_u (the apply step then updates the tables in place)
//   rk_als_bpr_apply   one wave per distinct row of the sorted keys: the row's segment summed in
//                      ascending slot order, one fmaf chain per element, then the row's own update.
//                      No atomics: nobody else writes the row
//
// WARP and dynamic negative sampling on the same step (rk_als_rank_sample, rk_als_warp_grad):
//   rk_als_rank_sample  one wave per slot: the sampler's draws 64 at a time, the candidates scored against p_u
//                       several rows in flight, decided in draw order (first margin violator / hardest of M)
//   rk_als_warp_grad    rk_als_bpr_grad's staging rows with g = the rank weight of the slot's trials
//
// LightGCN for the same model (rk_als_lgcn_*): the step of recoder_amd/lightgcn.py adds
//   rk_als_lgcn_propagate  one group of lanes per CSR row: the scaled sum of the row's gathered table rows,
//                          lanes own columns; long rows by a workgroup of 16 waves each, in fixed parts
//   rk_als_lgcn_scatter    the apply's segment walk, writing the gradient rows and the counts
//   rk_als_lgcn_adam       one elementwise pass: the L2 term and the Adam update of a base table
//
// SimGCL on top of it (rk_als_gcl_*): the step of recoder_amd/simgcl.py adds
//   rk_als_gcl_propagate   rk_als_lgcn_propagate's row pass (one template) with a counter-hash noise of length
//                          eps added to every row in the epilogue
//   rk_als_gcl_contrast    InfoNCE between two view tables over the distinct keys of a step: loss and gradient
//                          rows, the T x T scores tiled through LDS; fixed summation orders, no atomics
//
// DirectAU for the same model (rk_als_dau_*): the step of recoder_amd/directau.py adds
//   rk_als_dau_grad        alignment and uniformity over the slots of a step: the three losses and one gradient row
//                          per slot and side, on the contrast's tile code; the T x T weights are stored once and
//                          staged as they are by one dZ product per side
//
// Sampled softmax for the same model (rk_als_ssm_*): the step of recoder_amd/ssm.py adds
//   rk_als_ssm_grad        the softmax of every slot over the batch's positives and S shared uniform negatives: the
//                          T x (T + S) scores and both gradient products on the f32 MFMA through LDS, one expf per
//                          element; fixed summation orders, no atomics
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/recoder_als.h"
#include "side_error.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MAX_H = 512;

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

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

template <int NT>
__device__ __forceinline__ float wave_dot(const float (&a)[NT], const float (&b)[NT]) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) s = fmaf(a[t], b[t], s);
  return wave_sum(s);
}

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

// ------------------------------------------------------------------------ bpr
// The counter RNG, restated here (this translation unit does not include csrc/common.h): splitmix64's
// output function, z += 0x9E3779B97F4A7C15, two xor-shift-multiplies, a last xor-shift.
__host__ __device__ __forceinline__ uint64_t bpr_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// draw d of (seed, step, slot) mapped to [0, range): the high 32 bits times range, shifted down
__host__ __device__ __forceinline__ uint32_t bpr_draw(uint64_t slot_key, uint32_t d, uint32_t range) {
  const uint64_t r = bpr_mix(slot_key + d);
  return (uint32_t)(((r >> 32) * (uint64_t)range) >> 32);
}

constexpr int BPR_MAX_DRAWS = 32;

__global__ __launch_bounds__(256) void als_bpr_sample_kernel(const int64_t *__restrict__ indptr,
                                                             const int32_t *__restrict__ indices, int n_users,
                                                             int n_items, uint32_t nnz, uint64_t seed_key,
                                                             uint32_t step, int T, int32_t *__restrict__ users,
                                                             int32_t *__restrict__ pos, int32_t *__restrict__ neg) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const uint64_t key = bpr_mix(seed_key ^ (((uint64_t)step << 32) | (uint32_t)t));
  const int64_t e = (int64_t)bpr_draw(key, 0, nnz);
  // the row that holds e: the last u with indptr[u] <= e (empty rows share their successor's start)
  int lo = 0, hi = n_users;                 // (indptr[lo] <= e < indptr[hi] throughout)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (indptr[mid] <= e) lo = mid; else hi = mid;
  }
  const int u = lo;
  const int64_t r0 = indptr[u], r1 = indptr[u + 1];
  int j = -1;
  for (int d = 1; d <= BPR_MAX_DRAWS; ++d) {
    const int c = (int)bpr_draw(key, (uint32_t)d, (uint32_t)n_items);
    int64_t a = r0, b = r1;                 // first position in [r0, r1) with indices[.] >= c
    while (a < b) {
      const int64_t mid = a + ((b - a) >> 1);
      if (indices[mid] < c) a = mid + 1; else b = mid;
    }
    if (!(a < r1 && indices[a] == c)) {
      j = c;
      break;
    }
  }
  users[t] = u;
  pos[t] = indices[e];
  neg[t] = j;
}

// One wave per triple.  Lane l owns dimensions k = l + 64 t: d_k = q_ik - q_jk (one rounding), the dot
// is the lane's fmaf chain over t ascending from +0, then the xor butterfly of wave_sum, then + b_i,
// then - b_j.  A slot with neg < 0 (or an id outside the tables) is invalid: g, loss and both rows +0.
template <int NT>
__global__ __launch_bounds__(256) void als_bpr_grad_kernel(const int32_t *__restrict__ users,
                                                           const int32_t *__restrict__ pos,
                                                           const int32_t *__restrict__ neg, int T, int n_users,
                                                           int n_items, const float *__restrict__ X, int ldx,
                                                           const float *__restrict__ Y, int ldy,
                                                           const float *__restrict__ bias, int h,
                                                           float *__restrict__ g, float *__restrict__ loss,
                                                           float *__restrict__ xout, float *__restrict__ D,
                                                           float *__restrict__ P) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int u = users[t], i = pos[t], j = neg[t];
  const bool ok = u >= 0 && u < n_users && i >= 0 && i < n_items && j >= 0 && j < n_items;   // (wave-uniform)
  float p[NT], d[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    const bool in = ok && k < h;
    p[q] = in ? X[(int64_t)u * ldx + k] : 0.f;
    const float qi = in ? Y[(int64_t)i * ldy + k] : 0.f;
    const float qj = in ? Y[(int64_t)j * ldy + k] : 0.f;
    d[q] = qi - qj;
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) {
      D[(int64_t)t * h + k] = d[q];
      P[(int64_t)t * h + k] = p[q];
    }
  }
  if (!ok) {
    if (lane == 0) {
      g[t] = loss[t] = 0.f;
      if (xout) xout[t] = 0.f;
    }
    return;
  }
  const float x = (wave_dot<NT>(p, d) + bias[i]) - bias[j];
  if (lane == 0) {
    // sigma(-x) and softplus(-x) = max(-x, 0) + log1p(exp(-|x|)) through e = exp(-|x|) <= 1
    const float e = expf(-fabsf(x));
    g[t] = x >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);
    loss[t] = fmaxf(-x, 0.f) + log1pf(e);
    if (xout) xout[t] = x;
  }
}

// ----------------------------------------------------------------- rank (WARP / DNS)
// The model-aware sampler: one wave per slot.  Draw 0 is als_bpr_sample_kernel's; p_u stays in registers in
// als_bpr_grad_kernel's lane layout.  The draws go 64 at a time: lane l hashes draw d0 + l and searches the
// user's row for it, a ballot gives the candidates (the draws the user does not hold), and the candidates
// are scored G at a time in draw order -- the G row gathers are issued before any of them is reduced --
// and decided one after the other, as the sequential definition walks them.  A score computed behind the
// stopping point is dropped: it reaches neither `scores` nor any decision.  Every decision is taken on a
// butterfly's result, the same in all lanes, so every branch on it is wave-uniform.
constexpr int RANK_MAX_DRAWS = 256;
constexpr int RANK_WARP = 0;
constexpr int RANK_DNS = 1;

template <int NT, int G>
__global__ __launch_bounds__(256) void als_rank_sample_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, int n_users, int n_items, uint32_t nnz,
    uint64_t seed_key, uint32_t step, int T, const float *__restrict__ X, int ldx, const float *__restrict__ Y,
    int ldy, const float *__restrict__ bias, int h, int mode, int max_draws, int num_candidates, float margin,
    int32_t *__restrict__ users, int32_t *__restrict__ pos, int32_t *__restrict__ neg, int32_t *__restrict__ trials,
    float *__restrict__ s_pos, float *__restrict__ s_neg, float *__restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const uint64_t key = bpr_mix(seed_key ^ (((uint64_t)step << 32) | (uint32_t)t));
  const int64_t e = (int64_t)bpr_draw(key, 0, nnz);
  int lo = 0, hi = n_users;                 // (indptr[lo] <= e < indptr[hi] throughout)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (indptr[mid] <= e) lo = mid; else hi = mid;
  }
  const int u = lo;
  const int64_t r0 = indptr[u], r1 = indptr[u + 1];
  const int i = indices[e];
  const bool ok = i >= 0 && i < n_items;    // (a column outside the table: the slot is invalid, nothing is read)
  float p[NT], q0[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    const bool in = ok && k < h;
    p[q] = in ? X[(int64_t)u * ldx + k] : 0.f;
    q0[q] = in ? Y[(int64_t)i * ldy + k] : 0.f;
  }
  const float sp = ok ? wave_dot<NT>(p, q0) + bias[i] : 0.f;
  int j = -1, n_scored = 0;
  float sn = 0.f;
  bool done = !ok;
  for (int d0 = 1; d0 <= max_draws; d0 += 64) {
    const int d = d0 + lane;
    int c = 0;
    bool cand = false;
    if (!done && d <= max_draws) {
      c = (int)bpr_draw(key, (uint32_t)d, (uint32_t)n_items);
      int64_t a = r0, b = r1;               // first position in [r0, r1) with indices[.] >= c
      while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (indices[mid] < c) a = mid + 1; else b = mid;
      }
      cand = !(a < r1 && indices[a] == c);
    }
    uint64_t m = __ballot(cand);
    float mine = 0.f;                       // (the score of this lane's draw, once it has been decided on)
    while (m && !done) {
      // DNS knows how many it still wants; WARP scores G ahead and drops what lies behind the violator
      const int want = mode == RANK_DNS ? min(G, num_candidates - n_scored) : G;
      int L[G], cg[G];
      float qg[G][NT], bg[G], s[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const bool on = m != 0 && g < want;
        L[g] = on ? __ffsll((unsigned long long)m) - 1 : -1;
        if (on) m &= m - 1;
        cg[g] = __shfl(c, on ? L[g] : 0, 64);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int q = 0; q < NT; ++q) {
          const int k = lane + 64 * q;
          qg[g][q] = (L[g] >= 0 && k < h) ? Y[(int64_t)cg[g] * ldy + k] : 0.f;
        }
        bg[g] = L[g] >= 0 ? bias[cg[g]] : 0.f;
      }
#pragma unroll
      for (int g = 0; g < G; ++g) s[g] = wave_dot<NT>(p, qg[g]) + bg[g];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (L[g] >= 0 && !done) {
          ++n_scored;
          if (lane == L[g]) mine = s[g];
          if (mode == RANK_DNS) {
            if (n_scored == 1 || s[g] > sn) {     // (strictly: a tie stays with the earlier draw)
              sn = s[g];
              j = cg[g];
            }
            done = n_scored == num_candidates;
          } else if ((s[g] - sp) + margin > 0.f) {
            sn = s[g];
            j = cg[g];
            done = true;
          }
        }
      }
    }
    if (scores && d <= max_draws) scores[(int64_t)t * max_draws + (d - 1)] = mine;
  }
  if (lane == 0) {
    users[t] = u;
    pos[t] = i;
    neg[t] = j;
    trials[t] = j >= 0 ? n_scored : 0;
    if (s_pos) s_pos[t] = sp;
    if (s_neg) s_neg[t] = j >= 0 ? sn : 0.f;
  }
}

// One wave per slot, als_bpr_grad_kernel's layout: the two scores are the sampler's chain (dot, then + b),
// g is the rank weight of the slot's trials, the loss is the hinge that the violator crossed.
template <int NT>
__global__ __launch_bounds__(256) void als_warp_grad_kernel(
    const int32_t *__restrict__ users, const int32_t *__restrict__ pos, const int32_t *__restrict__ neg,
    const int32_t *__restrict__ trials, int T, int n_users, int n_items, const float *__restrict__ X, int ldx,
    const float *__restrict__ Y, int ldy, const float *__restrict__ bias, int h, float margin,
    const float *__restrict__ weight, float *__restrict__ g, float *__restrict__ loss, float *__restrict__ D,
    float *__restrict__ P) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int u = users[t], i = pos[t], j = neg[t], n = trials[t];
  const bool ok = u >= 0 && u < n_users && i >= 0 && i < n_items && j >= 0 && j < n_items && n >= 1 &&
                  n <= RANK_MAX_DRAWS;                                                       // (wave-uniform)
  float p[NT], qi[NT], qj[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    const bool in = ok && k < h;
    p[q] = in ? X[(int64_t)u * ldx + k] : 0.f;
    qi[q] = in ? Y[(int64_t)i * ldy + k] : 0.f;
    qj[q] = in ? Y[(int64_t)j * ldy + k] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) {
      D[(int64_t)t * h + k] = qi[q] - qj[q];
      P[(int64_t)t * h + k] = p[q];
    }
  }
  if (!ok) {
    if (lane == 0) g[t] = loss[t] = 0.f;
    return;
  }
  const float sp = wave_dot<NT>(p, qi) + bias[i];
  const float sn = wave_dot<NT>(p, qj) + bias[j];
  if (lane == 0) {
    const float w = weight[n];
    g[t] = w;
    loss[t] = w * ((sn - sp) + margin);
  }
}

// One wave per sorted position s; the wave at the head of a segment of equal keys owns that row, the
// others leave.  order[s] is the entry's position before the sort: slot t = order / roles, and with
// roles == 2 (the item side) an odd position is the slot's negative, which enters with -g.
//   acc_k = fmaf(+-g_t, V[t, k], acc_k) over the segment, from +0;  c = the segment's length
//   new_k = fmaf(lr, fmaf(-(reg * c), old_k, acc_k), old_k)           (the bias likewise, V = 1)
constexpr int BPR_UNROLL = 4;

template <int NT>
__global__ __launch_bounds__(256) void als_bpr_apply_kernel(const int32_t *__restrict__ keys,
                                                            const int64_t *__restrict__ order, int n, int roles,
                                                            const float *__restrict__ g,
                                                            const float *__restrict__ V, int h, float lr,
                                                            float reg, int n_rows, float *__restrict__ table,
                                                            int ldt, float *__restrict__ bias) {
  const int lane = threadIdx.x & 63;
  const int s0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s0 >= n) return;
  const int key = keys[s0];
  if (key < 0 || key >= n_rows) return;                  // (the invalid slots' sentinel, sorted last)
  if (s0 > 0 && keys[s0 - 1] == key) return;             // (not a head)
  // the segment's length: 64 keys at a time, the first lane whose key differs
  int c = 0;
  for (;;) {
    const int s = s0 + c + lane;
    const bool same = s < n && keys[s] == key;
    const uint64_t m = __ballot(!same);
    if (m) {
      c += __ffsll((unsigned long long)m) - 1;
      break;
    }
    c += 64;
  }
  float acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = 0.f;
  float bacc = 0.f;
  const int64_t slots = roles == 2 ? n >> 1 : n;
  for (int a0 = 0; a0 < c; a0 += BPR_UNROLL) {
    float v[BPR_UNROLL][NT], w[BPR_UNROLL];
#pragma unroll
    for (int r = 0; r < BPR_UNROLL; ++r) {
      const bool in = a0 + r < c;
      const int64_t e = in ? order[s0 + a0 + r] : 0;
      const int64_t t = roles == 2 ? e >> 1 : e;
      const bool ok = in && e >= 0 && t < slots;         // (an order outside the batch adds nothing)
      const float gt = ok ? g[t] : 0.f;
      w[r] = (roles == 2 && (e & 1)) ? -gt : gt;
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const int k = lane + 64 * q;
        v[r][q] = (ok && k < h) ? V[t * h + k] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < BPR_UNROLL; ++r) {
      if (a0 + r < c) {                                  // (wave-uniform: a tail entry must not touch the chain)
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[q] = fmaf(w[r], v[r][q], acc[q]);
        bacc += w[r];
      }
    }
  }
  const float rc = reg * (float)c;
  float *row = table + (int64_t)key * ldt;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) {
      const float old = row[k];
      row[k] = fmaf(lr, fmaf(-rc, old, acc[q]), old);
    }
  }
  if (bias && lane == 0) {
    const float old = bias[key];
    bias[key] = fmaf(lr, fmaf(-rc, old, bacc), old);
  }
}

// ----------------------------------------------------------------------- lgcn
// Out[r] = row_scale[r] * sum_j col_scale[col_j] * F[col_j], Acc[r] = (Acc[r] + Out[r]) * acc_scale.
// A group of G lanes (a power of two, 1..64) owns a row; lane c of the group owns the column chunks
// c + G q, q < NT, of VEC floats each (VEC 4: one 16-byte access).  A lane walks its row's entries alone
// -- no cross-lane step -- so a column's sum is one fmaf chain over the entries in ascending order from
// +0, whatever G and VEC are: the scalar and the 16-byte forms give the same bits.
// A row of >= RK_ALS_LGCN_LONG_ROW entries is left to a workgroup of 16 waves (the second launch, at most
// LG_LONG_GRID workgroups that share the rows out by stride): its entries are cut into lg_parts(h)
// contiguous parts (bounds e0 + p len / parts: a function of the length and h alone), part p is the
// chain of group p mod (1024 / G), the parts meet in LDS and are added in ascending p.
constexpr int LG_LONG = RK_ALS_LGCN_LONG_ROW;
constexpr int LG_LONG_THREADS = 1024;
constexpr int LG_LONG_GRID = 2048;                       // workgroups of the long-row launch, at most
__host__ __device__ constexpr int lg_parts(int h) { return h <= 128 ? 64 : 16; }    // (parts * h * 4 <= 32 KiB)

template <int VEC>
struct LgVec;
template <>
struct LgVec<1> {
  typedef float T;
  static __device__ __forceinline__ float get(const float &v, int) { return v; }
  static __device__ __forceinline__ void set(float &v, int, float x) { v = x; }
  static __device__ __forceinline__ float zero() { return 0.f; }
};
template <>
struct LgVec<4> {
  typedef float4 T;
  static __device__ __forceinline__ float get(const float4 &v, int i) {
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
  }
  static __device__ __forceinline__ void set(float4 &v, int i, float x) {
    if (i == 0) v.x = x; else if (i == 1) v.y = x; else if (i == 2) v.z = x; else v.w = x;
  }
  static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};

// acc[q] (+)= the chain over the entries [e0, e1) for the lane's column chunks (chunk index cg + G q < nch)
template <int VEC, int NT>
__device__ __forceinline__ void lgcn_walk(const int32_t *__restrict__ indices, const float *__restrict__ col_scale,
                                          const float *__restrict__ F, int ldf, int64_t e0, int64_t e1, int cg,
                                          int G, int nch, typename LgVec<VEC>::T (&acc)[NT]) {
  typedef typename LgVec<VEC>::T V;
  constexpr int LG_UNROLL = NT * VEC <= 4 ? 8 : 4;      // entries whose gathers are issued together
  for (int64_t a = e0; a < e1; a += LG_UNROLL) {
    V v[LG_UNROLL][NT];
    float w[LG_UNROLL];
#pragma unroll
    for (int r = 0; r < LG_UNROLL; ++r) {
      const bool in = a + r < e1;
      const int col = in ? indices[a + r] : 0;
      w[r] = in ? col_scale[col] : 0.f;
      const float *row = F + (int64_t)col * ldf;
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const int ch = cg + G * q;
        v[r][q] = (in && ch < nch) ? *(const V *)(row + (int64_t)ch * VEC) : LgVec<VEC>::zero();
      }
    }
#pragma unroll
    for (int r = 0; r < LG_UNROLL; ++r) {
      if (a + r < e1) {                                  // (a tail entry must not touch the chain)
#pragma unroll
        for (int q = 0; q < NT; ++q)
#pragma unroll
          for (int i = 0; i < VEC; ++i)
            LgVec<VEC>::set(acc[q], i, fmaf(w[r], LgVec<VEC>::get(v[r][q], i), LgVec<VEC>::get(acc[q], i)));
      }
    }
  }
}

// SimGCL's noise (rk_als_gcl_propagate; NOISE below): Out[r] = x + eps sign(x) u[r] / |u[r]|_2, x the row as
// rk_als_lgcn_propagate rounds it.  u[r, c] = m 2^-24 with m the ODD 24-bit integer of a counter hash -- never 0,
// exact in f32 -- and key a hash of (seed, step, view, layer, side): bit 31 of the low word is the domain
// tag, a sampler slot is below 2^24.  sum_c m^2 < 2^57 is an INTEGER sum: any lanes, in any order, give
// the same |u[r]|, so the noise depends on (key, row, h) alone.
struct GclNoise {
  uint64_t key;
  float eps;
};

uint64_t gcl_key(int64_t seed, int32_t step, int32_t view, int32_t layer, int32_t side) {
  const uint64_t low = 0x80000000ull | ((uint64_t)view << 16) | ((uint64_t)layer << 8) | (uint64_t)side;
  return bpr_mix(bpr_mix((uint64_t)seed) ^ (((uint64_t)(uint32_t)step << 32) | low));
}

__device__ __forceinline__ uint64_t gcl_row_key(uint64_t key, int64_t r) { return bpr_mix(key + (uint64_t)r); }

__device__ __forceinline__ uint32_t gcl_m(uint64_t row_key, int col) {
  return ((uint32_t)(bpr_mix(row_key + (uint64_t)(uint32_t)col) >> 41) << 1) | 1u;
}

// eps / |u[r]|: the integer sum rounded once to f32, 2^-48 exact, a square root and a division
__device__ __forceinline__ float gcl_scale(uint64_t ss, float eps) { return eps / sqrtf((float)ss * 0x1p-48f); }

// the three roundings after the sum: s * row_scale, + Acc, * acc_scale; with NOISE one more before Acc:
// fmaf(+-nscale, u, x) by the sign of x -- written as fmaf, so that no instance is left to contract it or
// not -- or (x == 0) x itself as it stands
template <int VEC, bool NOISE>
__device__ __forceinline__ void lgcn_finish(typename LgVec<VEC>::T s, float rs, int64_t r, int ch,
                                            float *__restrict__ Out, int ldo, float *__restrict__ Acc, int lda,
                                            float acc_scale, const uint32_t (&m)[VEC], float nscale) {
  typedef typename LgVec<VEC>::T V;
  V o;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    float x = rs * LgVec<VEC>::get(s, i);
    if constexpr (NOISE) {
      const float u = (float)m[i] * 0x1p-24f;
      x = x > 0.f ? fmaf(nscale, u, x) : x < 0.f ? fmaf(-nscale, u, x) : x;
    }
    LgVec<VEC>::set(o, i, x);
  }
  if (Out) *(V *)(Out + r * ldo + (int64_t)ch * VEC) = o;
  if (Acc) {
    V *p = (V *)(Acc + r * lda + (int64_t)ch * VEC);
    const V old = *p;
    V n;
#pragma unroll
    for (int i = 0; i < VEC; ++i)
      LgVec<VEC>::set(n, i, (LgVec<VEC>::get(old, i) + LgVec<VEC>::get(o, i)) * acc_scale);
    *p = n;
  }
}

template <int VEC, int NT, bool NOISE>
__global__ __launch_bounds__(256) void als_lgcn_propagate_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const float *__restrict__ row_scale,
    const float *__restrict__ col_scale, int row_lo, int row_hi, const float *__restrict__ F, int ldf, int h,
    int G, float *__restrict__ Out, int ldo, float *__restrict__ Acc, int lda, float acc_scale, GclNoise nz) {
  typedef typename LgVec<VEC>::T V;
  const int nch = (h + VEC - 1) / VEC;                   // (VEC 4: h is a multiple of 4)
  const int rpb = 256 / G;                               // rows of a workgroup = its groups
  const int grp = threadIdx.x / G, cg = threadIdx.x % G;
  const int64_t r = (int64_t)row_lo + (int64_t)blockIdx.x * rpb + grp;
  if (r >= row_hi) return;
  const int64_t e0 = indptr[r], e1 = indptr[r + 1];
  if (e1 - e0 >= LG_LONG) return;                        // (the long kernel's)
  V acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = LgVec<VEC>::zero();
  lgcn_walk<VEC, NT>(indices, col_scale, F, ldf, e0, e1, cg, G, nch, acc);
  const float rs = row_scale[r];
  uint32_t m[NT][VEC];
  float nscale = 0.f;
  if constexpr (NOISE) {                                 // (a row's group leaves or stays as one: its lanes meet here)
    const uint64_t row_key = gcl_row_key(nz.key, r);
    uint64_t ss = 0;
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        m[q][i] = cg + G * q < nch ? gcl_m(row_key, (cg + G * q) * VEC + i) : 0u;
        ss += (uint64_t)m[q][i] * m[q][i];
      }
    for (int off = 32; off > 0; off >>= 1)
      if (off < G) ss += __shfl_xor((unsigned long long)ss, off, 64);
    nscale = gcl_scale(ss, nz.eps);
  }
#pragma unroll
  for (int q = 0; q < NT; ++q)
    if (cg + G * q < nch)
      lgcn_finish<VEC, NOISE>(acc[q], rs, r, cg + G * q, Out, ldo, Acc, lda, acc_scale, m[q], nscale);
}

// Workgroups of 16 waves over the long rows: workgroup b looks at the rows row_lo + b, + gridDim.x, ... (two
// indptr loads each; long rows that sit side by side go to different workgroups) and sums the long ones,
// one at a time; a short row is als_lgcn_propagate_kernel's.
template <int VEC, int NT, bool NOISE>
__global__ __launch_bounds__(LG_LONG_THREADS) void als_lgcn_propagate_long_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const float *__restrict__ row_scale,
    const float *__restrict__ col_scale, int row_lo, int row_hi, const float *__restrict__ F, int ldf, int h, int G,
    float *__restrict__ Out, int ldo, float *__restrict__ Acc, int lda, float acc_scale, GclNoise nz) {
  typedef typename LgVec<VEC>::T V;
  extern __shared__ float4 lg_lds4[];                    // lg_parts(h) x h floats
  __shared__ unsigned long long lg_ss[LG_LONG_THREADS / 64];      // (NOISE: the waves' sums of m^2)
  float *part = (float *)lg_lds4;
  const int nch = (h + VEC - 1) / VEC, parts = lg_parts(h);
  const int groups = LG_LONG_THREADS / G, grp = threadIdx.x / G, cg = threadIdx.x % G;
  for (int64_t r = (int64_t)row_lo + blockIdx.x; r < row_hi; r += gridDim.x) {   // (workgroup-uniform throughout)
    const int64_t e0 = indptr[r], len = indptr[r + 1] - e0;
    if (len < LG_LONG) continue;
    for (int p = grp; p < parts; p += groups) {
      V acc[NT];
#pragma unroll
      for (int q = 0; q < NT; ++q) acc[q] = LgVec<VEC>::zero();
      lgcn_walk<VEC, NT>(indices, col_scale, F, ldf, e0 + len * p / parts, e0 + len * (p + 1) / parts, cg, G, nch,
                         acc);
#pragma unroll
      for (int q = 0; q < NT; ++q)
        if (cg + G * q < nch) *(V *)(part + (int64_t)p * nch * VEC + (cg + G * q) * VEC) = acc[q];
    }
    uint64_t row_key = 0;
    if constexpr (NOISE) {                               // thread c squares column c (h <= 512 < the threads)
      row_key = gcl_row_key(nz.key, r);
      uint64_t ss = 0;
      for (int c = threadIdx.x; c < h; c += LG_LONG_THREADS) {
        const uint64_t mc = gcl_m(row_key, c);
        ss += mc * mc;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor((unsigned long long)ss, off, 64);
      if ((threadIdx.x & 63) == 0) lg_ss[threadIdx.x >> 6] = ss;
    }
    __syncthreads();
    float nscale = 0.f;
    if constexpr (NOISE) {
      uint64_t ss = 0;
#pragma unroll
      for (int w = 0; w < LG_LONG_THREADS / 64; ++w) ss += lg_ss[w];
      nscale = gcl_scale(ss, nz.eps);
    }
    const float rs = row_scale[r];
    for (int ch = threadIdx.x; ch < nch; ch += LG_LONG_THREADS) {
      V sum = *(const V *)(part + ch * VEC);
      for (int p = 1; p < parts; ++p) {
        const V t = *(const V *)(part + (int64_t)p * nch * VEC + ch * VEC);
#pragma unroll
        for (int i = 0; i < VEC; ++i) LgVec<VEC>::set(sum, i, LgVec<VEC>::get(sum, i) + LgVec<VEC>::get(t, i));
      }
      uint32_t m[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) m[i] = NOISE ? gcl_m(row_key, ch * VEC + i) : 0u;
      lgcn_finish<VEC, NOISE>(sum, rs, r, ch, Out, ldo, Acc, lda, acc_scale, m, nscale);
    }
    __syncthreads();                                     // (the next long row reuses the parts and the sums)
  }
}

// rk_als_bpr_apply's segment walk with another ending: G[key] = scale * sum, count[key] = the segment's
// length.  The weight is -g_t for a user's entry and for a positive, +g_t for a negative.
template <int NT>
__global__ __launch_bounds__(256) void als_lgcn_scatter_kernel(const int32_t *__restrict__ keys,
                                                               const int64_t *__restrict__ order, int n, int roles,
                                                               const float *__restrict__ g,
                                                               const float *__restrict__ V, int h, float scale,
                                                               int n_rows, float *__restrict__ Gt, int ldg,
                                                               int32_t *__restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int s0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s0 >= n) return;
  const int key = keys[s0];
  if (key < 0 || key >= n_rows) return;                  // (the invalid slots' sentinel, sorted last)
  if (s0 > 0 && keys[s0 - 1] == key) return;             // (not a head)
  int c = 0;
  for (;;) {                                             // the segment's length, 64 keys at a time
    const int s = s0 + c + lane;
    const bool same = s < n && keys[s] == key;
    const uint64_t m = __ballot(!same);
    if (m) {
      c += __ffsll((unsigned long long)m) - 1;
      break;
    }
    c += 64;
  }
  float acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = 0.f;
  const int64_t slots = roles == 2 ? n >> 1 : n;
  for (int a0 = 0; a0 < c; a0 += BPR_UNROLL) {
    float v[BPR_UNROLL][NT], w[BPR_UNROLL];
#pragma unroll
    for (int r = 0; r < BPR_UNROLL; ++r) {
      const bool in = a0 + r < c;
      const int64_t e = in ? order[s0 + a0 + r] : 0;
      const int64_t t = roles == 2 ? e >> 1 : e;
      const bool ok = in && e >= 0 && t < slots;         // (an order outside the batch adds nothing)
      const float gt = ok ? g[t] : 0.f;
      w[r] = (roles == 2 && (e & 1)) ? gt : -gt;
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const int k = lane + 64 * q;
        v[r][q] = (ok && k < h) ? V[t * h + k] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < BPR_UNROLL; ++r) {
      if (a0 + r < c) {
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[q] = fmaf(w[r], v[r][q], acc[q]);
      }
    }
  }
  float *row = Gt + (int64_t)key * ldg;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) row[k] = scale * acc[q];
  }
  if (lane == 0) count[key] = c;
}

// One thread per element.  grad = fmaf(reg_scale * count[row], e, H); m = fmaf(b1, m, (1 - b1) grad);
// v = fmaf(b2, v, ((1 - b2) grad) grad); e = fmaf(-step, m / fmaf(sqrt(v), isb2, eps), e), with
// step = lr / (1 - b1^t) and isb2 = 1 / sqrt(1 - b2^t) from the host (float64, rounded once).
__global__ __launch_bounds__(256) void als_lgcn_adam_kernel(float *__restrict__ E0, int lde,
                                                            const float *__restrict__ H, int ldh,
                                                            const int32_t *__restrict__ count, float reg_scale,
                                                            float *__restrict__ M, float *__restrict__ Vv,
                                                            int rows, int h, float beta1, float beta2,
                                                            float omb1, float omb2, float eps, float step,
                                                            float isb2) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // a wave per row and 64 columns
  const int k = blockIdx.y * 64 + (threadIdx.x & 63);
  if (r >= rows || k >= h) return;
  const int64_t x = r * h + k;
  const float e = E0[r * lde + k];
  const float grad = fmaf(reg_scale * (float)count[r], e, H[r * ldh + k]);
  const float m = fmaf(beta1, M[x], omb1 * grad);
  const float v = fmaf(beta2, Vv[x], (omb2 * grad) * grad);
  M[x] = m;
  Vv[x] = v;
  E0[r * lde + k] = fmaf(-step, m / fmaf(sqrtf(v), isb2, eps), e);
}

// ------------------------------------------------------------------------ gcl
// The contrast of SimGCL over the sorted keys of a step (rk_als_gcl_contrast).  Slot t is ACTIVE when its key lies
// in the table and differs from the key before it; nothing is compacted: an inactive slot holds zero rows
// and is masked out of every sum, so all sums run over ascending slots and the bits depend on the inputs
// alone.  With z = v / |v| (0 for |v| = 0) per active slot, S = Z1 Z2^T / tau and m active slots:
//   als_gcl_gather_kernel  a wave per slot: act, 1 / |v|, the rows of Z1 and Z2
//   als_gcl_gemm_kernel    64 x 64 (dZ: 16 x 64) tiles, k in steps of 16 through LDS, one fmaf chain per
//                          output over k ascending: S (SCORES), then dZ1 = (P Z2 - Z2) / (tau m)
//                          (P = exp(S - lse) formed as the tile is staged) and dZ2 = (P^T Z1 - Z1) / (tau m)
//   als_gcl_lse_kernel     a wave per row: the row's maximum, then lse = max + log sum exp(S - max)
//   als_gcl_loss_kernel    one workgroup: m and the loss (1 / m) sum (lse_r - S_rr)
//   als_gcl_write_kernel   a wave per active slot: dv = (dz - z (z . dz)) / |v| for both views, and
//                          G[key] += weight dv.  Active keys are distinct: plain stores, no atomics
constexpr int GCL_MAX_T = RK_ALS_GCL_MAX_BATCH;
constexpr int GCL_TILE = 64, GCL_DZ_ROWS = 16, GCL_KT = 16, GCL_LD = GCL_TILE + 4;

struct GclWs {
  float *Z1, *Z2, *dZ1, *dZ2, *S, *inv1, *inv2, *lse, *term;
  int32_t *act;
  float *scal = nullptr;                                 // (rk_als_dau_grad's two coefficients, past the layout below)
};

int64_t gcl_ws_floats(int64_t T, int64_t h, GclWs *w, float *base) {
  int64_t off = 0;
  auto cut = [&](int64_t n) {
    float *p = base ? base + off : nullptr;
    off += (n + 63) / 64 * 64;
    return p;
  };
  GclWs v;
  v.Z1 = cut(T * h), v.Z2 = cut(T * h), v.dZ1 = cut(T * h), v.dZ2 = cut(T * h), v.S = cut(T * T);
  v.inv1 = cut(T), v.inv2 = cut(T), v.lse = cut(T), v.term = cut(T);
  v.act = (int32_t *)cut(T);
  if (w) *w = v;
  return off;
}

template <int NT>
__global__ __launch_bounds__(256) void als_gcl_gather_kernel(const int32_t *__restrict__ keys, int T, int n_rows,
                                                             const float *__restrict__ V1, int ld1,
                                                             const float *__restrict__ V2, int ld2, int h,
                                                             GclWs w) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int key = keys[t];
  const bool act = key >= 0 && key < n_rows && (t == 0 || keys[t - 1] != key);       // (wave-uniform)
  float a[NT], b[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    a[q] = (act && k < h) ? V1[(int64_t)key * ld1 + k] : 0.f;
    b[q] = (act && k < h) ? V2[(int64_t)key * ld2 + k] : 0.f;
  }
  const float sa = wave_dot<NT>(a, a), sb = wave_dot<NT>(b, b);
  const float ia = sa > 0.f ? 1.f / sqrtf(sa) : 0.f, ib = sb > 0.f ? 1.f / sqrtf(sb) : 0.f;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) {
      w.Z1[(int64_t)t * h + k] = a[q] * ia;
      w.Z2[(int64_t)t * h + k] = b[q] * ib;
    }
  }
  if (lane == 0) {
    w.inv1[t] = ia;
    w.inv2[t] = ib;
    w.act[t] = act ? 1 : 0;
  }
}

// C [M, N] tile (blockIdx.y, blockIdx.x) = sum_k A[i, k] B[k, j], k < Kn ascending.
//   SCORES:  A = Z1 [T, h], B^T = Z2 [T, h] (B[k, j] = Z2[j, k]), C = S = sum / tau                M = N = T, Kn = h
//   DZ1:     A[i, k] = P[i, k], B = Z2 [T, h], C = dZ1 = (sum - Z2[i]) c                          M = Kn = T, N = h
//   DZ2:     A[i, k] = P[k, i], B = Z1 [T, h], C = dZ2 = (sum - Z1[i]) c
// P[r, s] = exp(S[r, s] - lse[r]) for active r and s, else 0; c = 1 / (tau m), m read from mcount.
// DirectAU's two products on one side's rows (rk_als_dau_grad below; the fields named 2 are the side's own, Z1 is
// the other side's Z):
//   DAU_SCORES:  A = B^T = Z2, C = S = E^ = exp(-2 (n_i + n_j - 2 sum)), 0 on the diagonal     M = N = T, Kn = h
//   DAU_DZ:      A = E^ as stored (symmetric: no expf), B = Z2, C = dZ2 = c1 (sum - r_i Z2[i]) + c2 (Z2[i] - Z1[i])
// n = |z|^2 taken as 1, or 0 for a zero row (inv2 == 0); r = lse holds the row sums of E^, (c1, c2) = scal.
enum { GCL_SCORES = 0, GCL_DZ1 = 1, GCL_DZ2 = 2, DAU_SCORES = 3, DAU_DZ = 4 };

// A tile is TM rows by 64 columns, TM / 16 x 4 outputs a thread: 64 rows for S, 16 for dZ, whose grid is only
// (h / 64) wide -- at T = 2048, h = 64 that is 128 workgroups, not 32.  The chains do not depend on TM.
template <int MODE, int TM>
__global__ __launch_bounds__(256) void als_gcl_gemm_kernel(int T, int h, float tau, const int32_t *__restrict__ mcount,
                                                           GclWs w) {
  constexpr int XR = TM / 16;                            // rows of a thread = A elements it stages per k-step
  __shared__ float As[GCL_KT][GCL_LD], Bs[GCL_KT][GCL_LD];
  constexpr bool SC = MODE == GCL_SCORES || MODE == DAU_SCORES;
  const int M = T, N = SC ? T : h, Kn = SC ? h : T;
  const int i0 = blockIdx.y * TM, j0 = blockIdx.x * GCL_TILE;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const float *Zb = MODE == GCL_DZ2 ? w.Z1 : w.Z2;
  float acc[XR][4];
#pragma unroll
  for (int a = 0; a < XR; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int k0 = 0; k0 < Kn; k0 += GCL_KT) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {                        // B: 16 x 64
      const int e = threadIdx.x + 256 * j;
      if (SC) {                                          // (row-major over k: 16 consecutive k of a row of Z2)
        const int row = e >> 4, kk = e & 15, k = k0 + kk;
        Bs[kk][row] = (j0 + row < N && k < Kn) ? w.Z2[(int64_t)(j0 + row) * h + k] : 0.f;
      } else {                                           // (64 consecutive columns of slot k)
        const int kk = e >> 6, col = e & 63, k = k0 + kk;
        Bs[kk][col] = (k < Kn && j0 + col < N) ? Zb[(int64_t)k * h + j0 + col] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < XR; ++j) {                       // A: 16 x TM
      const int e = threadIdx.x + 256 * j;
      if (SC) {
        const float *Za = MODE == DAU_SCORES ? w.Z2 : w.Z1;
        const int row = e >> 4, kk = e & 15, k = k0 + kk;
        As[kk][row] = (i0 + row < M && k < Kn) ? Za[(int64_t)(i0 + row) * h + k] : 0.f;
      } else if (MODE == DAU_DZ) {                       // (the weights as DAU_SCORES stored them)
        const int ai = e >> 4, ak = e & 15, r = i0 + ai, sl = k0 + ak;
        As[ak][ai] = (r < T && sl < T) ? w.S[(int64_t)r * T + sl] : 0.f;
      } else {                                           // consecutive lanes along S's rows (its columns s)
        const int ai = MODE == GCL_DZ1 ? e >> 4 : e % TM, ak = MODE == GCL_DZ1 ? e & 15 : e / TM;
        const int r = MODE == GCL_DZ1 ? i0 + ai : k0 + ak, sl = MODE == GCL_DZ1 ? k0 + ak : i0 + ai;
        const bool in = r < T && sl < T && w.act[r] && w.act[sl];
        As[ak][ai] = in ? expf(w.S[(int64_t)r * T + sl] - w.lse[r]) : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GCL_KT; ++kk) {
      const float4 b4 = *(const float4 *)&Bs[kk][tx * 4];
      const float b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int x = 0; x < XR; ++x) {
        const float a = As[kk][ty * XR + x];
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = fmaf(a, b[y], acc[x][y]);
      }
    }
    __syncthreads();
  }
  if (MODE == DAU_SCORES || MODE == DAU_DZ) {
    const float c1 = MODE == DAU_DZ ? w.scal[0] : 0.f, c2 = MODE == DAU_DZ ? w.scal[1] : 0.f;
#pragma unroll
    for (int x = 0; x < XR; ++x) {
      const int i = i0 + ty * XR + x;
      if (i >= M) continue;
      const float ni = w.inv2[i] > 0.f ? 1.f : 0.f, ri = w.lse[i];
      const bool oi = w.act[i] != 0;
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const int j = j0 + tx * 4 + y;
        if (j >= N) continue;
        if (MODE == DAU_SCORES) {
          const float nj = w.inv2[j] > 0.f ? 1.f : 0.f;
          const float d2 = fmaxf(fmaf(-2.f, acc[x][y], ni + nj), 0.f);
          w.S[(int64_t)i * T + j] = (oi && i != j && w.act[j]) ? expf(-2.f * d2) : 0.f;
        } else {
          const float z = Zb[(int64_t)i * h + j];
          w.dZ2[(int64_t)i * h + j] = fmaf(c1, fmaf(-ri, z, acc[x][y]), c2 * (z - w.Z1[(int64_t)i * h + j]));
        }
      }
    }
    return;
  }
  const float c = MODE == GCL_SCORES ? 1.f / tau : 1.f / (tau * (float)max(mcount[0], 1));
  float *C = MODE == GCL_SCORES ? w.S : MODE == GCL_DZ1 ? w.dZ1 : w.dZ2;
#pragma unroll
  for (int x = 0; x < XR; ++x) {
    const int i = i0 + ty * XR + x;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int j = j0 + tx * 4 + y;
      if (i < M && j < N)
        C[(int64_t)i * N + j] = MODE == GCL_SCORES ? acc[x][y] * c : (acc[x][y] - Zb[(int64_t)i * h + j]) * c;
    }
  }
}

// lane l owns the columns l, l + 64, ...: its maximum, then its chain of exp(S - max) from +0, each met by the
// xor butterfly; term = lse - S[r, r].  An inactive row: lse = term = 0.
__global__ __launch_bounds__(256) void als_gcl_lse_kernel(int T, GclWs w) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= T) return;
  if (!w.act[r]) {                                       // (wave-uniform)
    if (lane == 0) w.lse[r] = w.term[r] = 0.f;
    return;
  }
  const float *row = w.S + (int64_t)r * T;
  float mx = -INFINITY;
  for (int s = lane; s < T; s += 64)
    if (w.act[s]) mx = fmaxf(mx, row[s]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  float sum = 0.f;                                       // (mx is finite: column r itself is active)
  for (int s = lane; s < T; s += 64)
    if (w.act[s]) sum += expf(row[s] - mx);
  sum = wave_sum(sum);
  if (lane == 0) {
    const float lse = mx + logf(sum);
    w.lse[r] = lse;
    w.term[r] = lse - row[r];
  }
}

// thread t adds the slots t, t + 256, ... in ascending order, then the tree of als_objective_final_kernel
__global__ __launch_bounds__(256) void als_gcl_loss_kernel(int T, GclWs w, float *__restrict__ loss,
                                                           int32_t *__restrict__ mcount) {
  __shared__ float red[256];
  __shared__ int cnt[256];
  const int tid = threadIdx.x;
  float s = 0.f;
  int c = 0;
  for (int t = tid; t < T; t += 256) {
    s += w.term[t];
    c += w.act[t];
  }
  red[tid] = s;
  cnt[tid] = c;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[tid] += red[tid + off];
      cnt[tid] += cnt[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    mcount[0] = cnt[0];
    loss[0] = cnt[0] > 0 ? red[0] / (float)cnt[0] : 0.f;
  }
}

template <int NT>
__global__ __launch_bounds__(256) void als_gcl_write_kernel(const int32_t *__restrict__ keys, int T, int h,
                                                            float weight, GclWs w, float *G1, int ldg1, float *G2,
                                                            int ldg2) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T || !w.act[t]) return;                       // (wave-uniform)
  const int key = keys[t];
#pragma unroll
  for (int view = 0; view < 2; ++view) {                 // (view 1 after view 0: G1 and G2 may be one table)
    const float *Z = view ? w.Z2 : w.Z1, *dZ = view ? w.dZ2 : w.dZ1;
    const float inv = view ? w.inv2[t] : w.inv1[t];
    float *row = (view ? G2 + (int64_t)key * ldg2 : G1 + (int64_t)key * ldg1);
    float z[NT], d[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int k = lane + 64 * q;
      z[q] = k < h ? Z[(int64_t)t * h + k] : 0.f;
      d[q] = k < h ? dZ[(int64_t)t * h + k] : 0.f;
    }
    const float zd = wave_dot<NT>(z, d);
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int k = lane + 64 * q;
      if (k < h) row[k] += weight * (fmaf(-zd, z[q], d[q]) * inv);
    }
  }
}

// ------------------------------------------------------------------------ dau
// DirectAU's loss and gradient rows over the T slots of a step (rk_als_dau_grad).  Slot t is VALID when both ids
// lie in their tables; nothing is compacted or deduplicated: an invalid slot holds zero rows and zero weights.  The
// workspace is the contrast's (GclWs: Z1 / dZ1 / inv1 the users' side, Z2 / dZ2 / inv2 the items', S the T x T
// weights, lse their row sums, term the alignment terms, act the validity) and two coefficients after it.
//   als_dau_gather_kernel  a wave per slot: valid, 1 / |v| and z for both sides, |a - b|^2
//   als_gcl_gemm_kernel    DAU_SCORES (64 x 64 tiles), then DAU_DZ (16 x 64) on the stored weights, one side after
//                          the other on the one T x T tile, the items' side with Z1 / Z2 (dZ, inv) exchanged
//   als_dau_rowsum_kernel  a wave per row: r_p = sum_q e^_pq, lane l the columns l, l + 64, ... ascending
//   als_dau_loss_kernel    one workgroup: m, sum_p r_p = 2 E, the side's uniformity (and, with the users' side, the
//                          alignment and m), c1 = 2 gamma / E and c2 = 2 / m for the product
//   als_dau_write_kernel   a wave per slot: dv = (dz - z (z . dz)) / |v| for both sides into the slot's own rows
template <int NT>
__global__ __launch_bounds__(256) void als_dau_gather_kernel(const int32_t *__restrict__ users,
                                                             const int32_t *__restrict__ items, int T, int n_users,
                                                             int n_items, const float *__restrict__ X, int ldx,
                                                             const float *__restrict__ Y, int ldy, int h, GclWs w,
                                                             float *__restrict__ valid) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int u = users[t], i = items[t];
  const bool ok = u >= 0 && u < n_users && i >= 0 && i < n_items;                      // (wave-uniform)
  float a[NT], b[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    a[q] = (ok && k < h) ? X[(int64_t)u * ldx + k] : 0.f;
    b[q] = (ok && k < h) ? Y[(int64_t)i * ldy + k] : 0.f;
  }
  const float sa = wave_dot<NT>(a, a), sb = wave_dot<NT>(b, b);
  const float ia = sa > 0.f ? 1.f / sqrtf(sa) : 0.f, ib = sb > 0.f ? 1.f / sqrtf(sb) : 0.f;
  float d[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    a[q] *= ia;
    b[q] *= ib;
    d[q] = a[q] - b[q];
    if (k < h) {
      w.Z1[(int64_t)t * h + k] = a[q];
      w.Z2[(int64_t)t * h + k] = b[q];
    }
  }
  const float dd = wave_dot<NT>(d, d);
  if (lane == 0) {
    w.inv1[t] = ia;
    w.inv2[t] = ib;
    w.act[t] = ok ? 1 : 0;
    w.term[t] = dd;
    valid[t] = ok ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(256) void als_dau_rowsum_kernel(int T, GclWs w) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= T) return;
  const float *row = w.S + (int64_t)r * T;
  float sum = 0.f;
  for (int s = lane; s < T; s += 64) sum += row[s];
  sum = wave_sum(sum);
  if (lane == 0) w.lse[r] = sum;
}

// thread t adds the slots t, t + 256, ... in ascending order, then the tree of als_gcl_loss_kernel
template <bool USERS>
__global__ __launch_bounds__(256) void als_dau_loss_kernel(int T, float gamma, GclWs w, float *__restrict__ loss,
                                                           int32_t *__restrict__ mcount) {
  __shared__ float red[256], ali[256];
  __shared__ int cnt[256];
  const int tid = threadIdx.x;
  float s = 0.f, a = 0.f;
  int c = 0;
  for (int t = tid; t < T; t += 256) {
    s += w.lse[t];
    a += w.term[t];
    c += w.act[t];
  }
  red[tid] = s;
  ali[tid] = a;
  cnt[tid] = c;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[tid] += red[tid + off];
      ali[tid] += ali[tid + off];
      cnt[tid] += cnt[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float m = (float)cnt[0];                       // (m (m - 1) < 2^24: exact)
    const bool pairs = cnt[0] >= 2 && red[0] > 0.f;
    loss[USERS ? 1 : 2] = pairs ? logf(red[0] / (m * (m - 1.f))) : 0.f;
    w.scal[0] = pairs ? 4.f * gamma / red[0] : 0.f;
    w.scal[1] = cnt[0] > 0 ? 2.f / m : 0.f;
    if (USERS) {
      loss[0] = cnt[0] > 0 ? ali[0] / m : 0.f;
      mcount[0] = cnt[0];
    }
  }
}

template <int NT>
__global__ __launch_bounds__(256) void als_dau_write_kernel(int T, int h, GclWs w, float *__restrict__ DU,
                                                            float *__restrict__ DI) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const float *Z = side ? w.Z2 : w.Z1, *dZ = side ? w.dZ2 : w.dZ1;
    const float inv = side ? w.inv2[t] : w.inv1[t];      // (0 for a zero row and for an invalid slot)
    float *row = (side ? DI : DU) + (int64_t)t * h;
    float z[NT], d[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int k = lane + 64 * q;
      z[q] = k < h ? Z[(int64_t)t * h + k] : 0.f;
      d[q] = k < h ? dZ[(int64_t)t * h + k] : 0.f;
    }
    const float zd = wave_dot<NT>(z, d);
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int k = lane + 64 * q;
      if (k < h) row[k] = fmaf(-zd, z[q], d[q]) * inv;
    }
  }
}

// ------------------------------------------------------------------------ ssm
// The sampled softmax over the T slots of a step and C = T + S candidate columns (rk_als_ssm_grad).  Column c < T
// is slot c's positive item, column T + n the n-th shared negative: item = bpr_draw(key, 0, n_items) with key a
// hash of (seed, step, n) whose low word carries the tag 0xC0000000 -- a sampler slot is below 2^24, SimGCL's noise
// has bit 31 alone of the top byte.  Slot t is VALID when both ids lie in their tables, column c < T when slot c is,
// a shared column always; entry (t, c) is LIVE when both are valid and not (c != t and cand[c] == items[t]).
// Nothing is compacted: a dead entry holds the weight 0.
//   als_ssm_gather_kernel  a wave per user row and per candidate row: valid, 1 / |v| and z (cosine) or v (dot), the
//                          column's item and its correction
//   als_ssm_count_kernel   one workgroup: m, the valid slots
//   als_ssm_scores_kernel  64 x 64 tiles of S [T, C] by four waves, each a 32 x 32 block on v_mfma_f32_32x32x2_f32,
//                          k ascending over h through LDS; s = fmaf(sum, 1 / tau, -corr) or -inf for a dead entry
//   als_ssm_row_kernel     a wave per row, lane l the columns l, l + 64, ... ascending: the maximum, e = expf(s - max)
//                          stored and summed (the one expf of an element), lse = max + logf(sum), then the row
//                          overwritten with W = (e / sum - [c == t]) / m
//   als_ssm_loss_kernel    one workgroup: the two means over the valid slots
//   als_ssm_dz_kernel      16 x 64 tiles by four waves, each a 16 x 16 block on v_mfma_f32_16x16x4_f32, the stored
//                          weights staged as they are: dA = W Zc (k over C ascending), dB = W^T Zu (k over T)
//   als_ssm_write_kernel   a wave per row: dz = d / tau, (cosine) dv = (dz - z (z . dz)) / |v|, into the row's slot
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SSM_MAX_T = RK_ALS_SSM_MAX_BATCH, SSM_MAX_S = RK_ALS_SSM_MAX_NEGATIVES;
constexpr uint32_t SSM_TAG = 0xC0000000u;
// LDS images, k-major.  Scores: a thread stages 16 consecutive k of a row, so that a half-wave writes k = 0..15 of
// two rows -- at a row length of 66 words those are the 32 banks (2 k + row) mod 32, each once; the MFMA reads 32
// consecutive words of one k.  dZ: the weights as [row][k] at 17 words (a half-wave reads 16 rows of two k), B as
// [k][64 columns] at 80 words: the two k of a half-wave's read lie 16 banks apart.
constexpr int SSM_KT = 16, SSM_LD = 66, SSM_DZ_ROWS = 16, SSM_LDA = 17, SSM_LDB = 80;

struct SsmWs {
  float *Zu, *Zc, *dA, *dB, *S, *invu, *invc, *corrc, *term, *prob;
  int32_t *actu, *actc;
};

int64_t ssm_ws_floats(int64_t T, int64_t C, int64_t h, SsmWs *w, float *base) {
  int64_t off = 0;
  auto cut = [&](int64_t n) {
    float *p = base ? base + off : nullptr;
    off += (n + 63) / 64 * 64;
    return p;
  };
  SsmWs v;
  v.Zu = cut(T * h), v.Zc = cut(C * h), v.dA = cut(T * h), v.dB = cut(C * h), v.S = cut(T * C);
  v.invu = cut(T), v.invc = cut(C), v.corrc = cut(C), v.term = cut(T), v.prob = cut(T);
  v.actu = (int32_t *)cut(T), v.actc = (int32_t *)cut(C);
  if (w) *w = v;
  return off;
}

template <int NT>
__global__ __launch_bounds__(256) void als_ssm_gather_kernel(const int32_t *__restrict__ users,
                                                             const int32_t *__restrict__ items, int T, int S,
                                                             int n_users, int n_items, uint64_t seed_key,
                                                             uint32_t step, const float *__restrict__ X, int ldx,
                                                             const float *__restrict__ Y, int ldy, int h, int cosine,
                                                             const float *__restrict__ corr, SsmWs w,
                                                             int32_t *__restrict__ cand, float *__restrict__ valid,
                                                             float *__restrict__ cvalid) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= 2 * T + S) return;
  const bool user = r < T;                                                             // (wave-uniform, as all below)
  const int c = r - T;
  int id;
  bool ok;
  if (user || c < T) {
    const int t = user ? r : c;
    const int u = users[t], i = items[t];
    ok = u >= 0 && u < n_users && i >= 0 && i < n_items;
    id = user ? u : i;
  } else {
    const uint64_t key = bpr_mix(seed_key ^ (((uint64_t)step << 32) | SSM_TAG | (uint32_t)(c - T)));
    id = (int)bpr_draw(key, 0, (uint32_t)n_items);
    ok = true;
  }
  const int64_t at = ok ? id : 0;
  const float *row = user ? X + at * ldx : Y + at * ldy;
  float a[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    a[q] = (ok && k < h) ? row[k] : 0.f;
  }
  float inv = ok ? 1.f : 0.f;
  if (cosine) {
    const float ss = wave_dot<NT>(a, a);
    inv = ss > 0.f ? 1.f / sqrtf(ss) : 0.f;
  }
  float *Z = user ? w.Zu + (int64_t)r * h : w.Zc + (int64_t)c * h;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) Z[k] = cosine ? a[q] * inv : a[q];
  }
  if (lane == 0) {
    if (user) {
      w.invu[r] = inv;
      w.actu[r] = ok ? 1 : 0;
      valid[r] = ok ? 1.f : 0.f;
    } else {
      w.invc[c] = inv;
      w.actc[c] = ok ? 1 : 0;
      w.corrc[c] = (corr && ok) ? corr[id] : 0.f;
      cvalid[c] = ok ? 1.f : 0.f;
      cand[c] = id;
    }
  }
}

// thread t counts the slots t, t + 256, ..., then the tree of als_gcl_loss_kernel (integers: any order would do)
__global__ __launch_bounds__(256) void als_ssm_count_kernel(int T, SsmWs w, int32_t *__restrict__ mcount) {
  __shared__ int cnt[256];
  const int tid = threadIdx.x;
  int c = 0;
  for (int t = tid; t < T; t += 256) c += w.actu[t];
  cnt[tid] = c;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) cnt[tid] += cnt[tid + off];
    __syncthreads();
  }
  if (tid == 0) mcount[0] = cnt[0];
}

// Wave (wm, wn) of the workgroup owns the 32 x 32 block at (32 wm, 32 wn) of the 64 x 64 tile.  Lane l holds
// A[m = l & 31][k = l >> 5] and B[k = l >> 5][n = l & 31]; rows past T or C and k past h are staged as 0 (a 0 * 0
// term leaves the chain's value as it is).  C/D map: column n = l & 31, row m = (q & 3) + 8 (q >> 2) + 4 (l >> 5).
__global__ __launch_bounds__(256) void als_ssm_scores_kernel(const int32_t *__restrict__ items,
                                                             const int32_t *__restrict__ cand, int T, int C, int h,
                                                             float inv_tau, SsmWs w) {
  __shared__ float As[SSM_KT][SSM_LD], Bs[SSM_KT][SSM_LD];
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wm = wv >> 1, wn = wv & 1, kh = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  for (int k0 = 0; k0 < h; k0 += SSM_KT) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = threadIdx.x + 256 * j;
      const int row = e >> 4, kk = e & 15, k = k0 + kk;
      As[kk][row] = (i0 + row < T && k < h) ? w.Zu[(int64_t)(i0 + row) * h + k] : 0.f;
      Bs[kk][row] = (j0 + row < C && k < h) ? w.Zc[(int64_t)(j0 + row) * h + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SSM_KT; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + kh][wm * 32 + (lane & 31)], Bs[kk + kh][wn * 32 + (lane & 31)],
                                                 acc, 0, 0, 0);
    __syncthreads();
  }
  const int j = j0 + wn * 32 + (lane & 31);
  if (j >= C) return;
  const bool cj = w.actc[j] != 0;
  const int item = cand[j];
  const float cr = w.corrc[j];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = i0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * kh;
    if (i >= T) continue;
    const bool live = cj && w.actu[i] != 0 && !(j != i && item == items[i]);
    w.S[(int64_t)i * C + j] = live ? fmaf(acc[q], inv_tau, -cr) : -INFINITY;
  }
}

// A valid row's own column is live, so its maximum is finite.  A lane reads back only what it wrote itself.
__global__ __launch_bounds__(256) void als_ssm_row_kernel(int T, int C, const int32_t *__restrict__ mcount, SsmWs w) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  float *row = w.S + (int64_t)t * C;
  if (!w.actu[t]) {                                      // (wave-uniform)
    for (int c = lane; c < C; c += 64) row[c] = 0.f;
    if (lane == 0) w.term[t] = w.prob[t] = 0.f;
    return;
  }
  const float stt = row[t];
  float mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, row[c]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float e = expf(row[c] - mx);                   // (a dead entry: expf(-inf) = 0)
    row[c] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  const float lse = mx + logf(sum), m = (float)mcount[0];
  for (int c = lane; c < C; c += 64) row[c] = (row[c] / sum - (c == t ? 1.f : 0.f)) / m;
  if (lane == 0) {
    w.term[t] = lse - stt;
    w.prob[t] = expf(stt - lse);
  }
}

// thread t adds the slots t, t + 256, ... in ascending order, then the tree of als_gcl_loss_kernel
__global__ __launch_bounds__(256) void als_ssm_loss_kernel(int T, SsmWs w, const int32_t *__restrict__ mcount,
                                                           float *__restrict__ loss) {
  __shared__ float red[256], prb[256];
  const int tid = threadIdx.x;
  float s = 0.f, p = 0.f;
  for (int t = tid; t < T; t += 256) {
    s += w.term[t];
    p += w.prob[t];
  }
  red[tid] = s;
  prb[tid] = p;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[tid] += red[tid + off];
      prb[tid] += prb[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int m = mcount[0];
    loss[0] = m > 0 ? red[0] / (float)m : 0.f;
    loss[1] = m > 0 ? prb[0] / (float)m : 0.f;
  }
}

// D [M, h] tile (blockIdx.y: 16 rows, blockIdx.x: 64 columns) = sum_k A[i, k] B[k, j], k < Kn ascending:
//   dA: A[i, k] = W[i, k], B = Zc, M = T, Kn = C;    dB (TRANS): A[i, k] = W[k, i], B = Zu, M = C, Kn = T.
// Wave w owns the columns 16 w .. 16 w + 15.  Lane l holds A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15];
// C/D map of the 16 x 16 forms: column n = l & 15, row m = 4 (l >> 4) + q.
template <bool TRANS>
__global__ __launch_bounds__(256) void als_ssm_dz_kernel(int T, int C, int h, SsmWs w) {
  __shared__ float As[SSM_DZ_ROWS][SSM_LDA], Bs[SSM_KT][SSM_LDB];
  const int M = TRANS ? C : T, Kn = TRANS ? T : C;
  const float *B = TRANS ? w.Zu : w.Zc;
  float *D = TRANS ? w.dB : w.dA;
  const int i0 = blockIdx.y * SSM_DZ_ROWS, j0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Kn; k0 += SSM_KT) {
    {                                                    // A: consecutive lanes along W's rows
      const int ai = TRANS ? threadIdx.x & 15 : threadIdx.x >> 4, ak = TRANS ? threadIdx.x >> 4 : threadIdx.x & 15;
      const int i = i0 + ai, k = k0 + ak;
      float v = 0.f;
      if (i < M && k < Kn) v = TRANS ? w.S[(int64_t)k * C + i] : w.S[(int64_t)i * C + k];
      As[ai][ak] = v;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {                        // B: 16 x 64, 64 consecutive columns of row k
      const int e = threadIdx.x + 256 * j;
      const int kk = e >> 6, col = e & 63, k = k0 + kk;
      Bs[kk][col] = (k < Kn && j0 + col < h) ? B[(int64_t)k * h + j0 + col] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SSM_KT; kk += 4)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(As[lane & 15][kk + (lane >> 4)], Bs[kk + (lane >> 4)][wv * 16 + (lane & 15)],
                                                 acc, 0, 0, 0);
    __syncthreads();
  }
  const int col = j0 + wv * 16 + (lane & 15);
  if (col >= h) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = i0 + 4 * (lane >> 4) + q;
    if (i < M) D[(int64_t)i * h + col] = acc[q];
  }
}

template <int NT>
__global__ __launch_bounds__(256) void als_ssm_write_kernel(int T, int C, int h, float inv_tau, int cosine, SsmWs w,
                                                            float *__restrict__ DU, float *__restrict__ DC) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= T + C) return;
  const bool user = r < T;
  const int x = user ? r : r - T;
  const float *Z = (user ? w.Zu : w.Zc) + (int64_t)x * h, *dZ = (user ? w.dA : w.dB) + (int64_t)x * h;
  const float inv = user ? w.invu[x] : w.invc[x];        // (0 for an invalid row, and for a zero row of the cosine)
  float *out = (user ? DU : DC) + (int64_t)x * h;
  float z[NT], d[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    z[q] = k < h ? Z[k] : 0.f;
    d[q] = k < h ? dZ[k] * inv_tau : 0.f;
  }
  const float zd = cosine ? wave_dot<NT>(z, d) : 0.f;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) out[k] = inv > 0.f ? (cosine ? fmaf(-zd, z[q], d[q]) * inv : d[q]) : 0.f;
  }
}

// ----------------------------------------------------------------------- ugcn
// UltraGCN's constraint loss (rk_als_ugcn_grad): one wave per slot, p_u in registers.  The E = 1 + R + K candidates
// go 64 at a time: lane l prepares candidate e0 + l -- the positive, a draw (item = bpr_draw(key, 0, n_items), key a
// hash of (seed, step, t R + r) whose low word carries the tag 0xA0000000: a sampler slot is below 2^24, SimGCL's
// noise has the top byte 0x80, the sampled softmax's shared draws 0xC0) or a neighbour of the positive -- with its
// weight a and the sign of its logit.  The candidates are then scored UG_G rows of a lane group at a time, the row
// gathers issued before any is reduced.  At h <= 32 a group is W = 32 or 16 lanes and the wave's 64 / W groups
// score as many candidates side by side; at larger h the group is the wave.  A score goes back to the lane that
// owns the candidate, which forms coef = sign a sigma(sign s); the owners' coefs come back to the groups, and DU
// takes coef y in ascending e (fmaf at W = 64; the groups' products one after the other below that).  The loss
// terms are formed once per 64 candidates, a lane each, and summed per lane over the chunks, then by wave_sum.
constexpr int UG_MAX_T = RK_ALS_UGCN_MAX_BATCH, UG_MAX_R = RK_ALS_UGCN_MAX_NEGATIVES;
constexpr int UG_MAX_K = RK_ALS_UGCN_MAX_NEIGHBOURS, UG_MAX_ENTRIES = RK_ALS_UGCN_MAX_ENTRIES;
constexpr uint32_t UGCN_TAG = 0xA0000000u;
constexpr int UG_G = 4;
constexpr int UG_LONG = RK_ALS_UGCN_LONG_KEY, UG_LONG_WAVES = 16;

// sigma(x) and softplus(x) = max(x, 0) + log1p(exp(-|x|)) through e = exp(-|x|) <= 1, as als_bpr_grad_kernel
__device__ __forceinline__ float ug_sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
__device__ __forceinline__ float ug_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

template <int NT, int W>
__global__ __launch_bounds__(256) void als_ugcn_grad_kernel(
    const int32_t *__restrict__ users, const int32_t *__restrict__ items, int T, int R, int K, uint64_t seed_key,
    uint32_t step, int n_users, int n_items, const float *__restrict__ X, int ldx, const float *__restrict__ Y, int ldy,
    int h, const float *__restrict__ bu, const float *__restrict__ bi, const int32_t *__restrict__ nbr_ids,
    const float *__restrict__ nbr_w, float w1, float w2, float w3, float w4, float neg_scale, float item_weight,
    int32_t *__restrict__ cand, float *__restrict__ coef, float *__restrict__ DU, float *__restrict__ valid,
    float *__restrict__ loss) {
  static_assert(W == 64 || NT == 1, "lane groups below the wave hold one dimension a lane");
  constexpr int C = 64 / W;                       // candidates scored side by side
  constexpr int ROUND = C * UG_G;                 // candidates of one round of gathers (divides 64)
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int E = 1 + R + K;
  const int u = users[t], i = items[t];
  const bool ok = u >= 0 && u < n_users && i >= 0 && i < n_items;       // (wave-uniform)
  int32_t *crow = cand + (int64_t)t * E;
  float *frow = coef + (int64_t)t * E;
  const int sub = lane / W, kk = lane % W;
  if (!ok) {
    for (int e = lane; e < E; e += 64) {
      crow[e] = n_items;
      frow[e] = 0.f;
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int k = lane + 64 * q;
      if (k < h) DU[(int64_t)t * h + k] = 0.f;
    }
    if (lane == 0) valid[t] = 0.f;
    if (lane < 3) loss[(int64_t)t * 3 + lane] = 0.f;
    return;
  }
  float p[NT], du[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = kk + 64 * q;
    p[q] = k < h ? X[(int64_t)u * ldx + k] : 0.f;
    du[q] = 0.f;
  }
  const float bu_u = bu[u];
  const uint32_t draw0 = (uint32_t)t * (uint32_t)R;
  float lpos = 0.f, lneg = 0.f, lnbr = 0.f;
  for (int e0 = 0; e0 < E; e0 += 64) {
    const int e = e0 + lane;
    int id = n_items;                             // (n_items: no candidate here)
    float a = 0.f, sg = -1.f;
    if (e == 0) {
      id = i;
      a = fmaf(w2, bu_u * bi[i], w1);
    } else if (e <= R) {
      const uint64_t key = bpr_mix(seed_key ^ (((uint64_t)step << 32) | UGCN_TAG | (draw0 + (uint32_t)(e - 1))));
      id = (int)bpr_draw(key, 0, (uint32_t)n_items);
      a = neg_scale * fmaf(w4, bu_u * bi[id], w3);
      sg = 1.f;
    } else if (e < E) {
      const int64_t at = (int64_t)i * K + (e - R - 1);
      const int j = nbr_ids[at];
      if (j >= 0 && j < n_items) {
        id = j;
        a = item_weight * nbr_w[at];
      }
    }
    float ms = 0.f, mc = 0.f;                     // this lane's candidate: its score and its coef
    const int live = min(64, E - e0);
    for (int r0 = 0; r0 < live; r0 += ROUND) {
      int cg[UG_G];
      float y[UG_G][NT], s[UG_G];
#pragma unroll
      for (int g = 0; g < UG_G; ++g) cg[g] = __shfl(id, r0 + g * C + sub, 64);
#pragma unroll
      for (int g = 0; g < UG_G; ++g) {
#pragma unroll
        for (int q = 0; q < NT; ++q) {
          const int k = kk + 64 * q;
          y[g][q] = (cg[g] < n_items && k < h) ? Y[(int64_t)cg[g] * ldy + k] : 0.f;
        }
      }
#pragma unroll
      for (int g = 0; g < UG_G; ++g) {
        float d = 0.f;
#pragma unroll
        for (int q = 0; q < NT; ++q) d = fmaf(p[q], y[g][q], d);
#pragma unroll
        for (int off = W / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
        s[g] = d;
      }
#pragma unroll
      for (int g = 0; g < UG_G; ++g) {            // the score to the lane that owns the candidate
        const int first = r0 + g * C;
        const float v = __shfl(s[g], ((lane - first) & (C - 1)) * W, 64);
        if ((unsigned)(lane - first) < (unsigned)C) ms = v;
      }
      const float cf = id < n_items ? (sg * a) * ug_sigmoid(sg * ms) : 0.f;
      if ((unsigned)(lane - r0) < (unsigned)ROUND) mc = cf;
#pragma unroll
      for (int g = 0; g < UG_G; ++g) {
        const float cfg = __shfl(mc, r0 + g * C + sub, 64);
        if (C == 1) {
#pragma unroll
          for (int q = 0; q < NT; ++q) du[q] = fmaf(cfg, y[g][q], du[q]);
        } else {
          const float prod = cfg * y[g][0];
#pragma unroll
          for (int c = 0; c < C; ++c) du[0] += __shfl(prod, c * W + kk, 64);
        }
      }
    }
    if (e < E) {
      crow[e] = id;
      frow[e] = mc;
    }
    const float l = (e < E && id < n_items) ? a * ug_softplus(sg * ms) : 0.f;
    if (e == 0) lpos = l;
    else if (e <= R) lneg += l;
    else lnbr += l;
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = kk + 64 * q;
    if (sub == 0 && k < h) DU[(int64_t)t * h + k] = du[q];
  }
  const float sp = wave_sum(lpos), sn = wave_sum(lneg), sb = wave_sum(lnbr);
  if (lane == 0) {
    valid[t] = 1.f;
    loss[(int64_t)t * 3] = sp;
    loss[(int64_t)t * 3 + 1] = sn;
    loss[(int64_t)t * 3 + 2] = sb;
  }
}

// The item side (rk_als_ugcn_scatter).  acc_k = fmaf(coef[e], X[users[e / E], k], acc_k) over the sorted positions
// [s_lo, s_hi) from what acc holds, BPR_UNROLL user rows gathered before any is added; cnt counts the positives.
template <int NT>
__device__ __forceinline__ void ugcn_walk(const int64_t *__restrict__ order, int s_lo, int s_hi, int n, int E,
                                          const int32_t *__restrict__ users, int n_users,
                                          const float *__restrict__ coef, const float *__restrict__ X, int ldx, int h,
                                          int lane, float (&acc)[NT], int &cnt) {
  for (int a0 = s_lo; a0 < s_hi; a0 += BPR_UNROLL) {
    float v[BPR_UNROLL][NT], w[BPR_UNROLL];
#pragma unroll
    for (int r = 0; r < BPR_UNROLL; ++r) {
      const int64_t e = a0 + r < s_hi ? order[a0 + r] : -1;
      const bool in = e >= 0 && e < n;
      const uint32_t ee = in ? (uint32_t)e : 0u;
      const uint32_t tt = ee / (uint32_t)E;
      const int u = in ? users[tt] : -1;
      const bool ok = u >= 0 && u < n_users;
      w[r] = ok ? coef[ee] : 0.f;
      if (ok && ee == tt * (uint32_t)E) ++cnt;
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const int k = lane + 64 * q;
        v[r][q] = (ok && k < h) ? X[(int64_t)u * ldx + k] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < BPR_UNROLL; ++r) {
      if (a0 + r < s_hi) {
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[q] = fmaf(w[r], v[r][q], acc[q]);
      }
    }
  }
}

// als_lgcn_scatter_kernel's hand-out: one wave per sorted position, the wave at the head of a segment of equal keys
// owns that row.  A segment of UG_LONG entries or more is left to als_ugcn_scatter_long_kernel.
template <int NT>
__global__ __launch_bounds__(256) void als_ugcn_scatter_kernel(
    const int32_t *__restrict__ keys, const int64_t *__restrict__ order, int n, int E,
    const int32_t *__restrict__ users, const float *__restrict__ coef, const float *__restrict__ X, int ldx,
    int n_users, int h, float scale, int n_rows, float *__restrict__ Gt, int ldg, int32_t *__restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int s0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s0 >= n) return;
  const int key = keys[s0];
  if (key < 0 || key >= n_rows) return;                  // (absent and invalid entries, sorted last)
  if (s0 > 0 && keys[s0 - 1] == key) return;             // (not a head)
  int c = 0;
  for (;;) {                                             // the segment's length, 64 keys at a time
    const int s = s0 + c + lane;
    const bool same = s < n && keys[s] == key;
    const uint64_t m = __ballot(!same);
    if (m) {
      c += __ffsll((unsigned long long)m) - 1;
      break;
    }
    c += 64;
    if (c >= UG_LONG) return;                            // (a long key)
  }
  if (c >= UG_LONG) return;
  float acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = 0.f;
  int cnt = 0;
  ugcn_walk<NT>(order, s0, s0 + c, n, E, users, n_users, coef, X, ldx, h, lane, acc, cnt);
  float *row = Gt + (int64_t)key * ldg;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) row[k] = scale * acc[q];
  }
  if (lane == 0) count[key] = cnt;
}

// The long keys: a segment of c >= UG_LONG equal keys holds a position that is a multiple of UG_LONG; workgroup b
// looks at position b UG_LONG, finds the ends of its segment in the sorted keys and takes the segment when that
// position is the first such multiple in it.  Wave w sums part w of UG_LONG_WAVES equal parts (the last may be
// shorter or empty) as one chain; thread k adds the parts' sums in ascending w.
template <int NT>
__global__ __launch_bounds__(64 * UG_LONG_WAVES) void als_ugcn_scatter_long_kernel(
    const int32_t *__restrict__ keys, const int64_t *__restrict__ order, int n, int E,
    const int32_t *__restrict__ users, const float *__restrict__ coef, const float *__restrict__ X, int ldx,
    int n_users, int h, float scale, int n_rows, float *__restrict__ Gt, int ldg, int32_t *__restrict__ count) {
  __shared__ float red[UG_LONG_WAVES][64 * NT];
  __shared__ int cnts[UG_LONG_WAVES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int at = blockIdx.x * UG_LONG;
  if (at >= n) return;                                   // (workgroup-uniform, as every return below)
  const int key = keys[at];
  if (key < 0 || key >= n_rows) return;
  int lo = 0, hi = at;                                   // the first position with keys[.] >= key, in [0, at]
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  const int s_lo = lo;
  if (at - s_lo >= UG_LONG) return;                      // (an earlier workgroup's)
  lo = at + 1, hi = n;                                   // the first position with keys[.] > key, in (at, n]
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] <= key) lo = mid + 1; else hi = mid;
  }
  const int s_hi = lo, c = s_hi - s_lo;
  if (c < UG_LONG) return;
  const int part = (c + UG_LONG_WAVES - 1) / UG_LONG_WAVES;
  float acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = 0.f;
  int cnt = 0;
  ugcn_walk<NT>(order, min(s_lo + wv * part, s_hi), min(s_lo + (wv + 1) * part, s_hi), n, E, users, n_users, coef, X,
                ldx, h, lane, acc, cnt);
#pragma unroll
  for (int q = 0; q < NT; ++q) red[wv][lane + 64 * q] = acc[q];
  if (lane == 0) cnts[wv] = cnt;
  __syncthreads();
  const int k = threadIdx.x;
  if (k < h) {
    float s = red[0][k];
    for (int w = 1; w < UG_LONG_WAVES; ++w) s += red[w][k];
    Gt[(int64_t)key * ldg + k] = scale * s;
  }
  if (k == 0) {
    int total = 0;
    for (int w = 0; w < UG_LONG_WAVES; ++w) total += cnts[w];
    count[key] = total;
  }
}

int64_t bpr_round256(int64_t x) { return (x + 255) / 256 * 256; }
constexpr int BPR_MAX_T = 1 << 24;

int nt_of(int h) { return h <= 64 ? 1 : h <= 128 ? 2 : h <= 256 ? 4 : 8; }

}  // namespace

extern "C" int rk_als_version(void) { return 100; }
extern "C" const char *rk_als_last_error(void) { return g_rk_side_err; }
extern "C" int rk_als_max_h(void) { return MAX_H; }

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

#define ALS_SOLVE_LAUNCH(NT)                                                                                  \
  do {                                                                                                        \
    hipLaunchKernelGGL(als_solve_long_kernel<NT>, dim3((unsigned)(row_hi - row_lo)), dim3(64 * LONG_WAVES), 0, \
                       st, indptr, indices, data, row_lo, F, ldf, h, G, v, col_bias, row_bias, alpha, cg_steps,  \
                       X, ldx);                                                                               \
    if (g_lds)                                                                                                \
      hipLaunchKernelGGL((als_solve_kernel<NT, true>), grid, dim3(256), lds, st, indptr, indices, data, row_lo, \
                         row_hi, F, ldf, h, G, v, col_bias, row_bias, alpha, cg_steps, X, ldx, stash_rows);   \
    else                                                                                                      \
      hipLaunchKernelGGL((als_solve_kernel<NT, false>), grid, dim3(256), lds, st, indptr, indices, data,       \
                         row_lo, row_hi, F, ldf, h, G, v, col_bias, row_bias, alpha, cg_steps, X, ldx,         \
                         stash_rows);                                                                         \
  } while (0)

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
  switch (nt_of(h)) {
    case 1: ALS_SOLVE_LAUNCH(1); break;
    case 2: ALS_SOLVE_LAUNCH(2); break;
    case 4: ALS_SOLVE_LAUNCH(4); break;
    default: ALS_SOLVE_LAUNCH(8); break;
  }
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
    switch (nt_of(h)) {
      case 1: hipLaunchKernelGGL(als_objective_rows_kernel<1>, grid, dim3(256), 0, st, indptr, indices, data, rows, X, ldx, Y, ldy, h, bias, alpha, part); break;
      case 2: hipLaunchKernelGGL(als_objective_rows_kernel<2>, grid, dim3(256), 0, st, indptr, indices, data, rows, X, ldx, Y, ldy, h, bias, alpha, part); break;
      case 4: hipLaunchKernelGGL(als_objective_rows_kernel<4>, grid, dim3(256), 0, st, indptr, indices, data, rows, X, ldx, Y, ldy, h, bias, alpha, part); break;
      default: hipLaunchKernelGGL(als_objective_rows_kernel<8>, grid, dim3(256), 0, st, indptr, indices, data, rows, X, ldx, Y, ldy, h, bias, alpha, part); break;
    }
    RK_SIDE_CHECK_LAUNCH("als_objective_rows");
  }
  hipLaunchKernelGGL(als_objective_final_kernel, dim3(1), dim3(256), 0, st, part, rows, cols, h, bias, reg, Gx, Gy,
                     sx, cy, out);
  RK_SIDE_CHECK_LAUNCH("als_objective_final");
  return 0;
}

extern "C" int64_t rk_als_bpr_workspace_bytes(int32_t T, int32_t h) {
  if (T < 1 || T > BPR_MAX_T || h < 1 || h > MAX_H) return -2;
  return 5 * bpr_round256((int64_t)T * 4) + 2 * bpr_round256((int64_t)T * h * 4);
}

extern "C" int rk_als_bpr_sample(const int64_t *indptr, const int32_t *indices, int32_t n_users, int32_t n_items,
                                 int64_t nnz, int64_t seed, int32_t step, int32_t T, int32_t *users, int32_t *pos,
                                 int32_t *neg, void *stream) {
  RK_SIDE_REQUIRE(n_users >= 1 && n_items >= 1, "n_users >= 1, n_items >= 1");
  RK_SIDE_REQUIRE(nnz >= 1 && nnz < ((int64_t)1 << 31), "1 <= nnz < 2^31");
  RK_SIDE_REQUIRE(step >= 0 && T >= 1 && T <= BPR_MAX_T, "step >= 0, 1 <= T <= 2^24");
  RK_SIDE_REQUIRE(indptr && indices && users && pos && neg, "null pointer");
  hipLaunchKernelGGL(als_bpr_sample_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     indptr, indices, n_users, n_items, (uint32_t)nnz, bpr_mix((uint64_t)seed), (uint32_t)step, T,
                     users, pos, neg);
  RK_SIDE_CHECK_LAUNCH("als_bpr_sample");
  return 0;
}

#define ALS_BPR_GRAD_LAUNCH(NT)                                                                                   \
  hipLaunchKernelGGL(als_bpr_grad_kernel<NT>, grid, dim3(256), 0, st, users, pos, neg, T, n_users, n_items, X, ldx, \
                     Y, ldy, bias, h, g, loss, x, D, P)

extern "C" int rk_als_bpr_grad(const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t T,
                               int32_t n_users, int32_t n_items, const float *X, int32_t ldx, const float *Y,
                               int32_t ldy, const float *bias, int32_t h, float *g, float *loss, float *x, float *D,
                               float *P, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldx >= h && ldy >= h, "1 <= h <= 512, ldx >= h, ldy >= h");
  RK_SIDE_REQUIRE(T >= 1 && T <= BPR_MAX_T && n_users >= 1 && n_items >= 1, "1 <= T <= 2^24, n_users, n_items >= 1");
  RK_SIDE_REQUIRE(users && pos && neg && X && Y && bias && g && loss && D && P, "null pointer");
  const dim3 grid((unsigned)((T + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  switch (nt_of(h)) {
    case 1: ALS_BPR_GRAD_LAUNCH(1); break;
    case 2: ALS_BPR_GRAD_LAUNCH(2); break;
    case 4: ALS_BPR_GRAD_LAUNCH(4); break;
    default: ALS_BPR_GRAD_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_bpr_grad");
  return 0;
}

#define ALS_BPR_APPLY_LAUNCH(NT)                                                                                 \
  hipLaunchKernelGGL(als_bpr_apply_kernel<NT>, grid, dim3(256), 0, st, keys, order, n, roles, g, V, h, lr, reg,  \
                     n_rows, table, ldt, bias)

extern "C" int rk_als_bpr_apply(const int32_t *keys, const int64_t *order, int32_t n, int32_t roles, const float *g,
                                const float *V, int32_t h, float lr, float reg, int32_t n_rows, float *table,
                                int32_t ldt, float *bias, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldt >= h, "1 <= h <= 512, ldt >= h");
  RK_SIDE_REQUIRE(roles == 1 || roles == 2, "roles is 1 (users) or 2 (items: positive, negative)");
  RK_SIDE_REQUIRE(n >= roles && n % roles == 0 && n / roles <= BPR_MAX_T, "n = roles * T, 1 <= T <= 2^24");
  RK_SIDE_REQUIRE(n_rows >= 1, "n_rows >= 1");
  RK_SIDE_REQUIRE(keys && order && g && V && table, "null pointer");
  const dim3 grid((unsigned)((n + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  switch (nt_of(h)) {
    case 1: ALS_BPR_APPLY_LAUNCH(1); break;
    case 2: ALS_BPR_APPLY_LAUNCH(2); break;
    case 4: ALS_BPR_APPLY_LAUNCH(4); break;
    default: ALS_BPR_APPLY_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_bpr_apply");
  return 0;
}

// (G: the candidates whose rows are in flight together; 8 rows of h <= 128, 4 of the wider ones)
#define ALS_RANK_SAMPLE_LAUNCH(NT, G)                                                                            \
  hipLaunchKernelGGL((als_rank_sample_kernel<NT, G>), grid, dim3(256), 0, st, indptr, indices, n_users, n_items, \
                     (uint32_t)nnz, bpr_mix((uint64_t)seed), (uint32_t)step, T, X, ldx, Y, ldy, bias, h, mode,   \
                     max_draws, num_candidates, margin, users, pos, neg, trials, s_pos, s_neg, scores)

extern "C" int rk_als_rank_sample(const int64_t *indptr, const int32_t *indices, int32_t n_users, int32_t n_items,
                                  int64_t nnz, int64_t seed, int32_t step, int32_t T, const float *X, int32_t ldx,
                                  const float *Y, int32_t ldy, const float *bias, int32_t h, int32_t mode,
                                  int32_t max_draws, int32_t num_candidates, float margin, int32_t *users,
                                  int32_t *pos, int32_t *neg, int32_t *trials, float *s_pos, float *s_neg,
                                  float *scores, void *stream) {
  RK_SIDE_REQUIRE(n_users >= 1 && n_items >= 1, "n_users >= 1, n_items >= 1");
  RK_SIDE_REQUIRE(nnz >= 1 && nnz < ((int64_t)1 << 31), "1 <= nnz < 2^31");
  RK_SIDE_REQUIRE(step >= 0 && T >= 1 && T <= BPR_MAX_T, "step >= 0, 1 <= T <= 2^24");
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldx >= h && ldy >= h, "1 <= h <= 512, ldx >= h, ldy >= h");
  RK_SIDE_REQUIRE(mode == RANK_WARP || mode == RANK_DNS, "mode is RK_ALS_RANK_WARP or RK_ALS_RANK_DNS");
  RK_SIDE_REQUIRE(max_draws >= 1 && max_draws <= RANK_MAX_DRAWS, "1 <= max_draws <= 256");
  RK_SIDE_REQUIRE(mode != RANK_DNS || (num_candidates >= 1 && num_candidates <= max_draws),
                  "1 <= num_candidates <= max_draws");
  RK_SIDE_REQUIRE(mode != RANK_WARP || (margin >= 0.f && margin <= FLT_MAX), "margin must be finite and >= 0");
  RK_SIDE_REQUIRE(indptr && indices && X && Y && bias && users && pos && neg && trials, "null pointer");
  const dim3 grid((unsigned)((T + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  switch (nt_of(h)) {
    case 1: ALS_RANK_SAMPLE_LAUNCH(1, 8); break;
    case 2: ALS_RANK_SAMPLE_LAUNCH(2, 8); break;
    case 4: ALS_RANK_SAMPLE_LAUNCH(4, 4); break;
    default: ALS_RANK_SAMPLE_LAUNCH(8, 4); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_rank_sample");
  return 0;
}

#define ALS_WARP_GRAD_LAUNCH(NT)                                                                                  \
  hipLaunchKernelGGL(als_warp_grad_kernel<NT>, grid, dim3(256), 0, st, users, pos, neg, trials, T, n_users, n_items, \
                     X, ldx, Y, ldy, bias, h, margin, weight, g, loss, D, P)

extern "C" int rk_als_warp_grad(const int32_t *users, const int32_t *pos, const int32_t *neg, const int32_t *trials,
                                int32_t T, int32_t n_users, int32_t n_items, const float *X, int32_t ldx,
                                const float *Y, int32_t ldy, const float *bias, int32_t h, float margin,
                                const float *weight, float *g, float *loss, float *D, float *P, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldx >= h && ldy >= h, "1 <= h <= 512, ldx >= h, ldy >= h");
  RK_SIDE_REQUIRE(T >= 1 && T <= BPR_MAX_T && n_users >= 1 && n_items >= 1, "1 <= T <= 2^24, n_users, n_items >= 1");
  RK_SIDE_REQUIRE(margin >= 0.f && margin <= FLT_MAX, "margin must be finite and >= 0");
  RK_SIDE_REQUIRE(users && pos && neg && trials && X && Y && bias && weight && g && loss && D && P, "null pointer");
  const dim3 grid((unsigned)((T + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  switch (nt_of(h)) {
    case 1: ALS_WARP_GRAD_LAUNCH(1); break;
    case 2: ALS_WARP_GRAD_LAUNCH(2); break;
    case 4: ALS_WARP_GRAD_LAUNCH(4); break;
    default: ALS_WARP_GRAD_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_warp_grad");
  return 0;
}

#define ALS_LGCN_PROP_LAUNCH(VEC, NT)                                                                         \
  do {                                                                                                         \
    hipLaunchKernelGGL((als_lgcn_propagate_kernel<VEC, NT, NOISE>), grid, dim3(256), 0, st, indptr, indices,   \
                       row_scale, col_scale, row_lo, row_hi, F, ldf, h, G, Out, ldo, Acc, lda, acc_scale, nz); \
    hipLaunchKernelGGL((als_lgcn_propagate_long_kernel<VEC, NT, NOISE>), long_grid, dim3(LG_LONG_THREADS), lds, \
                       st, indptr, indices, row_scale, col_scale, row_lo, row_hi, F, ldf, h, G, Out, ldo, Acc, \
                       lda, acc_scale, nz);                                                                    \
  } while (0)

// the row pass of rk_als_lgcn_propagate (NOISE false) and rk_als_gcl_propagate (true): both launches
template <bool NOISE>
void lgcn_propagate_launch(const int64_t *indptr, const int32_t *indices, const float *row_scale,
                           const float *col_scale, int32_t row_lo, int32_t row_hi, const float *F, int32_t ldf,
                           int32_t h, float *Out, int32_t ldo, float *Acc, int32_t lda, float acc_scale, GclNoise nz,
                           hipStream_t st) {
  // 16-byte accesses when every row of every matrix starts on a 16-byte boundary and holds whole float4s
  const bool vec = h % 4 == 0 && ldf % 4 == 0 && (uintptr_t)F % 16 == 0 &&
                   (!Out || (ldo % 4 == 0 && (uintptr_t)Out % 16 == 0)) &&
                   (!Acc || (lda % 4 == 0 && (uintptr_t)Acc % 16 == 0));
  const int nch = vec ? h / 4 : h;
  int G = 1;
  while (G < 64 && G < nch) G *= 2;
  const int nt = (nch + G - 1) / G;                      // (vec: 1..2; scalar: 1..8)
  const int rpb = 256 / G;
  const dim3 grid((unsigned)(((int64_t)row_hi - row_lo + rpb - 1) / rpb));
  const dim3 long_grid((unsigned)std::min<int64_t>((int64_t)row_hi - row_lo, LG_LONG_GRID));
  const size_t lds = (size_t)lg_parts(h) * h * sizeof(float);
  if (vec) {
    if (nt == 1) ALS_LGCN_PROP_LAUNCH(4, 1);
    else ALS_LGCN_PROP_LAUNCH(4, 2);
  } else {
    switch (nt_of(h)) {
      case 1: ALS_LGCN_PROP_LAUNCH(1, 1); break;
      case 2: ALS_LGCN_PROP_LAUNCH(1, 2); break;
      case 4: ALS_LGCN_PROP_LAUNCH(1, 4); break;
      default: ALS_LGCN_PROP_LAUNCH(1, 8); break;
    }
  }
}

extern "C" int rk_als_lgcn_propagate(const int64_t *indptr, const int32_t *indices, const float *row_scale,
                                     const float *col_scale, int32_t row_lo, int32_t row_hi, const float *F,
                                     int32_t ldf, int32_t h, float *Out, int32_t ldo, float *Acc, int32_t lda,
                                     float acc_scale, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldf >= h, "1 <= h <= 512, ldf >= h");
  RK_SIDE_REQUIRE(row_lo >= 0 && row_hi >= row_lo, "0 <= row_lo <= row_hi");
  RK_SIDE_REQUIRE(Out || Acc, "at least one of Out / Acc must be set");
  RK_SIDE_REQUIRE((!Out || ldo >= h) && (!Acc || lda >= h), "ldo >= h, lda >= h");
  if (row_hi == row_lo) return 0;
  RK_SIDE_REQUIRE(indptr && indices && row_scale && col_scale && F, "null pointer");
  lgcn_propagate_launch<false>(indptr, indices, row_scale, col_scale, row_lo, row_hi, F, ldf, h, Out, ldo, Acc, lda,
                               acc_scale, GclNoise{0, 0.f}, (hipStream_t)stream);
  RK_SIDE_CHECK_LAUNCH("als_lgcn_propagate");
  return 0;
}

extern "C" int rk_als_gcl_propagate(const int64_t *indptr, const int32_t *indices, const float *row_scale,
                                    const float *col_scale, int32_t row_lo, int32_t row_hi, const float *F,
                                    int32_t ldf, int32_t h, float *Out, int32_t ldo, float *Acc, int32_t lda,
                                    float acc_scale, float eps, int64_t seed, int32_t step, int32_t view,
                                    int32_t layer, int32_t side, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldf >= h, "1 <= h <= 512, ldf >= h");
  RK_SIDE_REQUIRE(row_lo >= 0 && row_hi >= row_lo, "0 <= row_lo <= row_hi");
  RK_SIDE_REQUIRE(Out || Acc, "at least one of Out / Acc must be set");
  RK_SIDE_REQUIRE((!Out || ldo >= h) && (!Acc || lda >= h), "ldo >= h, lda >= h");
  RK_SIDE_REQUIRE(eps >= 0.f && eps < INFINITY, "eps must be finite and >= 0");
  RK_SIDE_REQUIRE(step >= 0 && view >= 0 && view <= 255 && layer >= 0 && layer <= 255 && (side == 0 || side == 1),
                  "step >= 0, view and layer in 0..255, side is 0 (users) or 1 (items)");
  if (row_hi == row_lo) return 0;
  RK_SIDE_REQUIRE(indptr && indices && row_scale && col_scale && F, "null pointer");
  lgcn_propagate_launch<true>(indptr, indices, row_scale, col_scale, row_lo, row_hi, F, ldf, h, Out, ldo, Acc, lda,
                              acc_scale, GclNoise{gcl_key(seed, step, view, layer, side), eps}, (hipStream_t)stream);
  RK_SIDE_CHECK_LAUNCH("als_gcl_propagate");
  return 0;
}

extern "C" int64_t rk_als_gcl_contrast_workspace_bytes(int32_t T, int32_t h) {
  if (T < 1 || T > GCL_MAX_T || h < 1 || h > MAX_H) return -2;
  return gcl_ws_floats(T, h, nullptr, nullptr) * (int64_t)sizeof(float);
}

#define ALS_GCL_GATHER_LAUNCH(NT) \
  hipLaunchKernelGGL(als_gcl_gather_kernel<NT>, waves, dim3(256), 0, st, keys, T, n_rows, V1, ld1, V2, ld2, h, w)
#define ALS_GCL_WRITE_LAUNCH(NT) \
  hipLaunchKernelGGL(als_gcl_write_kernel<NT>, waves, dim3(256), 0, st, keys, T, h, weight, w, G1, ldg1, G2, ldg2)

extern "C" int rk_als_gcl_contrast(const int32_t *keys, int32_t T, int32_t n_rows, const float *V1, int32_t ld1,
                                   const float *V2, int32_t ld2, int32_t h, float tau, float weight, float *G1,
                                   int32_t ldg1, float *G2, int32_t ldg2, void *ws, int64_t ws_bytes, float *loss,
                                   int32_t *count, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ld1 >= h && ld2 >= h && ldg1 >= h && ldg2 >= h,
                  "1 <= h <= 512, ld1, ld2, ldg1, ldg2 >= h");
  RK_SIDE_REQUIRE(T >= 1 && T <= GCL_MAX_T && n_rows >= 1, "1 <= T <= 4096, n_rows >= 1");
  RK_SIDE_REQUIRE(tau > 0.f && tau < INFINITY && weight >= 0.f && weight < INFINITY,
                  "tau must be finite and > 0, weight finite and >= 0");
  RK_SIDE_REQUIRE(ws && ws_bytes >= rk_als_gcl_contrast_workspace_bytes(T, h), "workspace too small");
  RK_SIDE_REQUIRE((uintptr_t)ws % 16 == 0, "the workspace must start on a 16-byte boundary");
  RK_SIDE_REQUIRE(keys && V1 && V2 && G1 && G2 && loss && count, "null pointer");
  GclWs w;
  gcl_ws_floats(T, h, &w, (float *)ws);
  hipStream_t st = (hipStream_t)stream;
  const dim3 waves((unsigned)((T + 3) / 4));
  const unsigned tt = (unsigned)((T + GCL_TILE - 1) / GCL_TILE), th = (unsigned)((h + GCL_TILE - 1) / GCL_TILE);
  const unsigned td = (unsigned)((T + GCL_DZ_ROWS - 1) / GCL_DZ_ROWS);
  switch (nt_of(h)) {
    case 1: ALS_GCL_GATHER_LAUNCH(1); break;
    case 2: ALS_GCL_GATHER_LAUNCH(2); break;
    case 4: ALS_GCL_GATHER_LAUNCH(4); break;
    default: ALS_GCL_GATHER_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_gcl_gather");
  hipLaunchKernelGGL((als_gcl_gemm_kernel<GCL_SCORES, GCL_TILE>), dim3(tt, tt), dim3(256), 0, st, T, h, tau, count, w);
  hipLaunchKernelGGL(als_gcl_lse_kernel, waves, dim3(256), 0, st, T, w);
  hipLaunchKernelGGL(als_gcl_loss_kernel, dim3(1), dim3(256), 0, st, T, w, loss, count);
  hipLaunchKernelGGL((als_gcl_gemm_kernel<GCL_DZ1, GCL_DZ_ROWS>), dim3(th, td), dim3(256), 0, st, T, h, tau, count, w);
  hipLaunchKernelGGL((als_gcl_gemm_kernel<GCL_DZ2, GCL_DZ_ROWS>), dim3(th, td), dim3(256), 0, st, T, h, tau, count, w);
  RK_SIDE_CHECK_LAUNCH("als_gcl_gemm");
  switch (nt_of(h)) {
    case 1: ALS_GCL_WRITE_LAUNCH(1); break;
    case 2: ALS_GCL_WRITE_LAUNCH(2); break;
    case 4: ALS_GCL_WRITE_LAUNCH(4); break;
    default: ALS_GCL_WRITE_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_gcl_write");
  return 0;
}

extern "C" int64_t rk_als_dau_workspace_bytes(int32_t T, int32_t h) {
  if (T < 1 || T > GCL_MAX_T || h < 1 || h > MAX_H) return -2;
  return (gcl_ws_floats(T, h, nullptr, nullptr) + 64) * (int64_t)sizeof(float);
}

#define ALS_DAU_GATHER_LAUNCH(NT)                                                                              \
  hipLaunchKernelGGL(als_dau_gather_kernel<NT>, waves, dim3(256), 0, st, users, items, T, n_users, n_items, X, \
                     ldx, Y, ldy, h, wu, valid)
#define ALS_DAU_WRITE_LAUNCH(NT) hipLaunchKernelGGL(als_dau_write_kernel<NT>, waves, dim3(256), 0, st, T, h, wu, DU, DI)

extern "C" int rk_als_dau_grad(const int32_t *users, const int32_t *items, int32_t T, int32_t n_users,
                               int32_t n_items, const float *X, int32_t ldx, const float *Y, int32_t ldy, int32_t h,
                               float gamma, void *ws, int64_t ws_bytes, float *DU, float *DI, float *valid,
                               float *loss, int32_t *count, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldx >= h && ldy >= h, "1 <= h <= 512, ldx, ldy >= h");
  RK_SIDE_REQUIRE(T >= 1 && T <= GCL_MAX_T && n_users >= 1 && n_items >= 1, "1 <= T <= 4096, n_users, n_items >= 1");
  RK_SIDE_REQUIRE(gamma >= 0.f && gamma < INFINITY, "gamma must be finite and >= 0");
  RK_SIDE_REQUIRE(ws && ws_bytes >= rk_als_dau_workspace_bytes(T, h), "workspace too small");
  RK_SIDE_REQUIRE((uintptr_t)ws % 16 == 0, "the workspace must start on a 16-byte boundary");
  RK_SIDE_REQUIRE(users && items && X && Y && DU && DI && valid && loss && count, "null pointer");
  GclWs wu;
  wu.scal = (float *)ws + gcl_ws_floats(T, h, &wu, (float *)ws);
  GclWs ex = wu;                                         // the users' side as the products' own: 1 and 2 exchanged
  ex.Z1 = wu.Z2, ex.Z2 = wu.Z1, ex.dZ1 = wu.dZ2, ex.dZ2 = wu.dZ1, ex.inv1 = wu.inv2, ex.inv2 = wu.inv1;
  hipStream_t st = (hipStream_t)stream;
  const dim3 waves((unsigned)((T + 3) / 4));
  const unsigned tt = (unsigned)((T + GCL_TILE - 1) / GCL_TILE), th = (unsigned)((h + GCL_TILE - 1) / GCL_TILE);
  const unsigned td = (unsigned)((T + GCL_DZ_ROWS - 1) / GCL_DZ_ROWS);
  switch (nt_of(h)) {
    case 1: ALS_DAU_GATHER_LAUNCH(1); break;
    case 2: ALS_DAU_GATHER_LAUNCH(2); break;
    case 4: ALS_DAU_GATHER_LAUNCH(4); break;
    default: ALS_DAU_GATHER_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_dau_gather");
  for (int side = 0; side < 2; ++side) {
    const GclWs &w = side ? wu : ex;
    hipLaunchKernelGGL((als_gcl_gemm_kernel<DAU_SCORES, GCL_TILE>), dim3(tt, tt), dim3(256), 0, st, T, h, gamma, nullptr, w);
    hipLaunchKernelGGL(als_dau_rowsum_kernel, waves, dim3(256), 0, st, T, w);
    if (side == 0)
      hipLaunchKernelGGL(als_dau_loss_kernel<true>, dim3(1), dim3(256), 0, st, T, gamma, w, loss, count);
    else
      hipLaunchKernelGGL(als_dau_loss_kernel<false>, dim3(1), dim3(256), 0, st, T, gamma, w, loss, count);
    hipLaunchKernelGGL((als_gcl_gemm_kernel<DAU_DZ, GCL_DZ_ROWS>), dim3(th, td), dim3(256), 0, st, T, h, gamma, nullptr, w);
    RK_SIDE_CHECK_LAUNCH("als_dau_side");
  }
  switch (nt_of(h)) {
    case 1: ALS_DAU_WRITE_LAUNCH(1); break;
    case 2: ALS_DAU_WRITE_LAUNCH(2); break;
    case 4: ALS_DAU_WRITE_LAUNCH(4); break;
    default: ALS_DAU_WRITE_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_dau_write");
  return 0;
}

extern "C" int64_t rk_als_ssm_workspace_bytes(int32_t T, int32_t S, int32_t h) {
  if (T < 1 || T > SSM_MAX_T || S < 0 || S > SSM_MAX_S || h < 1 || h > MAX_H) return -2;
  return ssm_ws_floats(T, (int64_t)T + S, h, nullptr, nullptr) * (int64_t)sizeof(float);
}

#define ALS_SSM_GATHER_LAUNCH(NT)                                                                                    \
  hipLaunchKernelGGL(als_ssm_gather_kernel<NT>, dim3((unsigned)((T + C + 3) / 4)), dim3(256), 0, st, users, items, T, \
                     S, n_users, n_items, bpr_mix((uint64_t)seed), (uint32_t)step, X, ldx, Y, ldy, h, cosine, corr, w, \
                     cand, valid, cvalid)
#define ALS_SSM_WRITE_LAUNCH(NT)                                                                                   \
  hipLaunchKernelGGL(als_ssm_write_kernel<NT>, dim3((unsigned)((T + C + 3) / 4)), dim3(256), 0, st, T, C, h, inv_tau, \
                     cosine, w, DU, DC)

extern "C" int rk_als_ssm_grad(const int32_t *users, const int32_t *items, int32_t T, int32_t S, int64_t seed,
                               int32_t step, int32_t n_users, int32_t n_items, const float *X, int32_t ldx,
                               const float *Y, int32_t ldy, int32_t h, float inv_tau, int32_t cosine, const float *corr,
                               void *ws, int64_t ws_bytes, int32_t *cand, float *DU, float *DC, float *valid,
                               float *cvalid, float *loss, int32_t *count, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldx >= h && ldy >= h, "1 <= h <= 512, ldx, ldy >= h");
  RK_SIDE_REQUIRE(T >= 1 && T <= SSM_MAX_T && S >= 0 && S <= SSM_MAX_S, "1 <= T <= 4096, 0 <= S <= 4096");
  RK_SIDE_REQUIRE(n_users >= 1 && n_items >= 1 && step >= 0, "n_users, n_items >= 1, step >= 0");
  RK_SIDE_REQUIRE(inv_tau > 0.f && inv_tau < INFINITY && (cosine == 0 || cosine == 1),
                  "inv_tau must be finite and > 0, cosine 0 or 1");
  RK_SIDE_REQUIRE(ws && ws_bytes >= rk_als_ssm_workspace_bytes(T, S, h), "workspace too small");
  RK_SIDE_REQUIRE((uintptr_t)ws % 16 == 0, "the workspace must start on a 16-byte boundary");
  RK_SIDE_REQUIRE(users && items && X && Y && cand && DU && DC && valid && cvalid && loss && count, "null pointer");
  const int C = T + S;
  SsmWs w;
  ssm_ws_floats(T, C, h, &w, (float *)ws);
  hipStream_t st = (hipStream_t)stream;
  const dim3 rows((unsigned)((T + 3) / 4));
  const unsigned th = (unsigned)((h + 63) / 64);
  switch (nt_of(h)) {
    case 1: ALS_SSM_GATHER_LAUNCH(1); break;
    case 2: ALS_SSM_GATHER_LAUNCH(2); break;
    case 4: ALS_SSM_GATHER_LAUNCH(4); break;
    default: ALS_SSM_GATHER_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_ssm_gather");
  hipLaunchKernelGGL(als_ssm_count_kernel, dim3(1), dim3(256), 0, st, T, w, count);
  hipLaunchKernelGGL(als_ssm_scores_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)((T + 63) / 64)), dim3(256), 0,
                     st, items, cand, T, C, h, inv_tau, w);
  RK_SIDE_CHECK_LAUNCH("als_ssm_scores");
  hipLaunchKernelGGL(als_ssm_row_kernel, rows, dim3(256), 0, st, T, C, count, w);
  hipLaunchKernelGGL(als_ssm_loss_kernel, dim3(1), dim3(256), 0, st, T, w, count, loss);
  RK_SIDE_CHECK_LAUNCH("als_ssm_row");
  hipLaunchKernelGGL(als_ssm_dz_kernel<false>, dim3(th, (unsigned)((T + SSM_DZ_ROWS - 1) / SSM_DZ_ROWS)), dim3(256), 0,
                     st, T, C, h, w);
  hipLaunchKernelGGL(als_ssm_dz_kernel<true>, dim3(th, (unsigned)((C + SSM_DZ_ROWS - 1) / SSM_DZ_ROWS)), dim3(256), 0,
                     st, T, C, h, w);
  RK_SIDE_CHECK_LAUNCH("als_ssm_dz");
  switch (nt_of(h)) {
    case 1: ALS_SSM_WRITE_LAUNCH(1); break;
    case 2: ALS_SSM_WRITE_LAUNCH(2); break;
    case 4: ALS_SSM_WRITE_LAUNCH(4); break;
    default: ALS_SSM_WRITE_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_ssm_write");
  return 0;
}

extern "C" int64_t rk_als_ugcn_workspace_bytes(int32_t T, int32_t R, int32_t K, int32_t h) {
  if (T < 1 || T > UG_MAX_T || R < 1 || R > UG_MAX_R || K < 0 || K > UG_MAX_K || h < 1 || h > MAX_H) return -2;
  const int64_t n = (int64_t)T * (1 + R + K);
  if (n > UG_MAX_ENTRIES) return -2;
  return 2 * bpr_round256(4 * n) + bpr_round256(4 * 3 * (int64_t)T);
}

#define ALS_UGCN_GRAD_LAUNCH(NT, W)                                                                                  \
  hipLaunchKernelGGL((als_ugcn_grad_kernel<NT, W>), dim3((unsigned)((T + 3) / 4)), dim3(256), 0, (hipStream_t)stream, \
                     users, items, T, R, K, bpr_mix((uint64_t)seed), (uint32_t)step, n_users, n_items, X, ldx, Y, ldy, \
                     h, bu, bi, nbr_ids, nbr_w, w1, w2, w3, w4, negative_weight / (float)R, item_weight, cand, coef,  \
                     DU, valid, loss)

extern "C" int rk_als_ugcn_grad(const int32_t *users, const int32_t *items, int32_t T, int32_t R, int32_t K,
                                int64_t seed, int32_t step, int32_t n_users, int32_t n_items, const float *X,
                                int32_t ldx, const float *Y, int32_t ldy, int32_t h, const float *bu, const float *bi,
                                const int32_t *nbr_ids, const float *nbr_w, float w1, float w2, float w3, float w4,
                                float negative_weight, float item_weight, int32_t *cand, float *coef, float *DU,
                                float *valid, float *loss, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldx >= h && ldy >= h, "1 <= h <= 512, ldx, ldy >= h");
  RK_SIDE_REQUIRE(rk_als_ugcn_workspace_bytes(T, R, K, h) > 0,
                  "1 <= T <= 4096, 1 <= R <= 1024, 0 <= K <= 64, T (1 + R + K) <= 2^22");
  RK_SIDE_REQUIRE(n_users >= 1 && n_items >= 1 && step >= 0, "n_users, n_items >= 1, step >= 0");
  RK_SIDE_REQUIRE(users && items && X && Y && bu && bi && cand && coef && DU && valid && loss, "null pointer");
  RK_SIDE_REQUIRE(K == 0 || (nbr_ids && nbr_w), "K > 0 needs the neighbour lists");
  if (h <= 16) ALS_UGCN_GRAD_LAUNCH(1, 16);
  else if (h <= 32) ALS_UGCN_GRAD_LAUNCH(1, 32);
  else if (h <= 64) ALS_UGCN_GRAD_LAUNCH(1, 64);
  else if (h <= 128) ALS_UGCN_GRAD_LAUNCH(2, 64);
  else if (h <= 256) ALS_UGCN_GRAD_LAUNCH(4, 64);
  else ALS_UGCN_GRAD_LAUNCH(8, 64);
  RK_SIDE_CHECK_LAUNCH("als_ugcn_grad");
  return 0;
}

#define ALS_UGCN_SCATTER_LAUNCH(NT)                                                                                 \
  do {                                                                                                              \
    hipLaunchKernelGGL(als_ugcn_scatter_kernel<NT>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, keys, order, n, E, \
                       users, coef, X, ldx, n_users, h, scale, n_rows, G, ldg, count);                              \
    hipLaunchKernelGGL(als_ugcn_scatter_long_kernel<NT>, dim3((unsigned)((n + UG_LONG - 1) / UG_LONG)),             \
                       dim3(64 * UG_LONG_WAVES), 0, st, keys, order, n, E, users, coef, X, ldx, n_users, h, scale,   \
                       n_rows, G, ldg, count);                                                                      \
  } while (0)

extern "C" int rk_als_ugcn_scatter(const int32_t *keys, const int64_t *order, int32_t n, int32_t E,
                                   const int32_t *users, const float *coef, const float *X, int32_t ldx,
                                   int32_t n_users, int32_t h, float scale, int32_t n_rows, float *G, int32_t ldg,
                                   int32_t *count, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldx >= h && ldg >= h, "1 <= h <= 512, ldx, ldg >= h");
  RK_SIDE_REQUIRE(E >= 2 && E <= 1 + UG_MAX_R + UG_MAX_K && n >= E && n % E == 0 && n / E <= UG_MAX_T &&
                      n <= UG_MAX_ENTRIES,
                  "n = T E, 2 <= E <= 1089, 1 <= T <= 4096, n <= 2^22");
  RK_SIDE_REQUIRE(n_users >= 1 && n_rows >= 1, "n_users, n_rows >= 1");
  RK_SIDE_REQUIRE(keys && order && users && coef && X && G && count, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  switch (nt_of(h)) {
    case 1: ALS_UGCN_SCATTER_LAUNCH(1); break;
    case 2: ALS_UGCN_SCATTER_LAUNCH(2); break;
    case 4: ALS_UGCN_SCATTER_LAUNCH(4); break;
    default: ALS_UGCN_SCATTER_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_ugcn_scatter");
  return 0;
}

#define ALS_LGCN_SCATTER_LAUNCH(NT)                                                                           \
  hipLaunchKernelGGL(als_lgcn_scatter_kernel<NT>, grid, dim3(256), 0, st, keys, order, n, roles, g, V, h, scale, \
                     n_rows, G, ldg, count)

extern "C" int rk_als_lgcn_scatter(const int32_t *keys, const int64_t *order, int32_t n, int32_t roles,
                                   const float *g, const float *V, int32_t h, float scale, int32_t n_rows, float *G,
                                   int32_t ldg, int32_t *count, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldg >= h, "1 <= h <= 512, ldg >= h");
  RK_SIDE_REQUIRE(roles == 1 || roles == 2, "roles is 1 (users) or 2 (items: positive, negative)");
  RK_SIDE_REQUIRE(n >= roles && n % roles == 0 && n / roles <= BPR_MAX_T, "n = roles * T, 1 <= T <= 2^24");
  RK_SIDE_REQUIRE(n_rows >= 1, "n_rows >= 1");
  RK_SIDE_REQUIRE(keys && order && g && V && G && count, "null pointer");
  const dim3 grid((unsigned)((n + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  switch (nt_of(h)) {
    case 1: ALS_LGCN_SCATTER_LAUNCH(1); break;
    case 2: ALS_LGCN_SCATTER_LAUNCH(2); break;
    case 4: ALS_LGCN_SCATTER_LAUNCH(4); break;
    default: ALS_LGCN_SCATTER_LAUNCH(8); break;
  }
  RK_SIDE_CHECK_LAUNCH("als_lgcn_scatter");
  return 0;
}

extern "C" int rk_als_lgcn_adam(float *E0, int32_t lde, const float *H, int32_t ldh, const int32_t *count,
                                float reg_scale, float *M, float *V, int32_t rows, int32_t h, float lr, float beta1,
                                float beta2, float eps, int32_t t, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && lde >= h && ldh >= h, "1 <= h <= 512, lde >= h, ldh >= h");
  RK_SIDE_REQUIRE(rows >= 0 && t >= 1, "rows >= 0, t >= 1");
  RK_SIDE_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f,
                  "0 <= beta1, beta2 < 1, eps > 0");
  if (rows == 0) return 0;
  RK_SIDE_REQUIRE(E0 && H && count && M && V, "null pointer");
  // the bias corrections in float64 from the float arguments, each rounded once
  const float step = (float)((double)lr / (1.0 - pow((double)beta1, (double)t)));
  const float isb2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)t)));
  const dim3 grid((unsigned)((rows + 3) / 4), (unsigned)((h + 63) / 64));
  hipLaunchKernelGGL(als_lgcn_adam_kernel, grid, dim3(256), 0, (hipStream_t)stream, E0, lde, H, ldh, count,
                     reg_scale, M, V, rows, h, beta1, beta2, 1.f - beta1, 1.f - beta2, eps, step, isb2);
  RK_SIDE_CHECK_LAUNCH("als_lgcn_adam");
  return 0;
}
