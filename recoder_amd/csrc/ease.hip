// EASE: the closed-form item-item autoencoder (include/recoder_ease.h, librecoder_ease.so).
//
//   rk_ease_gram         A = X^T X + reg I: one workgroup per (row i, column strip held in LDS); each of
//                        its 16 waves owns 1024 columns of the strip and walks the users of item i in
//                        order, adding x_ui * X[u, its columns]; the strip is written out once, coalesced
//   rk_ease_spd_inverse  blocked Gauss-Jordan, block width 64, four launches per block: the pivot block
//                        inverted in float64 in LDS, the row panel R = D^-1 A[k, :] and a transposed copy
//                        of the column panel, the rank-64 update on v_mfma_f32_32x32x2_f32 (128 x 128
//                        tiles, 2 x 2 accumulators of 32 x 32 per wave), the panels written back.  The
//                        update is compensated (a second n x n image holds what each in-place
//                        subtraction lost): an item few users touched has a diagonal of about reg + a few,
//                        every block's update of it is below half an ulp, and uncompensated they all vanish
//   rk_ease_finalize     B = -P / diag(P) by columns, diagonal 0
//   rk_ease_scores       sparse row x dense matrix, one thread per output column, users fastest in the grid
//   rk_ease_lowrank_add  A += diag(alpha a) V V^T diag(b): the inverse's 128 x 128 MFMA tile walked over k in
//                        slabs of 32, the whole k inside one wave (one chain per output, no atomics), the two
//                        scalings and the add in the store
//   rk_ease_gemm         D = alpha A B + beta E: the same tile over general row-major operands, the next k-slab
//                        fetched into registers under this slab's MFMAs, edges padded with zeros in LDS
//   rk_ease_admm_update  the element-wise pass of an ADMM-SLIM iteration (recoder_amd/admm.py): one workgroup per
//                        row, the row's three statistics summed in a fixed order
//   rk_ease_elsa_*, rk_ease_csr_sub   the row passes of the low-rank autoencoder ELSA (recoder_amd/elsa.py): ease/elsa.h
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/recoder_ease.h"
#include "side_error.h"
#include "side_explain.h"      // rk_ease_explain: the order, the selection and the one-wave kernel

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ----------------------------------------------------------------------- gram
constexpr int GR_WAVES = 16;
constexpr int GR_SUB = 1024;                  // columns a wave owns
constexpr int GR_STRIP = GR_WAVES * GR_SUB;   // 64 KB of LDS: two workgroups (32 waves) per CU

// A popular item has tens of thousands of users: its row is spread over 16 waves per strip (each
// on its own columns), and the (user, row start, row end) triples are fetched 64 at a time, so the
// walk pays one memory latency per user row, not three.
__global__ __launch_bounds__(GR_WAVES * 64) void ease_gram_kernel(
    const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_indices, const float *__restrict__ t_data,
    const int64_t *__restrict__ u_indptr, const int32_t *__restrict__ u_indices, const float *__restrict__ u_data,
    int n_users, int n, float reg, float *__restrict__ A, int64_t lda) {
  __shared__ float strip[GR_STRIP];
  const int i = blockIdx.x, lo = blockIdx.y * GR_STRIP;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wlo = lo + wv * GR_SUB, whi = min(n, wlo + GR_SUB);
  float *mine = strip + wv * GR_SUB;
  for (int c = lane; c < GR_SUB; c += 64) mine[c] = 0.f;
  if (wlo < n) {
    const int64_t e0 = t_indptr[i], e1 = t_indptr[i + 1];
    for (int64_t eb = e0; eb < e1; eb += 64) {
      const int cnt = e1 - eb < 64 ? (int)(e1 - eb) : 64;
      int64_t r0 = 0, r1 = 0;
      float xi = 0.f;
      if (lane < cnt) {
        const int u = t_indices[eb + lane];
        if (u >= 0 && u < n_users) {           // (a bad index reads nothing)
          r0 = u_indptr[u];
          r1 = u_indptr[u + 1];
        }
        xi = t_data ? t_data[eb + lane] : 1.f;
      }
      for (int l = 0; l < cnt; ++l) {
        const int64_t p0 = __shfl(r0, l, 64), p1 = __shfl(r1, l, 64);
        const float x = __shfl(xi, l, 64);
        for (int64_t p = p0; p < p1; p += 64) {       // (wave-uniform bounds)
          const int64_t q = p + lane;
          if (q < p1) {
            const int c = u_indices[q];
            if (c >= wlo && c < whi) {                 // columns of one user are distinct: no two lanes meet
              const float v = u_data ? u_data[q] : 1.f;
              mine[c - wlo] = fmaf(x, v, mine[c - wlo]);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  const int width = min(GR_STRIP, n - lo);
  float *row = A + (int64_t)i * lda + lo;
  for (int c = threadIdx.x; c < width; c += GR_WAVES * 64) {
    float v = strip[c];
    if (lo + c == i) v += reg;
    row[c] = v;
  }
}

// -------------------------------------------------------------------- inverse
constexpr int NB = 64;            // block width of the elimination
constexpr int TILE = 128;         // update tile (rows and columns) of one workgroup

inline int64_t inv_ldw(int n) { return ((int64_t)n + TILE - 1) / TILE * TILE; }

// Dv [64][64] (float64) <- (A[k0 .. k0+64)[k0 .. k0+64))^-1, unpivoted Gauss-Jordan in float64, in place in LDS;
// rows / columns past n are those of the identity.  A pivot that is not > 0 (or not finite) is
// reported once (the first wins) and replaced by 1.
__global__ __launch_bounds__(256) void ease_pivot_kernel(const float *__restrict__ A,
                                                         const float *__restrict__ Cc, int n, int64_t lda, int k0,
                                                         double *__restrict__ Dv, int *__restrict__ status) {
  __shared__ double D[NB][NB + 1];
  const int c = threadIdx.x & 63, rb = threadIdx.x >> 6;
  for (int q = 0; q < 16; ++q) {
    const int r = rb + 4 * q, gi = k0 + r, gj = k0 + c;
    D[r][c] = (gi < n && gj < n) ? (double)A[(int64_t)gi * lda + gj] - (double)Cc[(int64_t)gi * n + gj]
                                 : (r == c ? 1.0 : 0.0);
  }
  for (int p = 0; p < NB; ++p) {
    __syncthreads();
    double piv = D[p][p];
    if (!(piv > 0.0) || !(piv <= 1.7976931348623157e308)) {
      if (threadIdx.x == 0) atomicCAS(status, 0, k0 + p + 1);
      piv = 1.0;
    }
    const double inv = 1.0 / piv;
    const double prc = D[p][c];
    double rp[16], rc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      rp[q] = D[rb + 4 * q][p];
      rc[q] = D[rb + 4 * q][c];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = rb + 4 * q;
      double v;
      if (r == p) v = c == p ? inv : prc * inv;
      else if (c == p) v = -rp[q] * inv;
      else v = rc[q] - rp[q] * (prc * inv);
      D[r][c] = v;
    }
  }
  __syncthreads();
  for (int q = 0; q < 16; ++q) {
    const int r = rb + 4 * q;
    Dv[r * NB + c] = D[r][c];
  }
}

// Thread j: Rw[k][j] = sum_l Dinv[k][l] A[k0 + l][j] (l ascending, one float64 fma chain, rounded once) and
// Ct[k][j] = A[j][k0 + k]; 0 past n (j up to ldw, k0 + k up to the block's 64).
__global__ __launch_bounds__(256) void ease_panel_kernel(const float *__restrict__ A,
                                                         const float *__restrict__ Cc, int n, int64_t lda, int k0,
                                                         const double *__restrict__ Dv, float *__restrict__ Rw,
                                                         float *__restrict__ Ct, int64_t ldw) {
  __shared__ double Dinv[NB * NB];
  for (int e = threadIdx.x; e < NB * NB; e += 256) Dinv[e] = Dv[e];
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= ldw) return;
  const int nbk = min(NB, n - k0);
  if (j >= n) {
    for (int k = 0; k < NB; ++k) {
      Rw[k * ldw + j] = 0.f;
      Ct[k * ldw + j] = 0.f;
    }
    return;
  }
  float a[NB], ac[NB];
#pragma unroll
  for (int l = 0; l < NB; ++l) {
    a[l] = l < nbk ? A[(int64_t)(k0 + l) * lda + j] : 0.f;
    ac[l] = l < nbk ? Cc[(int64_t)(k0 + l) * n + j] : 0.f;
  }
  for (int k = 0; k < NB; ++k) {
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < NB; ++l) s = fma(Dinv[k * NB + l], (double)a[l] - (double)ac[l], s);
    Rw[k * ldw + j] = k < nbk ? (float)s : 0.f;
  }
  const float *arow = A + j * lda + k0, *crow = Cc + j * n + k0;
#pragma unroll 8
  for (int k = 0; k < NB; ++k) Ct[k * ldw + j] = k < nbk ? (float)((double)arow[k] - (double)crow[k]) : 0.f;
}

// A[i][j] -= sum_k Ct[k][i] Rw[k][j] for every i, j outside the pivot block's rows and columns.
// One workgroup (4 waves) per 128 x 128 tile; both operands in LDS as [k][128] (a lane reads
// consecutive words: conflict-free for ds_read_b32); wave w takes the 64 x 64 quadrant
// (w >> 1, w & 1) as 2 x 2 accumulators; one k-ascending chain of 32 MFMAs (k = 64) per accumulator.
__global__ __launch_bounds__(256) void ease_update_kernel(float *__restrict__ A, float *__restrict__ Cc, int n,
                                                          int64_t lda, int k0,
                                                          const float *__restrict__ Rw, const float *__restrict__ Ct,
                                                          int64_t ldw) {
  __shared__ __attribute__((aligned(16))) float Cs[NB * TILE];
  __shared__ __attribute__((aligned(16))) float Rs[NB * TILE];
  const int i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
  // (ldw is a multiple of 128 and both images are padded with zeros up to it: float4 loads in bounds)
  for (int e = threadIdx.x; e < NB * TILE / 4; e += 256) {
    const int k = e >> 5, c4 = (e & 31) * 4;
    *reinterpret_cast<float4 *>(&Cs[k * TILE + c4]) = *reinterpret_cast<const float4 *>(&Ct[k * ldw + i0 + c4]);
    *reinterpret_cast<float4 *>(&Rs[k * TILE + c4]) = *reinterpret_cast<const float4 *>(&Rw[k * ldw + j0 + c4]);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int m0 = (wv >> 1) * 64, n0 = (wv & 1) * 64, l31 = lane & 31, kh = lane >> 5;
  f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc00[q] = acc01[q] = acc10[q] = acc11[q] = 0.f;
#pragma unroll 4
  for (int kk = 0; kk < NB; kk += 2) {
    const float *cs = Cs + (kk + kh) * TILE + m0 + l31, *rs = Rs + (kk + kh) * TILE + n0 + l31;
    const float a0 = cs[0], a1 = cs[32], b0 = rs[0], b1 = rs[32];
    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
    acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
  }
  // C/D map of the 32x32 forms: column n = lane & 31, row m = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
  const int k1 = k0 + NB;
#define EASE_STORE(acc, mi, ni)                                                         \
  {                                                                                     \
    const int gj = j0 + n0 + 32 * (ni) + l31;                                           \
    if (gj < n && (gj < k0 || gj >= k1)) {                                              \
      _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                  \
        const int gi = i0 + m0 + 32 * (mi) + (q & 3) + 8 * (q >> 2) + 4 * kh;           \
        if (gi < n && (gi < k0 || gi >= k1)) {                                          \
          /* compensated: the stored value is A - Cc; y is what to add, Cc the part of it that was lost */ \
          float *ap = A + (int64_t)gi * lda + gj, *cp = Cc + (int64_t)gi * n + gj;      \
          const float a = *ap, y = -acc[q] - *cp, t = a + y;                            \
          *cp = (t - a) - y;                                                            \
          *ap = t;                                                                      \
        }                                                                               \
      }                                                                                 \
    }                                                                                   \
  }
  EASE_STORE(acc00, 0, 0)
  EASE_STORE(acc01, 0, 1)
  EASE_STORE(acc10, 1, 0)
  EASE_STORE(acc11, 1, 1)
#undef EASE_STORE
}

// Thread t < n, outside the pivot block: A[k0 + k][t] = Rw[k][t] and A[t][k0 + k] = -sum_l Ct[l][t] Dinv[l][k];
// (float64 chains, rounded once); inside it (t = k0 + r): A[t][k0 + c] = Dinv[r][c].
__global__ __launch_bounds__(256) void ease_writeback_kernel(float *__restrict__ A, float *__restrict__ Cc, int n,
                                                             int64_t lda, int k0,
                                                             const double *__restrict__ Dv, const float *__restrict__ Rw,
                                                             const float *__restrict__ Ct, int64_t ldw) {
  __shared__ double Dinv[NB * NB];
  for (int e = threadIdx.x; e < NB * NB; e += 256) Dinv[e] = Dv[e];
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int nbk = min(NB, n - k0);
  float *arow = A + t * lda + k0;
  // (the panels are written as fresh values: their carries start again from 0)
  for (int k = 0; k < nbk; ++k) {
    Cc[(int64_t)(k0 + k) * n + t] = 0.f;
    Cc[t * n + k0 + k] = 0.f;
  }
  if (t >= k0 && t < k0 + NB) {
    const int r = (int)t - k0;
    for (int c = 0; c < nbk; ++c) arow[c] = (float)Dinv[r * NB + c];
    return;
  }
  for (int k = 0; k < nbk; ++k) A[(int64_t)(k0 + k) * lda + t] = Rw[k * ldw + t];
  float cv[NB];
#pragma unroll
  for (int l = 0; l < NB; ++l) cv[l] = Ct[l * ldw + t];
  for (int k = 0; k < nbk; ++k) {
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < NB; ++l) s = fma((double)cv[l], Dinv[l * NB + k], s);
    arow[k] = (float)-s;
  }
}

// A <- A - Cc: the carries folded in at the end (one rounding)
__global__ __launch_bounds__(256) void ease_fold_kernel(float *__restrict__ A, const float *__restrict__ Cc, int n,
                                                        int64_t lda) {
  const int ncb = (n + 255) / 256;
  const int64_t i = blockIdx.x / ncb;
  const int64_t j = (int64_t)(blockIdx.x % ncb) * 256 + threadIdx.x;
  if (j < n) A[i * lda + j] = (float)((double)A[i * lda + j] - (double)Cc[i * n + j]);
}

// ------------------------------------------------------------------- finalize
__global__ __launch_bounds__(256) void ease_diag_kernel(const float *__restrict__ P, int n, int64_t ldp,
                                                        float *__restrict__ diag) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) diag[j] = P[j * ldp + j];
}

__global__ __launch_bounds__(256) void ease_finalize_kernel(const float *P, int n, int64_t ldp, float *B,
                                                            int64_t ldb, const float *__restrict__ diag) {
  const int ncb = (n + 255) / 256;                      // (a 1-D grid: n may pass the 65535 of grid.y)
  const int64_t i = blockIdx.x / ncb;
  const int64_t j = (int64_t)(blockIdx.x % ncb) * 256 + threadIdx.x;
  if (j >= n) return;
  B[i * ldb + j] = i == j ? 0.f : __fdiv_rn(P[i * ldp + j], -diag[j]);
}

// --------------------------------------------------------------------- scores
constexpr int SC_COLS = 4;        // columns per thread, 256 apart: every load of a wave is 256 contiguous bytes

__global__ __launch_bounds__(256) void ease_scores_kernel(const int64_t *__restrict__ indptr,
                                                          const int32_t *__restrict__ indices,
                                                          const float *__restrict__ data, const float *__restrict__ W,
                                                          int64_t ldw, int lo, int width, float *__restrict__ out,
                                                          int64_t ldo) {
  const int u = blockIdx.x;                             // (users fastest: neighbours share a column tile)
  const int c0 = blockIdx.y * (256 * SC_COLS) + threadIdx.x;
  const int64_t e0 = indptr[u], e1 = indptr[u + 1];
  float acc[SC_COLS];
  bool ok[SC_COLS];
#pragma unroll
  for (int q = 0; q < SC_COLS; ++q) {
    acc[q] = 0.f;
    ok[q] = c0 + 256 * q < width;
  }
  for (int64_t e = e0; e < e1; ++e) {
    const float x = data ? data[e] : 1.f;
    const float *w = W + (int64_t)indices[e] * ldw + lo + c0;
#pragma unroll
    for (int q = 0; q < SC_COLS; ++q)
      if (ok[q]) acc[q] = fmaf(x, w[256 * q], acc[q]);
  }
#pragma unroll
  for (int q = 0; q < SC_COLS; ++q)
    if (ok[q]) out[(int64_t)u * ldo + c0 + 256 * q] = acc[q];
}

// ---------------------------------------------------------------- lowrank add
constexpr int LR_KS = 32;               // k-slab held in LDS
constexpr int LR_LD = TILE + 1;         // odd row stride: the transposing store [row][t] -> [t][row] is conflict-free

// A[i][j] += (alpha a_i) (sum_t V[i][t] V[j][t]) b_j for i in [row_lo, row_hi), j < n.  One workgroup (4 waves) per
// 128 x 128 tile; the rows i0.. and j0.. of V go through LDS as [t][128] slabs of 32 columns of V, zeros past n
// and past k (so k needs no alignment; a zero pair leaves the chain's value as it is); wave w takes the
// 64 x 64 quadrant (w >> 1, w & 1) as 2 x 2 accumulators, each ONE k-ascending chain over all the slabs.
__global__ __launch_bounds__(256) void ease_lowrank_add_kernel(float *__restrict__ A, int n, int64_t lda,
                                                               const float *__restrict__ V, int k, int64_t ldv,
                                                               const float *__restrict__ row_scale,
                                                               const float *__restrict__ col_scale, float alpha,
                                                               int row_lo, int row_hi) {
  __shared__ float Vi[LR_KS * LR_LD];
  __shared__ float Vj[LR_KS * LR_LD];
  const int i0 = row_lo + blockIdx.y * TILE, j0 = blockIdx.x * TILE;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int m0 = (wv >> 1) * 64, n0 = (wv & 1) * 64, l31 = lane & 31, kh = lane >> 5;
  f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc00[q] = acc01[q] = acc10[q] = acc11[q] = 0.f;
  for (int t0 = 0; t0 < k; t0 += LR_KS) {
    if (t0) __syncthreads();            // (the previous slab has been read)
    // thread e: row e / 32 of the tile, column t0 + e % 32 of V: a wave reads two rows' 128 contiguous bytes
    for (int e = threadIdx.x; e < TILE * LR_KS; e += 256) {
      const int r = e >> 5, t = e & 31;
      const bool tk = t0 + t < k;
      const int gi = i0 + r, gj = j0 + r;
      Vi[t * LR_LD + r] = (tk && gi < row_hi) ? V[(int64_t)gi * ldv + t0 + t] : 0.f;
      Vj[t * LR_LD + r] = (tk && gj < n) ? V[(int64_t)gj * ldv + t0 + t] : 0.f;
    }
    __syncthreads();
    const int kend = min(LR_KS, (k - t0 + 1) & ~1);
#pragma unroll 4
    for (int kk = 0; kk < kend; kk += 2) {
      const float *vi = Vi + (kk + kh) * LR_LD + m0 + l31, *vj = Vj + (kk + kh) * LR_LD + n0 + l31;
      const float a0 = vi[0], a1 = vi[32], b0 = vj[0], b1 = vj[32];
      acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
    }
  }
  // C/D map of the 32x32 forms: column n = lane & 31, row m = (q & 3) + 8 (q >> 2) + 4 (lane >> 5).
  // The order the header states: s = alpha * a_i; p = s * dot; A = fma(p, b_j, A) -- three roundings.
#define EASE_LR_STORE(acc, mi, ni)                                                      \
  {                                                                                     \
    const int gj = j0 + n0 + 32 * (ni) + l31;                                           \
    if (gj < n) {                                                                       \
      const float b = col_scale[gj];                                                    \
      _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                  \
        const int gi = i0 + m0 + 32 * (mi) + (q & 3) + 8 * (q >> 2) + 4 * kh;           \
        if (gi < row_hi) {                                                              \
          float *ap = A + (int64_t)gi * lda + gj;                                       \
          const float p = __fmul_rn(__fmul_rn(alpha, row_scale[gi]), acc[q]);           \
          *ap = fmaf(p, b, *ap);                                                        \
        }                                                                               \
      }                                                                                 \
    }                                                                                   \
  }
  EASE_LR_STORE(acc00, 0, 0)
  EASE_LR_STORE(acc01, 0, 1)
  EASE_LR_STORE(acc10, 1, 0)
  EASE_LR_STORE(acc11, 1, 1)
#undef EASE_LR_STORE
}

// ----------------------------------------------------------------------- gemm
constexpr int GM_KS = 32;               // k-slab held in LDS
constexpr int GM_LDA = TILE + 1;        // odd row stride: the transposing store of the A slab is (nearly) conflict-free

// D[i][j] = alpha (sum_t A[i][t] B[t][j]) + beta E[i][j] for i in [row_lo, row_hi), j < n.  One workgroup (4 waves) per
// 128 x 128 tile; the A rows go through LDS transposed as [t][129], the B rows as they lie as [t][128], in slabs of 32
// of k, zeros past the edges (so m, n and k need no alignment; a zero pair leaves the chain's value as it is).  The
// next slab is fetched into registers while the MFMAs of this one run.  Wave w takes the 64 x 64 quadrant
// (w >> 1, w & 1) as 2 x 2 accumulators, each ONE k-ascending chain over all the slabs.  E may be D: an element is
// read and then written by the same thread.
__global__ __launch_bounds__(256) void ease_gemm_kernel(const float *__restrict__ A, int64_t lda,
                                                        const float *__restrict__ B, int64_t ldb, const float *E,
                                                        int64_t lde, float *D, int64_t ldd, int n, int k, float alpha,
                                                        float beta, int row_lo, int row_hi) {
  __shared__ float As[GM_KS * GM_LDA];
  __shared__ float Bs[GM_KS * TILE];
  const int i0 = row_lo + blockIdx.y * TILE, j0 = blockIdx.x * TILE;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int m0 = (wv >> 1) * 64, n0 = (wv & 1) * 64, l31 = lane & 31, kh = lane >> 5;
  // thread e of the A slab: row e / 32 of the tile, column t0 + e % 32 (a wave reads two rows' 128 contiguous bytes);
  // of the B slab: row t0 + e / 128, column e % 128 (a wave reads 256 contiguous bytes)
  const int ar = threadIdx.x >> 5, at = threadIdx.x & 31, bt = threadIdx.x >> 7, bc = threadIdx.x & 127;
  const bool bok = j0 + bc < n;
  float ra[16], rb[16];
#define EASE_GM_FETCH(t0)                                                               \
  _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                      \
    const int gi = i0 + ar + 8 * q, tb = (t0) + bt + 2 * q;                             \
    ra[q] = ((t0) + at < k && gi < row_hi) ? A[(int64_t)gi * lda + (t0) + at] : 0.f;    \
    rb[q] = (tb < k && bok) ? B[(int64_t)tb * ldb + j0 + bc] : 0.f;                     \
  }
  f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc00[q] = acc01[q] = acc10[q] = acc11[q] = 0.f;
  EASE_GM_FETCH(0)
  for (int t0 = 0; t0 < k; t0 += GM_KS) {
    if (t0) __syncthreads();            // (the previous slab has been read)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      As[at * GM_LDA + ar + 8 * q] = ra[q];
      Bs[(bt + 2 * q) * TILE + bc] = rb[q];
    }
    __syncthreads();
    if (t0 + GM_KS < k) EASE_GM_FETCH(t0 + GM_KS)
    const int kend = min(GM_KS, (k - t0 + 1) & ~1);
#pragma unroll 4
    for (int kk = 0; kk < kend; kk += 2) {
      const float *as = As + (kk + kh) * GM_LDA + m0 + l31, *bs = Bs + (kk + kh) * TILE + n0 + l31;
      const float a0 = as[0], a1 = as[32], b0 = bs[0], b1 = bs[32];
      acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
    }
  }
#undef EASE_GM_FETCH
  // C/D map of the 32x32 forms: column n = lane & 31, row m = (q & 3) + 8 (q >> 2) + 4 (lane >> 5).
  // The order the header states: p = alpha * dot; D = p (E NULL) or fma(beta, E, p) -- one or two roundings.
#define EASE_GM_STORE(acc, mi, ni)                                                      \
  {                                                                                     \
    const int gj = j0 + n0 + 32 * (ni) + l31;                                           \
    if (gj < n) {                                                                       \
      _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                  \
        const int gi = i0 + m0 + 32 * (mi) + (q & 3) + 8 * (q >> 2) + 4 * kh;           \
        if (gi < row_hi) {                                                              \
          const float p = __fmul_rn(alpha, acc[q]);                                     \
          D[(int64_t)gi * ldd + gj] = E ? fmaf(beta, E[(int64_t)gi * lde + gj], p) : p; \
        }                                                                               \
      }                                                                                 \
    }                                                                                   \
  }
  EASE_GM_STORE(acc00, 0, 0)
  EASE_GM_STORE(acc01, 0, 1)
  EASE_GM_STORE(acc10, 1, 0)
  EASE_GM_STORE(acc11, 1, 1)
#undef EASE_GM_STORE
}

// true when [a, a + (rows - 1) lda + cols) and [b, ...) share an element
bool gm_overlap(const float *a, int64_t rows, int64_t cols, int64_t lda, const float *b, int64_t rows_b, int64_t cols_b,
                int64_t ldb) {
  const float *ae = a + (rows - 1) * lda + cols, *be = b + (rows_b - 1) * ldb + cols_b;
  return a < be && b < ae;
}

// ---------------------------------------------------------------- admm update
// gamma[j] = (T[j][j] + 1) / P[j][j]: one add, one correctly rounded divide
__global__ __launch_bounds__(256) void ease_admm_gamma_kernel(const float *__restrict__ T, int64_t ldt,
                                                              const float *__restrict__ P, int64_t ldp, int n,
                                                              float *__restrict__ gamma) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) gamma[j] = __fdiv_rn(__fadd_rn(T[j * ldt + j], 1.f), P[j * ldp + j]);
}

// One workgroup per row i: thread t takes the columns t, t + 256, ... in ascending order; the three row statistics are
// per-thread float64 partials in that order, then a pairwise tree over the 256 threads (a fixed order: no atomics).
__global__ __launch_bounds__(256) void ease_admm_update_kernel(const float *__restrict__ T, int64_t ldt,
                                                               const float *__restrict__ P, int64_t ldp,
                                                               float *__restrict__ C, int64_t ldc,
                                                               float *__restrict__ U, int64_t ldu,
                                                               float *__restrict__ M, int64_t ldm, int n, float theta,
                                                               int nonneg, const float *__restrict__ gamma,
                                                               float *__restrict__ row_primal,
                                                               float *__restrict__ row_dual,
                                                               int32_t *__restrict__ row_nnz, int row_lo) {
  __shared__ double sp[256], sd[256];
  __shared__ int sn[256];
  const int64_t i = (int64_t)row_lo + blockIdx.x;
  const float *t = T + i * ldt, *p = P + i * ldp;
  float *c = C + i * ldc, *u = U + i * ldu, *m = M + i * ldm;
  double ap = 0.0, ad = 0.0;
  int an = 0;
  for (int j = threadIdx.x; j < n; j += 256) {
    const float c_old = c[j];
    float b = 0.f, cn = 0.f, un = 0.f, mn = 0.f;
    if (j != i) {
      b = fmaf(-p[j], gamma[j], t[j]);
      const float v = __fadd_rn(b, u[j]);
      const float w = __fsub_rn(nonneg ? v : fabsf(v), theta);
      cn = w > 0.f ? (nonneg ? w : copysignf(w, v)) : 0.f;
      un = __fsub_rn(v, cn);
      mn = __fsub_rn(cn, un);
    }
    c[j] = cn;
    u[j] = un;
    m[j] = mn;
    const double d1 = (double)__fsub_rn(b, cn), d2 = (double)__fsub_rn(cn, c_old);
    ap = fma(d1, d1, ap);
    ad = fma(d2, d2, ad);
    an += cn != 0.f;
  }
  sp[threadIdx.x] = ap;
  sd[threadIdx.x] = ad;
  sn[threadIdx.x] = an;
  for (int s = 128; s > 0; s >>= 1) {
    __syncthreads();
    if (threadIdx.x < s) {
      sp[threadIdx.x] += sp[threadIdx.x + s];
      sd[threadIdx.x] += sd[threadIdx.x + s];
      sn[threadIdx.x] += sn[threadIdx.x + s];
    }
  }
  if (threadIdx.x == 0) {
    row_primal[i] = (float)sp[0];
    row_dual[i] = (float)sd[0];
    row_nnz[i] = sn[0];
  }
}

}  // namespace

// ------------------------------------------------------------------------ ABI
extern "C" {

int rk_ease_version(void) { return 100; }

const char *rk_ease_last_error(void) { return g_rk_side_err; }

int rk_ease_gram(const int64_t *t_indptr, const int32_t *t_indices, const float *t_data, const int64_t *u_indptr,
                 const int32_t *u_indices, const float *u_data, int32_t n_users, int32_t n_items, float reg,
                 float *A, int64_t lda, void *stream) {
  RK_SIDE_REQUIRE(t_indptr && t_indices && u_indptr && u_indices && A, "null pointer");
  RK_SIDE_REQUIRE(n_users >= 0 && n_items >= 1 && lda >= n_items, "bad sizes");
  RK_SIDE_REQUIRE((t_data == nullptr) == (u_data == nullptr), "t_data and u_data must both be given or both be NULL");
  const dim3 grid(n_items, (n_items + GR_STRIP - 1) / GR_STRIP);
  hipLaunchKernelGGL(ease_gram_kernel, grid, dim3(GR_WAVES * 64), 0, (hipStream_t)stream, t_indptr, t_indices,
                     t_data, u_indptr, u_indices, u_data, n_users, n_items, reg, A, lda);
  RK_SIDE_CHECK_LAUNCH("ease_gram_kernel");
  return 0;
}

int64_t rk_ease_spd_inverse_workspace_bytes(int32_t n) {
  if (n < 1) {
    rk_side_set_error("%s: n must be >= 1", __func__);
    return -2;
  }
  return 2 * NB * inv_ldw(n) * (int64_t)sizeof(float) + NB * NB * (int64_t)sizeof(double) +
         (int64_t)n * n * (int64_t)sizeof(float);
}

int rk_ease_spd_inverse(float *A, int32_t n, int64_t lda, void *ws, int64_t ws_bytes, int32_t *status,
                        void *stream) {
  RK_SIDE_REQUIRE(A && ws && status, "null pointer");
  RK_SIDE_REQUIRE(n >= 1 && lda >= n, "bad sizes");
  RK_SIDE_REQUIRE(ws_bytes >= rk_ease_spd_inverse_workspace_bytes(n), "workspace too small");
  RK_SIDE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t ldw = inv_ldw(n);
  float *Rw = (float *)ws, *Ct = Rw + NB * ldw;
  double *Dv = (double *)(Ct + NB * ldw);
  float *Cc = (float *)(Dv + NB * NB);        // [n, n]: the carries of the compensated update
  RK_SIDE_REQUIRE((int64_t)((n + 255) / 256) * n < ((int64_t)1 << 31), "n too large for one launch");
  if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(Cc, 0, (size_t)n * n * sizeof(float), s) != hipSuccess) {
    rk_side_set_error("%s: hipMemsetAsync failed", __func__);
    return -1;
  }
  const int tiles = (int)(ldw / TILE);
  for (int k0 = 0; k0 < n; k0 += NB) {
    hipLaunchKernelGGL(ease_pivot_kernel, dim3(1), dim3(256), 0, s, A, Cc, n, lda, k0, Dv, status);
    hipLaunchKernelGGL(ease_panel_kernel, dim3((unsigned)((ldw + 255) / 256)), dim3(256), 0, s, A, Cc, n, lda, k0,
                       Dv, Rw, Ct, ldw);
    if (n > NB)      // (one block: nothing outside the pivot block)
      hipLaunchKernelGGL(ease_update_kernel, dim3(tiles, tiles), dim3(256), 0, s, A, Cc, n, lda, k0, Rw, Ct,
                         ldw);
    hipLaunchKernelGGL(ease_writeback_kernel, dim3((n + 255) / 256), dim3(256), 0, s, A, Cc, n, lda, k0, Dv, Rw,
                       Ct, ldw);
  }
  hipLaunchKernelGGL(ease_fold_kernel, dim3((unsigned)((int64_t)((n + 255) / 256) * n)), dim3(256), 0, s, A, Cc, n, lda);
  RK_SIDE_CHECK_LAUNCH("rk_ease_spd_inverse");
  return 0;
}

int rk_ease_finalize(const float *P, int32_t n, int64_t ldp, float *B, int64_t ldb, float *diag, void *stream) {
  RK_SIDE_REQUIRE(P && B && diag, "null pointer");
  RK_SIDE_REQUIRE(n >= 1 && ldp >= n && ldb >= n, "bad sizes");
  RK_SIDE_REQUIRE((int64_t)((n + 255) / 256) * n < ((int64_t)1 << 31), "n too large for one launch");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ease_diag_kernel, dim3((n + 255) / 256), dim3(256), 0, s, P, n, ldp, diag);
  hipLaunchKernelGGL(ease_finalize_kernel, dim3((unsigned)((int64_t)((n + 255) / 256) * n)), dim3(256), 0, s, P, n, ldp, B, ldb,
                     diag);
  RK_SIDE_CHECK_LAUNCH("rk_ease_finalize");
  return 0;
}

int rk_ease_scores(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows, const float *W,
                   int64_t ldw, int32_t lo, int32_t hi, float *out, int64_t ldo, void *stream) {
  RK_SIDE_REQUIRE(indptr && indices && W && out, "null pointer");
  RK_SIDE_REQUIRE(n_rows >= 0 && 0 <= lo && lo < hi && ldw >= hi && ldo >= hi - lo, "bad sizes");
  if (n_rows == 0) return 0;
  const int width = hi - lo;
  const dim3 grid(n_rows, (width + 256 * SC_COLS - 1) / (256 * SC_COLS));
  hipLaunchKernelGGL(ease_scores_kernel, grid, dim3(256), 0, (hipStream_t)stream, indptr, indices, data, W, ldw, lo,
                     width, out, ldo);
  RK_SIDE_CHECK_LAUNCH("ease_scores_kernel");
  return 0;
}

int rk_ease_lowrank_add(float *A, int32_t n, int64_t lda, const float *V, int32_t k, int64_t ldv,
                        const float *row_scale, const float *col_scale, float alpha, int32_t row_lo, int32_t row_hi,
                        void *stream) {
  RK_SIDE_REQUIRE(A && V && row_scale && col_scale, "null pointer");
  RK_SIDE_REQUIRE(n >= 1 && lda >= n, "bad sizes");
  RK_SIDE_REQUIRE(k >= 1 && k <= 512 && ldv >= k, "k must be in [1, 512] and ldv >= k");
  RK_SIDE_REQUIRE(0 <= row_lo && row_lo <= row_hi && row_hi <= n, "bad row range");
  if (row_lo == row_hi) return 0;
  const int row_tiles = (row_hi - row_lo + TILE - 1) / TILE;
  RK_SIDE_REQUIRE(row_tiles <= 65535, "n too large for one launch");
  const dim3 grid((n + TILE - 1) / TILE, row_tiles);
  hipLaunchKernelGGL(ease_lowrank_add_kernel, grid, dim3(256), 0, (hipStream_t)stream, A, n, lda, V, k, ldv,
                     row_scale, col_scale, alpha, row_lo, row_hi);
  RK_SIDE_CHECK_LAUNCH("ease_lowrank_add_kernel");
  return 0;
}

int rk_ease_gemm(const float *A, int64_t lda, const float *B, int64_t ldb, const float *E, int64_t lde, float *D,
                 int64_t ldd, int32_t m, int32_t n, int32_t k, float alpha, float beta, int32_t row_lo, int32_t row_hi,
                 void *stream) {
  RK_SIDE_REQUIRE(A && B && D, "null pointer");
  RK_SIDE_REQUIRE(m >= 1 && n >= 1 && k >= 1 && lda >= k && ldb >= n && ldd >= n && (!E || lde >= n), "bad sizes");
  RK_SIDE_REQUIRE(0 <= row_lo && row_lo <= row_hi && row_hi <= m, "bad row range");
  RK_SIDE_REQUIRE(!gm_overlap(D, m, n, ldd, A, m, k, lda) && !gm_overlap(D, m, n, ldd, B, k, n, ldb),
                  "D must not overlap A or B");
  RK_SIDE_REQUIRE(!E || E == D || !gm_overlap(D, m, n, ldd, E, m, n, lde), "E must be NULL, D or not overlap D");
  RK_SIDE_REQUIRE(E != D || lde == ldd, "E == D needs lde == ldd");
  if (row_lo == row_hi) return 0;
  const int row_tiles = (row_hi - row_lo + TILE - 1) / TILE;
  RK_SIDE_REQUIRE(row_tiles <= 65535, "m too large for one launch");
  const dim3 grid((n + TILE - 1) / TILE, row_tiles);
  hipLaunchKernelGGL(ease_gemm_kernel, grid, dim3(256), 0, (hipStream_t)stream, A, lda, B, ldb, E, lde, D, ldd, n, k,
                     alpha, beta, row_lo, row_hi);
  RK_SIDE_CHECK_LAUNCH("ease_gemm_kernel");
  return 0;
}

int rk_ease_admm_update(const float *T, int64_t ldt, const float *P, int64_t ldp, float *C, int64_t ldc, float *U,
                        int64_t ldu, float *M, int64_t ldm, int32_t n, float theta, int32_t nonneg, float *gamma,
                        float *row_primal, float *row_dual, int32_t *row_nnz, int32_t row_lo, int32_t row_hi,
                        void *stream) {
  RK_SIDE_REQUIRE(T && P && C && U && M && gamma && row_primal && row_dual && row_nnz, "null pointer");
  RK_SIDE_REQUIRE(n >= 1 && ldt >= n && ldp >= n && ldc >= n && ldu >= n && ldm >= n, "bad sizes");
  RK_SIDE_REQUIRE(theta >= 0.f && theta <= 3.4028234663852886e38f, "theta must be finite and >= 0");
  RK_SIDE_REQUIRE(nonneg == 0 || nonneg == 1, "nonneg must be 0 or 1");
  RK_SIDE_REQUIRE(0 <= row_lo && row_lo <= row_hi && row_hi <= n, "bad row range");
  if (row_lo == row_hi) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ease_admm_gamma_kernel, dim3((n + 255) / 256), dim3(256), 0, s, T, ldt, P, ldp, n, gamma);
  hipLaunchKernelGGL(ease_admm_update_kernel, dim3(row_hi - row_lo), dim3(256), 0, s, T, ldt, P, ldp, C, ldc, U, ldu, M,
                     ldm, n, theta, nonneg, gamma, row_primal, row_dual, row_nnz, row_lo);
  RK_SIDE_CHECK_LAUNCH("rk_ease_admm_update");
  return 0;
}

}  // extern "C"

// ----------------------------------------------------------------- explanations
namespace {
struct XpDenseFetch {                             // W[i][j] of a dense matrix
  const float *W;
  int64_t ldw;
  __device__ __forceinline__ float operator()(int i, int j) const { return W[(int64_t)i * ldw + j]; }
};
}  // namespace

extern "C" int rk_ease_explain_max_contributors(void) { return XP_MAX_M; }

extern "C" int rk_ease_explain(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows,
                               const float *W, int64_t ldw, int32_t n_items, const int64_t *items, int32_t J, int32_t m,
                               int64_t *contributors, float *contributions, float *baseline, float *total,
                               void *stream) {
  RK_SIDE_REQUIRE(n_rows >= 0 && n_items >= 1 && ldw >= n_items, "bad sizes");
  RK_SIDE_REQUIRE(J >= 1 && m >= 1 && m <= XP_MAX_M && (int64_t)n_rows * J <= 0x7fffffff,
                  "J >= 1, 1 <= m <= 64, n_rows * J < 2^31");
  if (n_rows == 0) return 0;
  RK_SIDE_REQUIRE(indptr && indices && W && items && contributors && contributions && baseline && total,
                  "null pointer");
  const XpDenseFetch fetch{W, ldw};
  hipLaunchKernelGGL(xp_item_kernel<XpDenseFetch>, dim3((unsigned)((int64_t)n_rows * J)), dim3(64), 0,
                     (hipStream_t)stream, indptr, indices, data, n_items, items, J, m, fetch, contributors,
                     contributions, baseline, total);
  RK_SIDE_CHECK_LAUNCH("ease_explain_kernel");
  return 0;
}

#include "ease/elsa.h"    // rk_ease_elsa_normalize, _rows, _scatter, _project, _adam, rk_ease_csr_sub
