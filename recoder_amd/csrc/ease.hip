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
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/recoder_ease.h"
#include "side_error.h"

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

}  // extern "C"
