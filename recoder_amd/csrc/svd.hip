// PureSVD: the kernels of the randomized truncated SVD (include/recoder_svd.h, librecoder_svd.so).
//
//   rk_svd_gaussian      one thread per element, the counter RNG of common.h keyed on (seed, row, column)
//   rk_svd_spmm          CSR x tall dense: a lane owns 4 consecutive columns (16-byte loads), a narrow l
//                        packs several entries per wave-instruction; a row below RK_SVD_LONG_ROW entries
//                        is one wave's, a longer one goes to a workgroup of 16 waves whose pieces are
//                        added in wave order through LDS.  The (column, value) pairs are fetched 64 at a
//                        time and handed out by shuffles, so the gathers of a step do not wait on an
//                        index load of their own
//   rk_svd_chol_inverse  one workgroup, float64: right-looking Cholesky on the upper triangle (one
//                        barrier per pivot: the row is left unscaled until the end), then R^-1 one
//                        thread per column, kept transposed in the lower triangle
//   rk_svd_rotate        tall x small on v_mfma_f32_32x32x2_f32: a workgroup owns 64 rows x 256 columns,
//                        both operands staged in LDS 32 k at a time, every output one k-ascending chain
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "../../include/recoder_svd.h"
#include "side_error.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MAX_L = 512;

// ------------------------------------------------------------------- gaussian
constexpr uint64_t SEED_XOR = 0x5d3a1f9e27c4b861ULL;      // (keeps the stream apart from dropout's and the VAE's)

__device__ __forceinline__ float svd_normal(uint64_t seed, uint64_t row, uint64_t col) {
  uint64_t k = rk_mix64((seed ^ SEED_XOR) + 0x9e3779b97f4a7c15ULL);
  k = rk_mix64(k ^ (row * 0xd1342543de82ef95ULL + col + 0x632be59bd9b4e019ULL));
  const float u1 = (float)((k >> 40) + 1) * (1.0f / 16777216.0f);           // (0, 1]
  const float u2 = (float)((k >> 16) & 0xffffffULL) * (1.0f / 16777216.0f); // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

__global__ __launch_bounds__(256) void svd_gaussian_kernel(float *__restrict__ out, int64_t n, int l, int ld,
                                                           uint64_t seed) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int64_t r = e / l;
  const int c = (int)(e - r * l);
  out[r * ld + c] = svd_normal(seed, (uint64_t)r, (uint64_t)c);
}

// ----------------------------------------------------------------------- spmm
constexpr int LONG_WAVES = 16;
constexpr int SPMM_UNROLL = 4;

struct spmm_shape_t {
  int groups;      // ceil(l / 4): column groups of an entry
  int P;           // lanes per entry (a power of two, <= 64)
  int logP;
};

// The columns a lane owns: group sub + P t (t < T), 4 columns each.
template <bool VEC, int T>
__device__ __forceinline__ void spmm_load(const float *__restrict__ frow, bool valid, int sub, const spmm_shape_t &s,
                                          int l, float4 (&f)[T]) {
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int g = sub + s.P * t;
    f[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid && g < s.groups) {
      if (VEC) {
        f[t] = *reinterpret_cast<const float4 *>(frow + 4 * g);
      } else {
        const int c = 4 * g;
        f[t].x = frow[c];
        if (c + 1 < l) f[t].y = frow[c + 1];
        if (c + 2 < l) f[t].z = frow[c + 2];
        if (c + 3 < l) f[t].w = frow[c + 3];
      }
    }
  }
}

// One wave over the entries [e0, e1) of a row: slot (lane >> logP) takes entries slot, slot + E, ... of
// every 64 in order; the slots' sums are then added by a butterfly, so every lane of a column group ends
// with the same value.
template <bool VEC, int T>
__device__ __forceinline__ void spmm_piece(const int32_t *__restrict__ indices, const float *__restrict__ data,
                                           int64_t e0, int64_t e1, const float *__restrict__ F, int ldf, int l,
                                           const spmm_shape_t &s, float4 (&acc)[T]) {
  const int lane = threadIdx.x & 63, sub = lane & (s.P - 1), slot = lane >> s.logP;
  const int E = 64 >> s.logP;
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t eb = e0; eb < e1; eb += 64) {
    const int cnt = e1 - eb < 64 ? (int)(e1 - eb) : 64;
    int myc = 0;
    float myv = 0.f;
    if (lane < cnt) {
      myc = indices[eb + lane];
      myv = data ? data[eb + lane] : 1.f;
    }
    const int steps = (cnt + E - 1) >> (6 - s.logP);        // ceil(cnt / E), wave-uniform
    for (int k = 0; k < steps; k += SPMM_UNROLL) {
      // the gathers of SPMM_UNROLL steps are issued together; an entry past the end adds +0 (v = 0, f = 0)
      float4 f[SPMM_UNROLL][T];
      float v[SPMM_UNROLL];
#pragma unroll
      for (int u = 0; u < SPMM_UNROLL; ++u) {
        const int src = (k + u) * E + slot;
        const bool valid = src < cnt;                       // (cnt <= 64)
        const int c = __shfl(myc, src & 63, 64);
        v[u] = __shfl(myv, src & 63, 64);
        if (!valid) v[u] = 0.f;
        spmm_load<VEC, T>(F + (int64_t)c * ldf, valid, sub, s, l, f[u]);
      }
#pragma unroll
      for (int u = 0; u < SPMM_UNROLL; ++u)
#pragma unroll
        for (int t = 0; t < T; ++t) {
          acc[t].x = fmaf(v[u], f[u][t].x, acc[t].x);
          acc[t].y = fmaf(v[u], f[u][t].y, acc[t].y);
          acc[t].z = fmaf(v[u], f[u][t].z, acc[t].z);
          acc[t].w = fmaf(v[u], f[u][t].w, acc[t].w);
        }
    }
  }
  for (int off = 32; off >= s.P; off >>= 1) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      acc[t].x += __shfl_xor(acc[t].x, off, 64);
      acc[t].y += __shfl_xor(acc[t].y, off, 64);
      acc[t].z += __shfl_xor(acc[t].z, off, 64);
      acc[t].w += __shfl_xor(acc[t].w, off, 64);
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void spmm_store(float *__restrict__ yrow, int g, int l, const float4 &a) {
  if (VEC) {
    *reinterpret_cast<float4 *>(yrow + 4 * g) = a;
  } else {
    const int c = 4 * g;
    yrow[c] = a.x;
    if (c + 1 < l) yrow[c + 1] = a.y;
    if (c + 2 < l) yrow[c + 2] = a.z;
    if (c + 3 < l) yrow[c + 3] = a.w;
  }
}

// One wave per row, 4 rows per workgroup; a long row is left to svd_spmm_long_kernel.
template <bool VEC, int T>
__global__ __launch_bounds__(256) void svd_spmm_kernel(const int64_t *__restrict__ indptr,
                                                       const int32_t *__restrict__ indices,
                                                       const float *__restrict__ data, int row_lo, int row_hi,
                                                       const float *__restrict__ F, int ldf, int l, spmm_shape_t s,
                                                       float *__restrict__ Y, int ldy) {
  const int64_t r = (int64_t)row_lo + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= row_hi) return;
  const int64_t e0 = indptr[r], e1 = indptr[r + 1];
  if (e1 - e0 >= RK_SVD_LONG_ROW) return;
  float4 acc[T];
  spmm_piece<VEC, T>(indices, data, e0, e1, F, ldf, l, s, acc);
  const int lane = threadIdx.x & 63;
  if (lane < s.P) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int g = lane + s.P * t;
      if (g < s.groups) spmm_store<VEC>(Y + r * ldy, g, l, acc[t]);
    }
  }
}

// One workgroup of 16 waves per row; a short row is svd_spmm_kernel's.
template <bool VEC, int T>
__global__ __launch_bounds__(64 * LONG_WAVES) void svd_spmm_long_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const float *__restrict__ data,
    int row_lo, const float *__restrict__ F, int ldf, int l, spmm_shape_t s, float *__restrict__ Y, int ldy) {
  __shared__ __attribute__((aligned(16))) float red[LONG_WAVES * MAX_L];
  const int64_t r = (int64_t)row_lo + blockIdx.x;
  const int64_t e0 = indptr[r], e1 = indptr[r + 1];
  if (e1 - e0 < RK_SVD_LONG_ROW) return;                 // (workgroup-uniform: no barrier has run yet)
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t piece = (e1 - e0 + LONG_WAVES - 1) / LONG_WAVES;
  const int64_t p0 = e0 + wv * piece < e1 ? e0 + wv * piece : e1;
  const int64_t p1 = p0 + piece < e1 ? p0 + piece : e1;
  float4 acc[T];
  spmm_piece<VEC, T>(indices, data, p0, p1, F, ldf, l, s, acc);
  if (lane < s.P) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int g = lane + s.P * t;
      if (g < s.groups) *reinterpret_cast<float4 *>(&red[wv * MAX_L + 4 * g]) = acc[t];
    }
  }
  __syncthreads();
  for (int g = threadIdx.x; g < s.groups; g += 64 * LONG_WAVES) {
    float4 a = *reinterpret_cast<const float4 *>(&red[4 * g]);
    for (int w = 1; w < LONG_WAVES; ++w) {
      const float4 b = *reinterpret_cast<const float4 *>(&red[w * MAX_L + 4 * g]);
      a.x += b.x;
      a.y += b.y;
      a.z += b.z;
      a.w += b.w;
    }
    spmm_store<VEC>(Y + r * ldy, g, l, a);
  }
}

// --------------------------------------------------------------- chol inverse
constexpr int CH_THREADS = 1024;
constexpr int CH_LDS_L = 128;                     // the float64 matrix stays in LDS up to this l
constexpr int CH_LDS_LD = CH_LDS_L + 1;

__device__ __forceinline__ bool chol_bad_pivot(double piv, double floor_) {
  return !(piv > floor_) || !(piv <= 1.7976931348623157e308);
}

__global__ __launch_bounds__(CH_THREADS) void svd_chol_inverse_kernel(const float *__restrict__ G, int l,
                                                                      float *__restrict__ Rinv,
                                                                      double *__restrict__ ws,
                                                                      int *__restrict__ status) {
  __shared__ double lds[CH_LDS_L * CH_LDS_LD];
  __shared__ double floors[MAX_L];                // l 2^-23 G[k][k]: what a pivot must exceed
  const bool in_lds = l <= CH_LDS_L;
  double *A = in_lds ? lds : ws;
  const int ld = in_lds ? CH_LDS_LD : l;
  const int tid = threadIdx.x, tj = tid & 31, ti = tid >> 5;
  for (int i = ti; i < l; i += 32)
    for (int j = tj; j < l; j += 32) A[i * ld + j] = j >= i ? (double)G[(int64_t)i * l + j] : 0.0;
  for (int k = tid; k < l; k += CH_THREADS) floors[k] = (double)l * 1.1920928955078125e-07 * fabs((double)G[(int64_t)k * l + k]);
  // right-looking, on the upper triangle; row k stays unscaled (A[k][j] = R[k][j] sqrt(piv_k)) until the
  // loop is over, so a pivot costs one barrier
  for (int k = 0; k < l; ++k) {
    __syncthreads();
    double piv = A[k * ld + k];
    if (chol_bad_pivot(piv, floors[k])) {
      if (tid == 0) atomicCAS(status, 0, k + 1);
      piv = 1.0;
    }
    const double inv = 1.0 / piv;
    const double *rk = A + k * ld;
    for (int i = k + 1 + ti; i < l; i += 32) {
      const double ci = rk[i] * inv;
      double *ri = A + i * ld;
      for (int j = i + ((tj - i) & 31); j < l; j += 32) ri[j] = fma(-ci, rk[j], ri[j]);   // (j >= i, j = tj mod 32)
    }
  }
  __syncthreads();
  for (int k = ti; k < l; k += 32) {
    double piv = A[k * ld + k];
    if (chol_bad_pivot(piv, floors[k])) piv = 1.0;
    const double d = sqrt(piv), inv = 1.0 / d;
    for (int j = k + 1 + tj; j < l; j += 32) A[k * ld + j] *= inv;
  }
  __syncthreads();                                // (every off-diagonal read of a diagonal is over)
  for (int k = tid; k < l; k += CH_THREADS) {
    double piv = A[k * ld + k];
    if (chol_bad_pivot(piv, floors[k])) piv = 1.0;
    A[k * ld + k] = sqrt(piv);
  }
  __syncthreads();
  // X = R^-1, column j by thread j, from the diagonal up: X[i][j] = -(sum_{i < k <= j} R[i][k] X[k][j]) / R[i][i];
  // X[i][j] (i < j) is kept at A[j][i], which no other thread touches; X[j][j] = 1 / R[j][j]
  if (tid < l) {
    const int j = tid;
    double *xj = A + j * ld;
    const double xjj = 1.0 / A[j * ld + j];
    for (int i = j - 1; i >= 0; --i) {
      const double *ri = A + i * ld;
      double sum = ri[j] * xjj;
      for (int k = i + 1; k < j; ++k) sum = fma(ri[k], xj[k], sum);
      xj[i] = -sum / ri[i];
    }
  }
  __syncthreads();
  for (int i = ti; i < l; i += 32)
    for (int j = tj; j < l; j += 32) {
      double v = 0.0;
      if (j > i) v = A[j * ld + i];
      else if (j == i) v = 1.0 / A[i * ld + i];
      Rinv[(int64_t)i * l + j] = (float)v;
    }
}

// --------------------------------------------------------------------- rotate
constexpr int RT_ROWS = 64, RT_COLS = 256, RT_K = 32;
constexpr int RT_YLD = RT_ROWS + 1;               // (the transposing store: bank = (k + row) mod 32)

__global__ __launch_bounds__(256) void svd_rotate_kernel(const float *__restrict__ Y, int rows, int l, int ldy,
                                                         const float *__restrict__ M, int l2, int ldm,
                                                         float *__restrict__ Out, int ldo) {
  __shared__ float Ys[RT_K * RT_YLD];             // [k][row]
  __shared__ float Ms[RT_K * RT_COLS];            // [k][column]
  const int64_t row0 = (int64_t)blockIdx.x * RT_ROWS;
  const int col0 = blockIdx.y * RT_COLS;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l31 = lane & 31, kh = lane >> 5;
  const int m0 = (wv & 1) * 32, n0 = (wv >> 1) * 128;
  // 32-column tiles this wave owns that hold a column below l2 (wave-uniform)
  const int left = l2 - col0 - n0;
  const int nt = left <= 0 ? 0 : (left >= 128 ? 4 : (left + 31) >> 5);
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
  const int yk = threadIdx.x & 31, yr = threadIdx.x >> 5;
  for (int k0 = 0; k0 < l; k0 += RT_K) {
    __syncthreads();
#pragma unroll
    for (int p = 0; p < RT_ROWS / 8; ++p) {
      const int rr = yr + 8 * p;
      const int64_t gr = row0 + rr;
      Ys[yk * RT_YLD + rr] = (gr < rows && k0 + yk < l) ? Y[gr * ldy + k0 + yk] : 0.f;
    }
    {
      const int gc = col0 + threadIdx.x;
#pragma unroll 8
      for (int k = 0; k < RT_K; ++k)
        Ms[k * RT_COLS + threadIdx.x] = (gc < l2 && k0 + k < l) ? M[(int64_t)(k0 + k) * ldm + gc] : 0.f;
    }
    __syncthreads();
    if (nt > 0) {
#pragma unroll 4
      for (int kk = 0; kk < RT_K; kk += 2) {
        const float a = Ys[(kk + kh) * RT_YLD + m0 + l31];
        const float *ms = Ms + (kk + kh) * RT_COLS + n0 + l31;
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (t < nt) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ms[32 * t], acc[t], 0, 0, 0);
      }
    }
  }
  // C/D map of the 32x32 forms: column n = lane & 31, row m = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int gc = col0 + n0 + 32 * t + l31;
    if (t < nt && gc < l2) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t gr = row0 + m0 + (q & 3) + 8 * (q >> 2) + 4 * kh;
        if (gr < rows) Out[gr * ldo + gc] = acc[t][q];
      }
    }
  }
}

spmm_shape_t spmm_shape(int l) {
  spmm_shape_t s;
  s.groups = (l + 3) / 4;
  s.logP = 0;
  while ((1 << s.logP) < s.groups && s.logP < 6) ++s.logP;
  s.P = 1 << s.logP;
  return s;
}

template <bool VEC, int T>
void spmm_launch(const int64_t *indptr, const int32_t *indices, const float *data, int row_lo, int row_hi,
                 const float *F, int ldf, int l, float *Y, int ldy, hipStream_t st) {
  const spmm_shape_t s = spmm_shape(l);
  const int n = row_hi - row_lo;
  hipLaunchKernelGGL((svd_spmm_kernel<VEC, T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, indptr, indices, data,
                     row_lo, row_hi, F, ldf, l, s, Y, ldy);
  hipLaunchKernelGGL((svd_spmm_long_kernel<VEC, T>), dim3((unsigned)n), dim3(64 * LONG_WAVES), 0, st, indptr, indices,
                     data, row_lo, F, ldf, l, s, Y, ldy);
}

}  // namespace

// ------------------------------------------------------------------------ ABI
extern "C" {

int rk_svd_version(void) { return 100; }

const char *rk_svd_last_error(void) { return g_rk_side_err; }

int rk_svd_max_l(void) { return MAX_L; }

int rk_svd_gaussian(float *out, int32_t rows, int32_t l, int32_t ld, uint64_t seed, void *stream) {
  RK_SIDE_REQUIRE(out != nullptr, "null pointer");
  RK_SIDE_REQUIRE(rows >= 0 && l >= 1 && ld >= l, "bad sizes");
  const int64_t n = (int64_t)rows * l;
  if (n == 0) return 0;
  RK_SIDE_REQUIRE((n + 255) / 256 < ((int64_t)1 << 31), "too many elements for one launch");
  hipLaunchKernelGGL(svd_gaussian_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, n,
                     l, ld, seed);
  RK_SIDE_CHECK_LAUNCH("svd_gaussian_kernel");
  return 0;
}

int rk_svd_spmm(const int64_t *indptr, const int32_t *indices, const float *data, int32_t row_lo, int32_t row_hi,
                const float *F, int32_t ldf, int32_t l, float *Y, int32_t ldy, void *stream) {
  RK_SIDE_REQUIRE(indptr && indices && F && Y, "null pointer");
  RK_SIDE_REQUIRE(0 <= row_lo && row_lo <= row_hi, "bad row range");
  RK_SIDE_REQUIRE(l >= 1 && l <= MAX_L && ldf >= l && ldy >= l, "bad sizes");
  if (row_lo == row_hi) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = l % 4 == 0 && ldf % 4 == 0 && ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(F) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(Y) & 15) == 0;
  const bool two = (l + 3) / 4 > 64;              // (a lane owns two column groups past l = 256)
  if (vec && two) spmm_launch<true, 2>(indptr, indices, data, row_lo, row_hi, F, ldf, l, Y, ldy, st);
  else if (vec) spmm_launch<true, 1>(indptr, indices, data, row_lo, row_hi, F, ldf, l, Y, ldy, st);
  else if (two) spmm_launch<false, 2>(indptr, indices, data, row_lo, row_hi, F, ldf, l, Y, ldy, st);
  else spmm_launch<false, 1>(indptr, indices, data, row_lo, row_hi, F, ldf, l, Y, ldy, st);
  RK_SIDE_CHECK_LAUNCH("rk_svd_spmm");
  return 0;
}

int64_t rk_svd_chol_inverse_workspace_bytes(int32_t l) {
  if (l < 1 || l > MAX_L) {
    rk_side_set_error("%s: l must be in 1..%d", __func__, MAX_L);
    return -2;
  }
  return l <= CH_LDS_L ? 0 : (int64_t)l * l * (int64_t)sizeof(double);
}

int rk_svd_chol_inverse(const float *G, int32_t l, float *Rinv, void *ws, int64_t ws_bytes, int32_t *status,
                        void *stream) {
  RK_SIDE_REQUIRE(G && Rinv && status, "null pointer");
  RK_SIDE_REQUIRE(l >= 1 && l <= MAX_L, "bad sizes");
  const int64_t need = rk_svd_chol_inverse_workspace_bytes(l);
  RK_SIDE_REQUIRE(need == 0 || (ws != nullptr && ws_bytes >= need), "workspace too small");
  RK_SIDE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "workspace must be 16-byte aligned");
  hipLaunchKernelGGL(svd_chol_inverse_kernel, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, G, l, Rinv,
                     (double *)ws, status);
  RK_SIDE_CHECK_LAUNCH("svd_chol_inverse_kernel");
  return 0;
}

int rk_svd_rotate(const float *Y, int32_t rows, int32_t l, int32_t ldy, const float *M, int32_t l2, int32_t ldm,
                  float *Out, int32_t ldo, void *stream) {
  RK_SIDE_REQUIRE(Y && M && Out, "null pointer");
  RK_SIDE_REQUIRE(rows >= 0 && l >= 1 && l <= MAX_L && l2 >= 1 && l2 <= MAX_L, "bad sizes");
  RK_SIDE_REQUIRE(ldy >= l && ldm >= l2 && ldo >= l2, "bad leading dimensions");
  RK_SIDE_REQUIRE(Out != Y, "the rotation is out of place");
  if (rows == 0) return 0;
  const dim3 grid((unsigned)(((int64_t)rows + RT_ROWS - 1) / RT_ROWS), (l2 + RT_COLS - 1) / RT_COLS);
  hipLaunchKernelGGL(svd_rotate_kernel, grid, dim3(256), 0, (hipStream_t)stream, Y, rows, l, ldy, M, l2, ldm, Out, ldo);
  RK_SIDE_CHECK_LAUNCH("svd_rotate_kernel");
  return 0;
}

}  // extern "C"
