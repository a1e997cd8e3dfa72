// ELSA (Vancura, Alves, Kasalicky & Kordik, RecSys 2022): the low-rank shallow autoencoder
// scores = x (A A^T - I), A [n, h] the row-normalised W, trained by mini-batch steps on the cosine loss
// without the B x n prediction block (recoder_amd/elsa.py; the ABI and the numerics are in include/recoder_ease.h).
// Included by ease.hip inside nothing: it opens its own anonymous namespace and its own extern "C" block.
//
//   rk_ease_elsa_normalize  a wave per row of W: the row's sum of squares in float64, the norm, the normalised row;
//                           A^T by a second launch through a 64 x 65 LDS tile
//   rk_ease_elsa_rows       a wave per batch row: |Z_u|^2 and <Z_u, Q_u> in float64, the row scalars in float64, E and
//                           F rounded once; the batch loss by a one-workgroup launch in a fixed order
//   rk_ease_elsa_scatter    G0[j] = sum over the batch users of item j of x_uj E_u: the range [lo, hi) of positions is
//                           searched in row j of the item-major CSR; a wave per item, every output ONE ascending
//                           fmaf chain; items with RK_EASE_ELSA_LONG or more entries in the range go to a workgroup
//                           that splits the row's COLUMNS over 512 threads (the chain of an output is the same);
//                           the workgroups find them 512 rows at a time and list them in a fixed order
//   rk_ease_elsa_project    dW_j = (dA_j - <dA_j, A_j> A_j) / max(|W_j|, 1e-12), a wave per row
//   rk_ease_elsa_adam       the same projection, Adam, and the row's new norm and normalised image, a wave per row
//   rk_ease_csr_sub         out[u][j - lo] -= x_uj, a wave per CSR row
#pragma once

namespace {

constexpr int EL_MAX_H = 512;
constexpr int EL_NT = EL_MAX_H / 64;          // columns of a lane: lane, lane + 64, ...
constexpr float EL_TINY = 1e-12f;             // the floor of a row norm (torch's F.normalize eps)
// (sqrtf and / on f32 are correctly rounded: hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt; the
// __fsqrt_rn of the HIP headers is the native approximation)
constexpr int EL_LONG = RK_EASE_ELSA_LONG;
constexpr int EL_LONG_THREADS = 512;          // a column each (h <= 512)
constexpr int EL_LONG_GRID = 1024;

// The sum over a wave's 64 lanes of a float64, a butterfly over the lane distances 32, 16, .. 1: every lane ends with
// the same value (a + b == b + a), a fixed order.
__device__ __forceinline__ double el_wave_sum(double s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// lane l: the float64 fma chain of x[k] y[k] over k = l, l + 64, .. ascending, from 0
__device__ __forceinline__ double el_lane_dot(const float (&x)[EL_NT], const float (&y)[EL_NT], int lane, int h) {
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < EL_NT; ++q)
    if (lane + 64 * q < h) s = fma((double)x[q], (double)y[q], s);
  return s;
}

__device__ __forceinline__ void el_load_row(const float *__restrict__ p, int lane, int h, float (&x)[EL_NT]) {
#pragma unroll
  for (int q = 0; q < EL_NT; ++q) x[q] = lane + 64 * q < h ? p[lane + 64 * q] : 0.f;
}

// norm = sqrt((float)sum of squares), a = w / max(norm, 1e-12): written for the wave's row
__device__ __forceinline__ void el_normalize_row(const float (&w)[EL_NT], int lane, int h, float *__restrict__ arow,
                                                 float *__restrict__ norm_out) {
  const float ss = (float)el_wave_sum(el_lane_dot(w, w, lane, h));
  const float nrm = sqrtf(ss);
  const float d = fmaxf(nrm, EL_TINY);
#pragma unroll
  for (int q = 0; q < EL_NT; ++q)
    if (lane + 64 * q < h) arow[lane + 64 * q] = __fdiv_rn(w[q], d);
  if (lane == 0) *norm_out = nrm;
}

// ------------------------------------------------------------------ normalize
__global__ __launch_bounds__(256) void elsa_normalize_kernel(const float *__restrict__ W, int64_t ldw, int n, int h,
                                                             float *__restrict__ A, int64_t lda,
                                                             float *__restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  float w[EL_NT];
  el_load_row(W + j * ldw, lane, h, w);
  el_normalize_row(w, lane, h, A + j * lda, norms + j);
}

// At[k][j] = A[j][k]: a 64 x 64 tile through LDS, reads and writes both along rows
__global__ __launch_bounds__(256) void elsa_transpose_kernel(const float *__restrict__ A, int64_t lda, int n, int h,
                                                             float *__restrict__ At, int64_t ldt) {
  __shared__ float tile[64][65];
  const int64_t j0 = (int64_t)blockIdx.x * 64;
  const int k0 = blockIdx.y * 64;
  const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  for (int r = r0; r < 64; r += 4)
    tile[r][c] = (j0 + r < n && k0 + c < h) ? A[(j0 + r) * lda + k0 + c] : 0.f;
  __syncthreads();
  for (int r = r0; r < 64; r += 4)
    if (k0 + r < h && j0 + c < n) At[(int64_t)(k0 + r) * ldt + j0 + c] = tile[c][r];
}

// ----------------------------------------------------------------------- rows
// A wave per batch row.  Every scalar in float64; E and F rounded to f32 once.
__global__ __launch_bounds__(256) void elsa_rows_kernel(const float *__restrict__ Z, int64_t ldz,
                                                        const float *__restrict__ Q, int64_t ldq,
                                                        const float *__restrict__ t2, int B, int h, double bn,
                                                        float *__restrict__ E, int64_t lde, float *__restrict__ F,
                                                        int64_t ldf, double *__restrict__ row_loss) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= B) return;
  float z[EL_NT], q[EL_NT];
  el_load_row(Z + u * ldz, lane, h, z);
  el_load_row(Q + u * ldq, lane, h, q);
  const double z2 = el_wave_sum(el_lane_dot(z, z, lane, h));
  const double qq = el_wave_sum(el_lane_dot(z, q, lane, h));
  const double t = (double)t2[u];
  const double p2 = (qq - 2.0 * z2) + t;
  bool live = t > 0.0 && p2 > 0.0 && p2 <= 1.7976931348623157e308;     // (a NaN or an infinity is dead)
  double ce = 0.0, b = 0.0, loss = t > 0.0 ? 1.0 : 0.0;
  double c = 0.0;
  if (live) {
    const double sp = sqrt(p2), st = sqrt(t);
    c = (z2 - t) / (sp * st);
    const double a = -2.0 / (bn * sp * st);
    b = 2.0 * c / (bn * p2);
    ce = 2.0 * (a - b);
  }
  double e[EL_NT], f[EL_NT], big = 0.0;
#pragma unroll
  for (int k = 0; k < EL_NT; ++k) {
    e[k] = fma(ce, (double)z[k], b * (double)q[k]);
    f[k] = b * (double)z[k];
    // (fmax drops a NaN, so a NaN is looked for on its own)
    big = (e[k] != e[k] || f[k] != f[k]) ? 1.0 / 0.0 : fmax(big, fmax(fabs(e[k]), fabs(f[k])));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) big = fmax(big, __shfl_xor(big, off, 64));
  // a row whose E or F would leave the f32 range (a p2 next to nothing) is dead as well: nothing written is not finite
  live = live && big <= 3.4028234663852886e38;
  if (live) loss = 2.0 - 2.0 * c;
#pragma unroll
  for (int k = 0; k < EL_NT; ++k)
    if (lane + 64 * k < h) {
      // (a dead row writes +0 whatever Z and Q hold, a NaN included)
      E[u * lde + lane + 64 * k] = live ? (float)e[k] : 0.f;
      F[u * ldf + lane + 64 * k] = live ? (float)f[k] : 0.f;
    }
  if (lane == 0) row_loss[u] = loss;
}

// acc[0] += (sum of row_loss[0 .. B)) / bn: thread t sums the rows t, t + 256, .. ascending, then a pairwise tree
__global__ __launch_bounds__(256) void elsa_loss_kernel(const double *__restrict__ row_loss, int B, double bn,
                                                        double *__restrict__ acc) {
  __shared__ double s[256];
  double v = 0.0;
  for (int u = threadIdx.x; u < B; u += 256) v += row_loss[u];
  s[threadIdx.x] = v;
  for (int d = 128; d > 0; d >>= 1) {
    __syncthreads();
    if (threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
  }
  if (threadIdx.x == 0) acc[0] += s[0] / bn;
}

// -------------------------------------------------------------------- scatter
// the first entry of [e0, e1) whose index is >= key (indices ascending)
__device__ __forceinline__ int64_t el_lower_bound(const int32_t *__restrict__ idx, int64_t e0, int64_t e1, int key) {
  while (e0 < e1) {
    const int64_t mid = e0 + ((e1 - e0) >> 1);
    if (idx[mid] < key) e0 = mid + 1;
    else e1 = mid;
  }
  return e0;
}

template <int VEC> struct ElVec;
template <> struct ElVec<1> {
  typedef float T;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T fma(float x, T v, T a) { return fmaf(x, v, a); }
};
template <> struct ElVec<4> {
  typedef float4 T;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T fma(float x, T v, T a) {
    return make_float4(fmaf(x, v.x, a.x), fmaf(x, v.y, a.y), fmaf(x, v.z, a.z), fmaf(x, v.w, a.w));
  }
};

// A wave per item j; lane l owns the column chunks l, l + 64, .. of VEC columns.  The (position, value) pairs of the
// range are fetched 64 at a time and handed round by shuffles, so that the walk pays one latency per E row.
template <int VEC>
__global__ __launch_bounds__(256) void elsa_scatter_kernel(const int64_t *__restrict__ t_indptr,
                                                           const int32_t *__restrict__ t_indices,
                                                           const float *__restrict__ t_data, int n, int lo, int hi,
                                                           const float *__restrict__ E, int64_t lde, int h,
                                                           float *__restrict__ G, int64_t ldg) {
  typedef typename ElVec<VEC>::T V;
  constexpr int NT = EL_NT / VEC;                       // 8 scalar chunks or 2 float4 chunks
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;                                   // (a whole wave leaves)
  const int64_t r0 = t_indptr[j], r1 = t_indptr[j + 1];
  const int64_t a = el_lower_bound(t_indices, r0, r1, lo), b = el_lower_bound(t_indices, a, r1, hi);
  if (b - a >= EL_LONG) return;                         // (the long kernel's)
  const int nch = h / VEC;                              // (VEC 4: h is a multiple of 4)
  V acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = ElVec<VEC>::zero();
  for (int64_t eb = a; eb < b; eb += 64) {
    const int cnt = b - eb < 64 ? (int)(b - eb) : 64;
    int p = 0;
    float x = 0.f;
    if (lane < cnt) {
      p = t_indices[eb + lane] - lo;
      x = t_data ? t_data[eb + lane] : 1.f;
    }
    for (int l = 0; l < cnt; ++l) {
      const int pl = __shfl(p, l, 64);
      const float xl = __shfl(x, l, 64);
      const V *row = (const V *)(E + (int64_t)pl * lde);
#pragma unroll
      for (int q = 0; q < NT; ++q)
        if (lane + 64 * q < nch) acc[q] = ElVec<VEC>::fma(xl, row[lane + 64 * q], acc[q]);
    }
  }
  V *out = (V *)(G + j * ldg);
#pragma unroll
  for (int q = 0; q < NT; ++q)
    if (lane + 64 * q < nch) out[lane + 64 * q] = acc[q];
}

// Workgroups of 512 threads over the long items.  Workgroup b owns the items b, b + gridDim.x, ..; it looks at 512 of
// them at a time, a thread each (the row's length first: a row shorter than EL_LONG needs no search), and lists the
// long ones in ascending order through LDS (ballots and a prefix over the waves: a fixed order, no atomics), so the
// looking costs n / (512 gridDim.x) rounds and the rest follows the long rows' entries.  A listed item is summed by
// the whole workgroup: thread t owns column t, the (position, value) pairs go through LDS 512 at a time.
__global__ __launch_bounds__(EL_LONG_THREADS) void elsa_scatter_long_kernel(
    const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_indices, const float *__restrict__ t_data,
    int n, int lo, int hi, const float *__restrict__ E, int64_t lde, int h, float *__restrict__ G, int64_t ldg) {
  __shared__ int ps[EL_LONG_THREADS];
  __shared__ float xs[EL_LONG_THREADS];
  __shared__ int64_t la[EL_LONG_THREADS], lb[EL_LONG_THREADS];
  __shared__ int lj[EL_LONG_THREADS];
  __shared__ int wcnt[EL_LONG_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t stride = gridDim.x;
  for (int64_t base = 0; blockIdx.x + stride * base < n; base += EL_LONG_THREADS) {     // (workgroup-uniform throughout)
    const int64_t j = blockIdx.x + stride * (base + t);
    bool is_long = false;
    int64_t a = 0, b = 0;
    if (j < n) {
      const int64_t r0 = t_indptr[j], r1 = t_indptr[j + 1];
      if (r1 - r0 >= EL_LONG) {
        a = el_lower_bound(t_indices, r0, r1, lo);
        b = el_lower_bound(t_indices, a, r1, hi);
        is_long = b - a >= EL_LONG;
      }
    }
    const unsigned long long mask = __ballot(is_long);
    if (lane == 0) wcnt[wv] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < EL_LONG_THREADS / 64; ++w) {
      if (w < wv) off += wcnt[w];
      total += wcnt[w];
    }
    if (is_long) {
      const int k = off + __popcll(mask & ((1ull << lane) - 1ull));
      lj[k] = (int)j;
      la[k] = a;
      lb[k] = b;
    }
    __syncthreads();
    for (int i = 0; i < total; ++i) {
      const int64_t jj = lj[i], ea = la[i], ee = lb[i];
      float acc = 0.f;
      for (int64_t eb = ea; eb < ee; eb += EL_LONG_THREADS) {
        const int cnt = ee - eb < EL_LONG_THREADS ? (int)(ee - eb) : EL_LONG_THREADS;
        __syncthreads();                                         // (the previous chunk has been read)
        if (t < cnt) {
          ps[t] = t_indices[eb + t] - lo;
          xs[t] = t_data ? t_data[eb + t] : 1.f;
        }
        __syncthreads();
        if (t < h) {
          const float *col = E + t;
#pragma unroll 8
          for (int l = 0; l < cnt; ++l) acc = fmaf(xs[l], col[(int64_t)ps[l] * lde], acc);
        }
      }
      if (t < h) G[jj * ldg + t] = acc;
    }
    __syncthreads();                                             // (the next round reuses the list)
  }
}

// -------------------------------------------------------------- project, adam
// g[k] = (dA[k] - dot A[k]) / max(norm, 1e-12) with dot = (float)<dA, A> (float64 chains): an fmaf, a divide
__device__ __forceinline__ void el_project_row(const float (&da)[EL_NT], const float (&a)[EL_NT], float nrm, int lane,
                                               int h, float (&g)[EL_NT]) {
  const float dot = (float)el_wave_sum(el_lane_dot(da, a, lane, h));
  const float d = fmaxf(nrm, EL_TINY);
#pragma unroll
  for (int q = 0; q < EL_NT; ++q) g[q] = __fdiv_rn(fmaf(-dot, a[q], da[q]), d);
}

__global__ __launch_bounds__(256) void elsa_project_kernel(const float *__restrict__ dA, int64_t ldd,
                                                           const float *__restrict__ A, int64_t lda,
                                                           const float *__restrict__ norms, int n, int h,
                                                           float *__restrict__ dW, int64_t ldw) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  float da[EL_NT], a[EL_NT], g[EL_NT];
  el_load_row(dA + j * ldd, lane, h, da);
  el_load_row(A + j * lda, lane, h, a);
  el_project_row(da, a, norms[j], lane, h, g);
#pragma unroll
  for (int q = 0; q < EL_NT; ++q)
    if (lane + 64 * q < h) dW[j * ldw + lane + 64 * q] = g[q];
}

__global__ __launch_bounds__(256) void elsa_adam_kernel(float *__restrict__ W, int64_t ldw,
                                                        const float *__restrict__ dA, int64_t ldd,
                                                        float *__restrict__ A, int64_t lda,
                                                        float *__restrict__ norms, float *__restrict__ M,
                                                        float *__restrict__ Vv, int n, int h, float beta1,
                                                        float beta2, float omb1, float omb2, float eps, float step,
                                                        float isb2) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  float da[EL_NT], a[EL_NT], g[EL_NT], w[EL_NT];
  el_load_row(dA + j * ldd, lane, h, da);
  el_load_row(A + j * lda, lane, h, a);
  el_load_row(W + j * ldw, lane, h, w);
  el_project_row(da, a, norms[j], lane, h, g);
#pragma unroll
  for (int q = 0; q < EL_NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) {
      const int64_t x = j * (int64_t)h + k;                     // (the moments are packed [n, h])
      const float m = fmaf(beta1, M[x], __fmul_rn(omb1, g[q]));
      const float v = fmaf(beta2, Vv[x], __fmul_rn(__fmul_rn(omb2, g[q]), g[q]));
      M[x] = m;
      Vv[x] = v;
      w[q] = fmaf(-step, __fdiv_rn(m, fmaf(sqrtf(v), isb2, eps)), w[q]);
      W[j * ldw + k] = w[q];
    } else {
      w[q] = 0.f;
    }
  }
  el_normalize_row(w, lane, h, A + j * lda, norms + j);
}

// -------------------------------------------------------------------- csr sub
__global__ __launch_bounds__(256) void ease_csr_sub_kernel(const int64_t *__restrict__ indptr,
                                                           const int32_t *__restrict__ indices,
                                                           const float *__restrict__ data, int n_rows, int lo, int hi,
                                                           float *__restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_rows) return;
  const int64_t e0 = indptr[u], e1 = indptr[u + 1];
  for (int64_t e = e0 + lane; e < e1; e += 64) {                // (the items of a row are distinct: no two lanes meet)
    const int j = indices[e];
    if (j >= lo && j < hi) {
      float *o = out + u * ldo + (j - lo);
      *o = __fsub_rn(*o, data ? data[e] : 1.f);
    }
  }
}

inline unsigned el_row_grid(int64_t rows) { return (unsigned)((rows + 3) / 4); }

}  // namespace

// ------------------------------------------------------------------------ ABI
extern "C" {

int rk_ease_elsa_normalize(const float *W, int64_t ldw, int32_t n, int32_t h, float *A, int64_t lda, float *norms,
                           float *At, int64_t ldt, void *stream) {
  RK_SIDE_REQUIRE(W && A && norms, "null pointer");
  RK_SIDE_REQUIRE(n >= 1 && h >= 1 && h <= EL_MAX_H && ldw >= h && lda >= h, "n >= 1, 1 <= h <= 512, ldw, lda >= h");
  RK_SIDE_REQUIRE(!At || ldt >= n, "ldt >= n");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(elsa_normalize_kernel, dim3(el_row_grid(n)), dim3(256), 0, s, W, ldw, n, h, A, lda, norms);
  if (At)
    hipLaunchKernelGGL(elsa_transpose_kernel, dim3((n + 63) / 64, (h + 63) / 64), dim3(256), 0, s, A, lda, n, h, At,
                       ldt);
  RK_SIDE_CHECK_LAUNCH("rk_ease_elsa_normalize");
  return 0;
}

int rk_ease_elsa_rows(const float *Z, int64_t ldz, const float *Q, int64_t ldq, const float *t2, int32_t B, int32_t h,
                      int32_t n, float *E, int64_t lde, float *F, int64_t ldf, double *row_loss, double *loss_acc,
                      void *stream) {
  RK_SIDE_REQUIRE(B >= 0 && n >= 1 && h >= 1 && h <= EL_MAX_H, "B >= 0, n >= 1, 1 <= h <= 512");
  RK_SIDE_REQUIRE(ldz >= h && ldq >= h && lde >= h && ldf >= h, "ldz, ldq, lde, ldf >= h");
  if (B == 0) return 0;
  RK_SIDE_REQUIRE(Z && Q && t2 && E && F && row_loss, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const double bn = (double)B * (double)n;
  hipLaunchKernelGGL(elsa_rows_kernel, dim3(el_row_grid(B)), dim3(256), 0, s, Z, ldz, Q, ldq, t2, B, h, bn, E, lde, F,
                     ldf, row_loss);
  if (loss_acc) hipLaunchKernelGGL(elsa_loss_kernel, dim3(1), dim3(256), 0, s, row_loss, B, bn, loss_acc);
  RK_SIDE_CHECK_LAUNCH("rk_ease_elsa_rows");
  return 0;
}

int rk_ease_elsa_scatter(const int64_t *t_indptr, const int32_t *t_indices, const float *t_data, int32_t n, int32_t lo,
                         int32_t hi, const float *E, int64_t lde, int32_t h, float *G, int64_t ldg, void *stream) {
  RK_SIDE_REQUIRE(t_indptr && t_indices && G, "null pointer");
  RK_SIDE_REQUIRE(n >= 1 && h >= 1 && h <= EL_MAX_H && ldg >= h, "n >= 1, 1 <= h <= 512, ldg >= h");
  RK_SIDE_REQUIRE(0 <= lo && lo <= hi, "0 <= lo <= hi");
  RK_SIDE_REQUIRE(lo == hi || (E && lde >= h), "E must be given with lde >= h");
  hipStream_t s = (hipStream_t)stream;
  // 16-byte accesses when every row of E and G starts on a 16-byte boundary and holds whole float4s
  const bool vec = h % 4 == 0 && ldg % 4 == 0 && (uintptr_t)G % 16 == 0 &&
                   (lo == hi || (lde % 4 == 0 && (uintptr_t)E % 16 == 0));
  if (vec)
    hipLaunchKernelGGL(elsa_scatter_kernel<4>, dim3(el_row_grid(n)), dim3(256), 0, s, t_indptr, t_indices, t_data, n,
                       lo, hi, E, lde, h, G, ldg);
  else
    hipLaunchKernelGGL(elsa_scatter_kernel<1>, dim3(el_row_grid(n)), dim3(256), 0, s, t_indptr, t_indices, t_data, n,
                       lo, hi, E, lde, h, G, ldg);
  if (hi - lo >= EL_LONG)                                       // (a shorter range has no long item)
    hipLaunchKernelGGL(elsa_scatter_long_kernel, dim3(n < EL_LONG_GRID ? n : EL_LONG_GRID), dim3(EL_LONG_THREADS), 0,
                       s, t_indptr, t_indices, t_data, n, lo, hi, E, lde, h, G, ldg);
  RK_SIDE_CHECK_LAUNCH("rk_ease_elsa_scatter");
  return 0;
}

int rk_ease_elsa_project(const float *dA, int64_t ldd, const float *A, int64_t lda, const float *norms, int32_t n,
                         int32_t h, float *dW, int64_t ldw, void *stream) {
  RK_SIDE_REQUIRE(dA && A && norms && dW, "null pointer");
  RK_SIDE_REQUIRE(n >= 1 && h >= 1 && h <= EL_MAX_H && ldd >= h && lda >= h && ldw >= h,
                  "n >= 1, 1 <= h <= 512, ldd, lda, ldw >= h");
  hipLaunchKernelGGL(elsa_project_kernel, dim3(el_row_grid(n)), dim3(256), 0, (hipStream_t)stream, dA, ldd, A, lda,
                     norms, n, h, dW, ldw);
  RK_SIDE_CHECK_LAUNCH("rk_ease_elsa_project");
  return 0;
}

int rk_ease_elsa_adam(float *W, int64_t ldw, const float *dA, int64_t ldd, float *A, int64_t lda, float *norms,
                      float *M, float *V, int32_t n, int32_t h, float beta1, float beta2, float eps, float step,
                      float isb2, void *stream) {
  RK_SIDE_REQUIRE(W && dA && A && norms && M && V, "null pointer");
  RK_SIDE_REQUIRE(n >= 1 && h >= 1 && h <= EL_MAX_H && ldw >= h && ldd >= h && lda >= h,
                  "n >= 1, 1 <= h <= 512, ldw, ldd, lda >= h");
  RK_SIDE_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f && step > 0.f && isb2 > 0.f,
                  "0 <= beta < 1, eps, step, isb2 > 0");
  hipLaunchKernelGGL(elsa_adam_kernel, dim3(el_row_grid(n)), dim3(256), 0, (hipStream_t)stream, W, ldw, dA, ldd, A,
                     lda, norms, M, V, n, h, beta1, beta2, 1.f - beta1, 1.f - beta2, eps,
                     step, isb2);
  RK_SIDE_CHECK_LAUNCH("rk_ease_elsa_adam");
  return 0;
}

int rk_ease_csr_sub(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows, int32_t lo,
                    int32_t hi, float *out, int64_t ldo, void *stream) {
  RK_SIDE_REQUIRE(n_rows >= 0 && 0 <= lo && lo <= hi && ldo >= hi - lo, "n_rows >= 0, 0 <= lo <= hi, ldo >= hi - lo");
  if (n_rows == 0 || lo == hi) return 0;
  RK_SIDE_REQUIRE(indptr && indices && out, "null pointer");
  hipLaunchKernelGGL(ease_csr_sub_kernel, dim3(el_row_grid(n_rows)), dim3(256), 0, (hipStream_t)stream, indptr,
                     indices, data, n_rows, lo, hi, out, ldo);
  RK_SIDE_CHECK_LAUNCH("rk_ease_csr_sub");
  return 0;
}

}  // extern "C"
