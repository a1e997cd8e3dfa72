#pragma once
#include "common.h"
#include "pairwise.h"       // (BPR_MAX_T: the scatter takes the apply's keys)

namespace {

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
  return mix64(mix64((uint64_t)seed) ^ (((uint64_t)(uint32_t)step << 32) | low));
}

__device__ __forceinline__ uint64_t gcl_row_key(uint64_t key, int64_t r) { return mix64(key + (uint64_t)r); }

__device__ __forceinline__ uint32_t gcl_m(uint64_t row_key, int col) {
  return ((uint32_t)(mix64(row_key + (uint64_t)(uint32_t)col) >> 41) << 1) | 1u;
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
  int key, c;
  if (!segment_head(keys, n, n_rows, s0, lane, key, c)) return;
  float acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = 0.f;
  segment_sum<NT, true>(order, s0, c, n, roles, g, V, h, lane, acc);
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] *= scale;
  store_row<NT>(Gt, ldg, key, h, lane, acc);
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

}  // namespace

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
  auto launch = [&](auto vec_c, auto nt_c) {
    constexpr int VEC = decltype(vec_c)::value, NT = decltype(nt_c)::value;
    hipLaunchKernelGGL((als_lgcn_propagate_kernel<VEC, NT, NOISE>), grid, dim3(256), 0, st, indptr, indices,
                       row_scale, col_scale, row_lo, row_hi, F, ldf, h, G, Out, ldo, Acc, lda, acc_scale, nz);
    hipLaunchKernelGGL((als_lgcn_propagate_long_kernel<VEC, NT, NOISE>), long_grid, dim3(LG_LONG_THREADS), lds, st,
                       indptr, indices, row_scale, col_scale, row_lo, row_hi, F, ldf, h, G, Out, ldo, Acc, lda,
                       acc_scale, nz);
  };
  if (!vec) dispatch_nt(h, [&](auto nt_c) { launch(Int<1>{}, nt_c); });      // (NT >= the nt above)
  else if (nt == 1) launch(Int<4>{}, Int<1>{});
  else launch(Int<4>{}, Int<2>{});
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
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL(als_lgcn_scatter_kernel<decltype(nt)::value>, grid, dim3(256), 0, st, keys, order, n, roles, g,
                       V, h, scale, n_rows, G, ldg, count);
  });
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
