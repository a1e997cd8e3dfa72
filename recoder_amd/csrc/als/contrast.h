#pragma once
#include "common.h"

namespace {

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
  load_row<NT>(V1, ld1, key, h, lane, act, a);
  load_row<NT>(V2, ld2, key, h, lane, act, b);
  const float sa = wave_dot<NT>(a, a), sb = wave_dot<NT>(b, b);
  const float ia = sa > 0.f ? 1.f / sqrtf(sa) : 0.f, ib = sb > 0.f ? 1.f / sqrtf(sb) : 0.f;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    a[q] *= ia;
    b[q] *= ib;
  }
  store_row<NT>(w.Z1, h, t, h, lane, a);
  store_row<NT>(w.Z2, h, t, h, lane, b);
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
    load_row<NT>(Z, h, t, h, lane, true, z);
    load_row<NT>(dZ, h, t, h, lane, true, d);
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
  load_row<NT>(X, ldx, u, h, lane, ok, a);
  load_row<NT>(Y, ldy, i, h, lane, ok, b);
  const float sa = wave_dot<NT>(a, a), sb = wave_dot<NT>(b, b);
  const float ia = sa > 0.f ? 1.f / sqrtf(sa) : 0.f, ib = sb > 0.f ? 1.f / sqrtf(sb) : 0.f;
  float d[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    a[q] *= ia;
    b[q] *= ib;
    d[q] = a[q] - b[q];
  }
  store_row<NT>(w.Z1, h, t, h, lane, a);
  store_row<NT>(w.Z2, h, t, h, lane, b);
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
    float z[NT], d[NT];
    load_row<NT>(Z, h, t, h, lane, true, z);
    load_row<NT>(dZ, h, t, h, lane, true, d);
    const float zd = wave_dot<NT>(z, d);
#pragma unroll
    for (int q = 0; q < NT; ++q) d[q] = fmaf(-zd, z[q], d[q]) * inv;
    store_row<NT>(side ? DI : DU, h, t, h, lane, d);
  }
}

}  // namespace

extern "C" int64_t rk_als_gcl_contrast_workspace_bytes(int32_t T, int32_t h) {
  if (T < 1 || T > GCL_MAX_T || h < 1 || h > MAX_H) return -2;
  return gcl_ws_floats(T, h, nullptr, nullptr) * (int64_t)sizeof(float);
}

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
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL(als_gcl_gather_kernel<decltype(nt)::value>, waves, dim3(256), 0, st, keys, T, n_rows, V1, ld1,
                       V2, ld2, h, w);
  });
  RK_SIDE_CHECK_LAUNCH("als_gcl_gather");
  hipLaunchKernelGGL((als_gcl_gemm_kernel<GCL_SCORES, GCL_TILE>), dim3(tt, tt), dim3(256), 0, st, T, h, tau, count, w);
  hipLaunchKernelGGL(als_gcl_lse_kernel, waves, dim3(256), 0, st, T, w);
  hipLaunchKernelGGL(als_gcl_loss_kernel, dim3(1), dim3(256), 0, st, T, w, loss, count);
  hipLaunchKernelGGL((als_gcl_gemm_kernel<GCL_DZ1, GCL_DZ_ROWS>), dim3(th, td), dim3(256), 0, st, T, h, tau, count, w);
  hipLaunchKernelGGL((als_gcl_gemm_kernel<GCL_DZ2, GCL_DZ_ROWS>), dim3(th, td), dim3(256), 0, st, T, h, tau, count, w);
  RK_SIDE_CHECK_LAUNCH("als_gcl_gemm");
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL(als_gcl_write_kernel<decltype(nt)::value>, waves, dim3(256), 0, st, keys, T, h, weight, w, G1,
                       ldg1, G2, ldg2);
  });
  RK_SIDE_CHECK_LAUNCH("als_gcl_write");
  return 0;
}

extern "C" int64_t rk_als_dau_workspace_bytes(int32_t T, int32_t h) {
  if (T < 1 || T > GCL_MAX_T || h < 1 || h > MAX_H) return -2;
  return (gcl_ws_floats(T, h, nullptr, nullptr) + 64) * (int64_t)sizeof(float);
}

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
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL(als_dau_gather_kernel<decltype(nt)::value>, waves, dim3(256), 0, st, users, items, T, n_users,
                       n_items, X, ldx, Y, ldy, h, wu, valid);
  });
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
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL(als_dau_write_kernel<decltype(nt)::value>, waves, dim3(256), 0, st, T, h, wu, DU, DI);
  });
  RK_SIDE_CHECK_LAUNCH("als_dau_write");
  return 0;
}
