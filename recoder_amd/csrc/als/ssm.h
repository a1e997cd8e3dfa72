#pragma once
#include "common.h"

namespace {

// ------------------------------------------------------------------------ ssm
// The sampled softmax over the T slots of a step and C = T + S candidate columns (rk_als_ssm_grad).  Column c < T
// is slot c's positive item, column T + n the n-th shared negative: item = draw32(key, 0, n_items) with key a
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
    const uint64_t key = mix64(seed_key ^ (((uint64_t)step << 32) | SSM_TAG | (uint32_t)(c - T)));
    id = (int)draw32(key, 0, (uint32_t)n_items);
    ok = true;
  }
  float a[NT];
  load_row<NT>(user ? X : Y, user ? ldx : ldy, id, h, lane, ok, a);
  float inv = ok ? 1.f : 0.f;
  if (cosine) {
    const float ss = wave_dot<NT>(a, a);
    inv = ss > 0.f ? 1.f / sqrtf(ss) : 0.f;
#pragma unroll
    for (int q = 0; q < NT; ++q) a[q] *= inv;
  }
  store_row<NT>(user ? w.Zu : w.Zc, h, user ? r : c, h, lane, a);
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
  const float inv = user ? w.invu[x] : w.invc[x];        // (0 for an invalid row, and for a zero row of the cosine)
  float z[NT], d[NT];
  load_row<NT>(user ? w.Zu : w.Zc, h, x, h, lane, true, z);
  load_row<NT>(user ? w.dA : w.dB, h, x, h, lane, true, d);
#pragma unroll
  for (int q = 0; q < NT; ++q) d[q] *= inv_tau;
  const float zd = cosine ? wave_dot<NT>(z, d) : 0.f;
#pragma unroll
  for (int q = 0; q < NT; ++q) d[q] = inv > 0.f ? (cosine ? fmaf(-zd, z[q], d[q]) * inv : d[q]) : 0.f;
  store_row<NT>(user ? DU : DC, h, x, h, lane, d);
}

}  // namespace

extern "C" int64_t rk_als_ssm_workspace_bytes(int32_t T, int32_t S, int32_t h) {
  if (T < 1 || T > SSM_MAX_T || S < 0 || S > SSM_MAX_S || h < 1 || h > MAX_H) return -2;
  return ssm_ws_floats(T, (int64_t)T + S, h, nullptr, nullptr) * (int64_t)sizeof(float);
}

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
  const dim3 all_rows((unsigned)((T + C + 3) / 4));
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL(als_ssm_gather_kernel<decltype(nt)::value>, all_rows, dim3(256), 0, st, users, items, T, S,
                       n_users, n_items, mix64((uint64_t)seed), (uint32_t)step, X, ldx, Y, ldy, h, cosine, corr, w, cand,
                       valid, cvalid);
  });
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
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL(als_ssm_write_kernel<decltype(nt)::value>, all_rows, dim3(256), 0, st, T, C, h, inv_tau, cosine,
                       w, DU, DC);
  });
  RK_SIDE_CHECK_LAUNCH("als_ssm_write");
  return 0;
}
