#pragma once
#include "ccl.h"

namespace {

// -------------------------------------------------------------------- simplex
// SimpleX's history-pooled user rows under ccl.h's loss (rk_als_sx_forward, rk_als_sx_backward).
//
// Forward: one wave per slot, four slots a workgroup.  The slot's history H_u is the whole stored row (r <= L) or the
// entries at floor(j r / L), j < L, in 64-bit integers.  Lane l reads the item of entry j0 + l of a chunk of 64 and
// writes that entry of the list (hkey / hcoef: rk_als_ccl_scatter's layout); the rows are then gathered SX_UNROLL at
// a time, the ids by __shfl, and added in ascending j: one plain f32 add chain per column from +0, then one multiply
// by 1.f / |H|.  The pooled rows of the workgroup's four slots wait in LDS while W goes through a 64 x 64 LDS tile
// (pitch 65: lane a reads row a conflict-free) that the four waves load together, coalesced, and each wave runs the
// chain s_a = fmaf(W[a, c], b[c], s_a) over c ascending for its own slot; X = fmaf(gamma, p, (1.f - gamma) s).
constexpr int SX_MAX_HISTORY = RK_ALS_SX_MAX_HISTORY, SX_CHUNK = RK_ALS_SX_CHUNK;
constexpr int SX_UNROLL = 4;                      // history rows gathered before any is added
constexpr int SX_TILE = 64, SX_PITCH = SX_TILE + 1;
constexpr int SX_BT = 4;                          // slots a wave of the dB kernel takes: one read of W serves them all

template <int NT>
__global__ __launch_bounds__(256) void als_sx_forward_kernel(
    const int32_t *__restrict__ users, int T, const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
    int n_users, int n_items, const float *__restrict__ Q, int ldq, const float *__restrict__ P, int ldp,
    const float *__restrict__ W, int ldw, int h, float gamma, int L, int E, float *__restrict__ B,
    float *__restrict__ X, int ldx, int compact, int32_t *__restrict__ hkey, float *__restrict__ hcoef) {
  __shared__ float tile[SX_TILE * SX_PITCH];
  __shared__ float bs[4][64 * NT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int t = blockIdx.x * 4 + wv;
  const int u = t < T ? users[t] : -1;
  const bool ok = u >= 0 && u < n_users;          // (wave-uniform; no wave leaves before the last barrier)
  float b[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) b[q] = 0.f;
  int listed = 0;                                 // entries of the list written so far
  if (ok) {
    const int64_t e0 = indptr[u], r = indptr[u + 1] - e0;
    const int cnt = r <= 0 ? 0 : (r < (int64_t)L ? (int)r : L);
    const float inv = cnt > 0 ? 1.f / (float)cnt : 0.f;
    listed = hkey ? min(cnt, E) : 0;
    float acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = 0.f;
    for (int j0 = 0; j0 < cnt; j0 += 64) {
      const int j = j0 + lane;
      int id = n_items;                           // (n_items: no entry here, or an id that is no item)
      if (j < cnt) {
        const int64_t pos = r <= (int64_t)L ? (int64_t)j : (int64_t)j * r / (int64_t)L;
        const int v = indices[e0 + pos];
        if (v >= 0 && v < n_items) id = v;
      }
      if (j < listed) {
        hkey[(int64_t)t * E + j] = id;
        hcoef[(int64_t)t * E + j] = id < n_items ? inv : 0.f;
      }
      const int here = min(64, cnt - j0);
      for (int r0 = 0; r0 < here; r0 += SX_UNROLL) {
        float y[SX_UNROLL][NT];
#pragma unroll
        for (int g = 0; g < SX_UNROLL; ++g) {
          const int cg = __shfl(id, (r0 + g) & 63, 64);
#pragma unroll
          for (int q = 0; q < NT; ++q) {
            const int k = lane + 64 * q;
            y[g][q] = (r0 + g < here && cg < n_items && k < h) ? Q[(int64_t)cg * ldq + k] : 0.f;
          }
        }
#pragma unroll
        for (int g = 0; g < SX_UNROLL; ++g) {
          if (r0 + g < here) {                    // (wave-uniform: a tail entry must not touch the chain)
#pragma unroll
            for (int q = 0; q < NT; ++q) acc[q] += y[g][q];
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) b[q] = acc[q] * inv;
  }
  if (t < T) {
    if (hkey) {
      for (int e = listed + lane; e < E; e += 64) {
        hkey[(int64_t)t * E + e] = n_items;
        hcoef[(int64_t)t * E + e] = 0.f;
      }
    }
    if (B) store_row<NT>(B, h, t, h, lane, b);
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) bs[wv][lane + 64 * q] = b[q];      // (+0 past h and for a slot that is none)
  float s[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    s[q] = 0.f;
    if (64 * q < h) {                             // (workgroup-uniform, as the barriers below need)
      for (int c0 = 0; c0 < h; c0 += SX_TILE) {
        __syncthreads();                          // (the tile's last readers are done; bs is written)
        for (int i = wv * 16; i < wv * 16 + 16; ++i) {
          const int a = 64 * q + i, c = c0 + lane;
          tile[i * SX_PITCH + lane] = (a < h && c < h) ? W[(int64_t)a * ldw + c] : 0.f;
        }
        __syncthreads();
        const int cn = min(SX_TILE, h - c0);
        for (int cc = 0; cc < cn; ++cc) s[q] = fmaf(tile[lane * SX_PITCH + cc], bs[wv][c0 + cc], s[q]);
      }
    }
  }
  if (t >= T || (!ok && !compact)) return;
  const float og = 1.f - gamma;
  const int64_t xr = compact ? t : u;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) {
      const float p = (ok && P) ? P[(int64_t)u * ldp + k] : 0.f;
      X[xr * ldx + k] = ok ? fmaf(gamma, p, og * s[q]) : 0.f;
    }
  }
}

// dB[t, c] = scale sum_a W[a, c] DU[t, a]: lane c + 64 q, one fmaf chain over a ascending from +0 per element; a wave
// takes SX_BT slots, so that a row of W is read once for them.  An invalid slot's row is +0.
template <int NT>
__global__ __launch_bounds__(256) void als_sx_db_kernel(const float *__restrict__ DU, const float *__restrict__ valid,
                                                        int T, const float *__restrict__ W, int ldw, int h,
                                                        float scale, float *__restrict__ dB) {
  const int lane = threadIdx.x & 63;
  const int t0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * SX_BT;
  if (t0 >= T) return;
  float acc[SX_BT][NT];
  bool live[SX_BT];
#pragma unroll
  for (int i = 0; i < SX_BT; ++i) {
    live[i] = t0 + i < T && valid[t0 + i] > 0.f;
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[i][q] = 0.f;
  }
#pragma unroll 2
  for (int a = 0; a < h; ++a) {
    float w[NT];
    load_row<NT>(W, ldw, a, h, lane, true, w);
#pragma unroll
    for (int i = 0; i < SX_BT; ++i) {
      const float d = live[i] ? DU[(int64_t)(t0 + i) * h + a] : 0.f;
#pragma unroll
      for (int q = 0; q < NT; ++q) acc[i][q] = fmaf(w[q], d, acc[i][q]);
    }
  }
#pragma unroll
  for (int i = 0; i < SX_BT; ++i) {
    if (t0 + i < T) {
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const int k = lane + 64 * q;
        if (k < h) dB[(int64_t)(t0 + i) * h + k] = live[i] ? scale * acc[i][q] : 0.f;
      }
    }
  }
}

// part[ch, a, c] = sum over the valid slots t of chunk ch (SX_CHUNK consecutive slots) of DU[t, a] B[t, c]: one fmaf
// chain over t ascending from +0.  Workgroup (ch, a-tile of 16, c-tile of 64): wave w holds the rows a0 + 4 w .. + 3,
// lane l the column c0 + l.
__global__ __launch_bounds__(256) void als_sx_dw_part_kernel(const float *__restrict__ DU,
                                                             const float *__restrict__ valid,
                                                             const float *__restrict__ B, int T, int h,
                                                             float *__restrict__ part) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ch = blockIdx.x, a0 = blockIdx.y * 16 + wv * 4, c = blockIdx.z * 64 + lane;
  const int t_lo = ch * SX_CHUNK, t_hi = min(T, t_lo + SX_CHUNK);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int t = t_lo; t < t_hi; ++t) {
    const bool v = valid[t] > 0.f;
    const float bv = c < h ? B[(int64_t)t * h + c] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float d = (v && a0 + i < h) ? DU[(int64_t)t * h + a0 + i] : 0.f;
      acc[i] = fmaf(d, bv, acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (c < h && a0 + i < h) part[((int64_t)ch * h + a0 + i) * h + c] = acc[i];
}

// dW = scale (part[0] + part[1] + ...), the chunks in ascending order: whatever the grid of the launch above was
__global__ __launch_bounds__(256) void als_sx_dw_sum_kernel(const float *__restrict__ part, int chunks, int h,
                                                            float scale, float *__restrict__ dW) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= h * h) return;
  float s = part[idx];
  for (int ch = 1; ch < chunks; ++ch) s += part[(int64_t)ch * h * h + idx];
  dW[idx] = scale * s;
}

}  // namespace

extern "C" int64_t rk_als_sx_workspace_bytes(int32_t T, int32_t E, int32_t h) {
  if (T < 1 || T > RK_ALS_CCL_MAX_BATCH || E < 1 || E > SX_MAX_HISTORY || h < 1 || h > MAX_H) return -2;
  const int64_t n = (int64_t)T * E;
  if (n > RK_ALS_CCL_MAX_ENTRIES) return -2;
  const int64_t chunks = (T + SX_CHUNK - 1) / SX_CHUNK;
  return 2 * round256(4 * (int64_t)T * h) + 2 * round256(4 * n) + round256(4 * chunks * h * h) +
         round256(4 * (int64_t)h * h);
}

extern "C" int rk_als_sx_forward(const int32_t *users, int32_t T, const int64_t *indptr, const int32_t *indices,
                                 int32_t n_users, int32_t n_items, const float *Q, int32_t ldq, const float *P,
                                 int32_t ldp, const float *W, int32_t ldw, int32_t h, float gamma,
                                 int32_t max_history, int32_t E, float *B, float *X, int32_t ldx, int32_t compact,
                                 int32_t *hkey, float *hcoef, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldq >= h && ldw >= h && ldx >= h && (!P || ldp >= h),
                  "1 <= h <= 512, ldq, ldp, ldw, ldx >= h");
  RK_SIDE_REQUIRE(T >= 1 && T <= RK_ALS_CCL_MAX_BATCH && max_history >= 1 && max_history <= SX_MAX_HISTORY &&
                      E >= 1 && E <= SX_MAX_HISTORY && (int64_t)T * E <= RK_ALS_CCL_MAX_ENTRIES,
                  "1 <= T <= 4096, 1 <= max_history <= 1024, 1 <= E <= 1024, T E <= 2^22");
  RK_SIDE_REQUIRE(n_users >= 1 && n_items >= 1, "n_users, n_items >= 1");
  RK_SIDE_REQUIRE(gamma >= 0.f && gamma <= 1.f, "0 <= gamma <= 1");
  RK_SIDE_REQUIRE(users && indptr && indices && Q && W && X, "null pointer");
  RK_SIDE_REQUIRE((hkey == nullptr) == (hcoef == nullptr), "hkey and hcoef go together");
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL((als_sx_forward_kernel<decltype(nt)::value>), dim3((unsigned)((T + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, users, T, indptr, indices, n_users, n_items, Q, ldq, P, ldp, W, ldw, h,
                       gamma, max_history, E, B, X, ldx, compact, hkey, hcoef);
  });
  RK_SIDE_CHECK_LAUNCH("als_sx_forward");
  return 0;
}

extern "C" int rk_als_sx_backward(const float *DU, const float *valid, const float *B, int32_t T, const float *W,
                                  int32_t ldw, int32_t h, float scale, float *dB, float *part, float *dW,
                                  void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldw >= h, "1 <= h <= 512, ldw >= h");
  RK_SIDE_REQUIRE(T >= 1 && T <= RK_ALS_CCL_MAX_BATCH, "1 <= T <= 4096");
  RK_SIDE_REQUIRE(DU && valid && B && W && dB && part && dW, "null pointer");
  const int chunks = (T + SX_CHUNK - 1) / SX_CHUNK;
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL((als_sx_db_kernel<decltype(nt)::value>), dim3((unsigned)((T + 4 * SX_BT - 1) / (4 * SX_BT))),
                       dim3(256), 0, (hipStream_t)stream, DU, valid, T, W, ldw, h, scale, dB);
  });
  hipLaunchKernelGGL(als_sx_dw_part_kernel, dim3((unsigned)chunks, (unsigned)((h + 15) / 16), (unsigned)((h + 63) / 64)),
                     dim3(256), 0, (hipStream_t)stream, DU, valid, B, T, h, part);
  hipLaunchKernelGGL(als_sx_dw_sum_kernel, dim3((unsigned)((h * h + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     part, chunks, h, scale, dW);
  RK_SIDE_CHECK_LAUNCH("als_sx_backward");
  return 0;
}
