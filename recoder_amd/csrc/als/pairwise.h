#pragma once
#include "common.h"

namespace {

// ------------------------------------------------------------------------ bpr
constexpr int BPR_MAX_T = 1 << 24;
constexpr int BPR_MAX_DRAWS = 32;

// The start of a slot in both samplers: its key, a hash of (seed, step, slot); draw 0, a stored entry e; the row u
// that holds e -- the last u with indptr[u] <= e (empty rows share their successor's start) -- and its bounds.
struct SlotDraw {
  uint64_t key;
  int64_t e, r0, r1;
  int u;
};

__device__ __forceinline__ SlotDraw slot_draw(const int64_t *__restrict__ indptr, int n_users, uint32_t nnz,
                                              uint64_t seed_key, uint32_t step, int t) {
  SlotDraw s;
  s.key = mix64(seed_key ^ (((uint64_t)step << 32) | (uint32_t)t));
  s.e = (int64_t)draw32(s.key, 0, nnz);
  int lo = 0, hi = n_users;                 // (indptr[lo] <= e < indptr[hi] throughout)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (indptr[mid] <= s.e) lo = mid; else hi = mid;
  }
  s.u = lo;
  s.r0 = indptr[lo], s.r1 = indptr[lo + 1];
  return s;
}

// whether the row [r0, r1) of ascending indices holds c: the first position with indices[.] >= c
__device__ __forceinline__ bool row_holds(const int32_t *__restrict__ indices, int64_t r0, int64_t r1, int c) {
  int64_t a = r0, b = r1;
  while (a < b) {
    const int64_t mid = a + ((b - a) >> 1);
    if (indices[mid] < c) a = mid + 1; else b = mid;
  }
  return a < r1 && indices[a] == c;
}

__global__ __launch_bounds__(256) void als_bpr_sample_kernel(const int64_t *__restrict__ indptr,
                                                             const int32_t *__restrict__ indices, int n_users,
                                                             int n_items, uint32_t nnz, uint64_t seed_key,
                                                             uint32_t step, int T, int32_t *__restrict__ users,
                                                             int32_t *__restrict__ pos, int32_t *__restrict__ neg) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const SlotDraw s = slot_draw(indptr, n_users, nnz, seed_key, step, t);
  int j = -1;
  for (int d = 1; d <= BPR_MAX_DRAWS; ++d) {
    const int c = (int)draw32(s.key, (uint32_t)d, (uint32_t)n_items);
    if (!row_holds(indices, s.r0, s.r1, c)) {
      j = c;
      break;
    }
  }
  users[t] = s.u;
  pos[t] = indices[s.e];
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
  float p[NT], d[NT], qj[NT];
  load_row<NT>(X, ldx, u, h, lane, ok, p);
  load_row<NT>(Y, ldy, i, h, lane, ok, d);
  load_row<NT>(Y, ldy, j, h, lane, ok, qj);
#pragma unroll
  for (int q = 0; q < NT; ++q) d[q] -= qj[q];
  store_row<NT>(D, h, t, h, lane, d);
  store_row<NT>(P, h, t, h, lane, p);
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
  const SlotDraw sd = slot_draw(indptr, n_users, nnz, seed_key, step, t);
  const int u = sd.u, i = indices[sd.e];
  const bool ok = i >= 0 && i < n_items;    // (a column outside the table: the slot is invalid, nothing is read)
  float p[NT], q0[NT];
  load_row<NT>(X, ldx, u, h, lane, ok, p);
  load_row<NT>(Y, ldy, i, h, lane, ok, q0);
  const float sp = ok ? wave_dot<NT>(p, q0) + bias[i] : 0.f;
  int j = -1, n_scored = 0;
  float sn = 0.f;
  bool done = !ok;
  for (int d0 = 1; d0 <= max_draws; d0 += 64) {
    const int d = d0 + lane;
    int c = 0;
    bool cand = false;
    if (!done && d <= max_draws) {
      c = (int)draw32(sd.key, (uint32_t)d, (uint32_t)n_items);
      cand = !row_holds(indices, sd.r0, sd.r1, c);
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
  float p[NT], qi[NT], qj[NT], d[NT];
  load_row<NT>(X, ldx, u, h, lane, ok, p);
  load_row<NT>(Y, ldy, i, h, lane, ok, qi);
  load_row<NT>(Y, ldy, j, h, lane, ok, qj);
#pragma unroll
  for (int q = 0; q < NT; ++q) d[q] = qi[q] - qj[q];
  store_row<NT>(D, h, t, h, lane, d);
  store_row<NT>(P, h, t, h, lane, p);
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

// The segment walk (segment_head, segment_sum of common.h) with the table's own update as its ending: the
// slot's negative enters with -g, and with c the segment's length
//   new_k = fmaf(lr, fmaf(-(reg * c), old_k, acc_k), old_k)           (the bias likewise, V = 1)
template <int NT>
__global__ __launch_bounds__(256) void als_bpr_apply_kernel(const int32_t *__restrict__ keys,
                                                            const int64_t *__restrict__ order, int n, int roles,
                                                            const float *__restrict__ g,
                                                            const float *__restrict__ V, int h, float lr,
                                                            float reg, int n_rows, float *__restrict__ table,
                                                            int ldt, float *__restrict__ bias) {
  const int lane = threadIdx.x & 63;
  const int s0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  int key, c;
  if (!segment_head(keys, n, n_rows, s0, lane, key, c)) return;
  float acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = 0.f;
  const float bacc = segment_sum<NT, false>(order, s0, c, n, roles, g, V, h, lane, acc);
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

}  // namespace

extern "C" int64_t rk_als_bpr_workspace_bytes(int32_t T, int32_t h) {
  if (T < 1 || T > BPR_MAX_T || h < 1 || h > MAX_H) return -2;
  return 5 * round256((int64_t)T * 4) + 2 * round256((int64_t)T * h * 4);
}

extern "C" int rk_als_bpr_sample(const int64_t *indptr, const int32_t *indices, int32_t n_users, int32_t n_items,
                                 int64_t nnz, int64_t seed, int32_t step, int32_t T, int32_t *users, int32_t *pos,
                                 int32_t *neg, void *stream) {
  RK_SIDE_REQUIRE(n_users >= 1 && n_items >= 1, "n_users >= 1, n_items >= 1");
  RK_SIDE_REQUIRE(nnz >= 1 && nnz < ((int64_t)1 << 31), "1 <= nnz < 2^31");
  RK_SIDE_REQUIRE(step >= 0 && T >= 1 && T <= BPR_MAX_T, "step >= 0, 1 <= T <= 2^24");
  RK_SIDE_REQUIRE(indptr && indices && users && pos && neg, "null pointer");
  hipLaunchKernelGGL(als_bpr_sample_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     indptr, indices, n_users, n_items, (uint32_t)nnz, mix64((uint64_t)seed), (uint32_t)step, T,
                     users, pos, neg);
  RK_SIDE_CHECK_LAUNCH("als_bpr_sample");
  return 0;
}

extern "C" int rk_als_bpr_grad(const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t T,
                               int32_t n_users, int32_t n_items, const float *X, int32_t ldx, const float *Y,
                               int32_t ldy, const float *bias, int32_t h, float *g, float *loss, float *x, float *D,
                               float *P, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldx >= h && ldy >= h, "1 <= h <= 512, ldx >= h, ldy >= h");
  RK_SIDE_REQUIRE(T >= 1 && T <= BPR_MAX_T && n_users >= 1 && n_items >= 1, "1 <= T <= 2^24, n_users, n_items >= 1");
  RK_SIDE_REQUIRE(users && pos && neg && X && Y && bias && g && loss && D && P, "null pointer");
  const dim3 grid((unsigned)((T + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL(als_bpr_grad_kernel<decltype(nt)::value>, grid, dim3(256), 0, st, users, pos, neg, T, n_users,
                       n_items, X, ldx, Y, ldy, bias, h, g, loss, x, D, P);
  });
  RK_SIDE_CHECK_LAUNCH("als_bpr_grad");
  return 0;
}

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
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL(als_bpr_apply_kernel<decltype(nt)::value>, grid, dim3(256), 0, st, keys, order, n, roles, g, V,
                       h, lr, reg, n_rows, table, ldt, bias);
  });
  RK_SIDE_CHECK_LAUNCH("als_bpr_apply");
  return 0;
}

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
  dispatch_nt(h, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    constexpr int G = NT <= 2 ? 8 : 4;      // the candidates whose rows are in flight together: 8 of h <= 128, else 4
    hipLaunchKernelGGL((als_rank_sample_kernel<NT, G>), grid, dim3(256), 0, st, indptr, indices, n_users, n_items,
                       (uint32_t)nnz, mix64((uint64_t)seed), (uint32_t)step, T, X, ldx, Y, ldy, bias, h, mode,
                       max_draws, num_candidates, margin, users, pos, neg, trials, s_pos, s_neg, scores);
  });
  RK_SIDE_CHECK_LAUNCH("als_rank_sample");
  return 0;
}

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
  dispatch_nt(h, [&](auto nt) {
    hipLaunchKernelGGL(als_warp_grad_kernel<decltype(nt)::value>, grid, dim3(256), 0, st, users, pos, neg, trials, T,
                       n_users, n_items, X, ldx, Y, ldy, bias, h, margin, weight, g, loss, D, P);
  });
  RK_SIDE_CHECK_LAUNCH("als_warp_grad");
  return 0;
}
