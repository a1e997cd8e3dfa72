#pragma once
#include "common.h"

namespace {

// ----------------------------------------------------------------------- ugcn
// UltraGCN's constraint loss (rk_als_ugcn_grad): one wave per slot, p_u in registers.  The E = 1 + R + K candidates
// go 64 at a time: lane l prepares candidate e0 + l -- the positive, a draw (entry_draw) or a neighbour of the
// positive -- with its weight a and the sign of its logit.  The candidates are then scored a round at a time
// (entry_gather, entry_to_owner: the candidate round below, which als_ccl_grad_kernel of ccl.h runs too).  A score
// goes back to the lane that owns the candidate, which forms coef = sign a sigma(sign s); the owners' coefs come back
// to the groups, and DU takes coef y in ascending e (fmaf at W = 64; the groups' products one after the other below
// that).  The loss terms are formed once per 64 candidates, a lane each, and summed per lane over the chunks, then by
// wave_sum.
//
// This file also holds what every loss with private per-slot negatives shares: the candidate round of its grad kernel
// and the item side's entry scatter (als_entry_scatter_kernel and its long-key partner, launched by entry_scatter),
// which rk_als_ugcn_scatter and rk_als_ccl_scatter both are.
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

// ------------------------------------------------------------ candidate round
// A slot's wave is 64 / W lane groups of W lanes (W = 16 or 32 at h <= 16 or 32, a dimension a lane; else the wave,
// NT dimensions a lane: dispatch_group).  Lane l owns candidate e0 + l of a chunk of 64; a round scores
// ROUND = UG_G 64 / W of them, group sub taking the candidates r0 + g 64 / W + sub (g < UG_G), their UG_G rows
// gathered before any is reduced.
//
// Negative r (candidate e = 1 + r) of slot t: draw32 of a key that hashes (seed, step, t R + r), whose low word
// carries the tag 0xA0000000 (a sampler slot is below 2^24, SimGCL's noise has the top byte 0x80, the sampled
// softmax's shared draws 0xC0); draw0 = t R.
__device__ __forceinline__ int entry_draw(uint64_t seed_key, uint32_t step, uint32_t draw0, int e, int n_items) {
  const uint64_t key = mix64(seed_key ^ (((uint64_t)step << 32) | UGCN_TAG | (draw0 + (uint32_t)(e - 1))));
  return (int)draw32(key, 0, (uint32_t)n_items);
}

// y[g] = this lane's dimensions of the row of the g-th candidate of its group in the round at r0: the ids come from
// the owners by __shfl; +0 for an id that is no item (n_items: no candidate there) and past h.
template <int NT, int W>
__device__ __forceinline__ void entry_gather(int id, int r0, int lane, const float *__restrict__ Y, int ldy,
                                             int n_items, int h, float (&y)[UG_G][NT]) {
  constexpr int C = 64 / W;
  const int sub = lane / W, kk = lane % W;
  int cg[UG_G];
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
}

// mine = s[g] of the group that scored this lane's candidate, for the owners of the round at r0 (every lane of a
// group holds the same s[g]); the other lanes keep theirs.
template <int W>
__device__ __forceinline__ void entry_to_owner(const float (&s)[UG_G], int r0, int lane, float &mine) {
  constexpr int C = 64 / W;
#pragma unroll
  for (int g = 0; g < UG_G; ++g) {
    const int first = r0 + g * C;
    const float v = __shfl(s[g], ((lane - first) & (C - 1)) * W, 64);
    if ((unsigned)(lane - first) < (unsigned)C) mine = v;
  }
}

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
      id = entry_draw(seed_key, step, draw0, e, n_items);
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
      float y[UG_G][NT], s[UG_G];
      entry_gather<NT, W>(id, r0, lane, Y, ldy, n_items, h, y);
#pragma unroll
      for (int g = 0; g < UG_G; ++g) {
        float d = 0.f;
#pragma unroll
        for (int q = 0; q < NT; ++q) d = fmaf(p[q], y[g][q], d);
#pragma unroll
        for (int off = W / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
        s[g] = d;
      }
      entry_to_owner<W>(s, r0, lane, ms);         // the score to the lane that owns the candidate
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

// -------------------------------------------------------------- entry scatter
// The item side (rk_als_ugcn_scatter; with SELF, rk_als_ccl_scatter) over the n = T E entries sorted by key.
// acc_k = fmaf(coef[e], X[users[e / E], k], acc_k) over the sorted positions [s_lo, s_hi) from what acc holds,
// SEG_UNROLL user rows gathered before any is added; cnt counts the positives.
template <int NT>
__device__ __forceinline__ void ugcn_walk(const int64_t *__restrict__ order, int s_lo, int s_hi, int n, int E,
                                          const int32_t *__restrict__ users, int n_users,
                                          const float *__restrict__ coef, const float *__restrict__ X, int ldx, int h,
                                          int lane, float (&acc)[NT], int &cnt) {
  for (int a0 = s_lo; a0 < s_hi; a0 += SEG_UNROLL) {
    float v[SEG_UNROLL][NT], w[SEG_UNROLL];
#pragma unroll
    for (int r = 0; r < SEG_UNROLL; ++r) {
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
    for (int r = 0; r < SEG_UNROLL; ++r) {
      if (a0 + r < s_hi) {
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[q] = fmaf(w[r], v[r][q], acc[q]);
      }
    }
  }
}

// The sum of self over the sorted positions [s_lo, s_hi), under ugcn_walk's validity of an entry: lane l adds the
// positions s_lo + l + 64 j in ascending j, then wave_sum.
__device__ __forceinline__ float entry_self_sum(const int64_t *__restrict__ order, int s_lo, int s_hi, int n, int E,
                                                const int32_t *__restrict__ users, int n_users,
                                                const float *__restrict__ self, int lane) {
  float ss = 0.f;
  for (int s = s_lo + lane; s < s_hi; s += 64) {
    const int64_t e = order[s];
    const bool in = e >= 0 && e < n;
    const uint32_t ee = in ? (uint32_t)e : 0u;
    const int u = in ? users[ee / (uint32_t)E] : -1;
    ss += (u >= 0 && u < n_users) ? self[ee] : 0.f;
  }
  return wave_sum(ss);
}

// als_lgcn_scatter_kernel's hand-out: one wave per sorted position, the wave at the head of a segment of equal keys
// owns that row.  A segment of UG_LONG entries or more is left to als_entry_scatter_long_kernel.  The keys end at the
// first one outside [0, n_rows): absent and invalid entries and, with SELF, the dead ones, of which nothing is
// gathered.  The row is scale acc; with SELF (self, Y and ldy are read only then) it is
// scale fmaf(-ss, Y[key], acc), ss the run's entry_self_sum, taken after the walk.
template <int NT, bool SELF>
__global__ __launch_bounds__(256) void als_entry_scatter_kernel(
    const int32_t *__restrict__ keys, const int64_t *__restrict__ order, int n, int E,
    const int32_t *__restrict__ users, const float *__restrict__ coef, const float *__restrict__ self,
    const float *__restrict__ X, int ldx, int n_users, const float *__restrict__ Y, int ldy, int h, float scale,
    int n_rows, float *__restrict__ Gt, int ldg, int32_t *__restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int s0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s0 >= n) return;
  const int key = keys[s0];
  if (key < 0 || key >= n_rows) return;                  // (sorted last)
  if (s0 > 0 && keys[s0 - 1] == key) return;             // (not a head)
  int c = 0;
  for (;;) {                                             // segment_head's scan, leaving once the key is a long one
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
  float ss = 0.f;
  if constexpr (SELF) ss = entry_self_sum(order, s0, s0 + c, n, E, users, n_users, self, lane);
  float *row = Gt + (int64_t)key * ldg;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) {
      if constexpr (SELF) row[k] = scale * fmaf(-ss, Y[(int64_t)key * ldy + k], acc[q]);
      else row[k] = scale * acc[q];
    }
  }
  if (lane == 0) count[key] = cnt;
}

// The long keys: a segment of c >= UG_LONG equal keys holds a position that is a multiple of UG_LONG; workgroup b
// looks at position b UG_LONG, finds the ends of its segment in the sorted keys and takes the segment when that
// position is the first such multiple in it.  Wave w sums part w of UG_LONG_WAVES equal parts (the last may be
// shorter or empty): the coefficients' chain and, with SELF, the part's entry_self_sum after it; thread k adds the
// parts' sums in ascending w.
template <int NT, bool SELF>
__global__ __launch_bounds__(64 * UG_LONG_WAVES) void als_entry_scatter_long_kernel(
    const int32_t *__restrict__ keys, const int64_t *__restrict__ order, int n, int E,
    const int32_t *__restrict__ users, const float *__restrict__ coef, const float *__restrict__ self,
    const float *__restrict__ X, int ldx, int n_users, const float *__restrict__ Y, int ldy, int h, float scale,
    int n_rows, float *__restrict__ Gt, int ldg, int32_t *__restrict__ count) {
  __shared__ float red[UG_LONG_WAVES][64 * NT];
  __shared__ float selfs[UG_LONG_WAVES];                 // (SELF only)
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
  const int p_lo = min(s_lo + wv * part, s_hi), p_hi = min(s_lo + (wv + 1) * part, s_hi);
  float acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = 0.f;
  int cnt = 0;
  ugcn_walk<NT>(order, p_lo, p_hi, n, E, users, n_users, coef, X, ldx, h, lane, acc, cnt);
#pragma unroll
  for (int q = 0; q < NT; ++q) red[wv][lane + 64 * q] = acc[q];
  if (lane == 0) cnts[wv] = cnt;
  if constexpr (SELF) {
    const float ss = entry_self_sum(order, p_lo, p_hi, n, E, users, n_users, self, lane);
    if (lane == 0) selfs[wv] = ss;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < h) {
    float s = red[0][k];
    for (int w = 1; w < UG_LONG_WAVES; ++w) s += red[w][k];
    if constexpr (SELF) {
      float st = selfs[0];
      for (int w = 1; w < UG_LONG_WAVES; ++w) st += selfs[w];
      s = fmaf(-st, Y[(int64_t)key * ldy + k], s);
    }
    Gt[(int64_t)key * ldg + k] = scale * s;
  }
  if (k == 0) {
    int total = 0;
    for (int w = 0; w < UG_LONG_WAVES; ++w) total += cnts[w];
    count[key] = total;
  }
}

// The two launches of an entry scatter; the entry point has checked its arguments (self and Y null without SELF).
template <bool SELF>
void entry_scatter(const int32_t *keys, const int64_t *order, int n, int E, const int32_t *users, const float *coef,
                   const float *self, const float *X, int ldx, int n_users, const float *Y, int ldy, int h,
                   float scale, int n_rows, float *G, int ldg, int32_t *count, void *stream) {
  dispatch_nt(h, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    hipLaunchKernelGGL((als_entry_scatter_kernel<NT, SELF>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, keys, order, n, E, users, coef, self, X, ldx, n_users, Y, ldy, h, scale,
                       n_rows, G, ldg, count);
    hipLaunchKernelGGL((als_entry_scatter_long_kernel<NT, SELF>), dim3((unsigned)((n + UG_LONG - 1) / UG_LONG)),
                       dim3(64 * UG_LONG_WAVES), 0, (hipStream_t)stream, keys, order, n, E, users, coef, self, X, ldx,
                       n_users, Y, ldy, h, scale, n_rows, G, ldg, count);
  });
}

}  // namespace

extern "C" int64_t rk_als_ugcn_workspace_bytes(int32_t T, int32_t R, int32_t K, int32_t h) {
  if (T < 1 || T > UG_MAX_T || R < 1 || R > UG_MAX_R || K < 0 || K > UG_MAX_K || h < 1 || h > MAX_H) return -2;
  const int64_t n = (int64_t)T * (1 + R + K);
  if (n > UG_MAX_ENTRIES) return -2;
  return 2 * round256(4 * n) + round256(4 * 3 * (int64_t)T);
}

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
  auto launch = [&](auto nt, auto w) {
    hipLaunchKernelGGL((als_ugcn_grad_kernel<decltype(nt)::value, decltype(w)::value>), dim3((unsigned)((T + 3) / 4)),
                       dim3(256), 0, (hipStream_t)stream, users, items, T, R, K, mix64((uint64_t)seed), (uint32_t)step,
                       n_users, n_items, X, ldx, Y, ldy, h, bu, bi, nbr_ids, nbr_w, w1, w2, w3, w4,
                       negative_weight / (float)R, item_weight, cand, coef, DU, valid, loss);
  };
  dispatch_group(h, launch);
  RK_SIDE_CHECK_LAUNCH("als_ugcn_grad");
  return 0;
}

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
  entry_scatter<false>(keys, order, n, E, users, coef, nullptr, X, ldx, n_users, nullptr, 0, h, scale, n_rows, G, ldg,
                       count, stream);
  RK_SIDE_CHECK_LAUNCH("als_ugcn_scatter");
  return 0;
}
