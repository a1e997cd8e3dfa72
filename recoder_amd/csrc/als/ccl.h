#pragma once
#include "ugcn.h"

namespace {

// ------------------------------------------------------------------------ ccl
// SimpleX's cosine contrastive loss (rk_als_ccl_grad): one wave per slot, the user's row normalised once in
// registers (a = p / |p|).  The E = 1 + R candidates go 64 at a time, as in als_ugcn_grad_kernel: lane l prepares
// candidate e0 + l (the positive, or UltraGCN's draw of (seed, step, t R + r) under UGCN_TAG), and the candidates are
// scored UG_G rows of a lane group at a time, the row gathers issued before any is reduced.  Norm and dot product
// come from the one gathered copy of a row: two fmaf chains over the lane's registers, then the xor butterfly of the
// group's W lanes each, so that every lane of the group holds c = (a . y) (1 / sqrt(y . y)) and decides by itself
// whether the candidate is live.  A dead negative is never touched again; a live row (and the positive's) goes
// into the user's gradient while it is in registers: acc_k = fmaf(w / |y|, y_k, acc_k) and sc = fmaf(w, c, sc), in
// ascending e within the group (groups below the wave: group g holds the candidates e = g mod 64 / W of a round, and
// the groups' acc and sc are added in ascending g at the end), DU_k = (acc_k - sc a_k) / |p|.  c and 1 / |y| go back
// to the lane that owns the candidate, which forms key, coef and self and the loss terms: a lane's live negatives
// summed over the chunks in ascending e, then by wave_sum.
template <int NT, int W>
__global__ __launch_bounds__(256) void als_ccl_grad_kernel(
    const int32_t *__restrict__ users, const int32_t *__restrict__ items, int T, int R, uint64_t seed_key,
    uint32_t step, int n_users, int n_items, const float *__restrict__ X, int ldx, const float *__restrict__ Y, int ldy,
    int h, float margin, float neg_scale, int32_t *__restrict__ cand, int32_t *__restrict__ key,
    float *__restrict__ coef, float *__restrict__ self, float *__restrict__ DU, float *__restrict__ valid,
    float *__restrict__ loss, int32_t *__restrict__ live) {
  static_assert(W == 64 || NT == 1, "lane groups below the wave hold one dimension a lane");
  constexpr int C = 64 / W;                       // candidates scored side by side
  constexpr int ROUND = C * UG_G;                 // candidates of one round of gathers (divides 64)
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int E = 1 + R;
  const int u = users[t], i = items[t];
  const bool ok = u >= 0 && u < n_users && i >= 0 && i < n_items;       // (wave-uniform)
  int32_t *crow = cand + (int64_t)t * E, *krow = key + (int64_t)t * E;
  float *frow = coef + (int64_t)t * E, *srow = self + (int64_t)t * E;
  const int sub = lane / W, kk = lane % W;
  if (!ok) {
    for (int e = lane; e < E; e += 64) {
      crow[e] = n_items;
      krow[e] = n_items;
      frow[e] = 0.f;
      srow[e] = 0.f;
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int k = lane + 64 * q;
      if (k < h) DU[(int64_t)t * h + k] = 0.f;
    }
    if (lane == 0) {
      valid[t] = 0.f;
      live[t] = 0;
    }
    if (lane < 2) loss[(int64_t)t * 2 + lane] = 0.f;
    return;
  }
  float a[NT], acc[NT];
  float nu2 = 0.f;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = kk + 64 * q;
    a[q] = k < h ? X[(int64_t)u * ldx + k] : 0.f;
    acc[q] = 0.f;
    nu2 = fmaf(a[q], a[q], nu2);
  }
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) nu2 += __shfl_xor(nu2, off, 64);
  const float inv_nu = nu2 > 0.f ? 1.f / sqrtf(nu2) : 0.f;
#pragma unroll
  for (int q = 0; q < NT; ++q) a[q] *= inv_nu;
  const uint32_t draw0 = (uint32_t)t * (uint32_t)R;
  float sc = 0.f, lpos = 0.f, lneg = 0.f;
  int nlive = 0;
  for (int e0 = 0; e0 < E; e0 += 64) {
    const int e = e0 + lane;
    int id = n_items;                             // (n_items: no candidate here)
    if (e == 0) {
      id = i;
    } else if (e <= R) {
      const uint64_t dk = mix64(seed_key ^ (((uint64_t)step << 32) | UGCN_TAG | (draw0 + (uint32_t)(e - 1))));
      id = (int)draw32(dk, 0, (uint32_t)n_items);
    }
    float mc = 0.f, mi = 0.f;                     // this lane's candidate: its cosine and 1 / its norm
    const int here = min(64, E - e0);
    for (int r0 = 0; r0 < here; r0 += ROUND) {
      int cg[UG_G];
      float y[UG_G][NT], cs[UG_G], iv[UG_G];
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
#pragma unroll
      for (int g = 0; g < UG_G; ++g) {
        float d = 0.f, n2 = 0.f;
#pragma unroll
        for (int q = 0; q < NT; ++q) {
          d = fmaf(a[q], y[g][q], d);
          n2 = fmaf(y[g][q], y[g][q], n2);
        }
#pragma unroll
        for (int off = W / 2; off > 0; off >>= 1) {
          d += __shfl_xor(d, off, 64);
          n2 += __shfl_xor(n2, off, 64);
        }
        iv[g] = n2 > 0.f ? 1.f / sqrtf(n2) : 0.f;
        cs[g] = d * iv[g];
      }
#pragma unroll
      for (int g = 0; g < UG_G; ++g) {            // the user's gradient, from the rows in registers
        const int eg = e0 + r0 + g * C + sub;
        const float w = eg == 0 ? -1.f : ((eg <= R && cs[g] - margin > 0.f) ? neg_scale : 0.f);
        if (w != 0.f && iv[g] > 0.f) {            // (no shuffle below: the lanes of a group agree, the groups need not)
          const float wb = w * iv[g];
#pragma unroll
          for (int q = 0; q < NT; ++q) acc[q] = fmaf(wb, y[g][q], acc[q]);
          sc = fmaf(w, cs[g], sc);
        }
      }
#pragma unroll
      for (int g = 0; g < UG_G; ++g) {            // the cosine and the norm to the lane that owns the candidate
        const int first = r0 + g * C;
        const int from = ((lane - first) & (C - 1)) * W;
        const float vc = __shfl(cs[g], from, 64), vi = __shfl(iv[g], from, 64);
        if ((unsigned)(lane - first) < (unsigned)C) {
          mc = vc;
          mi = vi;
        }
      }
    }
    if (e < E) {
      const bool lv = e >= 1 && mc - margin > 0.f;
      const float w = e == 0 ? -1.f : (lv ? neg_scale : 0.f);
      const bool carries = w != 0.f && mi > 0.f && inv_nu > 0.f;
      crow[e] = id;
      krow[e] = carries ? id : n_items;
      frow[e] = carries ? (w * inv_nu) * mi : 0.f;
      srow[e] = carries ? ((w * mc) * mi) * mi : 0.f;
      if (e == 0) lpos = 1.f - mc;
      else if (lv) {
        lneg += mc - margin;
        ++nlive;
      }
    }
  }
  if (C > 1) {                                    // the groups' sums, in ascending group
    float tot = 0.f, st = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      tot += __shfl(acc[0], c * W + kk, 64);
      st += __shfl(sc, c * W + kk, 64);
    }
    acc[0] = tot;
    sc = st;
  }
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = kk + 64 * q;
    if (sub == 0 && k < h) DU[(int64_t)t * h + k] = fmaf(-sc, a[q], acc[q]) * inv_nu;
  }
  const float sp = wave_sum(lpos), sn = wave_sum(lneg);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nlive += __shfl_xor(nlive, off, 64);
  if (lane == 0) {
    valid[t] = 1.f;
    loss[(int64_t)t * 2] = sp;
    loss[(int64_t)t * 2 + 1] = neg_scale * sn;
    live[t] = nlive;
  }
}

// The sum of self over the sorted positions [s_lo, s_hi), under ugcn_walk's validity of an entry: lane l adds the
// positions s_lo + l + 64 j in ascending j, then wave_sum.
__device__ __forceinline__ float ccl_self_sum(const int64_t *__restrict__ order, int s_lo, int s_hi, int n, int E,
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

// The item side (rk_als_ccl_scatter): als_ugcn_scatter_kernel's hand-out and walk (ugcn_walk) over the sorted keys,
// which end at the first sentinel: a dead entry's key is not below n_rows, so nothing of it is gathered.
template <int NT>
__global__ __launch_bounds__(256) void als_ccl_scatter_kernel(
    const int32_t *__restrict__ keys, const int64_t *__restrict__ order, int n, int E,
    const int32_t *__restrict__ users, const float *__restrict__ coef, const float *__restrict__ self,
    const float *__restrict__ X, int ldx, int n_users, const float *__restrict__ Y, int ldy, int h, float scale,
    int n_rows, float *__restrict__ Gt, int ldg, int32_t *__restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int s0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s0 >= n) return;
  const int key = keys[s0];
  if (key < 0 || key >= n_rows) return;                  // (the sentinels and invalid entries, sorted last)
  if (s0 > 0 && keys[s0 - 1] == key) return;             // (not a head)
  int c = 0;
  for (;;) {
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
  const float ss = ccl_self_sum(order, s0, s0 + c, n, E, users, n_users, self, lane);
  float *row = Gt + (int64_t)key * ldg;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) row[k] = scale * fmaf(-ss, Y[(int64_t)key * ldy + k], acc[q]);
  }
  if (lane == 0) count[key] = cnt;
}

// The long keys, as als_ugcn_scatter_long_kernel hands them out: wave w sums part w of UG_LONG_WAVES equal parts,
// the coefficients' chain and the part's self sum; thread k adds the parts' sums in ascending w.
template <int NT>
__global__ __launch_bounds__(64 * UG_LONG_WAVES) void als_ccl_scatter_long_kernel(
    const int32_t *__restrict__ keys, const int64_t *__restrict__ order, int n, int E,
    const int32_t *__restrict__ users, const float *__restrict__ coef, const float *__restrict__ self,
    const float *__restrict__ X, int ldx, int n_users, const float *__restrict__ Y, int ldy, int h, float scale,
    int n_rows, float *__restrict__ Gt, int ldg, int32_t *__restrict__ count) {
  __shared__ float red[UG_LONG_WAVES][64 * NT];
  __shared__ float selfs[UG_LONG_WAVES];
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
  const float ss = ccl_self_sum(order, p_lo, p_hi, n, E, users, n_users, self, lane);
#pragma unroll
  for (int q = 0; q < NT; ++q) red[wv][lane + 64 * q] = acc[q];
  if (lane == 0) {
    cnts[wv] = cnt;
    selfs[wv] = ss;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < h) {
    float s = red[0][k], st = selfs[0];
    for (int w = 1; w < UG_LONG_WAVES; ++w) {
      s += red[w][k];
      st += selfs[w];
    }
    Gt[(int64_t)key * ldg + k] = scale * fmaf(-st, Y[(int64_t)key * ldy + k], s);
  }
  if (k == 0) {
    int total = 0;
    for (int w = 0; w < UG_LONG_WAVES; ++w) total += cnts[w];
    count[key] = total;
  }
}

}  // namespace

extern "C" int64_t rk_als_ccl_workspace_bytes(int32_t T, int32_t R, int32_t h) {
  if (T < 1 || T > RK_ALS_CCL_MAX_BATCH || R < 1 || R > RK_ALS_CCL_MAX_NEGATIVES || h < 1 || h > MAX_H) return -2;
  const int64_t n = (int64_t)T * (1 + R);
  if (n > RK_ALS_CCL_MAX_ENTRIES) return -2;
  return 4 * round256(4 * n) + round256(4 * 2 * (int64_t)T) + round256(4 * (int64_t)T);
}

extern "C" int rk_als_ccl_grad(const int32_t *users, const int32_t *items, int32_t T, int32_t R, int64_t seed,
                               int32_t step, int32_t n_users, int32_t n_items, const float *X, int32_t ldx,
                               const float *Y, int32_t ldy, int32_t h, float margin, float negative_weight,
                               int32_t *cand, int32_t *key, float *coef, float *self, float *DU, float *valid,
                               float *loss, int32_t *live, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldx >= h && ldy >= h, "1 <= h <= 512, ldx, ldy >= h");
  RK_SIDE_REQUIRE(rk_als_ccl_workspace_bytes(T, R, h) > 0, "1 <= T <= 4096, 1 <= R <= 1024, T (1 + R) <= 2^22");
  RK_SIDE_REQUIRE(n_users >= 1 && n_items >= 1 && step >= 0, "n_users, n_items >= 1, step >= 0");
  RK_SIDE_REQUIRE(users && items && X && Y && cand && key && coef && self && DU && valid && loss && live,
                  "null pointer");
  auto launch = [&](auto nt, auto w) {                   // (w: the lanes of a group, the wave itself above h = 32)
    hipLaunchKernelGGL((als_ccl_grad_kernel<decltype(nt)::value, decltype(w)::value>), dim3((unsigned)((T + 3) / 4)),
                       dim3(256), 0, (hipStream_t)stream, users, items, T, R, mix64((uint64_t)seed), (uint32_t)step,
                       n_users, n_items, X, ldx, Y, ldy, h, margin, negative_weight / (float)R, cand, key, coef, self,
                       DU, valid, loss, live);
  };
  if (h <= 16) launch(Int<1>{}, Int<16>{});
  else if (h <= 32) launch(Int<1>{}, Int<32>{});
  else dispatch_nt(h, [&](auto nt) { launch(nt, Int<64>{}); });
  RK_SIDE_CHECK_LAUNCH("als_ccl_grad");
  return 0;
}

extern "C" int rk_als_ccl_scatter(const int32_t *keys, const int64_t *order, int32_t n, int32_t E,
                                  const int32_t *users, const float *coef, const float *self, const float *X,
                                  int32_t ldx, int32_t n_users, const float *Y, int32_t ldy, int32_t h, float scale,
                                  int32_t n_rows, float *G, int32_t ldg, int32_t *count, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= MAX_H && ldx >= h && ldy >= h && ldg >= h, "1 <= h <= 512, ldx, ldy, ldg >= h");
  RK_SIDE_REQUIRE(E >= 2 && E <= 1 + RK_ALS_CCL_MAX_NEGATIVES && n >= E && n % E == 0 &&
                      n / E <= RK_ALS_CCL_MAX_BATCH && n <= RK_ALS_CCL_MAX_ENTRIES,
                  "n = T E, 2 <= E <= 1025, 1 <= T <= 4096, n <= 2^22");
  RK_SIDE_REQUIRE(n_users >= 1 && n_rows >= 1, "n_users, n_rows >= 1");
  RK_SIDE_REQUIRE(keys && order && users && coef && self && X && Y && G && count, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  dispatch_nt(h, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    hipLaunchKernelGGL(als_ccl_scatter_kernel<NT>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, keys, order, n, E,
                       users, coef, self, X, ldx, n_users, Y, ldy, h, scale, n_rows, G, ldg, count);
    hipLaunchKernelGGL(als_ccl_scatter_long_kernel<NT>, dim3((unsigned)((n + UG_LONG - 1) / UG_LONG)),
                       dim3(64 * UG_LONG_WAVES), 0, st, keys, order, n, E, users, coef, self, X, ldx, n_users, Y, ldy,
                       h, scale, n_rows, G, ldg, count);
  });
  RK_SIDE_CHECK_LAUNCH("als_ccl_scatter");
  return 0;
}
