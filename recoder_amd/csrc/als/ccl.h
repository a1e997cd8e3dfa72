#pragma once
#include "ugcn.h"

namespace {

// ------------------------------------------------------------------------ ccl
// SimpleX's cosine contrastive loss (rk_als_ccl_grad): one wave per slot, the user's row normalised once in
// registers (a = p / |p|).  The E = 1 + R candidates go 64 at a time through ugcn.h's candidate round: lane l prepares
// candidate e0 + l (the positive, or UltraGCN's draw: entry_draw), and the candidates are scored UG_G rows of a lane
// group at a time (entry_gather), the row gathers issued before any is reduced.  Norm and dot product
// come from the one gathered copy of a row: two fmaf chains over the lane's registers, then the xor butterfly of the
// group's W lanes each, so that every lane of the group holds c = (a . y) (1 / sqrt(y . y)) and decides by itself
// whether the candidate is live.  A dead negative is never touched again; a live row (and the positive's) goes
// into the user's gradient while it is in registers: acc_k = fmaf(w / |y|, y_k, acc_k) and sc = fmaf(w, c, sc), in
// ascending e within the group (groups below the wave: group g holds the candidates e = g mod 64 / W of a round, and
// the groups' acc and sc are added in ascending g at the end), DU_k = (acc_k - sc a_k) / |p|.  c and 1 / |y| go back
// to the lane that owns the candidate, which forms key, coef and self and the loss terms: a lane's live negatives
// summed over the chunks in ascending e, then by wave_sum.
// The item side (rk_als_ccl_scatter) has no kernel here: it is ugcn.h's entry scatter with SELF.
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
      id = entry_draw(seed_key, step, draw0, e, n_items);
    }
    float mc = 0.f, mi = 0.f;                     // this lane's candidate: its cosine and 1 / its norm
    const int here = min(64, E - e0);
    for (int r0 = 0; r0 < here; r0 += ROUND) {
      float y[UG_G][NT], cs[UG_G], iv[UG_G];
      entry_gather<NT, W>(id, r0, lane, Y, ldy, n_items, h, y);
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
      entry_to_owner<W>(cs, r0, lane, mc);        // the cosine and the norm to the lane that owns the candidate
      entry_to_owner<W>(iv, r0, lane, mi);
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
  auto launch = [&](auto nt, auto w) {
    hipLaunchKernelGGL((als_ccl_grad_kernel<decltype(nt)::value, decltype(w)::value>), dim3((unsigned)((T + 3) / 4)),
                       dim3(256), 0, (hipStream_t)stream, users, items, T, R, mix64((uint64_t)seed), (uint32_t)step,
                       n_users, n_items, X, ldx, Y, ldy, h, margin, negative_weight / (float)R, cand, key, coef, self,
                       DU, valid, loss, live);
  };
  dispatch_group(h, launch);
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
  // (the keys end at the first sentinel: a dead entry's key is not below n_rows, so nothing of it is gathered)
  entry_scatter<true>(keys, order, n, E, users, coef, self, X, ldx, n_users, Y, ldy, h, scale, n_rows, G, ldg, count,
                      stream);
  RK_SIDE_CHECK_LAUNCH("als_ccl_scatter");
  return 0;
}
