// What the three explanation kernels share (rk_ease_explain, rk_slim_explain, rk_als_explain): the order of the
// candidates, a wave's selection of its XP_MAX_M best, the in-order chains of `total`, and the one-wave kernel of the
// item-item models, which ease.hip and slim.hip instantiate with their own way of fetching W[i][j].  Device code
// only; like side_error.h it is included by translation units that each end up in a library of their own.
//
// A candidate is (value, position in the user's CSR row).  The order, best first:
//   a number before a NaN before an empty slot; among numbers the larger value (so -0 and +0 tie); then the smaller
//   position.  Positions are distinct, so the order is strict and a candidate's rank is a count.
// Selection: the wave keeps 64 slots in LDS, sorted.  A chunk of up to 64 new candidates goes beside them, every lane
// counts how many of the 128 come before its kept and its new candidate, and those of rank < 64 are stored at their
// rank.  Nothing depends on how many chunks a row makes or on m: the first m slots are the answer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int XP_MAX_M = 64;
constexpr int XP_EMPTY = 0x40000000;              // positions from here on are empty slots
constexpr int XP_LDS_WORDS = 256;                 // a wave's slots: 128 values, then 128 positions

// LDS written by one lane of the wave is read by another: order the wave's own accesses (no s_barrier: waves of one
// workgroup select independently, with different trip counts)
__device__ __forceinline__ void xp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool xp_before(float av, int ap, float bv, int bp) {
  const int ca = ap >= XP_EMPTY ? 2 : (av != av ? 1 : 0), cb = bp >= XP_EMPTY ? 2 : (bv != bv ? 1 : 0);
  if (ca != cb) return ca < cb;
  if (ca == 0 && av != bv) return av > bv;
  return ap < bp;
}

__device__ __forceinline__ void xp_init(float *sv, int *sp, int lane) {
  sv[lane] = 0.f;
  sp[lane] = XP_EMPTY + lane;
}

// the lane's candidate (c, pos), pos < 0: none, merged into the kept 64
__device__ __forceinline__ void xp_merge(float *sv, int *sp, int lane, float c, int pos) {
  sv[64 + lane] = c;
  sp[64 + lane] = pos >= 0 ? pos : XP_EMPTY + 64 + lane;
  xp_wave_sync();
  const float av = sv[lane], bv = sv[64 + lane];
  const int ap = sp[lane], bp = sp[64 + lane];
  int ra = 0, rb = 0;
  for (int i = 0; i < 128; ++i) {
    const float x = sv[i];
    const int p = sp[i];
    ra += xp_before(x, p, av, ap) ? 1 : 0;
    rb += xp_before(x, p, bv, bp) ? 1 : 0;
  }
  xp_wave_sync();
  if (ra < 64) {
    sv[ra] = av;
    sp[ra] = ap >= XP_EMPTY ? XP_EMPTY + ra : ap;     // (empty slots are renumbered: positions stay distinct)
  }
  if (rb < 64) {
    sv[rb] = bv;
    sp[rb] = bp >= XP_EMPTY ? XP_EMPTY + rb : bp;
  }
  xp_wave_sync();
}

// the first m slots as ids and values: row_ids the user's CSR indices; padding -1 / +0
__device__ __forceinline__ void xp_write(const float *sv, const int *sp, int lane, int m,
                                         const int32_t *__restrict__ row_ids, int64_t *__restrict__ contributors,
                                         float *__restrict__ contributions) {
  xp_wave_sync();
  if (lane < m) {
    const int p = sp[lane];
    const bool real = p < XP_EMPTY;
    contributors[lane] = real ? (int64_t)row_ids[p] : -1;
    contributions[lane] = real ? sv[lane] : 0.f;
  }
}

__device__ __forceinline__ float xp_lane(float x, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}

// total = fmaf(x_l, w_l, total) over the lanes l < cnt in order: one chain, whatever lane holds what
__device__ __forceinline__ float xp_chain_fma(float total, float x, float w, int cnt) {
  for (int l = 0; l < cnt; ++l) total = fmaf(xp_lane(x, l), xp_lane(w, l), total);
  return total;
}

// total = total + c_l over the lanes l < cnt in order
__device__ __forceinline__ float xp_chain_add(float total, float c, int cnt) {
  for (int l = 0; l < cnt; ++l) total = total + xp_lane(c, l);
  return total;
}

// One wave per (user, target) of an item-item model; fetch(i, j) = W[i][j].  XP_FLIGHT chunks of 64 entries are
// gathered before the first is used, so a lane has that many strided reads in flight.
constexpr int XP_FLIGHT = 4;

template <class Fetch>
__global__ __launch_bounds__(64) void xp_item_kernel(const int64_t *__restrict__ indptr,
                                                     const int32_t *__restrict__ indices,
                                                     const float *__restrict__ data, int n_items,
                                                     const int64_t *__restrict__ items, int J, int m, Fetch fetch,
                                                     int64_t *__restrict__ contributors,
                                                     float *__restrict__ contributions, float *__restrict__ baseline,
                                                     float *__restrict__ total) {
#pragma clang fp contract(off)                    // the contribution is a rounded product; the chain is written as fmaf
  __shared__ float sv[XP_LDS_WORDS];
  int *sp = (int *)(sv + 128);
  const int lane = threadIdx.x;
  const int64_t pair = blockIdx.x, u = pair / J;
  const int64_t j64 = items[pair];
  const bool real = j64 >= 0 && j64 < n_items;
  const int j = real ? (int)j64 : 0;
  const int64_t e0 = indptr[u];
  const int n = real ? (int)(indptr[u + 1] - e0) : 0;
  float tot = 0.f;
  xp_init(sv, sp, lane);
  for (int c0 = 0; c0 < n; c0 += 64 * XP_FLIGHT) {
    float x[XP_FLIGHT], w[XP_FLIGHT];
#pragma unroll
    for (int a = 0; a < XP_FLIGHT; ++a) {
      const int e = c0 + a * 64 + lane;
      x[a] = 0.f, w[a] = 0.f;
      if (e < n) {
        const int i = indices[e0 + e];
        x[a] = data ? data[e0 + e] : 1.f;
        if ((unsigned)i < (unsigned)n_items) w[a] = fetch(i, j);
      }
    }
#pragma unroll
    for (int a = 0; a < XP_FLIGHT; ++a) {
      const int b0 = c0 + a * 64, cnt = min(64, n - b0);
      if (cnt > 0) {
        tot = xp_chain_fma(tot, x[a], w[a], cnt);
        xp_merge(sv, sp, lane, x[a] * w[a], lane < cnt ? b0 + lane : -1);
      }
    }
  }
  xp_write(sv, sp, lane, real ? m : 0, indices + e0, contributors + pair * m, contributions + pair * m);
  if (!real && lane < m) {
    contributors[pair * m + lane] = -1;
    contributions[pair * m + lane] = 0.f;
  }
  if (lane == 0) {
    baseline[pair] = 0.f;
    total[pair] = tot;
  }
}

}  // namespace
