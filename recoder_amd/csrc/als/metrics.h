// rk_als_rank_metrics: Recall / NDCG / AveragePrecision of device-resident top-k lists against a device-resident
// target CSR (private to als.hip).  One wave per user; the hits of 64 ranks are one ballot, the hit count at a rank a
// popcount of the mask below it plus the carry of the earlier chunks; every floating-point sum is float64 in
// ascending rank order.  The sum over the users is a second launch of one workgroup in a fixed order.  No atomics.
#pragma once
#include "common.h"

namespace {

constexpr int RM_MAX = RK_ALS_RANK_METRICS_MAX;
constexpr int RM_SUM_THREADS = 256;

struct RankMetricSpec {
  int32_t n;
  int32_t kind[RM_MAX], k[RM_MAX], normalize[RM_MAX];
};

// values[u, m] of the users u < B, Kr = min(K, max k) ranks read per user
__global__ __launch_bounds__(256) void als_rank_metrics_kernel(const int64_t *__restrict__ recs, int B, int Kr,
                                                               int64_t ld, const int64_t *__restrict__ indptr,
                                                               const int32_t *__restrict__ indices, int64_t nnz,
                                                               RankMetricSpec spec, const double *__restrict__ inv_w,
                                                               const double *__restrict__ ideal,
                                                               double *__restrict__ values) {
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= B) return;                                    // (wave-uniform)
  const int64_t lo = min(max(indptr[u], (int64_t)0), nnz);
  const int64_t hi = min(max(indptr[u + 1], lo), nnz);
  const int64_t ny = hi - lo;
  double acc[RM_MAX];
  int hits[RM_MAX];
#pragma unroll
  for (int m = 0; m < RM_MAX; ++m) acc[m] = 0.0, hits[m] = 0;
  int carry = 0;                                         // the hits of the earlier chunks
  for (int c0 = 0; c0 < Kr; c0 += 64) {
    const int r = c0 + lane;
    bool hit = false;
    if (r < Kr && ny > 0) {
      const int64_t id = recs[(int64_t)u * ld + r];
      int64_t a = lo, b = hi;                            // the first target >= id, in [lo, hi]
      while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if ((int64_t)indices[mid] < id) a = mid + 1; else b = mid;
      }
      hit = a < hi && (int64_t)indices[a] == id;
    }
    const uint64_t mask = __ballot(hit);
    const int cum = carry + __popcll(mask & ((1ull << lane) - 1ull)) + 1;      // the hits up to this rank, itself included
    const double t_dcg = hit ? inv_w[r] : 0.0;
    const double t_ap = hit ? (double)cum / (double)(r + 1) : 0.0;
#pragma unroll
    for (int m = 0; m < RM_MAX; ++m) {
      const int below = min(spec.k[m], Kr) - c0;         // the chunk's ranks under the cutoff
      if (m < spec.n && below > 0) hits[m] += __popcll(below >= 64 ? mask : mask & ((1ull << below) - 1ull));
    }
    for (uint64_t rest = mask; rest; rest &= rest - 1) { // the hits in ascending rank order (wave-uniform)
      const int bit = __ffsll((unsigned long long)rest) - 1;
      const double d = __shfl(t_dcg, bit, 64), p = __shfl(t_ap, bit, 64);
#pragma unroll
      for (int m = 0; m < RM_MAX; ++m)
        if (m < spec.n && c0 + bit < spec.k[m]) acc[m] += spec.kind[m] == RK_ALS_METRIC_NDCG ? d : p;
    }
    carry += __popcll(mask);
  }
  if (lane != 0) return;
#pragma unroll
  for (int m = 0; m < RM_MAX; ++m) {
    if (m >= spec.n) break;
    const int64_t capped = min((int64_t)spec.k[m], ny);
    const double norm = (double)(spec.normalize[m] ? capped : ny);
    double v;
    if (spec.kind[m] == RK_ALS_METRIC_RECALL) v = (double)hits[m] / norm;
    else if (spec.kind[m] == RK_ALS_METRIC_AP) v = acc[m] / norm;
    else v = acc[m] / ideal[capped];
    values[(int64_t)u * spec.n + m] = v;                 // (no target: 0 / 0 = nan in every column)
  }
}

// sums[m] = the sum of the non-nan values[:, m], count = the non-nan rows of column 0: thread t adds the users
// t, t + 256, ... in ascending order, then a halving tree over the 256 partials.  One workgroup, whatever B is.
__global__ __launch_bounds__(RM_SUM_THREADS) void als_rank_metrics_sum_kernel(const double *__restrict__ values, int B,
                                                                              int n, double *__restrict__ sums,
                                                                              int64_t *__restrict__ count) {
  __shared__ double red[RM_SUM_THREADS];
  __shared__ long long cnt[RM_SUM_THREADS];
  const int t = threadIdx.x;
  for (int m = 0; m < n; ++m) {
    double s = 0.0;
    long long c = 0;
    for (int u = t; u < B; u += RM_SUM_THREADS) {
      const double v = values[(int64_t)u * n + m];
      if (v == v) s += v, ++c;
    }
    red[t] = s, cnt[t] = c;
    __syncthreads();
    for (int off = RM_SUM_THREADS / 2; off > 0; off >>= 1) {
      if (t < off) red[t] += red[t + off], cnt[t] += cnt[t + off];
      __syncthreads();
    }
    if (t == 0) {
      sums[m] = red[0];
      if (m == 0) count[0] = cnt[0];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int rk_als_rank_metrics(const int64_t *recs, int32_t B, int32_t K, int64_t ld, const int64_t *tgt_indptr,
                                   const int32_t *tgt_indices, int64_t tgt_nnz, int32_t n_metrics,
                                   const int32_t *kinds, const int32_t *ks, const int32_t *normalize,
                                   const double *inv_w, const double *ideal, double *values, double *sums,
                                   int64_t *count, void *stream) {
  RK_SIDE_REQUIRE(B >= 1 && K >= 1 && ld >= K, "B, K >= 1, ld >= K");
  RK_SIDE_REQUIRE(n_metrics >= 1 && n_metrics <= RM_MAX, "1 <= n_metrics <= 8");
  RK_SIDE_REQUIRE(recs && tgt_indptr && kinds && ks && normalize && inv_w && ideal && values && sums && count,
                  "null pointer");
  RK_SIDE_REQUIRE(tgt_nnz >= 0 && (tgt_nnz == 0 || tgt_indices), "tgt_nnz >= 0, and the indices with it");
  RankMetricSpec spec = {};
  spec.n = n_metrics;
  int max_k = 0;
  for (int m = 0; m < n_metrics; ++m) {
    RK_SIDE_REQUIRE(kinds[m] >= RK_ALS_METRIC_RECALL && kinds[m] <= RK_ALS_METRIC_AP, "kind is recall, ndcg or ap");
    RK_SIDE_REQUIRE(ks[m] >= 1, "k >= 1");
    spec.kind[m] = kinds[m], spec.k[m] = ks[m], spec.normalize[m] = normalize[m] != 0;
    max_k = std::max(max_k, ks[m]);
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(als_rank_metrics_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, recs, B,
                     std::min(K, max_k), ld, tgt_indptr, tgt_indices, tgt_nnz, spec, inv_w, ideal, values);
  hipLaunchKernelGGL(als_rank_metrics_sum_kernel, dim3(1), dim3(RM_SUM_THREADS), 0, st, values, B, n_metrics, sums,
                     count);
  RK_SIDE_CHECK_LAUNCH("als_rank_metrics");
  return 0;
}
