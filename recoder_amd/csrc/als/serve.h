// Constrained serving (private to als.hip): what recoder_amd/serve.py adds to Recoder.recommend.
//   rk_als_serve_mask    the deny bitmap [B][ldw] of a batch (bit 1 = the item is NOT eligible for the row) and the
//                        count of eligible items per row.  One workgroup a row, four phases on the row's own words,
//                        a fence and a barrier between them: (1) plain stores of the start value, (2) 32-bit atomicAnd
//                        clears the bits of the row's allow list, (3) 32-bit atomicOr sets the catalogue word, the
//                        seen entries with a positive value and the row's deny list, (4) every word read back past
//                        L1 and the complement's popcount summed.  AND and OR of bits do not depend on order: the
//                        bitmap is the same whatever the waves do.  Integer atomics only
//   rk_als_pair_scores   score[e] = z_r . Y[ids[e]] + bias[ids[e]] of a ragged candidate list; see PAIR ORDER below
//   rk_als_pairs_topk    the best k eligible entries of every row by (score descending, id ascending), padded with
//                        id -1 / score -inf past the row's count of eligible entries.  One workgroup a row, a bitonic
//                        sort of composite keys in LDS (topk.hip's f2key order, restated: this library does not link
//                        the training library)
//
// PAIR ORDER.  A lane group of W lanes takes an entry; W and Q depend on h alone:
//     h <= 16: W = 4, Q = 1     h <= 32: W = 8, Q = 1     h <= 64: W = 16, Q = 1    h <= 128: W = 32, Q = 1
//     h <= 256: W = 64, Q = 1   h <= 512: W = 64, Q = 2   h <= 1024: W = 64, Q = 4  else: W = 64, Q = 8
// Lane j of the group owns the dimensions d = 4 (j + W q) + c, q < Q, c < 4 (those below h).  Its partial is one fmaf
// chain from +0 over q ascending, inside it c ascending: s = fmaf(z[d], y[d], s).  The W partials are then added by
// an xor butterfly at the distances W / 2, W / 4, ..., 1 (p = p + p'), which gives every lane the same bits, and the
// bias is added last: score = p + bias.  Nothing else enters: not the entry's place in the list, not B, not the group
// that took it.  PAIR_ROWS entries are gathered by a group before any is reduced.
#pragma once
#include "common.h"

namespace {

constexpr int SERVE_TOPK_CAP = 8192;     // rk_als_pairs_topk_max_row()
constexpr int SERVE_THREADS = 256;

// ------------------------------------------------------------------------------------------------------- the mask
__device__ __forceinline__ void serve_row_range(const int64_t *indptr, int r, int64_t nnz, int64_t &lo, int64_t &hi) {
  lo = hi = 0;
  if (!indptr) return;
  lo = min(max(indptr[r], (int64_t)0), nnz);
  hi = min(max(indptr[r + 1], lo), nnz);
}

__global__ __launch_bounds__(SERVE_THREADS) void als_serve_mask_kernel(
    int n_items, int ldw, const int64_t *__restrict__ seen_indptr, const int32_t *__restrict__ seen_ids,
    const float *__restrict__ seen_vals, int64_t seen_nnz, const uint32_t *__restrict__ cat_allow,
    const uint32_t *__restrict__ cat_deny, const int64_t *__restrict__ ua_indptr, const int32_t *__restrict__ ua_ids,
    int64_t ua_nnz, const int64_t *__restrict__ ud_indptr, const int32_t *__restrict__ ud_ids, int64_t ud_nnz,
    uint32_t *bits, int32_t *__restrict__ eligible) {
  __shared__ int s_count;
  const int r = blockIdx.x, tid = threadIdx.x;
  uint32_t *row = bits + (int64_t)r * ldw;
  const int nw = (n_items + 31) >> 5;
  const bool has_ua = ua_indptr != nullptr;
  // the catalogue's word: ~allow | deny, the bits past n_items set
  auto cat_word = [&](int w) -> uint32_t {
    uint32_t v = (cat_allow ? ~cat_allow[w] : 0u) | (cat_deny ? cat_deny[w] : 0u);
    if (w == nw - 1 && (n_items & 31)) v |= ~0u << (n_items & 31);
    return v;
  };
  if (tid == 0) s_count = 0;
  // (1) a row with an allow list starts all-ones, any other at the catalogue's word; all-ones past the catalogue
  for (int w = tid; w < ldw; w += SERVE_THREADS) row[w] = (has_ua || w >= nw) ? ~0u : cat_word(w);
  __threadfence();
  __syncthreads();
  int64_t lo, hi;
  // (2) the row's allow list clears its bits
  if (has_ua) {
    serve_row_range(ua_indptr, r, ua_nnz, lo, hi);
    for (int64_t e = lo + tid; e < hi; e += SERVE_THREADS) {
      const int c = ua_ids[e];
      if (c >= 0 && c < n_items) atomicAnd(&row[c >> 5], ~(1u << (c & 31)));
    }
    __threadfence();
    __syncthreads();
    for (int w = tid; w < nw; w += SERVE_THREADS) {
      const uint32_t v = cat_word(w);
      if (v) atomicOr(&row[w], v);
    }
  }
  // (3) the seen entries (a stored value <= 0 does not mask) and the row's deny list set theirs
  serve_row_range(seen_indptr, r, seen_nnz, lo, hi);
  for (int64_t e = lo + tid; e < hi; e += SERVE_THREADS) {
    const int c = seen_ids[e];
    const bool pos = seen_vals ? seen_vals[e] > 0.f : true;
    if (pos && c >= 0 && c < n_items) atomicOr(&row[c >> 5], 1u << (c & 31));
  }
  serve_row_range(ud_indptr, r, ud_nnz, lo, hi);
  for (int64_t e = lo + tid; e < hi; e += SERVE_THREADS) {
    const int c = ud_ids[e];
    if (c >= 0 && c < n_items) atomicOr(&row[c >> 5], 1u << (c & 31));
  }
  __threadfence();
  __syncthreads();
  // (4) the count, once every OR of the row is complete: the words read at the device's scope, past L1
  int cnt = 0;
  for (int w = tid; w < nw; w += SERVE_THREADS)
    cnt += __popc(~__hip_atomic_load(&row[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((tid & 63) == 0 && cnt) atomicAdd(&s_count, cnt);
  __syncthreads();
  if (tid == 0) eligible[r] = s_count;
}

// ---------------------------------------------------------------------------------------------------- pair scores
__device__ __forceinline__ bool serve_denied(const uint32_t *__restrict__ deny, int64_t r, int ldw, int c) {
  return deny && ((deny[r * ldw + (c >> 5)] >> (c & 31)) & 1u);
}

template <int W>
__device__ __forceinline__ float group_sum(float s) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// grid (splits, B): the groups of a row's workgroups walk its entries PAIR_ROWS at a time
template <int W, int Q>
__global__ __launch_bounds__(SERVE_THREADS) void als_pair_scores_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ ids, int64_t nnz, const float *__restrict__ z,
    int ldz, const float *__restrict__ Y, int ldy, int n, int h, const float *__restrict__ bias,
    const uint32_t *__restrict__ deny, int ldw, float *__restrict__ out) {
  constexpr int R = Q >= 8 ? 2 : 4;                      // PAIR_ROWS: entries a group has in flight
  constexpr int G = SERVE_THREADS / W;                   // groups a workgroup
  const int r = blockIdx.y;
  const int j = threadIdx.x % W, g = threadIdx.x / W;
  int64_t lo, hi;
  serve_row_range(indptr, r, nnz, lo, hi);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 zr[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int d = 4 * (j + W * q);
    zr[q] = d < h ? *reinterpret_cast<const float4 *>(z + (int64_t)r * ldz + d) : zero4;
  }
  const int64_t stride = (int64_t)gridDim.x * G * R;
  for (int64_t e0 = lo + ((int64_t)blockIdx.x * G + g) * R; e0 < hi; e0 += stride) {   // (uniform over a group)
    float4 y[R][Q];
    float b[R];
    int state[R];                                        // 0: past the row, 1: scored, 2: not eligible
#pragma unroll
    for (int t = 0; t < R; ++t) {
      const int64_t e = e0 + t;
      const int c = e < hi ? ids[e] : -1;
      const bool ok = e < hi && c >= 0 && c < n && !serve_denied(deny, r, ldw, c);
      state[t] = e >= hi ? 0 : ok ? 1 : 2;
      b[t] = (ok && bias) ? bias[c] : 0.f;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int d = 4 * (j + W * q);
        y[t][q] = (ok && d < h) ? *reinterpret_cast<const float4 *>(Y + (int64_t)c * ldy + d) : zero4;
      }
    }
#pragma unroll
    for (int t = 0; t < R; ++t) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        s = fmaf(zr[q].x, y[t][q].x, s);
        s = fmaf(zr[q].y, y[t][q].y, s);
        s = fmaf(zr[q].z, y[t][q].z, s);
        s = fmaf(zr[q].w, y[t][q].w, s);
      }
      s = group_sum<W>(s);
      if (j == 0 && state[t]) out[e0 + t] = state[t] == 1 ? (bias ? s + b[t] : s) : -INFINITY;
    }
  }
}

// f(Int<W>{}, Int<Q>{}): PAIR ORDER's table
template <class F>
void dispatch_pair(int h, F &&f) {
  if (h <= 16) f(Int<4>{}, Int<1>{});
  else if (h <= 32) f(Int<8>{}, Int<1>{});
  else if (h <= 64) f(Int<16>{}, Int<1>{});
  else if (h <= 128) f(Int<32>{}, Int<1>{});
  else if (h <= 256) f(Int<64>{}, Int<1>{});
  else if (h <= 512) f(Int<64>{}, Int<2>{});
  else if (h <= 1024) f(Int<64>{}, Int<4>{});
  else f(Int<64>{}, Int<8>{});
}

// --------------------------------------------------------------------------------------------------- ragged top-k
// topk.hip's order: float32 by value, both zeros one value, a NaN without the sign bit above +inf
__device__ __forceinline__ uint32_t serve_f2key(float f) {
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float serve_key2f(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}

// An eligible entry's key is (f2key(score) << 32) | ~id, never 0 (id < 2^31): the others are 0 and sort last.  A row
// longer than cap (the launch's LDS keys, a power of two <= SERVE_TOPK_CAP) is cut there: the caller refuses it
// before the launch.
__global__ __launch_bounds__(SERVE_THREADS) void als_pairs_topk_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ ids, const float *__restrict__ scores, int64_t nnz,
    int n, const uint32_t *__restrict__ deny, int ldw, int cap, int k, int64_t *__restrict__ out_idx,
    float *__restrict__ out_val, int out_ld, int32_t *__restrict__ count) {
  extern __shared__ unsigned long long serve_keys[];
  __shared__ int s_elig;
  const int r = blockIdx.x, tid = threadIdx.x;
  int64_t lo, hi;
  serve_row_range(indptr, r, nnz, lo, hi);
  const int c0 = (int)min(hi - lo, (int64_t)cap);
  int P = 1;
  while (P < c0) P <<= 1;
  if (tid == 0) s_elig = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < P; i += SERVE_THREADS) {
    unsigned long long e = 0ull;
    if (i < c0) {
      const int c = ids[lo + i];
      if (c >= 0 && c < n && !serve_denied(deny, r, ldw, c)) {
        e = ((unsigned long long)serve_f2key(scores[lo + i]) << 32) | (uint32_t)(~(uint32_t)c);
        ++mine;
      }
    }
    serve_keys[i] = e;
  }
  if (mine) atomicAdd(&s_elig, mine);
  __syncthreads();
  const int elig = s_elig;
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < P; i += SERVE_THREADS) {
        const int jj = i ^ stride;
        if (jj > i) {
          const bool desc = ((i & size) == 0);
          const unsigned long long a = serve_keys[i], b = serve_keys[jj];
          if ((a < b) == desc) { serve_keys[i] = b; serve_keys[jj] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < k; i += SERVE_THREADS) {
    const bool real = i < elig;                            // (elig <= c0 <= P: a real rank is inside the sorted keys)
    const unsigned long long e = real ? serve_keys[i] : 0ull;
    out_idx[(int64_t)r * out_ld + i] = real ? (int64_t)(~(uint32_t)(e & 0xffffffffull)) : (int64_t)-1;
    if (out_val) out_val[(int64_t)r * out_ld + i] = real ? serve_key2f((uint32_t)(e >> 32)) : -INFINITY;
  }
  if (count && tid == 0) count[r] = elig;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int rk_als_serve_mask(int32_t B, int32_t n_items, int32_t ldw, const int64_t *seen_indptr,
                                 const int32_t *seen_ids, const float *seen_vals, int64_t seen_nnz,
                                 const uint32_t *cat_allow, const uint32_t *cat_deny, const int64_t *ua_indptr,
                                 const int32_t *ua_ids, int64_t ua_nnz, const int64_t *ud_indptr,
                                 const int32_t *ud_ids, int64_t ud_nnz, uint32_t *bits, int32_t *eligible,
                                 void *stream) {
  RK_SIDE_REQUIRE(B >= 0 && n_items >= 1 && (int64_t)ldw * 32 >= n_items, "B >= 0, n_items >= 1, 32 ldw >= n_items");
  RK_SIDE_REQUIRE(seen_nnz >= 0 && ua_nnz >= 0 && ud_nnz >= 0, "nnz >= 0");
  RK_SIDE_REQUIRE(!seen_indptr || seen_nnz == 0 || seen_ids, "the seen ids with their indptr");
  RK_SIDE_REQUIRE(!ua_indptr || ua_nnz == 0 || ua_ids, "the allow ids with their indptr");
  RK_SIDE_REQUIRE(!ud_indptr || ud_nnz == 0 || ud_ids, "the deny ids with their indptr");
  if (B == 0) return 0;
  RK_SIDE_REQUIRE(bits && eligible, "null pointer");
  hipLaunchKernelGGL(als_serve_mask_kernel, dim3((unsigned)B), dim3(SERVE_THREADS), 0, (hipStream_t)stream, n_items,
                     ldw, seen_indptr, seen_ids, seen_vals, seen_nnz, cat_allow, cat_deny, ua_indptr, ua_ids, ua_nnz,
                     ud_indptr, ud_ids, ud_nnz, bits, eligible);
  RK_SIDE_CHECK_LAUNCH("als_serve_mask");
  return 0;
}

extern "C" int rk_als_pair_scores(const int64_t *indptr, const int32_t *ids, int64_t nnz, int32_t B,
                                  int32_t max_row, const float *z, int32_t ldz, const float *Y, int32_t ldy, int32_t n,
                                  int32_t h, const float *bias, const uint32_t *deny, int32_t ldw, float *scores,
                                  void *stream) {
  RK_SIDE_REQUIRE(B >= 0 && nnz >= 0 && n >= 1 && max_row >= 0, "B, nnz, max_row >= 0, n >= 1");
  RK_SIDE_REQUIRE(h >= 4 && h % 4 == 0 && h <= rk_als_ials_max_h(), "h: a multiple of 4 in [4, rk_als_ials_max_h()]");
  RK_SIDE_REQUIRE(ldz >= h && ldy >= h && ldz % 4 == 0 && ldy % 4 == 0, "ldz, ldy >= h and multiples of 4");
  RK_SIDE_REQUIRE(!deny || (int64_t)ldw * 32 >= n, "32 ldw >= n with a deny bitmap");
  if (B == 0 || nnz == 0) return 0;
  RK_SIDE_REQUIRE(indptr && ids && z && Y && scores, "null pointer");
  RK_SIDE_REQUIRE(aligned16(z) && aligned16(Y), "z and Y must be 16-byte aligned");
  dispatch_pair(h, [&](auto w, auto q) {
    constexpr int W = decltype(w)::value, Q = decltype(q)::value;
    constexpr int per_block = (SERVE_THREADS / W) * (Q >= 8 ? 2 : 4);    // entries a workgroup takes in one round
    const int splits = std::max(1, std::min(64, (max_row + 2 * per_block - 1) / (2 * per_block)));
    hipLaunchKernelGGL((als_pair_scores_kernel<W, Q>), dim3((unsigned)splits, (unsigned)B), dim3(SERVE_THREADS), 0,
                       (hipStream_t)stream, indptr, ids, nnz, z, ldz, Y, ldy, n, h, bias, deny, ldw, scores);
  });
  RK_SIDE_CHECK_LAUNCH("als_pair_scores");
  return 0;
}

extern "C" int32_t rk_als_pairs_topk_max_row(void) { return SERVE_TOPK_CAP; }

extern "C" int rk_als_pairs_topk(const int64_t *indptr, const int32_t *ids, const float *scores, int64_t nnz,
                                 int32_t B, int32_t max_row, int32_t n, const uint32_t *deny, int32_t ldw, int32_t k,
                                 int64_t *out_idx, float *out_val, int32_t out_ld, int32_t *count, void *stream) {
  RK_SIDE_REQUIRE(B >= 0 && nnz >= 0 && n >= 1, "B, nnz >= 0, n >= 1");
  RK_SIDE_REQUIRE(max_row >= 0 && max_row <= SERVE_TOPK_CAP, "0 <= max_row <= rk_als_pairs_topk_max_row()");
  RK_SIDE_REQUIRE(k >= 1 && k <= SERVE_TOPK_CAP && out_ld >= k, "1 <= k <= 8192, out_ld >= k");
  RK_SIDE_REQUIRE(!deny || (int64_t)ldw * 32 >= n, "32 ldw >= n with a deny bitmap");
  if (B == 0) return 0;
  RK_SIDE_REQUIRE(indptr && out_idx && (nnz == 0 || (ids && scores)), "null pointer");
  int cap = 1;
  while (cap < max_row) cap <<= 1;
  hipLaunchKernelGGL(als_pairs_topk_kernel, dim3((unsigned)B), dim3(SERVE_THREADS), (size_t)cap * 8,
                     (hipStream_t)stream, indptr, ids, scores, nnz, n, deny, ldw, cap, k, out_idx, out_val, out_ld,
                     count);
  RK_SIDE_CHECK_LAUNCH("als_pairs_topk");
  return 0;
}
