// RP3beta: the sparse item-graph model (include/recoder_rp3.h, librecoder_rp3.so).
//
//   rk_rp3_fit     one workgroup (16 waves) per source item i at a time, rows handed out through a counter.
//                  accumulate: every wave walks the users of item i in order and adds user_w[v] to the
//                    columns of user v it owns (64-column granules, round robin over the waves): one add
//                    chain per column, ascending users, no atomics on data.  The accumulators are a row in
//                    LDS (n <= FT_LDS_ITEMS) or a row of the workspace; the workspace path also lists the
//                    columns it touches (a column's first touch is seen from its -0 fill), so that
//                    everything after costs the row's candidates, not n
//                  scale: W = (row_scale[i] * S) * col_scale[j], the diagonal 0
//                  select: radix selection (4 x 8 bits) of the K-th largest float, then of the id up to which
//                    values equal to it are kept
//                  compact: the kept entries gathered in LDS, sorted by id (bitonic), written with padding
//   rk_rp3_scores  one workgroup per (user, tile of 8192 columns held in LDS); each of its 8 waves owns
//                  1024 columns and walks the user's entries in order, adding x * w of the neighbours
//                  that fall in its columns
//
// ItemKNN, the shrunk item-neighbourhood model (cosine, asymmetric cosine, Tversky / Jaccard / Dice):
//   rk_rp3_item_fit  rk_rp3_fit's row pass for the own item j (hand-out, LDS / workspace split, first touch, selection):
//                  accumulate: the walked user's own value a_vj travels with (user, row start, row end) and a
//                    column i the wave owns takes fmaf(a_vj, a_vi, acc): one fmaf chain per column, ascending
//                    users, no atomics on data; without values (a template parameter) the chain is adds of 1.0
//                  scale: s / (own[j] * oth[i] + shrink) or s / (own[j] + oth[i] + g * s + shrink): the shrink
//                    term and the co-count in the denominator are what rk_rp3_fit's separable scale cannot spell
//
// UserKNN, the user-neighbourhood model served from the training matrix itself:
//   rk_rp3_user_neighbours  one workgroup per query row at a time, rows handed out through the same counter.
//                  accumulate: c[v] = |H_q and H_v| by integer atomics on the workgroup's own accumulator
//                    (LDS, or a workspace row that also lists the users it touches: a user's first touch is
//                    the add that returns 0); an item with few users belongs to one wave, an item with many
//                    is walked by all sixteen
//                  scale: sim = c / (qn[q] * un[v] + shrink); select, compact: the fit's (ft_select_store)
//   rk_rp3_user_scores  rk_rp3_scores' tiling: one workgroup per (query, tile of 8192 columns in LDS), a wave owns
//                  1024 columns and walks the query's neighbours in order; 64 neighbours at a time, a lane
//                  finds by binary search where its neighbour's row enters and leaves the wave's columns
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/recoder_rp3.h"
#include "side_error.h"

namespace {

// ------------------------------------------------------------------------ fit
constexpr int FT_WAVES = 16;
constexpr int FT_THREADS = FT_WAVES * 64;
constexpr int FT_LDS_ITEMS = 12288;           // 48 KB of accumulators + 9 KB of selection state: two workgroups per CU
constexpr int FT_MAX_K = 1024;
constexpr int FT_GROUPS = 512;                // resident workgroups: two on each of the 256 CUs
constexpr uint32_t FT_UNTOUCHED = 0x80000000u;    // -0: (first touch) 0 + w, bitwise the chain from +0

inline int64_t ft_acc_stride(int n) { return ((int64_t)n + 63) / 64 * 64; }
// entries of one wave's candidate list: the columns it owns (64 of every 1024, rounded up)
inline int64_t ft_list_stride(int n) { return ((int64_t)n + 1023) / 1024 * 64; }

__device__ inline uint32_t f2u(float v) { return __float_as_uint(v); }

// Wave 0, all 64 lanes: the bin in which the need-th element falls, counting from bin 255 down (desc)
// or from bin 0 up.  o[0] = bin (-1: fewer than need elements), o[1] = its rank inside the bin (1-based),
// o[2] = the bin's count, o[3] = the total.
__device__ void ft_pick(const int *hist, int need, int lane, bool desc, int *o) {
  int h[4], s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = 4 * lane + q;
    h[q] = hist[desc ? 255 - r : r];
    s += h[q];
  }
  int incl = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  const int total = __shfl(incl, 63, 64);
  if (lane == 0) o[3] = total;
  if (total < need) {
    if (lane == 0) o[0] = -1;
    return;
  }
  int run = incl - s;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (run < need && need <= run + h[q]) {
      const int r = 4 * lane + q;
      o[0] = desc ? 255 - r : r;
      o[1] = need - run;
      o[2] = h[q];
    }
    run += h[q];
  }
}

// What a row's pass does once its values stand in acc (every thread of the workgroup calls it): select,
// compact and store row ``row`` of the [*, K] lists.  On entry acc[j] holds the value of every candidate j
// (for_cands(f) calls f(j) once per candidate, spread over the threads), hist the histogram of the top
// byte of the values > 0 and sh[5] is 0; n bounds the ids.  kid / kw: FT_MAX_K entries; sh[1..5] are used.
template <class ForCands>
__device__ __forceinline__ void ft_select_store(const float *acc, ForCands for_cands, int K, int n, int row,
                                                int32_t *__restrict__ nbr_ids, float *__restrict__ nbr_w,
                                                int32_t *__restrict__ nbr_count, int *hist, int *sh, int *kid,
                                                float *kw, int tid, int lane, int wv) {
  // ---- select: T = the K-th largest value's bits, need = how many equal to T are kept, J = up to which id
  uint32_t T = 0, tmask = 0;
  int need = K, J = INT_MAX;
  bool all = false;
#pragma unroll 1
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (shift != 24) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for_cands([&](int j) {
        const float w = acc[j];
        const uint32_t k = f2u(w);
        if (w > 0.f && (k & tmask) == T) atomicAdd(&hist[(k >> shift) & 255], 1);
      });
      __syncthreads();
    }
    if (wv == 0) ft_pick(hist, need, lane, true, sh + 1);
    __syncthreads();
    if (shift == 24 && sh[4] <= K) {
      all = true;
      break;
    }
    T |= (uint32_t)sh[1] << shift;
    tmask |= 255u << shift;
    need = sh[2];
  }
  if (!all && sh[3] > need) {
    uint32_t jp = 0, jm = 0;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (((uint32_t)(n - 1) >> shift) != 0) {      // (otherwise: every id has zeros here)
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for_cands([&](int j) {
          if (f2u(acc[j]) == T && ((uint32_t)j & jm) == jp) atomicAdd(&hist[((uint32_t)j >> shift) & 255], 1);
        });
        __syncthreads();
        if (wv == 0) ft_pick(hist, need, lane, false, sh + 1);
        __syncthreads();
        jp |= (uint32_t)sh[1] << shift;
        need = sh[2];
      }
      jm |= 255u << shift;
    }
    J = (int)jp;
  }

  // ---- compact: gather (any order), sort by id, store
  for_cands([&](int j) {
    const float w = acc[j];
    const uint32_t k = f2u(w);
    if (w > 0.f && (all || k > T || (k == T && j <= J))) {
      const int pos = atomicAdd(&sh[5], 1);
      if (pos < FT_MAX_K) {
        kid[pos] = j;
        kw[pos] = w;
      }
    }
  });
  __syncthreads();
  const int kept = sh[5] < K ? sh[5] : K;
  int P = 1;
  while (P < kept) P <<= 1;
  if (tid >= kept && tid < P) kid[tid] = INT_MAX;
  __syncthreads();
  for (int k2 = 2; k2 <= P; k2 <<= 1)
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      const int o = tid ^ j2;
      if (tid < P && o > tid) {
        const int a = kid[tid], b = kid[o];
        if ((a > b) == ((tid & k2) == 0)) {
          kid[tid] = b;
          kid[o] = a;
          const float wa = kw[tid];
          kw[tid] = kw[o];
          kw[o] = wa;
        }
      }
      __syncthreads();
    }
  for (int c = tid; c < K; c += FT_THREADS) {
    nbr_ids[(int64_t)row * K + c] = c < kept ? kid[c] : -1;
    nbr_w[(int64_t)row * K + c] = c < kept ? kw[c] : 0.f;
  }
  if (tid == 0) nbr_count[row] = kept;
}

template <bool WS>
__global__ __launch_bounds__(FT_THREADS) void rp3_fit_kernel(
    const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_indices,
    const int64_t *__restrict__ u_indptr, const int32_t *__restrict__ u_indices, int n_users, int n,
    const float *__restrict__ user_w, const float *__restrict__ row_scale, const float *__restrict__ col_scale,
    int K, int row_lo, int row_hi, int32_t *__restrict__ nbr_ids, float *__restrict__ nbr_w,
    int32_t *__restrict__ nbr_count, int *counter, float *ws_acc, int *ws_cand, int64_t acc_stride, int ch) {
  __shared__ float lds_acc[WS ? 1 : FT_LDS_ITEMS];
  __shared__ int kid[FT_MAX_K];
  __shared__ float kw[FT_MAX_K];
  __shared__ int hist[256];
  __shared__ int wcnt[FT_WAVES];
  __shared__ int sh[8];          // 0: the row's offset; 1..4: ft_pick's answer; 5: entries gathered
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float *acc = WS ? ws_acc + (int64_t)blockIdx.x * acc_stride : lds_acc;
  int *cand = WS ? ws_cand + (int64_t)blockIdx.x * FT_WAVES * ch : nullptr;
  int *mylist = WS ? cand + (int64_t)wv * ch : nullptr;

  auto for_cands = [&](auto f) {
    if (!WS) {
      for (int j = tid; j < n; j += FT_THREADS) f(j);
    } else {
#pragma unroll 1
      for (int w = 0; w < FT_WAVES; ++w) {
        const int c = wcnt[w];
        const int *L = cand + (int64_t)w * ch;
        for (int s = tid; s < c; s += FT_THREADS) f(L[s]);
      }
    }
  };

  if (WS)
    for (int c = tid; c < n; c += FT_THREADS) acc[c] = -0.f;

  for (;;) {
    __syncthreads();
    if (tid == 0) sh[0] = atomicAdd(counter, 1);
    __syncthreads();
    const int64_t i64 = (int64_t)row_lo + sh[0];
    if (i64 >= row_hi) break;
    const int i = (int)i64;
    if (!WS) {
      for (int c = tid; c < n; c += FT_THREADS) acc[c] = 0.f;
      __syncthreads();
    }

    // ---- accumulate: (user, row start, row end, weight) fetched 64 at a time, as rk_ease_gram does
    int mycnt = 0;
    const int64_t e0 = t_indptr[i], e1 = t_indptr[i + 1];
    for (int64_t eb = e0; eb < e1; eb += 64) {
      const int cnt = e1 - eb < 64 ? (int)(e1 - eb) : 64;
      int64_t r0 = 0, r1 = 0;
      float uw = 0.f;
      if (lane < cnt) {
        const int u = t_indices[eb + lane];
        if (u >= 0 && u < n_users) {           // (a bad index reads nothing)
          r0 = u_indptr[u];
          r1 = u_indptr[u + 1];
          uw = user_w[u];
        }
      }
      for (int l = 0; l < cnt; ++l) {
        const int64_t p0 = __shfl(r0, l, 64), p1 = __shfl(r1, l, 64);
        const float w = __shfl(uw, l, 64);
        for (int64_t p = p0; p < p1; p += 64) {       // (wave-uniform bounds)
          const int64_t q = p + lane;
          int c = 0;
          bool mine = false;
          if (q < p1) {
            c = u_indices[q];
            mine = c >= 0 && c < n && ((c >> 6) & (FT_WAVES - 1)) == wv;
          }
          if (WS) {
            // columns of one user are distinct: no two lanes meet.  The next user's adds may come from
            // other lanes of this wave: the fence keeps them behind these stores
            bool first = false;
            if (mine) {
              const float old = acc[c];
              first = f2u(old) == FT_UNTOUCHED;
              acc[c] = (first ? 0.f : old) + w;
            }
            const unsigned long long m = __ballot(first);
            if (first) {
              const int pos = mycnt + __popcll(m & ((1ull << lane) - 1ull));
              if (pos < ch) mylist[pos] = c;
            }
            mycnt += __popcll(m);
            __threadfence_block();
          } else {
            if (mine) acc[c] += w;
          }
        }
      }
    }
    if (WS && lane == 0) wcnt[wv] = mycnt < ch ? mycnt : ch;
    if (tid < 256) hist[tid] = 0;
    if (tid == 0) sh[5] = 0;
    __syncthreads();

    // ---- scale, and the histogram of the top byte
    const float rs = row_scale[i];
    for_cands([&](int j) {
      float w = __fmul_rn(__fmul_rn(rs, acc[j]), col_scale[j]);
      if (j == i) w = 0.f;
      acc[j] = w;
      if (w > 0.f) atomicAdd(&hist[f2u(w) >> 24], 1);
    });
    __syncthreads();

    ft_select_store(acc, for_cands, K, n, i, nbr_ids, nbr_w, nbr_count, hist, sh, kid, kw, tid, lane, wv);
    if (WS) for_cands([&](int j) { acc[j] = -0.f; });
  }
}

// ----------------------------------------------------------- user neighbours
constexpr int UN_WIDE = 256;                  // an item with at least this many users is walked by every wave

// c / ((qs * u) + shrink): three f32 operations, each correctly rounded.  hipcc's default -ffp-contract=fast
// would fuse the product and the sum into one fma (__fmul_rn / __fadd_rn are plain * and + to it), hence the pragma
__device__ inline float un_sim(float c, float qs, float u, float shrink) {
#pragma clang fp contract(off)
  const float prod = qs * u;
  const float den = prod + shrink;
  return __fdiv_rn(c, den);
}

// (the accumulator row holds counts while a row accumulates and the similarities afterwards: one 32-bit
// word per user either way, so that ft_select_store reads it as the fit's)
template <bool WS>
__global__ __launch_bounds__(FT_THREADS) void rp3_user_neighbours_kernel(
    const int64_t *__restrict__ q_indptr, const int32_t *__restrict__ q_indices,
    const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_indices, int n_users, int n,
    const float *__restrict__ un, const float *__restrict__ qn, float shrink, int K, int row_lo, int row_hi,
    int32_t *__restrict__ nbr_ids, float *__restrict__ nbr_sim, int32_t *__restrict__ nbr_count, int *counter,
    float *ws_acc, int *ws_cand, int64_t acc_stride) {
  __shared__ float lds_acc[WS ? 1 : FT_LDS_ITEMS];
  __shared__ int kid[FT_MAX_K];
  __shared__ float kw[FT_MAX_K];
  __shared__ int hist[256];
  __shared__ int sh[8];          // 0: the row's offset; 1..4: ft_pick's answer; 5: entries gathered; 6: users touched
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float *acc = WS ? ws_acc + (int64_t)blockIdx.x * acc_stride : lds_acc;
  int *cand = WS ? ws_cand + (int64_t)blockIdx.x * acc_stride : nullptr;

  auto for_cands = [&](auto f) {
    if (!WS) {
      for (int v = tid; v < n_users; v += FT_THREADS) f(v);
    } else {
      const int c = sh[6] < acc_stride ? sh[6] : (int)acc_stride;
      for (int s = tid; s < c; s += FT_THREADS) f(cand[s]);
    }
  };

  if (WS)
    for (int v = tid; v < n_users; v += FT_THREADS) acc[v] = 0.f;

  for (;;) {
    __syncthreads();
    if (tid == 0) {
      sh[0] = atomicAdd(counter, 1);
      sh[6] = 0;
    }
    __syncthreads();
    const int64_t q64 = (int64_t)row_lo + sh[0];
    if (q64 >= row_hi) break;
    const int q = (int)q64;
    if (!WS) {
      for (int v = tid; v < n_users; v += FT_THREADS) acc[v] = 0.f;
      __syncthreads();
    }

    // ---- accumulate: (row start, row end) of 64 query items at a time; integer adds commute, so who
    // adds first changes nothing
    const int64_t e0 = q_indptr[q], e1 = q_indptr[q + 1];
    for (int64_t eb = e0; eb < e1; eb += 64) {
      const int cnt = e1 - eb < 64 ? (int)(e1 - eb) : 64;
      int64_t r0 = 0, r1 = 0;
      if (lane < cnt) {
        const int it = q_indices[eb + lane];
        if (it >= 0 && it < n) {               // (an item outside the catalogue adds nothing)
          r0 = t_indptr[it];
          r1 = t_indptr[it + 1];
        }
      }
      for (int l = 0; l < cnt; ++l) {
        const int64_t p0 = __shfl(r0, l, 64), p1 = __shfl(r1, l, 64);
        const bool wide = p1 - p0 >= UN_WIDE;                    // (the same answer in every wave)
        if (!wide && (l & (FT_WAVES - 1)) != wv) continue;
        const int step = wide ? FT_THREADS : 64;
        for (int64_t pb = p0 + (wide ? wv * 64 : 0); pb < p1; pb += step) {      // (wave-uniform bounds)
          const int64_t p = pb + lane;
          int v = -1;
          if (p < p1) {
            v = t_indices[p];
            if (v < 0 || v >= n_users) v = -1;                  // (a bad index adds nothing)
          }
          if (WS) {
            const bool first = v >= 0 && atomicAdd(reinterpret_cast<unsigned int *>(acc + v), 1u) == 0u;
            const unsigned long long m = __ballot(first);
            if (m) {
              int base = 0;
              if (lane == 0) base = atomicAdd(&sh[6], __popcll(m));
              base = __shfl(base, 0, 64);
              const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
              if (first && pos < acc_stride) cand[pos] = v;
            }
          } else {
            if (v >= 0) atomicAdd(reinterpret_cast<unsigned int *>(acc + v), 1u);
          }
        }
      }
    }
    if (tid < 256) hist[tid] = 0;
    if (tid == 0) sh[5] = 0;
    if (WS) __threadfence();                   // (the adds were made in L2: nothing of this row is read before them)
    __syncthreads();

    // ---- scale, and the histogram of the top byte
    const float qs = qn[q];
    for_cands([&](int v) {
      // (workspace: the count is read where the atomics made it, past this CU's L1)
      const uint32_t c = WS ? __hip_atomic_load(reinterpret_cast<unsigned int *>(acc + v), __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT)
                            : f2u(acc[v]);
      float w = 0.f;
      if (c) w = un_sim((float)c, qs, un[v], shrink);
      acc[v] = w;
      if (w > 0.f) atomicAdd(&hist[f2u(w) >> 24], 1);
    });
    __syncthreads();

    ft_select_store(acc, for_cands, K, n_users, q, nbr_ids, nbr_sim, nbr_count, hist, sh, kid, kw, tid, lane, wv);
    if (WS)
      for_cands([&](int v) {
        __hip_atomic_store(reinterpret_cast<unsigned int *>(acc + v), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      });
  }
}

// ------------------------------------------------------------------ item fit
// s / den, den = (own * oth) + shrink (form 0) or ((own + oth) + (g * s)) + shrink (form 1): every operation a
// separately rounded f32 operation (see un_sim for the pragma), +0 unless s > 0 and den > 0
__device__ inline float it_sim(float s, float own, float oth, int form, float g, float shrink) {
#pragma clang fp contract(off)
  float den;
  if (form == 0) {
    const float prod = own * oth;
    den = prod + shrink;
  } else {
    const float sum = own + oth;
    const float gs = g * s;
    const float t = sum + gs;
    den = t + shrink;
  }
  return s > 0.f && den > 0.f ? __fdiv_rn(s, den) : 0.f;
}

// (rp3_fit_kernel's structure; DATA false: t_data / u_data are not read and every value is 1.0)
template <bool WS, bool DATA>
__global__ __launch_bounds__(FT_THREADS) void rp3_item_fit_kernel(
    const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_indices, const float *__restrict__ t_data,
    const int64_t *__restrict__ u_indptr, const int32_t *__restrict__ u_indices, const float *__restrict__ u_data,
    int n_users, int n, const float *__restrict__ own, const float *__restrict__ oth, int form, float g,
    float shrink, int K, int col_lo, int col_hi, int32_t *__restrict__ nbr_ids, float *__restrict__ nbr_w,
    int32_t *__restrict__ nbr_count, int *counter, float *ws_acc, int *ws_cand, int64_t acc_stride, int ch) {
  __shared__ float lds_acc[WS ? 1 : FT_LDS_ITEMS];
  __shared__ int kid[FT_MAX_K];
  __shared__ float kw[FT_MAX_K];
  __shared__ int hist[256];
  __shared__ int wcnt[FT_WAVES];
  __shared__ int sh[8];          // 0: the column's offset; 1..4: ft_pick's answer; 5: entries gathered
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float *acc = WS ? ws_acc + (int64_t)blockIdx.x * acc_stride : lds_acc;
  int *cand = WS ? ws_cand + (int64_t)blockIdx.x * FT_WAVES * ch : nullptr;
  int *mylist = WS ? cand + (int64_t)wv * ch : nullptr;

  auto for_cands = [&](auto f) {
    if (!WS) {
      for (int i = tid; i < n; i += FT_THREADS) f(i);
    } else {
#pragma unroll 1
      for (int w = 0; w < FT_WAVES; ++w) {
        const int c = wcnt[w];
        const int *L = cand + (int64_t)w * ch;
        for (int s = tid; s < c; s += FT_THREADS) f(L[s]);
      }
    }
  };

  if (WS)
    for (int c = tid; c < n; c += FT_THREADS) acc[c] = -0.f;

  for (;;) {
    __syncthreads();
    if (tid == 0) sh[0] = atomicAdd(counter, 1);
    __syncthreads();
    const int64_t j64 = (int64_t)col_lo + sh[0];
    if (j64 >= col_hi) break;
    const int j = (int)j64;
    if (!WS) {
      for (int c = tid; c < n; c += FT_THREADS) acc[c] = 0.f;
      __syncthreads();
    }

    // ---- accumulate: (user, row start, row end, the own item's value) fetched 64 at a time
    int mycnt = 0;
    const int64_t e0 = t_indptr[j], e1 = t_indptr[j + 1];
    for (int64_t eb = e0; eb < e1; eb += 64) {
      const int cnt = e1 - eb < 64 ? (int)(e1 - eb) : 64;
      int64_t r0 = 0, r1 = 0;
      float av = 0.f;
      if (lane < cnt) {
        const int u = t_indices[eb + lane];
        if (u >= 0 && u < n_users) {           // (a bad index reads nothing)
          r0 = u_indptr[u];
          r1 = u_indptr[u + 1];
          if (DATA) av = t_data[eb + lane];
        }
      }
      for (int l = 0; l < cnt; ++l) {
        const int64_t p0 = __shfl(r0, l, 64), p1 = __shfl(r1, l, 64);
        const float a = DATA ? __shfl(av, l, 64) : 1.f;
        for (int64_t p = p0; p < p1; p += 64) {       // (wave-uniform bounds)
          const int64_t q = p + lane;
          int c = 0;
          float x = 1.f;
          bool mine = false;
          if (q < p1) {
            c = u_indices[q];
            mine = c >= 0 && c < n && ((c >> 6) & (FT_WAVES - 1)) == wv;
            if (DATA && mine) x = u_data[q];
          }
          if (WS) {
            // (rp3_fit_kernel's first touch: a product is >= +0, so fmaf(a, x, +0) is bitwise the chain's start)
            bool first = false;
            if (mine) {
              const float old = acc[c];
              first = f2u(old) == FT_UNTOUCHED;
              acc[c] = DATA ? fmaf(a, x, first ? 0.f : old) : (first ? 0.f : old) + 1.f;
            }
            const unsigned long long m = __ballot(first);
            if (first) {
              const int pos = mycnt + __popcll(m & ((1ull << lane) - 1ull));
              if (pos < ch) mylist[pos] = c;
            }
            mycnt += __popcll(m);
            __threadfence_block();
          } else {
            if (mine) acc[c] = DATA ? fmaf(a, x, acc[c]) : acc[c] + 1.f;
          }
        }
      }
    }
    if (WS && lane == 0) wcnt[wv] = mycnt < ch ? mycnt : ch;
    if (tid < 256) hist[tid] = 0;
    if (tid == 0) sh[5] = 0;
    __syncthreads();

    // ---- scale, and the histogram of the top byte
    const float oj = own[j];
    for_cands([&](int i) {
      float w = it_sim(acc[i], oj, oth[i], form, g, shrink);
      if (i == j) w = 0.f;
      acc[i] = w;
      if (w > 0.f) atomicAdd(&hist[f2u(w) >> 24], 1);
    });
    __syncthreads();

    ft_select_store(acc, for_cands, K, n, j, nbr_ids, nbr_w, nbr_count, hist, sh, kid, kw, tid, lane, wv);
    if (WS) for_cands([&](int i) { acc[i] = -0.f; });
  }
}

// --------------------------------------------------------------------- scores
constexpr int SC_WAVES = 8;
constexpr int SC_SUB = 1024;                  // columns a wave owns
constexpr int SC_TILE = SC_WAVES * SC_SUB;    // 32 KB of LDS

__global__ __launch_bounds__(SC_WAVES * 64) void rp3_scores_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const float *__restrict__ data,
    int n_items, const int32_t *__restrict__ nbr_ids, const float *__restrict__ nbr_w,
    const int32_t *__restrict__ nbr_count, int K, int lo, int width, float *__restrict__ out, int64_t ldo) {
  __shared__ float tile[SC_TILE];
  const int u = blockIdx.x;                             // (users fastest: neighbours share a column tile)
  const int t0 = blockIdx.y * SC_TILE;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t wlo = (int64_t)lo + t0 + wv * SC_SUB;
  const int64_t whi = wlo + SC_SUB < (int64_t)lo + width ? wlo + SC_SUB : (int64_t)lo + width;
  float *mine = tile + wv * SC_SUB;
  for (int c = lane; c < SC_SUB; c += 64) mine[c] = 0.f;
  if (wlo < whi) {
    const int64_t e0 = indptr[u], e1 = indptr[u + 1];
    for (int64_t eb = e0; eb < e1; eb += 64) {
      const int cnt = e1 - eb < 64 ? (int)(e1 - eb) : 64;
      int it = 0, nc = 0;
      float xv = 0.f;
      if (lane < cnt) {
        it = indices[eb + lane];
        if (it >= 0 && it < n_items) {         // (a bad index adds nothing)
          nc = nbr_count[it];
          nc = nc < 0 ? 0 : (nc > K ? K : nc);
          xv = data ? data[eb + lane] : 1.f;
        }
      }
      for (int l = 0; l < cnt; ++l) {
        const int c = __shfl(nc, l, 64);
        const float x = __shfl(xv, l, 64);
        const int64_t base = (int64_t)__shfl(it, l, 64) * K;
        for (int s = lane; s < c; s += 64) {            // ids of one row are distinct: no two lanes meet
          const int j = nbr_ids[base + s];
          if (j >= wlo && j < whi) mine[j - wlo] = fmaf(x, nbr_w[base + s], mine[j - wlo]);
        }
      }
    }
  }
  __syncthreads();
  const int w = width - t0 < SC_TILE ? width - t0 : SC_TILE;
  float *row = out + (int64_t)u * ldo + t0;
  for (int c = threadIdx.x; c < w; c += SC_WAVES * 64) row[c] = tile[c];
}

// first position in [a, b) of the ascending idx whose value is >= key
__device__ inline int64_t sc_lower_bound(const int32_t *__restrict__ idx, int64_t a, int64_t b, int64_t key) {
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (idx[m] < key) a = m + 1; else b = m;
  }
  return a;
}

__global__ __launch_bounds__(SC_WAVES * 64) void rp3_user_scores_kernel(
    const int32_t *__restrict__ nbr_ids, const float *__restrict__ nbr_sim, const int32_t *__restrict__ nbr_count,
    int K, const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const float *__restrict__ data,
    int n_users, int lo, int width, float *__restrict__ out, int64_t ldo) {
  __shared__ float tile[SC_TILE];
  const int q = blockIdx.x;                             // (queries fastest: neighbours' rows are shared)
  const int t0 = blockIdx.y * SC_TILE;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t wlo = (int64_t)lo + t0 + wv * SC_SUB;
  const int64_t whi = wlo + SC_SUB < (int64_t)lo + width ? wlo + SC_SUB : (int64_t)lo + width;
  float *mine = tile + wv * SC_SUB;
  for (int c = lane; c < SC_SUB; c += 64) mine[c] = 0.f;
  if (wlo < whi) {
    int nc = nbr_count[q];
    nc = nc < 0 ? 0 : (nc > K ? K : nc);
    const int64_t base = (int64_t)q * K;
    for (int sb = 0; sb < nc; sb += 64) {
      const int cnt = nc - sb < 64 ? nc - sb : 64;
      int64_t a = 0, b = 0;
      float sv = 0.f;
      if (lane < cnt) {
        const int v = nbr_ids[base + sb + lane];
        if (v >= 0 && v < n_users) {           // (a bad id adds nothing)
          const int64_t r1 = indptr[v + 1];
          a = sc_lower_bound(indices, indptr[v], r1, wlo);
          b = sc_lower_bound(indices, a, r1, whi);
          sv = nbr_sim[base + sb + lane];
        }
      }
      for (int l = 0; l < cnt; ++l) {          // neighbours ascending: a column's chain stays in this wave
        const int64_t p0 = __shfl(a, l, 64), p1 = __shfl(b, l, 64);
        const float s = __shfl(sv, l, 64);
        for (int64_t p = p0 + lane; p < p1; p += 64) {  // items of one row are distinct: no two lanes meet
          const int64_t j = indices[p] - wlo;
          if (j >= 0 && j < SC_SUB) mine[j] = fmaf(s, data ? data[p] : 1.f, mine[j]);   // (holds for an ascending row)
        }
      }
    }
  }
  __syncthreads();
  const int w = width - t0 < SC_TILE ? width - t0 : SC_TILE;
  float *row = out + (int64_t)q * ldo + t0;
  for (int c = threadIdx.x; c < w; c += SC_WAVES * 64) row[c] = tile[c];
}

}  // namespace

// ------------------------------------------------------------------------ ABI
extern "C" {

int rk_rp3_version(void) { return 102; }

const char *rk_rp3_last_error(void) { return g_rk_side_err; }

int rk_rp3_max_neighbours(void) { return FT_MAX_K; }

int rk_rp3_lds_items(void) { return FT_LDS_ITEMS; }

int64_t rk_rp3_fit_workspace_bytes(int32_t n_items) {
  if (n_items < 1) {
    rk_side_set_error("%s: n_items must be >= 1", __func__);
    return -2;
  }
  if (n_items <= FT_LDS_ITEMS) return 256;
  return 256 + (int64_t)FT_GROUPS * (ft_acc_stride(n_items) + FT_WAVES * ft_list_stride(n_items)) * 4;
}

int rk_rp3_fit(const int64_t *t_indptr, const int32_t *t_indices, const int64_t *u_indptr,
               const int32_t *u_indices, int32_t n_users, int32_t n_items, const float *user_w,
               const float *row_scale, const float *col_scale, int32_t K, int32_t row_lo, int32_t row_hi,
               int32_t *nbr_ids, float *nbr_w, int32_t *nbr_count, void *ws, int64_t ws_bytes, void *stream) {
  RK_SIDE_REQUIRE(t_indptr && t_indices && u_indptr && u_indices && user_w && row_scale && col_scale && nbr_ids &&
                  nbr_w && nbr_count && ws, "null pointer");
  RK_SIDE_REQUIRE(n_users >= 0 && n_items >= 1 && n_items < INT_MAX - 2048, "bad sizes");
  RK_SIDE_REQUIRE(K >= 1 && K <= FT_MAX_K, "K outside [1, rk_rp3_max_neighbours()]");
  RK_SIDE_REQUIRE(0 <= row_lo && row_lo <= row_hi && row_hi <= n_items, "bad row range");
  RK_SIDE_REQUIRE(ws_bytes >= rk_rp3_fit_workspace_bytes(n_items), "workspace too small");
  RK_SIDE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
  if (row_lo == row_hi) return 0;
  hipStream_t s = (hipStream_t)stream;
  int *counter = (int *)ws;
  if (hipMemsetAsync(counter, 0, sizeof(int), s) != hipSuccess) {
    rk_side_set_error("%s: hipMemsetAsync failed", __func__);
    return -1;
  }
  const int rows = row_hi - row_lo;
  const int groups = rows < FT_GROUPS ? rows : FT_GROUPS;
  if (n_items <= FT_LDS_ITEMS) {
    hipLaunchKernelGGL(rp3_fit_kernel<false>, dim3(groups), dim3(FT_THREADS), 0, s, t_indptr, t_indices, u_indptr,
                       u_indices, n_users, n_items, user_w, row_scale, col_scale, K, row_lo, row_hi, nbr_ids, nbr_w,
                       nbr_count, counter, (float *)nullptr, (int *)nullptr, (int64_t)0, 0);
  } else {
    const int64_t stride = ft_acc_stride(n_items), ch = ft_list_stride(n_items);
    float *acc = (float *)((char *)ws + 256);
    int *cand = (int *)(acc + (int64_t)FT_GROUPS * stride);
    hipLaunchKernelGGL(rp3_fit_kernel<true>, dim3(groups), dim3(FT_THREADS), 0, s, t_indptr, t_indices, u_indptr,
                       u_indices, n_users, n_items, user_w, row_scale, col_scale, K, row_lo, row_hi, nbr_ids, nbr_w,
                       nbr_count, counter, acc, cand, stride, (int)ch);
  }
  RK_SIDE_CHECK_LAUNCH("rp3_fit_kernel");
  return 0;
}

int64_t rk_rp3_item_workspace_bytes(int32_t n_items) {
  if (n_items < 1) {
    rk_side_set_error("%s: n_items must be >= 1", __func__);
    return -2;
  }
  return rk_rp3_fit_workspace_bytes(n_items);
}

int rk_rp3_item_fit(const int64_t *t_indptr, const int32_t *t_indices, const float *t_data, const int64_t *u_indptr,
                    const int32_t *u_indices, const float *u_data, int32_t n_users, int32_t n_items,
                    const float *own, const float *oth, int32_t form, float g, float shrink, int32_t K,
                    int32_t col_lo, int32_t col_hi, int32_t *nbr_ids, float *nbr_w, int32_t *nbr_count, void *ws,
                    int64_t ws_bytes, void *stream) {
  RK_SIDE_REQUIRE(t_indptr && t_indices && u_indptr && u_indices && own && oth && nbr_ids && nbr_w && nbr_count && ws,
                  "null pointer");
  RK_SIDE_REQUIRE((t_data == nullptr) == (u_data == nullptr), "t_data and u_data must be given together or both be NULL");
  RK_SIDE_REQUIRE(n_users >= 0 && n_items >= 1 && n_items < INT_MAX - 2048, "bad sizes");
  RK_SIDE_REQUIRE(form == 0 || form == 1, "form must be 0 (product) or 1 (sum)");
  RK_SIDE_REQUIRE(g >= -3.0e38f && g <= 3.0e38f, "g must be finite");
  RK_SIDE_REQUIRE(shrink >= 0.f && shrink <= 3.0e38f, "shrink must be finite and >= 0");
  RK_SIDE_REQUIRE(K >= 1 && K <= FT_MAX_K, "K outside [1, rk_rp3_max_neighbours()]");
  RK_SIDE_REQUIRE(0 <= col_lo && col_lo <= col_hi && col_hi <= n_items, "bad column range");
  RK_SIDE_REQUIRE(ws_bytes >= rk_rp3_item_workspace_bytes(n_items), "workspace too small");
  RK_SIDE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
  if (col_lo == col_hi) return 0;
  hipStream_t s = (hipStream_t)stream;
  int *counter = (int *)ws;
  if (hipMemsetAsync(counter, 0, sizeof(int), s) != hipSuccess) {
    rk_side_set_error("%s: hipMemsetAsync failed", __func__);
    return -1;
  }
  const int cols = col_hi - col_lo;
  const int groups = cols < FT_GROUPS ? cols : FT_GROUPS;
  const bool data = t_data != nullptr;
  auto launch = [&](auto kernel, float *acc, int *cand, int64_t stride, int ch) {
    hipLaunchKernelGGL(kernel, dim3(groups), dim3(FT_THREADS), 0, s, t_indptr, t_indices, t_data, u_indptr, u_indices,
                       u_data, n_users, n_items, own, oth, form, g, shrink, K, col_lo, col_hi, nbr_ids, nbr_w, nbr_count,
                       counter, acc, cand, stride, ch);
  };
  if (n_items <= FT_LDS_ITEMS) {
    launch(data ? rp3_item_fit_kernel<false, true> : rp3_item_fit_kernel<false, false>, nullptr, nullptr, 0, 0);
  } else {
    const int64_t stride = ft_acc_stride(n_items), ch = ft_list_stride(n_items);
    float *acc = (float *)((char *)ws + 256);
    launch(data ? rp3_item_fit_kernel<true, true> : rp3_item_fit_kernel<true, false>, acc,
           (int *)(acc + (int64_t)FT_GROUPS * stride), stride, (int)ch);
  }
  RK_SIDE_CHECK_LAUNCH("rp3_item_fit_kernel");
  return 0;
}

int rk_rp3_scores(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows,
                  int32_t n_items, const int32_t *nbr_ids, const float *nbr_w, const int32_t *nbr_count,
                  int32_t K, int32_t lo, int32_t hi, float *out, int64_t ldo, void *stream) {
  RK_SIDE_REQUIRE(indptr && indices && nbr_ids && nbr_w && nbr_count && out, "null pointer");
  RK_SIDE_REQUIRE(n_rows >= 0 && n_items >= 1 && K >= 1 && K <= FT_MAX_K, "bad sizes");
  RK_SIDE_REQUIRE(0 <= lo && lo < hi && hi <= n_items && ldo >= hi - lo, "bad strip");
  if (n_rows == 0) return 0;
  const int width = hi - lo;
  const dim3 grid(n_rows, (width + SC_TILE - 1) / SC_TILE);
  hipLaunchKernelGGL(rp3_scores_kernel, grid, dim3(SC_WAVES * 64), 0, (hipStream_t)stream, indptr, indices, data,
                     n_items, nbr_ids, nbr_w, nbr_count, K, lo, width, out, ldo);
  RK_SIDE_CHECK_LAUNCH("rp3_scores_kernel");
  return 0;
}

int64_t rk_rp3_user_workspace_bytes(int32_t n_users) {
  if (n_users < 1) {
    rk_side_set_error("%s: n_users must be >= 1", __func__);
    return -2;
  }
  if (n_users <= FT_LDS_ITEMS) return 256;
  return 256 + (int64_t)FT_GROUPS * 2 * ft_acc_stride(n_users) * 4;
}

int rk_rp3_user_neighbours(const int64_t *q_indptr, const int32_t *q_indices, const int64_t *t_indptr,
                           const int32_t *t_indices, int32_t n_users, int32_t n_items, const float *un,
                           const float *qn, float shrink, int32_t N, int32_t row_lo, int32_t row_hi,
                           int32_t *nbr_ids, float *nbr_sim, int32_t *nbr_count, void *ws, int64_t ws_bytes,
                           void *stream) {
  RK_SIDE_REQUIRE(q_indptr && q_indices && t_indptr && t_indices && un && qn && nbr_ids && nbr_sim && nbr_count && ws,
                  "null pointer");
  RK_SIDE_REQUIRE(n_users >= 1 && n_users < INT_MAX - 2048 && n_items >= 1, "bad sizes");
  RK_SIDE_REQUIRE(N >= 1 && N <= FT_MAX_K, "N outside [1, rk_rp3_max_neighbours()]");
  RK_SIDE_REQUIRE(shrink >= 0.f && shrink <= 3.0e38f, "shrink must be finite and >= 0");
  RK_SIDE_REQUIRE(0 <= row_lo && row_lo <= row_hi, "bad row range");
  RK_SIDE_REQUIRE(ws_bytes >= rk_rp3_user_workspace_bytes(n_users), "workspace too small");
  RK_SIDE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
  if (row_lo == row_hi) return 0;
  hipStream_t s = (hipStream_t)stream;
  int *counter = (int *)ws;
  if (hipMemsetAsync(counter, 0, sizeof(int), s) != hipSuccess) {
    rk_side_set_error("%s: hipMemsetAsync failed", __func__);
    return -1;
  }
  const int rows = row_hi - row_lo;
  const int groups = rows < FT_GROUPS ? rows : FT_GROUPS;
  if (n_users <= FT_LDS_ITEMS) {
    hipLaunchKernelGGL(rp3_user_neighbours_kernel<false>, dim3(groups), dim3(FT_THREADS), 0, s, q_indptr, q_indices,
                       t_indptr, t_indices, n_users, n_items, un, qn, shrink, N, row_lo, row_hi, nbr_ids, nbr_sim,
                       nbr_count, counter, (float *)nullptr, (int *)nullptr, (int64_t)0);
  } else {
    const int64_t stride = ft_acc_stride(n_users);
    float *acc = (float *)((char *)ws + 256);
    int *cand = (int *)(acc + (int64_t)FT_GROUPS * stride);
    hipLaunchKernelGGL(rp3_user_neighbours_kernel<true>, dim3(groups), dim3(FT_THREADS), 0, s, q_indptr, q_indices,
                       t_indptr, t_indices, n_users, n_items, un, qn, shrink, N, row_lo, row_hi, nbr_ids, nbr_sim,
                       nbr_count, counter, acc, cand, stride);
  }
  RK_SIDE_CHECK_LAUNCH("rp3_user_neighbours_kernel");
  return 0;
}

int rk_rp3_user_scores(const int32_t *nbr_ids, const float *nbr_sim, const int32_t *nbr_count, int32_t n_rows,
                       int32_t N, const int64_t *u_indptr, const int32_t *u_indices, const float *u_data,
                       int32_t n_users, int32_t n_items, int32_t lo, int32_t hi, float *out, int64_t ldo,
                       void *stream) {
  RK_SIDE_REQUIRE(nbr_ids && nbr_sim && nbr_count && u_indptr && u_indices && out, "null pointer");
  RK_SIDE_REQUIRE(n_rows >= 0 && n_users >= 1 && n_items >= 1 && N >= 1 && N <= FT_MAX_K, "bad sizes");
  RK_SIDE_REQUIRE(0 <= lo && lo < hi && hi <= n_items && ldo >= hi - lo, "bad strip");
  if (n_rows == 0) return 0;
  const int width = hi - lo;
  const dim3 grid(n_rows, (width + SC_TILE - 1) / SC_TILE);
  hipLaunchKernelGGL(rp3_user_scores_kernel, grid, dim3(SC_WAVES * 64), 0, (hipStream_t)stream, nbr_ids, nbr_sim,
                     nbr_count, N, u_indptr, u_indices, u_data, n_users, lo, width, out, ldo);
  RK_SIDE_CHECK_LAUNCH("rp3_user_scores_kernel");
  return 0;
}

}  // extern "C"
