// The neighbour-list models (include/recoder_rp3.h, librecoder_rp3.so): RP3beta, ItemKNN and UserKNN.
//
// The three fits are one row pass (FtPass) with a model's accumulate and scale plugged in: one workgroup
// (16 waves) per row at a time, rows handed out through a counter.
//   accumulate: a row's values, one 32-bit word per candidate, in LDS (n <= FT_LDS_ITEMS) or in a row of the
//     workspace; the workspace form also lists the words it touches (a word's first touch is seen from its
//     fill), so that everything after costs the row's candidates, not n
//   scale: every candidate's word becomes the row's value for it
//   select: radix selection (4 x 8 bits) of the K-th largest float, then of the id up to which values equal to
//     it are kept
//   compact: the kept entries gathered in LDS, sorted by id (bitonic), written with padding
//
//   rk_rp3_fit (RP3beta, the sparse item-graph model), source item i:
//     accumulate: ft_walk_users; every wave walks the users of item i in order and adds user_w[v] to the
//       columns of user v it owns: one add chain per column, ascending users, no atomics on data
//     scale: W = (row_scale[i] * S) * col_scale[j], the diagonal 0
//   rk_rp3_item_fit (ItemKNN: cosine, asymmetric cosine, Tversky / Jaccard / Dice), own item j:
//     accumulate: ft_walk_users; the walked user's own value a_vj travels with it and a column i takes
//       fmaf(a_vj, a_vi, acc); without values (a template parameter) the chain is adds of 1.0
//     scale: s / (own[j] * oth[i] + shrink) or s / (own[j] + oth[i] + g * s + shrink): the shrink term and the
//       co-count in the denominator are what rk_rp3_fit's separable scale cannot spell
//   rk_rp3_user_neighbours (UserKNN, served from the training matrix itself), query row q:
//     accumulate: its own; c[v] = |H_q and H_v| by integer atomics on the workgroup's accumulators (a user's
//       first touch is the add that returns 0); an item with few users belongs to one wave, an item with many
//       is walked by all sixteen
//     scale: sim = c / (qn[q] * un[v] + shrink)
//
// The two scores kernels share their tiling (sc_begin, sc_store): one workgroup per (row, tile of 8192 columns
// held in LDS), each of its 8 waves owns 1024 columns.
//   rk_rp3_scores  a wave walks the user's entries in order, adding x * w of the neighbours that fall in its
//                  columns
//   rk_rp3_user_scores  a wave walks the query's neighbours in order; 64 neighbours at a time, a lane finds by
//                  binary search where its neighbour's row enters and leaves the wave's columns
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

// ------------------------------------------------------------------ row pass
// What the three fit kernels share.  A workgroup takes rows from a counter until none is left; a row's
// values are accumulated (by the model's own code) in n 32-bit words, a row in LDS or (WS) the workgroup's
// row of the workspace; finish() turns them into the row's values and hands them to ft_select_store.  WS
// also lists the words a row touches, so that everything after the accumulate costs the row's candidates,
// not n: a word's first touch is seen from its fill, and finish() puts the touched words back at it.
//   COUNTS false (RP3beta, ItemKNN): f32 sums, fill -0, a candidate list per wave (its entries in cnt[wave])
//   COUNTS true (UserKNN): integer counts made by atomics in L2, fill 0, one list (its entries in cnt[0]);
//     the counts are read and cleared at agent scope, past this CU's L1
template <bool WS>
struct FtState {                 // the workgroup's LDS
  int kid[FT_MAX_K];
  float kw[FT_MAX_K];
  int hist[256];
  int cnt[FT_WAVES];
  int sh[8];                     // 0: the row's offset; 1..4: ft_pick's answer; 5: entries gathered
  float acc[WS ? 1 : FT_LDS_ITEMS];      // (last: in front, WS's one unused word takes the arrays off their alignment
};                                       // and the selection past 64 VGPRs, the two-workgroups-per-CU budget)

template <bool WS, bool COUNTS>
struct FtPass {
  static constexpr int LISTS = COUNTS ? 1 : FT_WAVES;
  FtState<WS> &S;
  const int n, ch, tid, lane, wv;          // ch: entries of one candidate list
  float *acc;
  int *cand;

  __device__ __forceinline__ FtPass(FtState<WS> &S, int n, float *ws_acc, int *ws_cand, int64_t acc_stride, int ch)
      : S(S), n(n), ch(ch), tid(threadIdx.x), lane(tid & 63), wv(tid >> 6),
        acc(WS ? ws_acc + (int64_t)blockIdx.x * acc_stride : S.acc),
        cand(WS ? ws_cand + (int64_t)blockIdx.x * LISTS * ch : nullptr) {
    if (WS)
      for (int c = tid; c < n; c += FT_THREADS) acc[c] = COUNTS ? 0.f : -0.f;
  }

  // f(j) once per candidate j of the row, spread over the threads
  template <class F>
  __device__ __forceinline__ void for_cands(F f) const {
    if (!WS) {
      for (int j = tid; j < n; j += FT_THREADS) f(j);
    } else {
#pragma unroll 1
      for (int l = 0; l < LISTS; ++l) {
        const int c = S.cnt[l] < ch ? S.cnt[l] : ch;
        const int *L = cand + (int64_t)l * ch;
        for (int s = tid; s < c; s += FT_THREADS) f(L[s]);
      }
    }
  }

  // the workgroup's next row of [lo, hi), its accumulators at their start; -1 when none is left
  __device__ __forceinline__ int next_row(int *counter, int lo, int hi) {
    __syncthreads();
    if (tid == 0) {
      S.sh[0] = atomicAdd(counter, 1);
      if (COUNTS) S.cnt[0] = 0;
    }
    __syncthreads();
    const int64_t row = (int64_t)lo + S.sh[0];
    if (row >= hi) return -1;
    if (!WS) {
      for (int c = tid; c < n; c += FT_THREADS) acc[c] = 0.f;
      __syncthreads();
    }
    return (int)row;
  }

  // After the accumulate: candidate j's word becomes scale(j, the word's bits), the row's value; then
  // select, compact and store the row (ft_select_store) and leave the touched words at their fill.
  template <class Scale>
  __device__ __forceinline__ void finish(Scale scale, int K, int row, int32_t *__restrict__ nbr_ids,
                                         float *__restrict__ nbr_w, int32_t *__restrict__ nbr_count) {
    if (tid < 256) S.hist[tid] = 0;
    if (tid == 0) S.sh[5] = 0;
    if (WS && COUNTS) __threadfence();         // (the adds were made in L2: nothing of this row is read before them)
    __syncthreads();

    // ---- scale, and the histogram of the top byte
    for_cands([&](int j) {
      const uint32_t a = WS && COUNTS ? __hip_atomic_load(reinterpret_cast<unsigned int *>(acc + j), __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT)
                                      : f2u(acc[j]);
      const float w = scale(j, a);
      acc[j] = w;
      if (w > 0.f) atomicAdd(&S.hist[f2u(w) >> 24], 1);
    });
    __syncthreads();

    ft_select_store(acc, [&](auto f) { for_cands(f); }, K, n, row, nbr_ids, nbr_w, nbr_count, S.hist, S.sh, S.kid,
                    S.kw, tid, lane, wv);
    if (WS)
      for_cands([&](int j) {
        if (COUNTS)
          __hip_atomic_store(reinterpret_cast<unsigned int *>(acc + j), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
          acc[j] = -0.f;
      });
  }
};

// The accumulate of the two item models: every wave walks the users of item ``row`` in order and updates the
// columns of each user that it owns (64-column granules, round robin over the waves): one chain per column,
// ascending users, no atomics on data.  (user, row start, row end, m.payload) are fetched 64 at a time, as
// rk_ease_gram does, and a column takes m.update(its value so far, the user's payload, m.value(the entry)).
template <bool WS, class Model>
__device__ __forceinline__ void ft_walk_users(FtPass<WS, false> &ps, const Model &m, int row,
                                              const int64_t *__restrict__ t_indptr,
                                              const int32_t *__restrict__ t_indices,
                                              const int64_t *__restrict__ u_indptr,
                                              const int32_t *__restrict__ u_indices, int n_users) {
  const int lane = ps.lane, wv = ps.wv, n = ps.n, ch = ps.ch;
  float *acc = ps.acc;
  int *mylist = WS ? ps.cand + (int64_t)wv * ch : nullptr;
  int mycnt = 0;
  const int64_t e0 = t_indptr[row], e1 = t_indptr[row + 1];
  for (int64_t eb = e0; eb < e1; eb += 64) {
    const int cnt = e1 - eb < 64 ? (int)(e1 - eb) : 64;
    int64_t r0 = 0, r1 = 0;
    float pay = 0.f;
    if (lane < cnt) {
      const int u = t_indices[eb + lane];
      if (u >= 0 && u < n_users) {           // (a bad index reads nothing)
        r0 = u_indptr[u];
        r1 = u_indptr[u + 1];
        pay = m.payload(eb + lane, u);
      }
    }
    for (int l = 0; l < cnt; ++l) {
      const int64_t p0 = __shfl(r0, l, 64), p1 = __shfl(r1, l, 64);
      const float a = __shfl(pay, l, 64);
      for (int64_t p = p0; p < p1; p += 64) {       // (wave-uniform bounds)
        const int64_t q = p + lane;
        int c = 0;
        float x = 1.f;
        bool mine = false;
        if (q < p1) {
          c = u_indices[q];
          mine = c >= 0 && c < n && ((c >> 6) & (FT_WAVES - 1)) == wv;
          if (mine) x = m.value(q);
        }
        // columns of one user are distinct: no two lanes meet.  A first touch starts the chain from +0: an
        // update's term is >= +0, so that is bitwise the chain of the LDS form
        bool first = false;
        if (mine) {
          const float old = acc[c];
          first = WS && f2u(old) == FT_UNTOUCHED;
          acc[c] = m.update(first ? 0.f : old, a, x);
        }
        if (WS) {
          const unsigned long long mask = __ballot(first);
          if (first) {
            const int pos = mycnt + __popcll(mask & ((1ull << lane) - 1ull));
            if (pos < ch) mylist[pos] = c;
          }
          mycnt += __popcll(mask);
          // the next user's updates may come from other lanes of this wave: the fence keeps them behind these stores
          __threadfence_block();
        }
      }
    }
  }
  if (WS && lane == 0) ps.S.cnt[wv] = mycnt;
}

// --------------------------------------------------------------------- RP3beta
struct Rp3Walk {                 // the walked user's weight travels with it and is added to every column
  const float *__restrict__ user_w;
  __device__ __forceinline__ float payload(int64_t, int u) const { return user_w[u]; }
  __device__ __forceinline__ float value(int64_t) const { return 1.f; }
  __device__ __forceinline__ float update(float s, float w, float) const { return s + w; }
};

template <bool WS>
__global__ __launch_bounds__(FT_THREADS) void rp3_fit_kernel(
    const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_indices,
    const int64_t *__restrict__ u_indptr, const int32_t *__restrict__ u_indices, int n_users, int n,
    const float *__restrict__ user_w, const float *__restrict__ row_scale, const float *__restrict__ col_scale,
    int K, int row_lo, int row_hi, int32_t *__restrict__ nbr_ids, float *__restrict__ nbr_w,
    int32_t *__restrict__ nbr_count, int *counter, float *ws_acc, int *ws_cand, int64_t acc_stride, int ch) {
  __shared__ FtState<WS> S;
  FtPass<WS, false> ps(S, n, ws_acc, ws_cand, acc_stride, ch);
  const Rp3Walk walk{user_w};
  for (int i; (i = ps.next_row(counter, row_lo, row_hi)) >= 0;) {
    ft_walk_users(ps, walk, i, t_indptr, t_indices, u_indptr, u_indices, n_users);
    const float rs = row_scale[i];
    ps.finish([&](int j, uint32_t s) {
      return j == i ? 0.f : __fmul_rn(__fmul_rn(rs, __uint_as_float(s)), col_scale[j]);
    }, K, i, nbr_ids, nbr_w, nbr_count);
  }
}

// --------------------------------------------------------------------- ItemKNN
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

// the walked user's value for the own item travels with it: one fmaf chain per column; DATA false: t_data /
// u_data are not read, every value is 1.0 and the chain is adds of 1.0
template <bool DATA>
struct ItemWalk {
  const float *__restrict__ t_data, *__restrict__ u_data;
  __device__ __forceinline__ float payload(int64_t e, int) const { return DATA ? t_data[e] : 1.f; }
  __device__ __forceinline__ float value(int64_t q) const { return DATA ? u_data[q] : 1.f; }
  __device__ __forceinline__ float update(float s, float a, float x) const { return DATA ? fmaf(a, x, s) : s + 1.f; }
};

template <bool WS, bool DATA>
__global__ __launch_bounds__(FT_THREADS) void rp3_item_fit_kernel(
    const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_indices, const float *__restrict__ t_data,
    const int64_t *__restrict__ u_indptr, const int32_t *__restrict__ u_indices, const float *__restrict__ u_data,
    int n_users, int n, const float *__restrict__ own, const float *__restrict__ oth, int form, float g,
    float shrink, int K, int col_lo, int col_hi, int32_t *__restrict__ nbr_ids, float *__restrict__ nbr_w,
    int32_t *__restrict__ nbr_count, int *counter, float *ws_acc, int *ws_cand, int64_t acc_stride, int ch) {
  __shared__ FtState<WS> S;
  FtPass<WS, false> ps(S, n, ws_acc, ws_cand, acc_stride, ch);
  const ItemWalk<DATA> walk{t_data, u_data};
  for (int j; (j = ps.next_row(counter, col_lo, col_hi)) >= 0;) {
    ft_walk_users(ps, walk, j, t_indptr, t_indices, u_indptr, u_indices, n_users);
    const float oj = own[j];
    ps.finish([&](int i, uint32_t s) {
      return i == j ? 0.f : it_sim(__uint_as_float(s), oj, oth[i], form, g, shrink);
    }, K, j, nbr_ids, nbr_w, nbr_count);
  }
}

// --------------------------------------------------------------------- UserKNN
constexpr int UN_WIDE = 256;                  // an item with at least this many users is walked by every wave

// c / ((qs * u) + shrink): three f32 operations, each correctly rounded.  hipcc's default -ffp-contract=fast
// would fuse the product and the sum into one fma (__fmul_rn / __fadd_rn are plain * and + to it), hence the pragma
__device__ inline float un_sim(float c, float qs, float u, float shrink) {
#pragma clang fp contract(off)
  const float prod = qs * u;
  const float den = prod + shrink;
  return __fdiv_rn(c, den);
}

// (a word holds a count while a row accumulates and the similarity afterwards.  The accumulate is this
// kernel's own: integer adds commute, so an item with few users belongs to one wave, an item with many is
// walked by all sixteen, and a user's first touch is the add that returns 0)
template <bool WS>
__global__ __launch_bounds__(FT_THREADS) void rp3_user_neighbours_kernel(
    const int64_t *__restrict__ q_indptr, const int32_t *__restrict__ q_indices,
    const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_indices, int n_users, int n,
    const float *__restrict__ un, const float *__restrict__ qn, float shrink, int K, int row_lo, int row_hi,
    int32_t *__restrict__ nbr_ids, float *__restrict__ nbr_sim, int32_t *__restrict__ nbr_count, int *counter,
    float *ws_acc, int *ws_cand, int64_t acc_stride) {
  __shared__ FtState<WS> S;
  FtPass<WS, true> ps(S, n_users, ws_acc, ws_cand, acc_stride, (int)acc_stride);
  const int lane = ps.lane, wv = ps.wv;
  float *acc = ps.acc;
  for (int q; (q = ps.next_row(counter, row_lo, row_hi)) >= 0;) {
    // ---- accumulate: (row start, row end) of 64 query items at a time
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
              if (lane == 0) base = atomicAdd(&S.cnt[0], __popcll(m));
              base = __shfl(base, 0, 64);
              const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
              if (first && pos < ps.ch) ps.cand[pos] = v;
            }
          } else {
            if (v >= 0) atomicAdd(reinterpret_cast<unsigned int *>(acc + v), 1u);
          }
        }
      }
    }
    const float qs = qn[q];
    ps.finish([&](int v, uint32_t c) { return c ? un_sim((float)c, qs, un[v], shrink) : 0.f; }, K, q, nbr_ids, nbr_sim,
              nbr_count);
  }
}

// --------------------------------------------------------------------- scores
constexpr int SC_WAVES = 8;
constexpr int SC_SUB = 1024;                  // columns a wave owns
constexpr int SC_TILE = SC_WAVES * SC_SUB;    // 32 KB of LDS

// a scores workgroup's start: the calling wave's columns of the tile (returned) at 0, [wlo, whi) their range
// in the catalogue (empty past the strip's end)
__device__ __forceinline__ float *sc_begin(float *tile, int lo, int width, int64_t &wlo, int64_t &whi) {
  const int t0 = blockIdx.y * SC_TILE;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  wlo = (int64_t)lo + t0 + wv * SC_SUB;
  whi = wlo + SC_SUB < (int64_t)lo + width ? wlo + SC_SUB : (int64_t)lo + width;
  float *mine = tile + wv * SC_SUB;
  for (int c = lane; c < SC_SUB; c += 64) mine[c] = 0.f;
  return mine;
}

// ... and its end: the tile's columns inside the strip written to row ``r`` of out
__device__ __forceinline__ void sc_store(const float *tile, int r, int width, float *__restrict__ out, int64_t ldo) {
  __syncthreads();
  const int t0 = blockIdx.y * SC_TILE;
  const int w = width - t0 < SC_TILE ? width - t0 : SC_TILE;
  float *row = out + (int64_t)r * ldo + t0;
  for (int c = threadIdx.x; c < w; c += SC_WAVES * 64) row[c] = tile[c];
}

__global__ __launch_bounds__(SC_WAVES * 64) void rp3_scores_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const float *__restrict__ data,
    int n_items, const int32_t *__restrict__ nbr_ids, const float *__restrict__ nbr_w,
    const int32_t *__restrict__ nbr_count, int K, int lo, int width, float *__restrict__ out, int64_t ldo) {
  __shared__ float tile[SC_TILE];
  const int u = blockIdx.x;                             // (users fastest: neighbours share a column tile)
  const int lane = threadIdx.x & 63;
  int64_t wlo, whi;
  float *mine = sc_begin(tile, lo, width, wlo, whi);
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
  sc_store(tile, u, width, out, ldo);
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
  const int lane = threadIdx.x & 63;
  int64_t wlo, whi;
  float *mine = sc_begin(tile, lo, width, wlo, whi);
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
  sc_store(tile, q, width, out, ldo);
}

// What the three fits do on the host after their own argument checks (fn: the entry point, for the
// messages; n: the accumulators of a row; need: the entry point's workspace bytes): the workspace checks,
// nothing for an empty range, the counter at 0, then launch(kernel, groups, counter, acc, cand, stride, ch)
// with the LDS form (no accumulators in the workspace) or with the workspace form, whose accumulator rows
// and candidate lists follow the counter's 256 bytes.
template <class Kernel, class Launch>
int ft_run(const char *fn, const char *kernel_name, Kernel lds_form, Kernel ws_form, int n, int lo, int hi, void *ws,
           int64_t ws_bytes, int64_t need, hipStream_t s, Launch launch) {
  const char *bad = ws_bytes < need ? "workspace too small"
                    : (reinterpret_cast<uintptr_t>(ws) & 255) != 0 ? "workspace must be 256-byte aligned" : nullptr;
  if (bad) {
    rk_side_set_error("%s: %s", fn, bad);
    return -2;
  }
  if (lo == hi) return 0;
  int *counter = (int *)ws;
  if (hipMemsetAsync(counter, 0, sizeof(int), s) != hipSuccess) {
    rk_side_set_error("%s: hipMemsetAsync failed", fn);
    return -1;
  }
  const int groups = hi - lo < FT_GROUPS ? hi - lo : FT_GROUPS;
  if (n <= FT_LDS_ITEMS) {
    launch(lds_form, groups, counter, (float *)nullptr, (int *)nullptr, (int64_t)0, 0);
  } else {
    const int64_t stride = ft_acc_stride(n);
    float *acc = (float *)((char *)ws + 256);
    launch(ws_form, groups, counter, acc, (int *)(acc + (int64_t)FT_GROUPS * stride), stride, (int)ft_list_stride(n));
  }
  RK_SIDE_CHECK_LAUNCH(kernel_name);
  return 0;
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
  hipStream_t s = (hipStream_t)stream;
  return ft_run(__func__, "rp3_fit_kernel", rp3_fit_kernel<false>, rp3_fit_kernel<true>, n_items, row_lo, row_hi, ws,
                ws_bytes, rk_rp3_fit_workspace_bytes(n_items), s,
                [&](auto kernel, int groups, int *counter, float *acc, int *cand, int64_t stride, int ch) {
                  hipLaunchKernelGGL(kernel, dim3(groups), dim3(FT_THREADS), 0, s, t_indptr, t_indices, u_indptr,
                                     u_indices, n_users, n_items, user_w, row_scale, col_scale, K, row_lo, row_hi,
                                     nbr_ids, nbr_w, nbr_count, counter, acc, cand, stride, ch);
                });
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
  hipStream_t s = (hipStream_t)stream;
  const bool data = t_data != nullptr;
  return ft_run(__func__, "rp3_item_fit_kernel",
                data ? rp3_item_fit_kernel<false, true> : rp3_item_fit_kernel<false, false>,
                data ? rp3_item_fit_kernel<true, true> : rp3_item_fit_kernel<true, false>, n_items, col_lo, col_hi, ws,
                ws_bytes, rk_rp3_item_workspace_bytes(n_items), s,
                [&](auto kernel, int groups, int *counter, float *acc, int *cand, int64_t stride, int ch) {
                  hipLaunchKernelGGL(kernel, dim3(groups), dim3(FT_THREADS), 0, s, t_indptr, t_indices, t_data,
                                     u_indptr, u_indices, u_data, n_users, n_items, own, oth, form, g, shrink, K, col_lo,
                                     col_hi, nbr_ids, nbr_w, nbr_count, counter, acc, cand, stride, ch);
                });
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
  hipStream_t s = (hipStream_t)stream;
  return ft_run(__func__, "rp3_user_neighbours_kernel", rp3_user_neighbours_kernel<false>,
                rp3_user_neighbours_kernel<true>, n_users, row_lo, row_hi, ws, ws_bytes,
                rk_rp3_user_workspace_bytes(n_users), s,
                [&](auto kernel, int groups, int *counter, float *acc, int *cand, int64_t stride, int) {
                  hipLaunchKernelGGL(kernel, dim3(groups), dim3(FT_THREADS), 0, s, q_indptr, q_indices, t_indptr,
                                     t_indices, n_users, n_items, un, qn, shrink, N, row_lo, row_hi, nbr_ids, nbr_sim,
                                     nbr_count, counter, acc, cand, stride);      // (one list of stride entries)
                });
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
