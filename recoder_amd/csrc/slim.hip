// SLIM: the sparse linear item model (include/recoder_slim.h, librecoder_slim.so).
//
//   rk_slim_fit     one wave (a workgroup of 64 threads) per column j at a time, columns handed out through a
//                   counter.
//                   candidates: two passes over row j of G (count, then fill): {k != j : G[j][k] > l1} ascending,
//                     with q = G[j][k], w = +0, G[k][k] and inv_denom[k] beside them, in LDS (up to SL_LDS_CANDS)
//                     or in the workgroup's slice of the workspace
//                   sweep: the wave evaluates the update of 64 coordinates at once from the current state,
//                     ballots for the first whose weight changes, applies it (every lane updates its q entries
//                     from row k of G: element-wise, no reduction) and evaluates again from the coordinate
//                     behind it.  A coordinate whose new weight equals the old one leaves the state as it is,
//                     so this is the sequential sweep bit for bit
//                   cut: a bisection on the float bits finds the K-th largest weight, ties at it go to the
//                     lower ids; the candidates are ascending, so an ordered compaction stores ascending ids
//   rk_slim_fit_sparse  fsSLIM: column j over its candidate list only, a workgroup of four waves per column at a time,
//                   columns handed out through a counter.
//                   local Gram: the candidate list (ascending) sits in LDS; the waves take the candidate rows
//                     through a counter in LDS.  The wave of row c walks the users v of candidate c in ascending
//                     order, 64 of them fetched at a time, and one user after the other: the lanes take the items
//                     of v, look each up in the candidate list by binary search and step
//                     L[c][c'] = fmaf(a_vc, a_vc', L[c][c']) (q[c] where the item is j itself).  A user holds an item
//                     once, so the lanes of one step touch different entries; no atomics, no reductions
//                   screen: wave 0 compacts the candidates with q > l1 into the state of rk_slim_fit's sweep
//                   sweep and cut: sl_sweep_cut, the code rk_slim_fit runs, reading rows of L through the
//                     candidates' positions where the dense kernel reads rows of G through their ids
//                   L and the state live in LDS up to SLS_LDS_CANDS candidates, else in the workgroup's slice
//                     of the workspace
//   rk_slim_scores  one thread per (user, column): the column's kept entries in order, each looked up in the
//                   user's ascending indices by a binary search that starts behind the last one
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/recoder_slim.h"
#include "side_error.h"
#include "side_explain.h"      // rk_slim_explain: the order, the selection and the one-wave kernel

namespace {

// ------------------------------------------------------------------------ fit
constexpr int SL_LDS_CANDS = 960;             // 5 arrays x 960 x 4 B = 18.75 KB: eight workgroups on a CU's 160 KB
constexpr int SL_MAX_K = 1024;
constexpr int SL_GROUPS = 2048;               // resident workgroups: eight waves on each of the 256 CUs
constexpr int SL_ARRAYS = 5;                  // cand, q, w, G_kk, inv_denom

inline int64_t sl_stride(int n) { return ((int64_t)n + 63) / 64 * 64; }

__device__ inline uint32_t f2u(float v) { return __float_as_uint(v); }

__device__ inline int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// The Gram as the sweep reads it: entry (c, c') of the candidates is base[idx[c] * ld + idx[c']].  rk_slim_fit:
// G itself, idx = the candidates' ids; rk_slim_fit_sparse: the local Gram, idx = the candidates' positions in it.
struct SlGram {
  const float *base;
  int64_t ld;
  const int *idx;
};

// What orders a wave's writes of the state before its next reads of it: the workgroup's barrier where the
// workgroup is that one wave, a fence where other waves of the workgroup wait elsewhere.
struct SlBarrierSync {
  __device__ __forceinline__ static void sync() { __syncthreads(); }
};
struct SlWaveSync {
  __device__ __forceinline__ static void sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
};

__device__ __forceinline__ void sl_empty_column(int j, int K, int32_t *__restrict__ nbr_ids, float *__restrict__ nbr_w,
                                                int32_t *__restrict__ nbr_count, int32_t *__restrict__ col_sweeps,
                                                int32_t *__restrict__ col_support, int lane) {
  for (int c = lane; c < K; c += 64) {
    nbr_ids[(int64_t)j * K + c] = -1;
    nbr_w[(int64_t)j * K + c] = 0.f;
  }
  if (lane == 0) {
    nbr_count[j] = 0;
    col_sweeps[j] = 0;
    col_support[j] = 0;
  }
}

// The sweeps, the stop rule and the cut of column j with C candidates (0 < C), by one wave, from the filled state
// (cand ascending, q, w = +0, G_kk, inv_denom).
template <class Sync>
__device__ __forceinline__ void sl_sweep_cut(const SlGram gram, float l1, int K, int max_sweeps, float tol, int j,
                                             int C, const int *cand, float *q, float *w, const float *dg,
                                             const float *iv, int32_t *__restrict__ nbr_ids,
                                             float *__restrict__ nbr_w, int32_t *__restrict__ nbr_count,
                                             int32_t *__restrict__ col_sweeps, int32_t *__restrict__ col_support,
                                             int lane) {
  // ---- sweeps
  int sweeps = 0;
#pragma unroll 1
  for (int s = 0; s < max_sweeps; ++s) {
    ++sweeps;
    float maxd = 0.f;
#pragma unroll 1
    for (int b = 0; b < C; b += 64) {
      const int c = b + lane;
      const bool in = c < C;
      const float dk = in ? dg[c] : 0.f, ik = in ? iv[c] : 0.f;
      int done = b;                            // coordinates below are finished in this sweep
#pragma unroll 1
      for (;;) {                               // (at most 64 rounds: done grows every time)
        float nw = 0.f, dl = 0.f;
        if (in && c >= done) {
          const float wc = w[c];
          const float t = fmaf(dk, wc, q[c]);
          nw = t > l1 ? __fmul_rn(__fsub_rn(t, l1), ik) : 0.f;
          dl = __fsub_rn(nw, wc);
        }
        const unsigned long long m = __ballot(dl != 0.f);
        if (m == 0) break;
        const int f = __ffsll((long long)m) - 1;
        const float delta = __shfl(dl, f, 64), nv = __shfl(nw, f, 64);
        const float *rk = gram.base + (int64_t)gram.idx[b + f] * gram.ld;
        maxd = fmaxf(maxd, fabsf(delta));
        for (int c2 = lane; c2 < C; c2 += 64) q[c2] = fmaf(-delta, rk[gram.idx[c2]], q[c2]);
        if (lane == f) w[c] = nv;
        Sync::sync();
        done = b + f + 1;
      }
    }
    if (maxd <= tol) break;
  }

  // ---- the support, and the K-th largest weight when it is larger than K
  int S = 0;
  for (int b = 0; b < C; b += 64) S += __popcll(__ballot(b + lane < C && w[b + lane] > 0.f));
  const bool all = S <= K;
  uint32_t T = 0;
  int need = 0;
  if (!all) {
    // the largest T with at least K weights whose bits are >= T (weights > 0: the bits order as the values)
    uint32_t lo = 1u, hi = 0x7f800000u;
#pragma unroll 1
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo + 1u) / 2u;
      int ge = 0;
      for (int b = 0; b < C; b += 64) {
        const float v = b + lane < C ? w[b + lane] : 0.f;
        ge += __popcll(__ballot(v > 0.f && f2u(v) >= mid));
      }
      if (ge >= K) lo = mid; else hi = mid - 1u;
    }
    T = lo;
    int gt = 0;
    for (int b = 0; b < C; b += 64) {
      const float v = b + lane < C ? w[b + lane] : 0.f;
      gt += __popcll(__ballot(v > 0.f && f2u(v) > T));
    }
    need = K - gt;                             // how many of those equal to T are kept: the lowest ids
  }

  // ---- ordered compaction
  int kept = 0, eq = 0;
  for (int b = 0; b < C; b += 64) {
    const int c = b + lane;
    const float v = c < C ? w[c] : 0.f;
    const bool pos = v > 0.f;
    const bool iseq = pos && !all && f2u(v) == T;
    const unsigned long long me = __ballot(iseq);
    const bool keep = pos && (all || f2u(v) > T || (iseq && eq + lanes_below(me, lane) < need));
    const unsigned long long mk = __ballot(keep);
    const int p = kept + lanes_below(mk, lane);
    if (keep && p < K) {
      nbr_ids[(int64_t)j * K + p] = cand[c];
      nbr_w[(int64_t)j * K + p] = v;
    }
    kept += __popcll(mk);
    eq += __popcll(me);
  }
  kept = kept < K ? kept : K;
  for (int c = kept + lane; c < K; c += 64) {
    nbr_ids[(int64_t)j * K + c] = -1;
    nbr_w[(int64_t)j * K + c] = 0.f;
  }
  if (lane == 0) {
    nbr_count[j] = kept;
    col_sweeps[j] = sweeps;
    col_support[j] = S;
  }
}

// Column j of rk_slim_fit with C candidates (0 < C <= cap), the state in the five arrays (LDS or workspace).
__device__ __forceinline__ void sl_column(const float *__restrict__ G, int64_t ldg, int n,
                                          const float *__restrict__ inv_denom, float l1, int K, int max_sweeps,
                                          float tol, int j, int C, int *cand, float *q, float *w, float *dg,
                                          float *iv, int32_t *__restrict__ nbr_ids, float *__restrict__ nbr_w,
                                          int32_t *__restrict__ nbr_count, int32_t *__restrict__ col_sweeps,
                                          int32_t *__restrict__ col_support, int lane) {
  const float *row = G + (int64_t)j * ldg;
  // ---- fill (the same predicate as the count, so cnt ends at C)
  int cnt = 0;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    float g = 0.f;
    bool is = false;
    if (k < n) {
      g = row[k];
      is = k != j && g > l1;
    }
    const unsigned long long m = __ballot(is);
    const int pos = cnt + lanes_below(m, lane);
    if (is && pos < C) {
      cand[pos] = k;
      q[pos] = g;
      w[pos] = 0.f;
      dg[pos] = G[(int64_t)k * ldg + k];
      iv[pos] = inv_denom[k];
    }
    cnt += __popcll(m);
  }
  __syncthreads();

  sl_sweep_cut<SlBarrierSync>(SlGram{G, ldg, cand}, l1, K, max_sweeps, tol, j, C, cand, q, w, dg, iv, nbr_ids, nbr_w,
                              nbr_count, col_sweeps, col_support, lane);
}

__global__ __launch_bounds__(64) void slim_fit_kernel(
    const float *__restrict__ G, int64_t ldg, int n, const float *__restrict__ inv_denom, float l1, int K,
    int max_sweeps, float tol, int col_lo, int col_hi, int32_t *__restrict__ nbr_ids, float *__restrict__ nbr_w,
    int32_t *__restrict__ nbr_count, int32_t *__restrict__ col_sweeps, int32_t *__restrict__ col_support,
    int *counter, float *ws_state, int64_t stride) {
  __shared__ int l_cand[SL_LDS_CANDS];
  __shared__ float l_q[SL_LDS_CANDS], l_w[SL_LDS_CANDS], l_dg[SL_LDS_CANDS], l_iv[SL_LDS_CANDS];
  const int lane = threadIdx.x;
  float *g_base = ws_state + (int64_t)blockIdx.x * SL_ARRAYS * stride;

  for (;;) {
    __syncthreads();                           // (the state of the column before is no longer read)
    int t = 0;
    if (lane == 0) t = atomicAdd(counter, 1);
    t = __shfl(t, 0, 64);
    const int64_t j64 = (int64_t)col_lo + t;
    if (j64 >= col_hi) break;
    const int j = (int)j64;

    const float *row = G + (int64_t)j * ldg;
    int C = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
      const int k = k0 + lane;
      C += __popcll(__ballot(k < n && k != j && row[k] > l1));
    }
    if (C == 0) {
      sl_empty_column(j, K, nbr_ids, nbr_w, nbr_count, col_sweeps, col_support, lane);
    } else if (C <= SL_LDS_CANDS) {
      sl_column(G, ldg, n, inv_denom, l1, K, max_sweeps, tol, j, C, l_cand, l_q, l_w, l_dg, l_iv, nbr_ids, nbr_w,
                nbr_count, col_sweeps, col_support, lane);
    } else {                                   // (C <= n - 1 < stride)
      sl_column(G, ldg, n, inv_denom, l1, K, max_sweeps, tol, j, C, (int *)g_base, g_base + stride,
                g_base + 2 * stride, g_base + 3 * stride, g_base + 4 * stride, nbr_ids, nbr_w, nbr_count,
                col_sweeps, col_support, lane);
    }
  }
}

// ----------------------------------------------------------------- sparse fit
constexpr int SLS_THREADS = 256;              // four waves: the candidate rows of a column are split over them
constexpr int SLS_MAX_M = 1024;               // rk_rp3_max_neighbours(): the longest list the ItemKNN fit makes
// L [104, 104] (42.25 KB), the candidate list (4 KB) and the seven state arrays (2.8 KB) are 49 KB: three
// workgroups, twelve waves, on a CU's 160 KB.  The walk waits on dependent loads, so resident waves count.
constexpr int SLS_LDS_CANDS = 104;
constexpr int SLS_GROUPS = 768;               // resident workgroups: three on each of the 256 CUs
constexpr int SLS_ARRAYS = 7;                 // cand, q, w, G_kk, inv_denom, pos, the unscreened q

inline int64_t sls_pad(int M) { return ((int64_t)M + 63) / 64 * 64; }
inline int64_t sls_slice_floats(int M) { return sls_pad(M) * sls_pad(M) + SLS_ARRAYS * sls_pad(M); }

// Row c of the local Gram of column j, by one wave: L[c * Cj + c'] for every candidate c' and qraw[c].  The fence
// behind a user's steps orders them before the next user's, whose lanes may step the same entries (in LDS and in
// the workspace alike; it also keeps the compiler from holding qraw[c] in a register of one lane).
__device__ __forceinline__ void sls_build_row(
    const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_indices, const float *__restrict__ t_data,
    const int64_t *__restrict__ u_indptr, const int32_t *__restrict__ u_indices, const float *__restrict__ u_data,
    int n_users, int n, int j, int c, int Cj, const int *cid, float *L, float *qraw, int lane) {
  float *Lc = L + (int64_t)c * Cj;
  for (int c2 = lane; c2 < Cj; c2 += 64) Lc[c2] = 0.f;
  if (lane == 0) qraw[c] = 0.f;
  SlWaveSync::sync();
  const int k = cid[c];
  if (k < 0 || k >= n || k == j) return;     // (no candidate: the screen drops it, its row is never read)
  const int64_t e0 = t_indptr[k], e1 = t_indptr[k + 1];
#pragma unroll 1
  for (int64_t eb = e0; eb < e1; eb += 64) {
    // 64 users of candidate c at a time: their value for c and where their rows are
    float av = 0.f;
    long long st = 0;
    int rv = 0;
    if (eb + lane < e1) {
      const int v = t_indices[eb + lane];
      av = t_data ? t_data[eb + lane] : 1.f;
      if (v >= 0 && v < n_users) {
        st = u_indptr[v];
        rv = (int)(u_indptr[v + 1] - st);
      }
    }
    const int cnt = e1 - eb < 64 ? (int)(e1 - eb) : 64;
#pragma unroll 1
    for (int t = 0; t < cnt; ++t) {            // one user after the other, ascending: the order of every chain
      const float a = __shfl(av, t, 64);
      const long long s0 = __shfl(st, t, 64);
      const int r = __shfl(rv, t, 64);
      for (int off = lane; off < r; off += 64) {
        const int i = u_indices[s0 + off];
        const float x = u_data ? u_data[s0 + off] : 1.f;
        if (i == j) {
          qraw[c] = fmaf(a, x, qraw[c]);
        } else {
          int lo = 0, hi = Cj;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cid[mid] < i) lo = mid + 1; else hi = mid;
          }
          if (lo < Cj && cid[lo] == i) Lc[lo] = fmaf(a, x, Lc[lo]);
        }
      }
      SlWaveSync::sync();
    }
  }
}

// The arguments of the sparse fit as one kernel argument: the fields are read from the kernel-argument segment where
// they are used (the build, the screen and the sweep use disjoint sets), not held in scalar registers throughout.
struct SlsArgs {
  const int64_t *t_indptr;
  const int32_t *t_indices;
  const float *t_data;
  const int64_t *u_indptr;
  const int32_t *u_indices;
  const float *u_data;
  const int32_t *cand_ids, *cand_count;
  const float *inv_denom;
  int32_t *nbr_ids;
  float *nbr_w;
  int32_t *nbr_count, *col_sweeps, *col_support, *col_screened;
  int *counter;
  float *ws_state;
  int64_t slice_floats;
  int n_users, n, M, K, max_sweeps, col_lo, col_hi;
  float l1, tol;
};
typedef const __attribute__((address_space(4))) SlsArgs *SlsArgsSegment;

// The arguments where they lie in the kernel-argument segment (the struct is the kernel's only argument), through a
// pointer the compiler cannot see through: what a phase needs is fetched where the phase begins, with scalar loads,
// and nothing is hoisted to the kernel's entry to sit in scalar registers through the other phases.
__device__ __forceinline__ SlsArgsSegment sls_args() {
  SlsArgsSegment p = (SlsArgsSegment)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// Column j with Cj candidates in cid, by the four waves of the workgroup: the local Gram into L, then wave 0 alone
// screens, sweeps and cuts (the others return to the next column's barrier).  st: the seven state arrays of cap
// entries each.
__device__ __forceinline__ void sls_column(const SlsArgs &a, int j, int Cj, const int *l_cid, int *next, float *L,
                                           float *st, int cap, int lane, int wave) {
  float *qraw = st + 6 * cap;

  // ---- the local Gram: a wave takes the next candidate row
  for (;;) {
    int c = 0;
    if (lane == 0) c = atomicAdd(next, 1);
    c = __shfl(c, 0, 64);
    if (c >= Cj) break;
    SlsArgsSegment bp = sls_args();
    sls_build_row(bp->t_indptr, bp->t_indices, bp->t_data, bp->u_indptr, bp->u_indices, bp->u_data, bp->n_users, bp->n, j,
                  c, Cj, l_cid, L, qraw, lane);
  }
  __syncthreads();
  if (wave != 0) return;
  SlsArgsSegment op = sls_args();             // (the outputs, inv_denom, the sweep's numbers)

  // ---- the screen: the candidates with q > op->l1, in order, into the state of the sweep
  int *cand = (int *)st, *pos = (int *)(st + 5 * cap);
  float *q = st + cap, *w = st + 2 * cap, *dg = st + 3 * cap, *iv = st + 4 * cap;
  int C = 0;
  for (int b = 0; b < Cj; b += 64) {
    const int c = b + lane;
    int k = -1;
    float g = 0.f;
    if (c < Cj) {
      k = l_cid[c];
      g = qraw[c];
    }
    const bool is = k >= 0 && k < op->n && k != j && g > op->l1;
    const unsigned long long m = __ballot(is);
    const int p = C + lanes_below(m, lane);
    if (is) {
      cand[p] = k;
      pos[p] = c;
      q[p] = g;
      w[p] = 0.f;
      dg[p] = L[(int64_t)c * Cj + c];
      iv[p] = op->inv_denom[k];
    }
    C += __popcll(m);
  }
  SlWaveSync::sync();
  if (op->col_screened && lane == 0) op->col_screened[j] = C;
  if (C == 0)
    sl_empty_column(j, op->K, op->nbr_ids, op->nbr_w, op->nbr_count, op->col_sweeps, op->col_support, lane);
  else
    sl_sweep_cut<SlWaveSync>(SlGram{L, Cj, pos}, op->l1, op->K, op->max_sweeps, op->tol, j, C, cand, q, w, dg, iv, op->nbr_ids, op->nbr_w,
                             op->nbr_count, op->col_sweeps, op->col_support, lane);
}

__global__ __launch_bounds__(SLS_THREADS) void slim_fit_sparse_kernel(const SlsArgs a) {
  __shared__ float l_L[SLS_LDS_CANDS * SLS_LDS_CANDS];
  __shared__ float l_state[SLS_ARRAYS * SLS_LDS_CANDS];
  __shared__ int l_cid[SLS_MAX_M];
  __shared__ int l_col, l_next;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float *g_base = a.ws_state + (int64_t)blockIdx.x * a.slice_floats;

  for (;;) {
    __syncthreads();                           // (the column before is finished: its state is no longer read)
    if (tid == 0) {
      l_col = atomicAdd(a.counter, 1);
      l_next = 0;
    }
    __syncthreads();
    const int64_t j64 = (int64_t)a.col_lo + l_col;
    if (j64 >= a.col_hi) break;
    const int j = (int)j64;
    int Cj = a.cand_count[j];
    Cj = Cj < 0 ? 0 : (Cj > a.M ? a.M : Cj);
    for (int c = tid; c < Cj; c += SLS_THREADS) l_cid[c] = a.cand_ids[(int64_t)j * a.M + c];
    __syncthreads();

    // (two instances of the column: in the LDS one every state pointer is a constant of the kernel)
    if (Cj <= SLS_LDS_CANDS)
      sls_column(a, j, Cj, l_cid, &l_next, l_L, l_state, SLS_LDS_CANDS, lane, wave);
    else                                       // (Cj <= M <= the padded M of the slice)
      sls_column(a, j, Cj, l_cid, &l_next, g_base, g_base + (int64_t)Cj * Cj, Cj, lane, wave);
  }
}

// --------------------------------------------------------------------- scores
constexpr int SC_THREADS = 256;

__global__ __launch_bounds__(SC_THREADS) void slim_scores_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const float *__restrict__ data,
    const int32_t *__restrict__ nbr_ids, const float *__restrict__ nbr_w, const int32_t *__restrict__ nbr_count,
    int K, int lo, int width, float *__restrict__ out, int64_t ldo) {
  const int u = blockIdx.x;                             // (users fastest: neighbours share the columns' entries)
  const int c = blockIdx.y * SC_THREADS + threadIdx.x;
  if (c >= width) return;
  const int64_t e0 = indptr[u];
  const int64_t len = indptr[u + 1] - e0;
  float acc = 0.f;
  if (len > 0) {
    const int64_t j = (int64_t)lo + c;
    int cnt = nbr_count[j];
    cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);
    const int32_t *ids = nbr_ids + j * K;
    const float *wj = nbr_w + j * K;
    const int32_t *ui = indices + e0;
    int64_t from = 0;                                   // both lists ascend: the next search starts here
    for (int s = 0; s < cnt && from < len; ++s) {
      const int k = ids[s];
      int64_t a = from, b = len;
      while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (ui[mid] < k) a = mid + 1; else b = mid;
      }
      from = a;
      if (a < len && ui[a] == k) acc = fmaf(data ? data[e0 + a] : 1.f, wj[s], acc);
    }
  }
  out[(int64_t)u * ldo + c] = acc;
}

// ----------------------------------------------------------------- explanations
// W[i][j] of a neighbour-list model: the list of column j (columns) or of row i searched for the other id.  The
// lists ascend, as every fit stores them; a pair the list does not hold is +0.
struct XpListFetch {
  const int32_t *ids;
  const float *w;
  const int32_t *count;
  int K, columns;
  __device__ __forceinline__ float operator()(int i, int j) const {
    const int list = columns ? j : i, key = columns ? i : j;
    int cnt = count[list];
    cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);
    const int32_t *l = ids + (int64_t)list * K;
    int a = 0, b = cnt;
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (l[mid] < key) a = mid + 1; else b = mid;
    }
    return (a < cnt && l[a] == key) ? w[(int64_t)list * K + a] : 0.f;
  }
};

}  // namespace

// ------------------------------------------------------------------------ ABI
extern "C" {

int rk_slim_version(void) { return 101; }

const char *rk_slim_last_error(void) { return g_rk_side_err; }

int rk_slim_max_neighbours(void) { return SL_MAX_K; }

int rk_slim_lds_candidates(void) { return SL_LDS_CANDS; }

int64_t rk_slim_fit_workspace_bytes(int32_t n_items) {
  if (n_items < 1) {
    rk_side_set_error("%s: n_items must be >= 1", __func__);
    return -2;
  }
  if (n_items <= SL_LDS_CANDS) return 256;              // (at most n - 1 candidates: the LDS always holds them)
  return 256 + (int64_t)SL_GROUPS * SL_ARRAYS * sl_stride(n_items) * 4;
}

int rk_slim_fit(const float *G, int64_t ldg, int32_t n_items, const float *inv_denom, float l1, int32_t K,
                int32_t max_sweeps, float tol, int32_t col_lo, int32_t col_hi, int32_t *nbr_ids, float *nbr_w,
                int32_t *nbr_count, int32_t *col_sweeps, int32_t *col_support, void *ws, int64_t ws_bytes,
                void *stream) {
  RK_SIDE_REQUIRE(G && inv_denom && nbr_ids && nbr_w && nbr_count && col_sweeps && col_support && ws, "null pointer");
  RK_SIDE_REQUIRE(n_items >= 1 && n_items < INT_MAX - 2048 && ldg >= n_items, "bad sizes");
  RK_SIDE_REQUIRE(K >= 1 && K <= SL_MAX_K, "K outside [1, rk_slim_max_neighbours()]");
  RK_SIDE_REQUIRE(l1 >= 0.f && l1 < INFINITY, "l1 must be finite and >= 0");
  RK_SIDE_REQUIRE(tol >= 0.f, "tol must be >= 0");
  RK_SIDE_REQUIRE(max_sweeps >= 1, "max_sweeps must be >= 1");
  RK_SIDE_REQUIRE(0 <= col_lo && col_lo <= col_hi && col_hi <= n_items, "bad column range");
  RK_SIDE_REQUIRE(ws_bytes >= rk_slim_fit_workspace_bytes(n_items), "workspace too small");
  RK_SIDE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
  if (col_lo == col_hi) return 0;
  hipStream_t s = (hipStream_t)stream;
  int *counter = (int *)ws;
  if (hipMemsetAsync(counter, 0, sizeof(int), s) != hipSuccess) {
    rk_side_set_error("%s: hipMemsetAsync failed", __func__);
    return -1;
  }
  const int cols = col_hi - col_lo;
  const int groups = cols < SL_GROUPS ? cols : SL_GROUPS;
  hipLaunchKernelGGL(slim_fit_kernel, dim3(groups), dim3(64), 0, s, G, ldg, n_items, inv_denom, l1, K, max_sweeps,
                     tol, col_lo, col_hi, nbr_ids, nbr_w, nbr_count, col_sweeps, col_support, counter,
                     (float *)((char *)ws + 256), sl_stride(n_items));
  RK_SIDE_CHECK_LAUNCH("slim_fit_kernel");
  return 0;
}

int rk_slim_sparse_lds_candidates(void) { return SLS_LDS_CANDS; }

int64_t rk_slim_fit_sparse_workspace_bytes(int32_t M) {
  if (M < 1 || M > SLS_MAX_M) {
    rk_side_set_error("%s: M outside [1, %d]", __func__, SLS_MAX_M);
    return -2;
  }
  if (M <= SLS_LDS_CANDS) return 256;                   // (at most M candidates: the LDS always holds them)
  return 256 + (int64_t)SLS_GROUPS * sls_slice_floats(M) * 4;
}

int rk_slim_fit_sparse(const int64_t *t_indptr, const int32_t *t_indices, const float *t_data, const int64_t *u_indptr,
                       const int32_t *u_indices, const float *u_data, int32_t n_users, int32_t n_items,
                       const int32_t *cand_ids, const int32_t *cand_count, int32_t M, const float *inv_denom, float l1,
                       int32_t K, int32_t max_sweeps, float tol, int32_t col_lo, int32_t col_hi, int32_t *nbr_ids,
                       float *nbr_w, int32_t *nbr_count, int32_t *col_sweeps, int32_t *col_support,
                       int32_t *col_screened, void *ws, int64_t ws_bytes, void *stream) {
  RK_SIDE_REQUIRE(t_indptr && t_indices && u_indptr && u_indices && cand_ids && cand_count && inv_denom && nbr_ids &&
                  nbr_w && nbr_count && col_sweeps && col_support && ws, "null pointer");
  RK_SIDE_REQUIRE((t_data == nullptr) == (u_data == nullptr), "t_data and u_data must both be given or both be NULL");
  RK_SIDE_REQUIRE(n_users >= 0 && n_items >= 1 && n_items < INT_MAX - 2048, "bad sizes");
  RK_SIDE_REQUIRE(M >= 1 && M <= SLS_MAX_M, "M outside [1, rk_rp3_max_neighbours()]");
  RK_SIDE_REQUIRE(K >= 1 && K <= SL_MAX_K, "K outside [1, rk_slim_max_neighbours()]");
  RK_SIDE_REQUIRE(l1 >= 0.f && l1 < INFINITY, "l1 must be finite and >= 0");
  RK_SIDE_REQUIRE(tol >= 0.f, "tol must be >= 0");
  RK_SIDE_REQUIRE(max_sweeps >= 1, "max_sweeps must be >= 1");
  RK_SIDE_REQUIRE(0 <= col_lo && col_lo <= col_hi && col_hi <= n_items, "bad column range");
  RK_SIDE_REQUIRE(ws_bytes >= rk_slim_fit_sparse_workspace_bytes(M), "workspace too small");
  RK_SIDE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
  if (col_lo == col_hi) return 0;
  hipStream_t s = (hipStream_t)stream;
  int *counter = (int *)ws;
  if (hipMemsetAsync(counter, 0, sizeof(int), s) != hipSuccess) {
    rk_side_set_error("%s: hipMemsetAsync failed", __func__);
    return -1;
  }
  const int cols = col_hi - col_lo;
  const int groups = cols < SLS_GROUPS ? cols : SLS_GROUPS;
  SlsArgs a;
  a.t_indptr = t_indptr; a.t_indices = t_indices; a.t_data = t_data;
  a.u_indptr = u_indptr; a.u_indices = u_indices; a.u_data = u_data;
  a.cand_ids = cand_ids; a.cand_count = cand_count; a.inv_denom = inv_denom;
  a.nbr_ids = nbr_ids; a.nbr_w = nbr_w; a.nbr_count = nbr_count;
  a.col_sweeps = col_sweeps; a.col_support = col_support; a.col_screened = col_screened;
  a.counter = counter; a.ws_state = (float *)((char *)ws + 256); a.slice_floats = sls_slice_floats(M);
  a.n_users = n_users; a.n = n_items; a.M = M; a.K = K; a.max_sweeps = max_sweeps;
  a.col_lo = col_lo; a.col_hi = col_hi; a.l1 = l1; a.tol = tol;
  hipLaunchKernelGGL(slim_fit_sparse_kernel, dim3(groups), dim3(SLS_THREADS), 0, s, a);
  RK_SIDE_CHECK_LAUNCH("slim_fit_sparse_kernel");
  return 0;
}

int rk_slim_scores(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows,
                   int32_t n_items, const int32_t *nbr_ids, const float *nbr_w, const int32_t *nbr_count,
                   int32_t K, int32_t lo, int32_t hi, float *out, int64_t ldo, void *stream) {
  RK_SIDE_REQUIRE(indptr && indices && nbr_ids && nbr_w && nbr_count && out, "null pointer");
  RK_SIDE_REQUIRE(n_rows >= 0 && n_items >= 1 && K >= 1 && K <= SL_MAX_K, "bad sizes");
  RK_SIDE_REQUIRE(0 <= lo && lo < hi && hi <= n_items && ldo >= hi - lo, "bad strip");
  if (n_rows == 0) return 0;
  const int width = hi - lo;
  const dim3 grid(n_rows, (width + SC_THREADS - 1) / SC_THREADS);
  hipLaunchKernelGGL(slim_scores_kernel, grid, dim3(SC_THREADS), 0, (hipStream_t)stream, indptr, indices, data,
                     nbr_ids, nbr_w, nbr_count, K, lo, width, out, ldo);
  RK_SIDE_CHECK_LAUNCH("slim_scores_kernel");
  return 0;
}

int rk_slim_explain(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows, int32_t n_items,
                    const int32_t *nbr_ids, const float *nbr_w, const int32_t *nbr_count, int32_t K,
                    int32_t lists_are_columns, const int64_t *items, int32_t J, int32_t m, int64_t *contributors,
                    float *contributions, float *baseline, float *total, void *stream) {
  RK_SIDE_REQUIRE(n_rows >= 0 && n_items >= 1 && K >= 1 && K <= SL_MAX_K, "bad sizes");
  RK_SIDE_REQUIRE(lists_are_columns == 0 || lists_are_columns == 1, "lists_are_columns must be 0 or 1");
  RK_SIDE_REQUIRE(J >= 1 && m >= 1 && m <= XP_MAX_M && (int64_t)n_rows * J <= 0x7fffffff,
                  "J >= 1, 1 <= m <= 64, n_rows * J < 2^31");
  if (n_rows == 0) return 0;
  RK_SIDE_REQUIRE(indptr && indices && nbr_ids && nbr_w && nbr_count && items && contributors && contributions &&
                  baseline && total, "null pointer");
  const XpListFetch fetch{nbr_ids, nbr_w, nbr_count, K, lists_are_columns};
  hipLaunchKernelGGL(xp_item_kernel<XpListFetch>, dim3((unsigned)((int64_t)n_rows * J)), dim3(64), 0,
                     (hipStream_t)stream, indptr, indices, data, n_items, items, J, m, fetch, contributors,
                     contributions, baseline, total);
  RK_SIDE_CHECK_LAUNCH("slim_explain_kernel");
  return 0;
}

}  // extern "C"
