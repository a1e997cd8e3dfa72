// What the families of librecoder_als.so share (private to als.hip, which is the one translation unit): the lane
// layout of a row and its reductions, the counter hash and its draws, the walk over a run of equal sorted keys,
// and the host's choice of a kernel's template parameters from h.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../../include/recoder_als.h"
#include "../side_error.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MAX_H = 512;

int64_t round256(int64_t x) { return (x + 255) / 256 * 256; }

// ------------------------------------------------------------------ dispatch
// f(Int<NT>{}) with NT = 1, 2, 4 or 8 registers a lane for a row of h <= 64 NT floats: the template parameter of
// every kernel in the lane layout below, as  dispatch_nt(h, [&](auto nt) { ...kernel<decltype(nt)::value>... });
template <int N>
using Int = std::integral_constant<int, N>;

template <class F>
void dispatch_nt(int h, F &&f) {
  if (h <= 64) f(Int<1>{});
  else if (h <= 128) f(Int<2>{});
  else if (h <= 256) f(Int<4>{});
  else f(Int<8>{});
}

// f(Int<NT>{}, Int<W>{}) for the kernels whose wave is 64 / W lane groups of W lanes (the candidate round of
// als/ugcn.h): W = 16 or 32 with a dimension a lane while h fits a group, else the wave itself with dispatch_nt's NT.
template <class F>
void dispatch_group(int h, F &&f) {
  if (h <= 16) f(Int<1>{}, Int<16>{});
  else if (h <= 32) f(Int<1>{}, Int<32>{});
  else dispatch_nt(h, [&](auto nt) { f(nt, Int<64>{}); });
}

// ---------------------------------------------------------------------- rows
// Lane l of a wave owns dimensions k = l + 64 q (q < NT) of a row; every dot product is a per-lane fmaf chain over
// q ascending from +0, then an xor butterfly (a + b == b + a bitwise: every lane ends with the same value, so
// every branch on it is wave-uniform).
__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

template <int NT>
__device__ __forceinline__ float wave_dot(const float (&a)[NT], const float (&b)[NT]) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) s = fmaf(a[t], b[t], s);
  return wave_sum(s);
}

// out = T[row, :h] (T's leading dimension ld), +0 past h and everywhere when !ok (nothing is read then)
template <int NT>
__device__ __forceinline__ void load_row(const float *T, int ld, int64_t row, int h, int lane, bool ok,
                                         float (&out)[NT]) {
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    out[q] = (ok && k < h) ? T[row * ld + k] : 0.f;
  }
}

template <int NT>
__device__ __forceinline__ void store_row(float *T, int ld, int64_t row, int h, int lane, const float (&v)[NT]) {
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int k = lane + 64 * q;
    if (k < h) T[row * ld + k] = v[q];
  }
}

// ---------------------------------------------------------------------- hash
// The counter RNG, restated here (this translation unit does not include csrc/common.h): splitmix64's
// output function, z += 0x9E3779B97F4A7C15, two xor-shift-multiplies, a last xor-shift.
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// draw d of (seed, step, slot) mapped to [0, range): the high 32 bits times range, shifted down
__host__ __device__ __forceinline__ uint32_t draw32(uint64_t slot_key, uint32_t d, uint32_t range) {
  const uint64_t r = mix64(slot_key + d);
  return (uint32_t)(((r >> 32) * (uint64_t)range) >> 32);
}

// ------------------------------------------------------------------ segments
// The hand-out of rk_als_bpr_apply and rk_als_lgcn_scatter: one wave per sorted position s0; the wave at the head
// of a run of equal keys owns that row, the others leave (false).  So does a key outside [0, n_rows): the invalid
// slots' sentinel, sorted last.  c = the run's length: 64 keys at a time, the first lane whose key differs.
// (als_entry_scatter_kernel of ugcn.h keeps this scan written out, with its hand-over of long keys: through this
// function it once compiled to other, slower code.  When UltraGCN's and CCL's scatters became that one kernel the scan
// was left where it was, now the only copy beside this one, and was not routed through here again: every
// instantiation kept the registers it had.)
__device__ __forceinline__ bool segment_head(const int32_t *__restrict__ keys, int n, int n_rows, int s0, int lane,
                                             int &key, int &c) {
  if (s0 >= n) return false;
  key = keys[s0];
  if (key < 0 || key >= n_rows) return false;
  if (s0 > 0 && keys[s0 - 1] == key) return false;       // (not a head)
  c = 0;
  for (;;) {
    const int s = s0 + c + lane;
    const bool same = s < n && keys[s] == key;
    const uint64_t m = __ballot(!same);
    if (m) {
      c += __ffsll((unsigned long long)m) - 1;
      return true;
    }
    c += 64;
  }
}

// The run's sum.  order[s] is the entry's position before the sort: slot t = order / roles, and with roles == 2
// (the item side) an odd position is the slot's negative.  Its weight w is -g_t and every other entry's +g_t
// (NEGATE: the other way round);  acc_k = fmaf(w, V[t, k], acc_k) over the run in the order given, from what acc
// holds, SEG_UNROLL rows gathered before any is added.  Returns the sum of the weights, the bias' chain: only the
// apply reads it, and in the scatter, which drops it, the compiler removes the sum as dead code.
constexpr int SEG_UNROLL = 4;

template <int NT, bool NEGATE>
__device__ __forceinline__ float segment_sum(const int64_t *__restrict__ order, int s0, int c, int n, int roles,
                                             const float *__restrict__ g, const float *__restrict__ V, int h, int lane,
                                             float (&acc)[NT]) {
  float wsum = 0.f;
  const int64_t slots = roles == 2 ? n >> 1 : n;
  for (int a0 = 0; a0 < c; a0 += SEG_UNROLL) {
    float v[SEG_UNROLL][NT], w[SEG_UNROLL];
#pragma unroll
    for (int r = 0; r < SEG_UNROLL; ++r) {
      const bool in = a0 + r < c;
      const int64_t e = in ? order[s0 + a0 + r] : 0;
      const int64_t t = roles == 2 ? e >> 1 : e;
      const bool ok = in && e >= 0 && t < slots;         // (an order outside the batch adds nothing)
      const float gt = ok ? g[t] : 0.f;
      w[r] = ((roles == 2 && (e & 1)) != NEGATE) ? -gt : gt;
      load_row<NT>(V, h, t, h, lane, ok, v[r]);
    }
#pragma unroll
    for (int r = 0; r < SEG_UNROLL; ++r) {
      if (a0 + r < c) {                                  // (wave-uniform: a tail entry must not touch the chain)
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[q] = fmaf(w[r], v[r][q], acc[q]);
        wsum += w[r];
      }
    }
  }
  return wsum;
}

}  // namespace
