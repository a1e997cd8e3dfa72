// fp32 MFMA GEMMs of the hot path (gfx950: v_mfma_f32_32x32x2_f32, exact fp32
// fma chains -> parity with the reference's fp32 CPU path to rounding).
//
//   decode + loss : O[B,n_t] = Z[B,h] . W_de[T]^T + b_de[T]   (reference
//                   nn.py:271-280) with the loss and dLoss/dO fused into the
//                   epilogue (losses.py:43-47, BCEWithLogits): the logits never
//                   go to HBM for MSE/BCE, only dO does; the epilogue also
//                   emits per-row-tile column sums of dO (bias gradient).
//   bwd dZ        : dZ[B,h]   = dO[B,n_t] . W_de[T]      (split-K over n_t)
//   bwd dW        : G[n_t,h]  = dO^T . Z
//   hidden layers : nn.Linear stack fwd/bwd (nn.py:242-249)
//
// One templated LDS-tiled kernel: block = 4 waves (WM x WN), each wave owns
// TM x TN tiles of 32x32, BK = 16.  Operands are staged global -> registers ->
// LDS (double buffered; the next tile's global loads are issued before the
// MFMAs of the current one).  All bounds handling is branch-free (clamped
// address + select) so the tile's loads issue back to back -- a branchy loader
// made hipcc wait vmcnt(0) after every load (7% of MFMA peak, profiles/r01_a).
// K-contiguous operands sit in LDS as [row][20] floats (80-B stride = odd
// multiple of 16 B -> conflict-free ds_read_b128: one read feeds 4 MFMA k-steps
// because the two lane halves take k = {0..3} / {4..7} of each 8-group);
// k-major operands sit as [16][tile] and are read with ds_read_b32.
#include <stdlib.h>

#include <algorithm>

#include <type_traits>

#include "common.h"
#include "splitk_reduce.h"
#include "encoder_bwd.h"

// rk_gemm_probe(buffer): when set, every GEMM workgroup records wall_clock64() at entry, after
// the prologue (first tile staged), after the k-loop, after the epilogue, plus its tile index
// (tools/gemm_probe.py turns that into a per-phase timeline).  One uniform branch per stamp.
static unsigned long long *g_gemm_probe = nullptr;
#define RK_STAMP(k)                                                                  \
  do {                                                                               \
    if (p.probe && threadIdx.x == 0) p.probe[(size_t)L * 8 + (k)] = wall_clock64();  \
  } while (0)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

enum { EPI_STORE = 0, EPI_LOSS_MSE = 1, EPI_SPLITK = 2, EPI_LOSS_BCE = 3 };
// operand precision of the contraction
//   PREC_F32 : v_mfma_f32_32x32x2_f32 on the fp32 values (64 cycles per 2 k; exact fma chains)
//   PREC_H3  : gfx950 has no fast fp32 matrix path (157 TF vs 2.5 PF for 16-bit operands), so
//              every fp32 operand x is split when it is staged into LDS:
//                  s.x = hi + lo + r,  hi = fp16_rne(s.x),  lo = fp16_rne(s.x - hi)
//              (s = a power of two that puts the matrix into fp16's range, exact; s.x - hi is
//              exact in fp32; |r| <= 2^-22 |s.x| or 2^-25 absolute in the subnormal range) and
//              a.b is accumulated in fp32 as lo.hi + hi.lo + hi.hi on
//              v_mfma_f32_32x32x16_f16 (32 cycles per 16 k: 3 MFMAs do the work of 8 fp32 ones,
//              5.3x the matrix rate).  The dropped lo.lo and r terms are zero-mean (round to
//              nearest on both levels) and <= 3 . 2^-22 relative per product -- the size of the
//              rounding an fp32 fma chain of this length accumulates itself.  The accumulator
//              is rescaled by 1 / (s_a s_b) (exact) before the epilogue.
//              Range: |s.x| must stay below 65504.  Every operand therefore gets its scale ON THE
//              DEVICE from a published maximum / upper bound of its magnitude (a_amax / b_amax:
//              dLoss/dLogits from the loss kernels, Z from rk_amax when the activation is
//              unbounded, W_de from the running maximum the Adam sweep keeps) -- max . s in
//              [2^13, 2^14); the constants below only serve callers that pass no bound (then
//              |W| < 512, |Z| < 2048).
enum { PREC_F32 = 0, PREC_H3 = 1 };
// Full 22-bit precision needs |s.x| >= 2^-3 (below that the lo half goes subnormal: absolute error
// 2^-25 / s); overflow at |s.x| >= 65504.
constexpr float SCALE_W = 128.0f;      // embedding rows:  |w| < 512,  exact split for |w| >= 1e-3
constexpr float SCALE_Z = 32.0f;       // activations:     |z| < 2048, exact split for |z| >= 4e-3
// dLoss/dLogits scales with 1 / batch rows, the confidence weight and the logits themselves, so its
// scale is chosen on the device from the running maximum |g| that the loss kernels publish in
// rk_block_t.counts[8..71] (a_amax): max|g| . s lands in [2^13, 2^14).  SCALE_DO is the fallback for
// a dO the caller filled without publishing a maximum (slots all zero).
constexpr float SCALE_DO = 1024.0f;

// 4 consecutive-k fp32 values -> 4 fp16 "hi" + 4 fp16 "lo" of s.x
// (v_pk_mul_f32, v_cvt_pk_f16_f32, v_cvt_f32_f16, v_pk_fma_f32)
__device__ __forceinline__ void split4(const float4 v, const float s, uint2 &hi, uint2 &lo) {
  const f32x2 a = {v.x * s, v.y * s}, b = {v.z * s, v.w * s};
  const f16x2 ha = __builtin_convertvector(a, f16x2), hb = __builtin_convertvector(b, f16x2);
  const f32x2 la = a - __builtin_convertvector(ha, f32x2), lb = b - __builtin_convertvector(hb, f32x2);
  const f16x2 qa = __builtin_convertvector(la, f16x2), qb = __builtin_convertvector(lb, f16x2);
  hi.x = __builtin_bit_cast(uint32_t, ha); hi.y = __builtin_bit_cast(uint32_t, hb);
  lo.x = __builtin_bit_cast(uint32_t, qa); lo.y = __builtin_bit_cast(uint32_t, qb);
}

// running max |dLoss/dLogit| of a block: slot (0..63) of counts[8..71] <- max(slot, v) as fp32 bit
// patterns (monotonic for v >= 0).  64 slots: with 8, the ~10^3 workgroups of a decode launch
// queued ~140 deep on each address at the L2 and the launch grew by 4-8 us.
__device__ __forceinline__ void publish_amax(int32_t *counts, int slot, float v) {
  atomicMax(reinterpret_cast<unsigned int *>(counts) + 8 + (slot & 63), __float_as_uint(v));
}

struct GemmP {
  unsigned long long *probe;   // tuning probe (null in production): 5 wall-clock stamps per workgroup
  const float *A;
  const float *Bm;
  const int32_t *bidx;      // gather rows of the B operand (item ids) or null
  int lda, ldb;
  const int32_t *lda_dev, *ldb_dev;   // leading dimension read from the device when non-null
  int M, N, K;              // host sizes (capacities when *_dev given)
  const int32_t *Mdev, *Ndev, *Kdev;
  int tiles_m;              // host: ceil(Mcap / BM) (grid sizing only)
  int n_fastest;            // tile order inside a split: nt fastest (else mt fastest)
  int kchunk;               // K range per blockIdx.y
  float a_scale, b_scale;   // PREC_H3: powers of two applied to the operands before the fp16 split
  const uint32_t *a_amax;   // PREC_H3, nullable: 64 slots of fp32 bit patterns, max |A| (see SCALE_DO)
  const uint32_t *b_amax;   // the same for the B operand (all slots zero: b_scale as given)
  // store epilogue
  float *C;
  int ldc;                  // <=0 : read ld from ld_dev
  const int32_t *ld_dev;
  const float *bias;        // per output column (null = none)
  int bias_gather;          // bias index = bidx[n]
  int act;
  int accumulate;
  // loss epilogue
  rk_block_t blk;
  int row_off;
  int loss_kind;
  float confidence, inv_B;
  float *loss_part;
  float *gb_part;           // [tiles_m][ld] column sums of dO per row tile (nullable)
};

// Branch-free guarded staging of 4 consecutive floats, split in two so that the
// global load can stay in flight across the MFMA block:
//   ld4_raw  : the load alone, from a clamped (always readable) address
//   mask4    : zero the elements that are logically out of range -- applied
//              when the registers are written to LDS, one phase later.
// `valid` (<= 0 .. >= 4) = how many of the 4 floats are in range.  VEC: one
// 16-B load (caller guarantees alignment and that the 4 floats lie inside the
// allocation whenever valid > 0).
template <bool VEC>
__device__ __forceinline__ float4 ld4_raw(const float *base, int64_t off, int valid) {
  float4 r;
  if (VEC) {
    r = *reinterpret_cast<const float4 *>(base + (valid > 0 ? off : 0));
  } else {
    r.x = base[valid > 0 ? off : 0];
    r.y = base[valid > 1 ? off + 1 : 0];
    r.z = base[valid > 2 ? off + 2 : 0];
    r.w = base[valid > 3 ? off + 3 : 0];
  }
  return r;
}
__device__ __forceinline__ float4 mask4(float4 v, int valid) {
  float4 r;
  r.x = valid > 0 ? v.x : 0.f;
  r.y = valid > 1 ? v.y : 0.f;
  r.z = valid > 2 ? v.z : 0.f;
  r.w = valid > 3 ? v.w : 0.f;
  return r;
}

template <int WM, int WN, int TM, int TN, int AMODE, int BMODE, int EPI, bool VEC, int BK = 16,
          int PREC = PREC_F32>
__device__ __forceinline__ void gemm_body(const GemmP &p, const int L, const int nsplit) {
  static_assert(WM * WN == 4, "4 waves per block");
  static_assert(BK == 16 || BK == 32 || BK == 40 || BK == 64, "BK");
  static_assert(PREC == PREC_F32 || (VEC && BK % 16 == 0), "split-fp16 tiles: 16-B loads, k-steps of 16");
  constexpr bool H3 = (PREC == PREC_H3);
  constexpr int BM = 32 * WM * TM, BN = 32 * WN * TN;
  constexpr int LDK = BK + 4;          // K-contiguous LDS row stride (odd multiple of 16 B)
  constexpr int QK = BK / 4;           // float4 per K-contiguous row
  // PREC_H3: every operand sits K-contiguous in LDS, a row = BK fp16 "hi" then BK fp16 "lo" (+16 B:
  // the same 4*(BK+4)-byte stride, conflict-free ds_read_b128); k-major operands are transposed
  // on the way in (4k x 4m register blocks)
  constexpr int LDB = 4 * LDK;         // that row stride in bytes
  constexpr int A_SZ = (AMODE == 0 || H3) ? BM * LDK : BK * BM;
  constexpr int B_SZ = (BMODE == 0 || H3) ? BN * LDK : BK * BN;
  constexpr int A_F4 = BM * BK / 4, B_F4 = BN * BK / 4;      // float4 per tile
  // k-major operands under PREC_H3 are staged in units of 4 k-rows x one float4 (4 loads per unit)
  constexpr bool A_UNIT = H3 && AMODE == 1, B_UNIT = H3 && BMODE == 1;
  constexpr int A_UN = A_F4 / 4, B_UN = B_F4 / 4;            // units per tile
  constexpr int A_PT = A_UNIT ? 4 * ((A_UN + 255) / 256) : (A_F4 + 255) / 256;
  constexpr int B_PT = B_UNIT ? 4 * ((B_UN + 255) / 256) : (B_F4 + 255) / 256;
  // staging double buffer; the epilogue reuses it (4 per-wave 32x36 transpose areas +
  // the loss partials), so it is at least that large
  constexpr int STAGE_F = 2 * (A_SZ + B_SZ);
  constexpr int EPI_F = 4 * 32 * 36 + 8 + WM * BN;
  __shared__ __attribute__((aligned(16))) float smem[STAGE_F > EPI_F ? STAGE_F : EPI_F];

  const int M = p.Mdev ? *p.Mdev : p.M;
  const int N = p.Ndev ? *p.Ndev : p.N;
  const int K = p.Kdev ? *p.Kdev : p.K;
  const int lda = p.lda_dev ? *p.lda_dev : p.lda;
  const int ldb = p.ldb_dev ? *p.ldb_dev : p.ldb;
  // scale of an operand from its published maximum (64 slots of fp32 bit patterns; an upper bound
  // is as good): max . s in [2^13, 2^14) -- nothing can overflow fp16, and every element within
  // 2^-17 of the maximum keeps its full 22 bits
  auto scale_from = [&](const uint32_t *slots, float dflt) -> float {
    if (!H3 || slots == nullptr) return dflt;
    uint32_t m = slots[threadIdx.x & 63];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
    if (m == 0) return dflt;
    const int e = min(max((int)(m >> 23) - 127, -100), 100);
    return __uint_as_float((uint32_t)(13 - e + 127) << 23);
  };
  const float a_scale = scale_from(p.a_amax, p.a_scale);
  const float b_scale = scale_from(p.b_amax, p.b_scale);
  // XCD-aware tile mapping.  Workgroup L runs on XCD L % 8 (each XCD has its own
  // L2), so XCD x gets the contiguous chunk [x*chunk, (x+1)*chunk) of the LIVE
  // tile list -- tiles that share an operand panel (same nt for gathered W rows,
  // same mt for a dO column panel, same split) then hit the same L2.  The live
  // tile count comes from the device-resident M/N, the grid from capacities.
  const int tm = (M + BM - 1) / BM, tn = (N + BN - 1) / BN;
  const int per_split = tm * tn;
  const int total = per_split * nsplit;
  const int chunk = (total + 7) >> 3;
  const int t = (L & 7) * chunk + (L >> 3);
  if ((L >> 3) >= chunk || t >= total) return;
  const int split = t / per_split, rt = t % per_split;
  const int mt = p.n_fastest ? rt / tn : rt % tm;
  const int nt = p.n_fastest ? rt % tn : rt / tm;
  const int m0 = mt * BM, n0 = nt * BN;
  // split-K: the chunk follows the device-resident K so that every split is live
  const int kchunk = (p.kchunk > 0) ? p.kchunk : (((K + nsplit - 1) / nsplit + 31) & ~31);
  const int kbeg = split * kchunk;
  const int kend = min(K, kbeg + kchunk);
  if (kbeg >= kend) return;

  RK_STAMP(0);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int l31 = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- loop-invariant per-thread addressing of the staged tiles ----
  // Rows / columns outside the problem are CLAMPED to a readable address instead
  // of masked: the garbage they bring only reaches output rows/columns that the
  // epilogue never stores.  Only the K direction needs real zeros, and only in
  // the last (partial) K-tile -- interior tiles take the lean path below: one
  // pointer per staged float4, no selects.
  // split-fp16 staging of a K-contiguous operand: a thread's 8-byte hi / lo stores go to LDS rows of
  // 144 bytes (an odd number of 16-byte slots: conflict-free ds_read_b128 fragments).  With 8
  // consecutive lanes per row, the 4 rows a 32-lane store pass covers must lie 4 apart -- 144 r mod
  // 256 for r, r+4, r+8, r+12 are the four disjoint 64-byte ranges; consecutive rows overlap (2-way
  // conflicts on half the banks: SQ_LDS_BANK_CONFLICT 28 % of the decode's LDS cycles in round 1).
  // So slot s of the staging order handles row row_of(s), a permutation inside every 16 rows.
  auto row_of = [](int s) -> int { return H3 ? ((s & ~15) | ((s & 3) << 2) | ((s >> 2) & 3)) : s; };
  const float *a_ptr[A_PT], *b_ptr[B_PT];
  int a_k[A_PT], b_k[B_PT];           // k index of the element inside the tile
  int b_n[B_PT];                      // BMODE 1: column offset (row pointer varies with the gather)
  // k-major operands, scalar loads: how many more elements the row holds behind the group's first one.  Where the
  // leading dimension is no multiple of 4 the row's last group is ragged, and its loads stop at the row's last
  // element (the repeats land in columns past ld, which no epilogue stores).  VEC: the caller guarantees ld % 4 == 0.
  int a_rem[A_PT], b_rem[B_PT];
#pragma unroll
  for (int i = 0; i < A_PT; ++i) {
    const int idx = min(tid + i * 256, A_F4 - 1);
    if (AMODE == 0) {
      const int row = row_of(idx / QK), q = idx % QK;
      a_k[i] = q * 4;
      a_ptr[i] = p.A + (int64_t)min(m0 + row, M - 1) * lda + q * 4 + kbeg;
    } else {
      // unit u = (k-quad kq, column group m4), kq fastest over the lanes; load i&3 is row kq*4 + (i&3)
      const int u = min(tid + (i >> 2) * 256, A_UN - 1);
      const int k = A_UNIT ? (u % QK) * 4 + (i & 3) : idx / (BM / 4);
      const int m4 = A_UNIT ? u / QK : idx % (BM / 4);
      const int m = m0 + m4 * 4;
      a_k[i] = k;
      const int mc = VEC ? ((m + 3 < lda) ? m : 0) : ((m < lda) ? m : 0);
      a_rem[i] = lda - 1 - mc;
      a_ptr[i] = p.A + (int64_t)(kbeg + k) * lda + mc;
    }
  }
#pragma unroll
  for (int i = 0; i < B_PT; ++i) {
    const int idx = min(tid + i * 256, B_F4 - 1);
    if (BMODE == 0) {
      const int row = row_of(idx / QK), q = idx % QK;
      const int nc = min(n0 + row, N - 1);
      const int64_t src = p.bidx ? (int64_t)p.bidx[nc] : (int64_t)nc;   // gather index: once
      b_k[i] = q * 4;
      b_n[i] = 0;
      b_ptr[i] = p.Bm + src * ldb + q * 4 + kbeg;
    } else {
      const int u = min(tid + (i >> 2) * 256, B_UN - 1);
      const int k = B_UNIT ? (u % QK) * 4 + (i & 3) : idx / (BN / 4);
      const int n4 = B_UNIT ? u / QK : idx % (BN / 4);
      const int n = n0 + n4 * 4;
      b_k[i] = k;
      b_n[i] = VEC ? ((n + 3 < ldb) ? n : 0) : ((n < ldb) ? n : 0);
      b_rem[i] = ldb - 1 - b_n[i];
      b_ptr[i] = p.Bm + b_n[i];          // + row * ldb per tile
    }
  }

  float4 ra0[A_PT], rb0[B_PT], ra1[A_PT], rb1[B_PT];   // two staged tiles in flight
  const bool gather_k = (BMODE == 1) && (p.bidx != nullptr);

  // kt = tile index inside this block's K range; tiles with (kt+1)*BK <= klen are
  // interior.  The tail tile clamps k to the last valid index (readable) and is
  // masked to zero when written to LDS.
  const int klen = kend - kbeg;
  // 4 consecutive floats along K starting at (tile-relative) k: interior tiles
  // read them as they are; the tail tile clamps k to the last readable group
  auto load_kcontig = [&](const float *ptr_k0, int k, bool tail) -> float4 {
    // ptr_k0 points at tile-relative k = 0 of this thread's row
    const int kk = tail ? min(k, (klen - 1) & ~3) : k;
    const float *q = ptr_k0 + kk;
    if (VEC) return *reinterpret_cast<const float4 *>(q);
    const int last = klen - 1 - kk;          // >= 0
    return make_float4(q[0], q[last > 0 ? 1 : 0], q[last > 1 ? 2 : 0], q[last > 2 ? 3 : 0]);
  };
  auto load4 = [&](const float *q, int rem) -> float4 {
    if (VEC) return *reinterpret_cast<const float4 *>(q);
    return make_float4(q[0], q[rem > 0 ? 1 : 0], q[rem > 1 ? 2 : 0], q[rem > 2 ? 3 : 0]);
  };
  auto gload = [&](float4 (&ra)[A_PT], float4 (&rb)[B_PT], int kt) {
    const int kb = kt * BK;
    const bool tail = (kb + BK > klen);
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      if (AMODE == 0) {
        ra[i] = load_kcontig(a_ptr[i] - a_k[i], kb + a_k[i], tail);
      } else {
        const int row = tail ? min(kb + a_k[i], klen - 1) : kb + a_k[i];
        ra[i] = load4(a_ptr[i] + (int64_t)(row - a_k[i]) * lda, a_rem[i]);
      }
    }
    if (BMODE == 0) {
#pragma unroll
      for (int i = 0; i < B_PT; ++i) rb[i] = load_kcontig(b_ptr[i] - b_k[i], kb + b_k[i], tail);
    } else {
      // k-major B with an optional row gather: fetch every gather index first
      // (independent loads), then every row segment
      int src[B_PT];
#pragma unroll
      for (int i = 0; i < B_PT; ++i) src[i] = kbeg + (tail ? min(kb + b_k[i], klen - 1) : kb + b_k[i]);
      if (gather_k) {
#pragma unroll
        for (int i = 0; i < B_PT; ++i) src[i] = p.bidx[src[i]];
      }
#pragma unroll
      for (int i = 0; i < B_PT; ++i) rb[i] = load4(b_ptr[i] + (int64_t)src[i] * ldb, b_rem[i]);
    }
  };
  auto sstore = [&](int buf, const float4 (&ra)[A_PT], const float4 (&rb)[B_PT], int kt) {
    const int kb = kt * BK;
    const bool tail = (kb + BK > klen);
    float *As = smem + buf * (A_SZ + B_SZ);
    float *Bs = As + A_SZ;
    if (H3) {
      // split into fp16 hi / lo and store K-contiguous: row r holds hi[0..BK) | lo[0..BK)
      auto put = [&](float *base, float scale, int row, int kq, const float4 v) {
        uint2 hi, lo;
        split4(v, scale, hi, lo);
        char *d = reinterpret_cast<char *>(base) + row * LDB + kq * 8;
        *reinterpret_cast<uint2 *>(d) = hi;
        *reinterpret_cast<uint2 *>(d + BK * 2) = lo;
      };
      // (sizes as types: a run-time bound here leaves exec-masked branches around the LDS stores
      // and hipcc then waits for the loads it has just issued -- see the note at the k-loop)
      // Only A is masked in the K tail: a product needs ONE zero factor, and the clamped tail
      // loads of B are real (finite) table / activation values -- masking both cost 2 VALU per
      // staged element on every tile, as much again as the split itself.
      auto stage = [&](float *base, float scale, auto &regs, auto &kk, auto mode_tag, auto pt_tag,
                       auto f4_tag, auto un_tag, auto mask_tag) {
        constexpr bool MASK = decltype(mask_tag)::value;
        constexpr int MODE = decltype(mode_tag)::value;
        constexpr bool UNIT = (MODE == 1);
        constexpr int PT = decltype(pt_tag)::value;
        constexpr int f4 = decltype(f4_tag)::value, un = decltype(un_tag)::value;
        if (!UNIT) {
#pragma unroll
          for (int i = 0; i < PT; ++i) {
            const int idx = tid + i * 256;
            if ((f4 % 256 == 0) || idx < f4) {
              // (selects, not a branch on `tail`: control flow between the staged loads and their
              // LDS stores makes hipcc drain vmcnt at the top of every iteration)
              const float4 v = MASK ? mask4(regs[i], tail ? klen - kb - kk[i] : 4) : regs[i];
              put(base, scale, row_of(idx / QK), idx % QK, v);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < PT / 4; ++j) {
            const int u = tid + j * 256;
            if ((un % 256 == 0) || u < un) {
              float4 v[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                v[r] = MASK ? mask4(regs[j * 4 + r], (!tail || kb + kk[j * 4 + r] < klen) ? 4 : 0)
                            : regs[j * 4 + r];
              }
              const int kq = u % QK, c4 = u / QK;
              put(base, scale, c4 * 4 + 0, kq, make_float4(v[0].x, v[1].x, v[2].x, v[3].x));
              put(base, scale, c4 * 4 + 1, kq, make_float4(v[0].y, v[1].y, v[2].y, v[3].y));
              put(base, scale, c4 * 4 + 2, kq, make_float4(v[0].z, v[1].z, v[2].z, v[3].z));
              put(base, scale, c4 * 4 + 3, kq, make_float4(v[0].w, v[1].w, v[2].w, v[3].w));
            }
          }
        }
      };
      stage(As, a_scale, ra, a_k, std::integral_constant<int, AMODE>{}, std::integral_constant<int, A_PT>{},
            std::integral_constant<int, A_F4>{}, std::integral_constant<int, A_UN>{}, std::true_type{});
      stage(Bs, b_scale, rb, b_k, std::integral_constant<int, BMODE>{}, std::integral_constant<int, B_PT>{},
            std::integral_constant<int, B_F4>{}, std::integral_constant<int, B_UN>{}, std::false_type{});
      return;
    }
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int idx = tid + i * 256;
      if ((A_F4 % 256 == 0) || idx < A_F4) {
        float4 v = ra[i];
        if (tail) v = mask4(v, (AMODE == 0) ? (klen - kb - a_k[i]) : ((kb + a_k[i] < klen) ? 4 : 0));
        if (AMODE == 0) {
          const int row = idx / QK, q = idx % QK;
          *reinterpret_cast<float4 *>(As + row * LDK + q * 4) = v;
        } else {
          const int k = idx / (BM / 4), m4 = idx % (BM / 4);
          *reinterpret_cast<float4 *>(As + k * BM + m4 * 4) = v;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < B_PT; ++i) {
      const int idx = tid + i * 256;
      if ((B_F4 % 256 == 0) || idx < B_F4) {
        float4 v = rb[i];
        if (tail) v = mask4(v, (BMODE == 0) ? (klen - kb - b_k[i]) : ((kb + b_k[i] < klen) ? 4 : 0));
        if (BMODE == 0) {
          const int row = idx / QK, q = idx % QK;
          *reinterpret_cast<float4 *>(Bs + row * LDK + q * 4) = v;
        } else {
          const int k = idx / (BN / 4), n4 = idx % (BN / 4);
          *reinterpret_cast<float4 *>(Bs + k * BN + n4 * 4) = v;
        }
      }
    }
  };

  auto compute = [&](int buf, int kt) {
    const float *As = smem + buf * (A_SZ + B_SZ);
    const float *Bs = As + A_SZ;
    if (H3) {
      // every k-step of the tile is computed: the K padding holds zeros (masked / zero padded)
      const char *Ab = reinterpret_cast<const char *>(As) + ((wm * TM) * 32 + l31) * LDB + lh * 16;
      const char *Bb = reinterpret_cast<const char *>(Bs) + ((wn * TN) * 32 + l31) * LDB + lh * 16;
#pragma unroll
      for (int ks = 0; ks < BK / 16; ++ks) {
        {
          f16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const char *q = Ab + i * 32 * LDB + ks * 32;
            ah[i] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4 *>(q));
            al[i] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4 *>(q + BK * 2));
          }
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const char *q = Bb + j * 32 * LDB + ks * 32;
            bh[j] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4 *>(q));
            bl[j] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4 *>(q + BK * 2));
          }
          // small terms first
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
      }
      return;
    }
#pragma unroll
    for (int kg = 0; kg < BK / 8; ++kg) {
      float af[TM][4], bf[TN][4];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = (wm * TM + i) * 32 + l31;
        if (AMODE == 0) {
          const float4 v = *reinterpret_cast<const float4 *>(As + row * LDK + kg * 8 + lh * 4);
          af[i][0] = v.x; af[i][1] = v.y; af[i][2] = v.z; af[i][3] = v.w;
        } else {
#pragma unroll
          for (int s = 0; s < 4; ++s) af[i][s] = As[(kg * 8 + lh * 4 + s) * BM + row];
        }
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = (wn * TN + j) * 32 + l31;
        if (BMODE == 0) {
          const float4 v = *reinterpret_cast<const float4 *>(Bs + col * LDK + kg * 8 + lh * 4);
          bf[j][0] = v.x; bf[j][1] = v.y; bf[j][2] = v.z; bf[j][3] = v.w;
        } else {
#pragma unroll
          for (int s = 0; s < 4; ++s) bf[j][s] = Bs[(kg * 8 + lh * 4 + s) * BN + col];
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
    }
  };

  // Pipeline: tile kt is computed from LDS buffer kt&1 while the global loads of
  // tiles kt+1 (already issued, landing in one register set) and kt+2 (issued
  // now into the other set) are in flight; hipcc's counted vmcnt only waits for
  // the older set when it is written to LDS.
  const int nk = (kend - kbeg + BK - 1) / BK;
  // Loss epilogue operands (gathered bias, bitmap words) are fetched NOW so that
  // their two dependent round trips overlap the k-loop instead of the epilogue.
  constexpr bool LOSS = (EPI == EPI_LOSS_MSE || EPI == EPI_LOSS_BCE);
  float pre_bv[LOSS ? TN : 1][4];
  uint32_t pre_w[LOSS ? TM : 1][LOSS ? TN : 1][4];
  if (LOSS) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nb = n0 + (wn * TN + j) * 32;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int nc = min(nb + (lane & 7) * 4 + e, N - 1);
        pre_bv[j][e] = p.bias[p.bidx ? p.bidx[nc] : nc];
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int m = m0 + (wm * TM + i) * 32 + (lane >> 3) + 8 * it;
          const int row = p.row_off + min(m, M - 1);
          pre_w[i][j][it] = p.blk.bits_rc[(int64_t)row * p.blk.ldw_rc + min(nb >> 5, p.blk.ldw_rc - 1)];
        }
    }
  }
  gload(ra0, rb0, 0);
  gload(ra1, rb1, min(1, nk - 1));
  sstore(0, ra0, rb0, 0);
  __syncthreads();
  RK_STAMP(1);
  for (int kt = 0; kt < nk; kt += 2) {
    // prefetch UNCONDITIONALLY (past the end: re-read the last tile, never stored):
    // a branch around the loads makes hipcc merge the vmcnt state pessimistically
    // and wait for the loads just issued before every LDS store
    gload(ra0, rb0, min(kt + 2, nk - 1));
    compute(0, kt);
    if (kt + 1 < nk) sstore(1, ra1, rb1, kt + 1);
    __syncthreads();
    if (kt + 1 >= nk) break;
    gload(ra1, rb1, min(kt + 3, nk - 1));
    compute(1, kt + 1);
    if (kt + 2 < nk) sstore(0, ra0, rb0, kt + 2);
    __syncthreads();
  }
  // ------------------------------------------------------------- epilogues
  // Every 32x32 accumulator tile goes through a per-wave LDS transpose: the MFMA
  // layout gives a lane 16 rows of ONE column (16 scalar stores, 16 bitmap words);
  // read back row-major a lane owns 4 x (one row, 4 consecutive columns), so the
  // epilogue issues 4x fewer, 16-byte-wide global stores / loads per tile.
  if (H3) {
    const float inv = 1.0f / (a_scale * b_scale);         // exact: powers of two
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] *= inv;
  }
  RK_STAMP(2);
  constexpr int TLD = 36;                                   // 32 + 4 floats: 16-B aligned rows
  float *wlds = smem + wid * (32 * TLD);                    // private to this wave
  const int rr0 = lane >> 3, c4 = lane & 7;                 // row-major role of the lane
  auto transpose_tile = [&](const f32x16 &a, float4 (&v)[4]) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 16; ++r) wlds[((r & 3) + 8 * (r >> 2) + 4 * lh) * TLD + l31] = a[r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 4; ++it)
      v[it] = *reinterpret_cast<const float4 *>(wlds + (rr0 + 8 * it) * TLD + c4 * 4);
    __builtin_amdgcn_wave_barrier();
  };

  if (EPI == EPI_STORE) {
    const int ldc = p.ldc > 0 ? p.ldc : *p.ld_dev;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        float4 v[4];
        transpose_tile(acc[i][j], v);
        const int n = n0 + (wn * TN + j) * 32 + c4 * 4;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int nc = min(n + e, N - 1);
            bv[e] = p.bias[p.bias_gather ? (p.bidx ? p.bidx[nc] : nc) : nc];
          }
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int m = m0 + (wm * TM + i) * 32 + rr0 + 8 * it;
          if (m < M && n < N) {
            float o[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = rk_act(o[e] + bv[e], p.act);
            float *dst = p.C + (int64_t)m * ldc + n;
            if (VEC && n + 3 < N) {
              float4 w4 = make_float4(o[0], o[1], o[2], o[3]);
              if (p.accumulate) {
                const float4 old = *reinterpret_cast<const float4 *>(dst);
                w4.x += old.x; w4.y += old.y; w4.z += old.z; w4.w += old.w;
              }
              *reinterpret_cast<float4 *>(dst) = w4;
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (n + e < N) dst[e] = p.accumulate ? (o[e] + dst[e]) : o[e];
            }
          }
        }
      }
  } else if (EPI == EPI_SPLITK) {
    float *ws = p.C + (int64_t)split * p.M * p.N;   // [split][Mcap][Ncap]
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        float4 v[4];
        transpose_tile(acc[i][j], v);
        const int n = n0 + (wn * TN + j) * 32 + c4 * 4;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int m = m0 + (wm * TM + i) * 32 + rr0 + 8 * it;
          if (m < M && n < N) {
            float *dst = ws + (int64_t)m * p.N + n;
            if (VEC && n + 3 < N) {
              *reinterpret_cast<float4 *>(dst) = v[it];
            } else {
              const float o[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (n + e < N) dst[e] = o[e];
            }
          }
        }
      }
  } else {  // EPI_LOSS_* : bias + loss + dLoss/dLogits (+ column sums of dO); the loss kind is a
            // compile-time choice (a runtime select made hipcc emit the exp/log code of
            // BCE for every element of an MSE run: ~7.8k instructions per wave)
    float *lred = smem + 4 * (32 * TLD);          // after the 4 per-wave transpose areas
    float *cpart = lred + 8;                      // [WM][BN] column partial sums
    const int ldc = *p.ld_dev;
    const rk_block_t &b = p.blk;
    const bool implicit = b.implicit != 0;
    float lsum = 0.f, gmax = 0.f;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int nb = n0 + (wn * TN + j) * 32;   // multiple of 32: one bitmap word per row
      const int n = nb + c4 * 4;
      float bv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[e] = pre_bv[LOSS ? j : 0][e];
      float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        float4 v[4];
        transpose_tile(acc[i][j], v);
        uint32_t w[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) w[it] = pre_w[LOSS ? i : 0][LOSS ? j : 0][it];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int m = m0 + (wm * TM + i) * 32 + rr0 + 8 * it;
          const float ov[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
          float g[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = (m < M) && (n + e < N);
            const float o = ov[e] + bv[e];
            float t = 0.f;
            if (ok && ((w[it] >> (c4 * 4 + e)) & 1u)) {
              t = 1.0f;
              if (!implicit) t = b.vals[rk_entry_index(b, p.row_off + m, n + e, w[it])];
            }
            float l;
            if (EPI == EPI_LOSS_MSE) {
              const float wgt = (t > 0.f) ? (1.0f + p.confidence) : 1.0f;
              const float d = o - t;
              l = wgt * (d * d);
              g[e] = (2.0f * d) * (wgt * p.inv_B);
            } else {  // BCE with logits: (1-t)*o - logsigmoid(o)
              const float ls = fminf(o, 0.f) - log1pf(expf(-fabsf(o)));
              l = (1.0f - t) * o - ls;
              const float sg = 1.0f / (1.0f + expf(-o));
              g[e] = (sg - t) * p.inv_B;
            }
            if (ok) { lsum += l; cs[e] += g[e]; gmax = fmaxf(gmax, fabsf(g[e])); }
          }
          // columns in [N, ld) are padding of the dO row: storing them is harmless
          if (m < M && n < N)
            *reinterpret_cast<float4 *>(p.C + (int64_t)m * ldc + n) = make_float4(g[0], g[1], g[2], g[3]);
        }
      }
      // column sums over this wave's rows: lanes with equal c4 hold different rows
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        cs[e] += __shfl_xor(cs[e], 8, 64);
        cs[e] += __shfl_xor(cs[e], 16, 64);
        cs[e] += __shfl_xor(cs[e], 32, 64);
      }
      if (rr0 == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) cpart[wm * BN + (wn * TN + j) * 32 + c4 * 4 + e] = cs[e];
      }
    }
    lsum = rk_wave_sum(lsum);
    gmax = rk_wave_max(gmax);
    if (lane == 0) { lred[wid] = lsum; lred[4 + wid] = gmax; }
    __syncthreads();
    if (tid == 0) {
      p.loss_part[rt] = (lred[0] + lred[1]) + (lred[2] + lred[3]);
      // running max |dLoss/dLogit| of this block (8 slots: one per XCD, fewer same-address
      // atomics); the backward contraction picks its fp16 split scale from it
      const float gm = fmaxf(fmaxf(lred[4], lred[5]), fmaxf(lred[6], lred[7]));
      publish_amax(b.counts, L, gm);
    }
    if (p.gb_part && tid < BN) {
      // one gb_part row per DEC_BM (= 64) rows of dO: a tile of BM rows writes BM / 64 of them
      constexpr int GR = BM >= 64 ? BM / 64 : 1;   // row groups per tile
      constexpr int WPG = WM >= GR ? WM / GR : 1;  // waves (along M) per group
      static_assert(!LOSS || (BM % 64 == 0 && WM % GR == 0), "decode tiles are multiples of 64 rows");
      const int n = n0 + tid;
      if (n < N) {
#pragma unroll
        for (int g = 0; g < GR; ++g) {
          float s2 = cpart[g * WPG * BN + tid];
#pragma unroll
          for (int w2 = 1; w2 < WPG; ++w2) s2 += cpart[(g * WPG + w2) * BN + tid];
          if (m0 + g * 64 < M) p.gb_part[(int64_t)(mt * GR + g) * ldc + n] = s2;
        }
      }
    }
  }
  RK_STAMP(3);
  if (p.probe && threadIdx.x == 0) p.probe[(size_t)L * 8 + 4] = (unsigned long long)t + 1;
}

template <int WM, int WN, int TM, int TN, int AMODE, int BMODE, int EPI, bool VEC, int BK = 16,
          int PREC = PREC_F32>
__global__ __launch_bounds__(256) void gemm_kernel(GemmP p) {
  gemm_body<WM, WN, TM, TN, AMODE, BMODE, EPI, VEC, BK, PREC>(
      p, (int)(blockIdx.y * gridDim.x + blockIdx.x), (int)gridDim.y);
}

// dW GEMM tiles and the encoder backward in ONE launch (workgroups [0, n_dw) are dW
// tiles, the rest encoder-backward columns).  The two are independent (both only read
// dO / dZ0) and complementary -- MFMA-bound tiles next to latency-bound gathers --
// and the step is a serial chain of launches, so running them side by side takes the
// encoder backward off the critical path without a second stream.
template <int HV, bool SPLIT>
__global__ __launch_bounds__(256) void dw_encode_bwd_kernel(
    GemmP p, int n_dw, int nsplit, rk_block_t b, int row_off, int B, const float *__restrict__ dZ,
    int h, float *__restrict__ G_en, float *__restrict__ gb, int n_gb, int n_seg,
    int64_t seg_stride) {
  if ((int)blockIdx.x < n_dw)
    gemm_body<1, 4, 1, 1, 1, 1, SPLIT ? EPI_SPLITK : EPI_STORE, true, 16>(p, (int)blockIdx.x, nsplit);
  else
    ae_encode_bwd_body<HV>(b, row_off, B, dZ, h, G_en, 0, gb, n_gb, (int)blockIdx.x - n_dw, n_seg,
                           seg_stride);
}

// ws[split][M][N] -> out[M][N] (fixed split order), optional * act'(Zact): body in splitk_reduce.h
constexpr int RED_W = rkred::RED_W;
__global__ __launch_bounds__(RED_W * 64) void splitk_reduce_kernel(
    const float *__restrict__ ws, int M, int N, const int32_t *__restrict__ Kdev, int tile_k,
    int max_splits, const float *__restrict__ Zact, int act, float *__restrict__ out) {
  __shared__ float4 part[RED_W - 1][64];
  const rkred::Args a = {ws, M, N, Kdev, tile_k, max_splits, Zact, act, out};
  rkred::body(a, (int)blockIdx.x, part);
}

// out[i] = sum_z ws[z][i] over the live rows of a [splits][M_cap][N] slab stack (dW split-K)
__global__ __launch_bounds__(256) void slab_sum_kernel(const float *__restrict__ ws, int M_cap, int N,
                                                       const int32_t *__restrict__ Mdev, int splits,
                                                       float *__restrict__ out) {
  const int64_t live4 = ((int64_t)(*Mdev) * N) >> 2, slab4 = ((int64_t)M_cap * N) >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= live4) return;
  const float4 *w = reinterpret_cast<const float4 *>(ws);
  float4 s = w[i];
  for (int z = 1; z < splits; ++z) {
    const float4 v = w[(int64_t)z * slab4 + i];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  reinterpret_cast<float4 *>(out)[i] = s;
}

constexpr int MNLL_CACHE = 12;      // quads of a row per thread kept in registers by mnll_finish_kernel
// MNLL second pass, one block per row (see rk_mnll_finish in the header)
// ext_* (nullable, per row): the softmax statistics and the target sum of the WHOLE row when
// the block only holds a shard of its items (item-parallel training)
__global__ __launch_bounds__(256) void mnll_finish_kernel(float *dO, rk_block_t b, int row_off,
                                                          float inv_B, float *loss_part,
                                                          const float *ext_max, const float *ext_logsum,
                                                          const float *ext_tsum) {
  __shared__ float red[4];
  __shared__ float red2[8];
  const int r = blockIdx.x, row = row_off + r;
  const int n = b.counts[0], ld = b.counts[2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool implicit = b.implicit != 0;
  float *orow = dO + (int64_t)r * ld;
  // 16-byte accesses throughout (ld is a multiple of 32 floats, the row 16-byte aligned); a lane's
  // 4 columns lie in one bitmap word.  Columns >= n of the last quad are padding: masked.
  const float4 *orow4 = reinterpret_cast<const float4 *>(orow);
  const int n4 = (n + 3) >> 2;
  // the sparse part's operands of this thread's FIRST stored entry (rows of up to 256 entries need no
  // more) are fetched now, in front of the statistics pass: indptr -> column -> logit are three
  // dependent round trips that used to start behind it
  const int beg = b.indptr[row], end = b.indptr[row + 1];
  float t0 = 0.f, x0 = 0.f;
  if (beg + tid < end) {
    t0 = implicit ? 1.0f : b.vals[beg + tid];
    x0 = orow[b.cols[beg + tid]];
  }
  // The row's first MNLL_CACHE * 1024 logits are fetched ONCE, all loads in flight together, and stay in registers
  // for both passes (C3: 8.4 k columns = 9 quads per thread; the statistics pass and the gradient pass each walked
  // them as a chain of dependent round trips: 19-21 us for 51 MB); longer rows continue from memory as before
  float4 xc[MNLL_CACHE];
  uint32_t wc[MNLL_CACHE];
  const uint32_t *brow = b.bits_rc + (int64_t)row * b.ldw_rc;
#pragma unroll
  for (int u = 0; u < MNLL_CACHE; ++u) {
    const int i = tid + u * 256;
    xc[u] = i < n4 ? orow4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    wc[u] = i < n4 ? brow[i >> 3] : 0u;
  }
  float mx = -INFINITY, lsum;
  if (ext_max) {
    mx = ext_max[r];
    lsum = ext_logsum[r];
  } else {
    // ONE pass for the maximum and the sum of exponentials: running maximum, the partial sum is
    // rescaled when it moves (online softmax); the (max, sum) pairs of the threads are merged the
    // same way in fixed order
    float m = -INFINITY, se = 0.f;
#pragma unroll
    for (int u = 0; u < MNLL_CACHE; ++u) {
      const int i = tid + u * 256;
      if (i < n4) {
        float4 x = xc[u];
        const int c = i << 2;
        if (c + 1 >= n) x.y = -INFINITY;
        if (c + 2 >= n) x.z = -INFINITY;
        if (c + 3 >= n) x.w = -INFINITY;
        const float m4 = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
        if (m4 > m) { se *= expf(m - m4); m = m4; }      // (expf(-inf) = 0 on the first quad)
        se += (expf(x.x - m) + expf(x.y - m)) + (expf(x.z - m) + expf(x.w - m));
      }
    }
    for (int i = tid + MNLL_CACHE * 256; i < n4; i += 256) {
      float4 x = orow4[i];
      const int c = i << 2;
      if (c + 1 >= n) x.y = -INFINITY;
      if (c + 2 >= n) x.z = -INFINITY;
      if (c + 3 >= n) x.w = -INFINITY;
      const float m4 = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
      if (m4 > m) { se *= expf(m - m4); m = m4; }      // (expf(-inf) = 0 on the first quad)
      se += (expf(x.x - m) + expf(x.y - m)) + (expf(x.z - m) + expf(x.w - m));
    }
    const float wm = __shfl(rk_wave_max(m), 0, 64);      // (the reduction leaves it in lane 0)
    se = rk_wave_sum(m == -INFINITY ? 0.f : se * expf(m - wm));     // (a thread without columns: 0)
    if (lane == 0) red[wid] = wm;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    if (lane == 0) red[wid] = wm == -INFINITY ? 0.f : se * expf(wm - mx);
    __syncthreads();
    lsum = logf((red[0] + red[1]) + (red[2] + red[3]));
    __syncthreads();
  }
  // sparse part: loss = -sum_t t*lsm ; sum_g = sum_t (-t*inv_B)
  float lp = 0.f, sg = 0.f;
  if (beg + tid < end) {
    const float lsm = (x0 - mx) - lsum;
    lp += -t0 * lsm;
    sg += -t0 * inv_B;
  }
  for (int j = beg + tid + 256; j < end; j += 256) {
    const float t = implicit ? 1.0f : b.vals[j];
    const float lsm = (orow[b.cols[j]] - mx) - lsum;
    lp += -t * lsm;
    sg += -t * inv_B;
  }
  lp = rk_wave_sum(lp);
  sg = rk_wave_sum(sg);
  // (both block sums through one barrier pair: red2 = 8 floats)
  if (lane == 0) { red2[wid] = lp; red2[4 + wid] = sg; }
  __syncthreads();
  if (tid == 0) loss_part[r] = (red2[0] + red2[1]) + (red2[2] + red2[3]);
  const float sum_g = ext_tsum ? -ext_tsum[r] * inv_B : (red2[4] + red2[5]) + (red2[6] + red2[7]);
  float gmax = 0.f;
  // dense part: dO = g - softmax * sum_g,  g = -t*inv_B at stored positions
  auto grad_quad = [&](const int i, const float4 x, const uint32_t word) {
    const int c = i << 2;
    const uint32_t nib = (word >> (c & 31)) & 15u;
    float xs[4] = {x.x, x.y, x.z, x.w}, go[4];
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      const float e = expf((xs[e4] - mx) - lsum);
      float g = 0.f;
      if ((nib >> e4) & 1u) {
        const float t = implicit ? 1.0f : b.vals[rk_entry_index(b, row, c + e4, word)];
        g = -t * inv_B;
      }
      go[e4] = (c + e4 < n) ? g - e * sum_g : 0.f;      // (padding columns of the last quad: 0)
      gmax = fmaxf(gmax, fabsf(go[e4]));
    }
    reinterpret_cast<float4 *>(orow)[i] = make_float4(go[0], go[1], go[2], go[3]);
  };
#pragma unroll
  for (int u = 0; u < MNLL_CACHE; ++u) {
    const int i = tid + u * 256;
    if (i < n4) grad_quad(i, xc[u], wc[u]);
  }
  for (int i = tid + MNLL_CACHE * 256; i < n4; i += 256) grad_quad(i, orow4[i], brow[i >> 3]);
  // running max |dLoss/dLogit| of the block, as the MSE / BCE epilogue publishes it
  gmax = rk_wave_max(gmax);
  __syncthreads();
  if (lane == 0) red[wid] = gmax;
  __syncthreads();
  if (tid == 0) publish_amax(b.counts, r, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

// local softmax statistics of a row's shard: stats[r] = {max, sum exp(o - max)}
__global__ __launch_bounds__(256) void mnll_row_stats_kernel(const float *dO, rk_block_t b,
                                                             float *stats) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  const int n = b.counts[0], ld = b.counts[2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float *orow = dO + (int64_t)r * ld;
  float mx = -INFINITY;
  for (int c = tid; c < n; c += 256) mx = fmaxf(mx, orow[c]);
  mx = rk_wave_max(mx);
  if (lane == 0) red[wid] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float se = 0.f;
  for (int c = tid; c < n; c += 256) se += expf(orow[c] - mx);
  se = rk_wave_sum(se);
  if (lane == 0) red[wid] = se;
  __syncthreads();
  if (tid == 0) {
    stats[2 * r] = mx;
    stats[2 * r + 1] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// one workgroup of 1024 threads: thread-strided double sums (8 independent loads in flight per
// thread -- item-heavy blocks have ~10^4 partials, which a single wave took 110 us to walk) and a
// fixed LDS tree (order-deterministic); re-zeroes the partials so the next rk_decode_loss finds
// them clean
__global__ __launch_bounds__(1024) void loss_reduce_kernel(float *part, int n, float denom,
                                                           float *loss) {
  __shared__ double red[1024];
  const int tid = threadIdx.x;
  double s = 0.0;
  int i = tid;
  for (; i + 7 * 1024 < n; i += 8 * 1024) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[i + u * 1024];
#pragma unroll
    for (int u = 0; u < 8; ++u) { s += (double)v[u]; part[i + u * 1024] = 0.f; }
  }
  for (; i < n; i += 1024) {
    s += (double)part[i];
    part[i] = 0.f;
  }
  red[tid] = s;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)red[0] / denom;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

constexpr int DZ_SPLITS = 64;        // at most; see dz_splits
// split-K factor of the dZ GEMM: enough (row tile, split) pairs to fill the chip twice, a
// multiple of 8 (the XCD tile mapping), never more than DZ_SPLITS -- at B = 500 that is 64, at
// B = 4000 (item-parallel global batches) 16, so the partial slabs stay ~6x the output
// split-K factor of the dW GEMM (K = B): its output has only n_b/32 x h/128 tiles, too few to
// fill the chip once the batch is large and the item shard small (item-parallel ranks)
inline int dw_splits(int B) {
  return B >= 3000 ? 4 : (B >= 1500 ? 2 : 1);
}

inline int dz_splits(int B) {
  const int tiles_m = rk_cdiv(B, 128);
  const int v = rk_tune_get(RK_TUNE_DZ_SPLITS);
  const int cap = (v >= 8 && v <= DZ_SPLITS) ? (v & ~7) : DZ_SPLITS;
  int s = (512 / tiles_m) & ~7;
  return s < 8 ? 8 : (s > cap ? cap : s);
}
constexpr int DEC_BM = 64;          // rows per decode tile (rk_loss_partials, gb_part rows)

// RK_GEMM_PREC = f32 : the three decoder contractions on the fp32 MFMA (exact fma chains);
// default: the split-fp16 path (PREC_H3 above).
inline bool use_h3() {
  static const int v = [] {
    const char *e = getenv("RK_GEMM_PREC");
    return (e && (e[0] == 'f' || e[0] == 'F')) ? 0 : 1;
  }();
  return v != 0;
}

}  // namespace

namespace {
// slots[0] <- max |x| as an fp32 bit pattern, slots[1..63] <- 0 (one workgroup; x is [B, h]-sized)
__global__ __launch_bounds__(1024) void amax_kernel(const float *__restrict__ x, int64_t n,
                                                    uint32_t *__restrict__ slots) {
  __shared__ float red[16];
  float m = 0.f;
  const int64_t n4 = n >> 2;
  for (int64_t i = threadIdx.x; i < n4; i += 1024) {
    const float4 v = reinterpret_cast<const float4 *>(x)[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 1024) m = fmaxf(m, fabsf(x[i]));
  m = rk_wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x < 64) {
    float t = 0.f;
    if (threadIdx.x == 0)
      for (int k = 0; k < 16; ++k) t = fmaxf(t, red[k]);
    slots[threadIdx.x] = threadIdx.x == 0 ? __float_as_uint(t) : 0u;
  }
}
}  // namespace

extern "C" int rk_amax(const float *x, int64_t n, int32_t *slots, void *stream_) {
  RK_REQUIRE(x != nullptr && slots != nullptr && (((uintptr_t)x) & 15) == 0, "x (16-byte aligned), slots");
  RK_LAUNCH(amax_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream_, x, n,
            reinterpret_cast<uint32_t *>(slots));
  RK_CHECK_LAUNCH("amax");
  return 0;
}

int rk_dz_splits(int B) { return dz_splits(B); }

int rk_splitk_reduce(const float *ws, int M, int N, const int32_t *Kdev, int splits, const float *Zact,
                     int act, float *out, void *stream_) {
  const int grid = rk_cdiv((int64_t)M * N / 4, 64);
  RK_LAUNCH(splitk_reduce_kernel, dim3(grid), dim3(RED_W * 64), 0, (hipStream_t)stream_, ws, M, N, Kdev, 0,
            splits, Zact, act, out);
  RK_CHECK_LAUNCH("splitk_reduce");
  return 0;
}

int rk_splitk_reduce_tiles(const float *ws, int M, int N, const int32_t *Kdev, int max_splits, int tile_k,
                           const float *Zact, int act, float *out, void *stream_) {
  const int grid = rk_cdiv((int64_t)M * N / 4, 64);
  RK_LAUNCH(splitk_reduce_kernel, dim3(grid), dim3(RED_W * 64), 0, (hipStream_t)stream_, ws, M, N, Kdev, tile_k,
            max_splits, Zact, act, out);
  RK_CHECK_LAUNCH("splitk_reduce");
  return 0;
}

extern "C" void rk_gemm_probe(unsigned long long *buffer) { g_gemm_probe = buffer; }

extern "C" int32_t rk_gemm_split16(void) { return use_h3() ? 1 : 0; }

// RK_GEMM_PREC=bf16: the one-call step's decoder contractions on PLAIN bf16 operands (one product,
// fp32 accumulate) -- BASELINE configs[1]'s dtype, a separate data point that misses the 1e-5
// parity bar by design; everything else keeps the split operands
extern "C" int32_t rk_gemm_plain_bf16(void) {
  static const int v = [] {
    const char *e = getenv("RK_GEMM_PREC");
    return (e && (e[0] == 'b' || e[0] == 'B')) ? 1 : 0;
  }();
  return v;
}

extern "C" int64_t rk_dz_workspace_bytes(int32_t B, int32_t h) {
  // (slabs x rows is not monotone in the batch size: cover every batch size up to the capacity)
  int64_t rows = 0;
  for (int b = 1; b <= B; ++b) rows = std::max(rows, (int64_t)dz_splits(b) * b);
  return rows * h * (int64_t)sizeof(float);
}

// row segments of the encoder backward inside rk_decode_bwd_dw_encode_bwd (see encoder_bwd.h)
int32_t rk_encode_bwd_segments(int32_t B) {
  const int s = rk_cdiv(B, 512);
  return s < 1 ? 1 : (s > 8 ? 8 : s);
}

extern "C" int64_t rk_dw_workspace_bytes(int32_t B, int32_t h, int32_t n_cap) {
  const int s = dw_splits(B);
  return s > 1 ? (int64_t)s * n_cap * h * sizeof(float) : 0;
}

extern "C" int32_t rk_decode_row_tile(void) { return DEC_BM; }

extern "C" int32_t rk_dw_splits(int32_t B) { return dw_splits(B); }

extern "C" int32_t rk_loss_partials(int32_t B, int32_t n_cap) {
  // worst case over the decode tilings (64-row x 64-column tiles); MNLL uses one per row
  const int tiles = rk_cdiv(B, DEC_BM) * rk_cdiv(n_cap, 64);
  return tiles > B ? tiles : B;
}


extern "C" int rk_decode_loss(const float *Z, int32_t B, int32_t h, const rk_block_t *tgt,
                              int32_t row_off, const float *W_de, const float *b_de,
                              int32_t loss_kind, float confidence, float inv_B, float *dO,
                              int32_t ld_out, float *loss_part, float *gb_part,
                              const int32_t *ranges, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RK_REQUIRE(h % 4 == 0, "h must be a multiple of 4");
  RK_REQUIRE(aligned16(Z) && aligned16(W_de), "Z and W_de must be 16-byte aligned");
  RK_REQUIRE(row_off >= 0 && row_off + B <= tgt->S_cap, "row slice out of range");
  if (B == 0) return 0;
  GemmP p = {};
  p.probe = g_gemm_probe;
  p.A = Z; p.lda = h;
  p.Bm = W_de; p.ldb = h; p.bidx = tgt->items;
  p.a_scale = SCALE_Z; p.b_scale = SCALE_W;
  if (ranges) {      // published bounds of |Z| / |W_de| (rk_amax, rk_adam_job_t.amax_out)
    p.a_amax = reinterpret_cast<const uint32_t *>(ranges);
    p.b_amax = reinterpret_cast<const uint32_t *>(ranges) + 64;
  }
  p.M = B; p.N = tgt->n_cap; p.K = h;
  p.Ndev = tgt->counts;          // n_t
  p.tiles_m = rk_cdiv(B, DEC_BM);
  p.kchunk = h;
  p.C = dO; p.bias = b_de; p.bias_gather = 1; p.act = RK_ACT_NONE;
  p.blk = *tgt; p.row_off = row_off; p.loss_kind = loss_kind;
  p.confidence = confidence; p.inv_B = inv_B; p.loss_part = loss_part; p.gb_part = gb_part;
  const int tiles = rk_cdiv(p.tiles_m * rk_cdiv(tgt->n_cap, 128), 8) * 8;
  // K = h is short: a K-tile of 40 divides h = 200 (40, 80, 120, ...) exactly -- 5 k-tiles
  // instead of 7 of 32 with the last one 3/4 padding (12 % fewer MFMAs, 2 fewer barriers)
  const bool bk40 = (h % 40 == 0) && (h % 32 != 0);
  // 64x128 tiles, BK = 32: ~2x the workgroups of a 128x128 tiling (two resident
  // per CU hide the staging latency) and 2x the MFMA work per staged tile
  if (loss_kind == RK_LOSS_MSE || loss_kind == RK_LOSS_BCE) {
    // loss_part must be all-zero on entry (surplus tiles never write their slot):
    // it is allocated zeroed and rk_loss_reduce re-zeroes what it consumed
    RK_REQUIRE(tgt->implicit || tgt->pref_rc != nullptr, "explicit values need pref_rc");
    p.ld_dev = tgt->counts + 2;
    if (use_h3()) {
      // 64 x 128 tiles (measured against 64 x 64 / 128 x 128 at C2: 0.146 / 0.160 / 0.153 ms per
      // step, on an 8-way item shard 0.223 / 0.249 / 0.238)
      const bool mse = (loss_kind == RK_LOSS_MSE);
      p.tiles_m = rk_cdiv(B, DEC_BM);
      const int g = rk_cdiv(p.tiles_m * rk_cdiv(tgt->n_cap, 128), 8) * 8;
#define LAUNCH(TM, TN, BKK)                                                                      \
  do {                                                                                           \
    if (mse)                                                                                     \
      RK_LAUNCH((gemm_kernel<2, 2, TM, TN, 0, 0, EPI_LOSS_MSE, true, BKK, PREC_H3>), dim3(g, 1), \
                dim3(256), 0, stream, p);                                                        \
    else                                                                                         \
      RK_LAUNCH((gemm_kernel<2, 2, TM, TN, 0, 0, EPI_LOSS_BCE, true, BKK, PREC_H3>), dim3(g, 1), \
                dim3(256), 0, stream, p);                                                        \
  } while (0)
      LAUNCH(1, 2, 32);
#undef LAUNCH
      RK_CHECK_LAUNCH("decode_loss");
      return 0;
    }
    // large batches (item-parallel ranks: thousands of rows against a small item shard) run
    // 64 x 64 tiles with BK = 16 -- 4-5 workgroups per CU instead of 2 keep the matrix pipe
    // busier once every CU holds many tiles (-20 % at B = 4000, n_b = 2.3k; no gain at B = 500)
    if (B >= 1500) {
      const int t64 = rk_cdiv(p.tiles_m * rk_cdiv(tgt->n_cap, 64), 8) * 8;
      if (loss_kind == RK_LOSS_MSE)
        RK_LAUNCH((gemm_kernel<2, 2, 1, 1, 0, 0, EPI_LOSS_MSE, true, 16>), dim3(t64, 1), dim3(256), 0,
                  stream, p);
      else
        RK_LAUNCH((gemm_kernel<2, 2, 1, 1, 0, 0, EPI_LOSS_BCE, true, 16>), dim3(t64, 1), dim3(256), 0,
                  stream, p);
    } else if (bk40 && loss_kind == RK_LOSS_MSE)
      RK_LAUNCH((gemm_kernel<2, 2, 1, 2, 0, 0, EPI_LOSS_MSE, true, 40>), dim3(tiles, 1),
                         dim3(256), 0, stream, p);
    else if (bk40)
      RK_LAUNCH((gemm_kernel<2, 2, 1, 2, 0, 0, EPI_LOSS_BCE, true, 40>), dim3(tiles, 1),
                         dim3(256), 0, stream, p);
    else if (loss_kind == RK_LOSS_MSE)
      RK_LAUNCH((gemm_kernel<2, 2, 1, 2, 0, 0, EPI_LOSS_MSE, true, 32>), dim3(tiles, 1),
                         dim3(256), 0, stream, p);
    else
      RK_LAUNCH((gemm_kernel<2, 2, 1, 2, 0, 0, EPI_LOSS_BCE, true, 32>), dim3(tiles, 1),
                         dim3(256), 0, stream, p);
  } else {
    if (loss_kind == RK_LOSS_MNLL) { p.ldc = 0; p.ld_dev = tgt->counts + 2; }
    else { RK_REQUIRE(ld_out > 0, "ld_out"); p.ldc = ld_out; }
    if (use_h3())
      RK_LAUNCH((gemm_kernel<2, 2, 1, 2, 0, 0, EPI_STORE, true, 32, PREC_H3>), dim3(tiles, 1),
                dim3(256), 0, stream, p);
    else if (bk40)
      RK_LAUNCH((gemm_kernel<2, 2, 1, 2, 0, 0, EPI_STORE, true, 40>), dim3(tiles, 1), dim3(256),
                         0, stream, p);
    else
      RK_LAUNCH((gemm_kernel<2, 2, 1, 2, 0, 0, EPI_STORE, true, 32>), dim3(tiles, 1), dim3(256),
                         0, stream, p);
  }
  RK_CHECK_LAUNCH("decode_loss");
  return 0;
}

extern "C" int rk_mnll_row_stats(const float *logits, int32_t B, const rk_block_t *tgt, float *stats,
                                 void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B == 0) return 0;
  RK_LAUNCH(mnll_row_stats_kernel, dim3(B), dim3(256), 0, stream, logits, *tgt, stats);
  RK_CHECK_LAUNCH("mnll_row_stats");
  return 0;
}

// row_max / row_logsum / row_tsum: all NULL (the block holds whole rows) or all given (item parallel)
extern "C" int rk_mnll_finish(float *dO, int32_t B, const rk_block_t *tgt, int32_t row_off,
                              float inv_B, const float *row_max, const float *row_logsum,
                              const float *row_tsum, float *loss_part, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B == 0) return 0;
  RK_REQUIRE(tgt->implicit || tgt->pref_rc != nullptr, "explicit values need pref_rc");
  RK_REQUIRE((row_max && row_logsum && row_tsum) || (!row_max && !row_logsum && !row_tsum),
             "row statistics: all three or none");
  RK_LAUNCH(mnll_finish_kernel, dim3(B), dim3(256), 0, stream, dO, *tgt, row_off, inv_B, loss_part,
            row_max, row_logsum, row_tsum);
  RK_CHECK_LAUNCH("mnll_finish");
  return 0;
}

extern "C" int rk_loss_reduce(float *loss_part, int32_t n, float denom, float *loss,
                              void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RK_LAUNCH(loss_reduce_kernel, dim3(1), dim3(1024), 0, stream, loss_part, n, denom, loss);
  RK_CHECK_LAUNCH("loss_reduce");
  return 0;
}

// dZ = dO . W_de[T]   (M = B, N = h, K = n_t) split-K, then reduce (* act')
extern "C" int rk_decode_bwd_dz(const float *dO, int32_t B, int32_t h, const rk_block_t *tgt,
                                const float *W_de, const float *Zact, int32_t act, float *dZ,
                                float *workspace, const int32_t *ranges, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RK_REQUIRE(h % 4 == 0, "h must be a multiple of 4");
  RK_REQUIRE(aligned16(dO) && aligned16(W_de) && aligned16(workspace) && aligned16(dZ),
             "operands must be 16-byte aligned");
  if (B == 0) return 0;
  GemmP p = {};
  p.probe = g_gemm_probe;
  p.A = dO; p.lda_dev = tgt->counts + 2;
  p.Bm = W_de; p.ldb = h; p.bidx = tgt->items;
  p.a_scale = SCALE_DO; p.b_scale = SCALE_W;
  p.a_amax = reinterpret_cast<const uint32_t *>(tgt->counts) + 8;
  if (ranges) p.b_amax = reinterpret_cast<const uint32_t *>(ranges) + 64;
  p.M = B; p.N = h; p.K = tgt->n_cap; p.Kdev = tgt->counts;
  p.C = workspace;
  p.kchunk = 0;                       // derived in-kernel from the device-resident n_t
  const int splits = dz_splits(B);
  const int kchunk = 0;
  // wave tile 32 x (32*TN): pick TN by h
  // split-fp16: 128-column tiles up to h = 256 (two resident workgroups per CU at 74 KB of LDS;
  // the 224-wide tile of the fp32 path needs 101 KB here: 29 vs 31 us at C2, 52 vs 57 us on an
  // 8-way item shard, although dO is then split once per column tile)
  // (long contractions -- a 1 M-item catalogue, K ~ 50 k -- run many k-tiles per workgroup: there
  // the 128-column tile with two resident workgroups beats the 256-column one with a single one,
  // 0.855 vs 0.912 ms per C5-shaped step)
  const int tn = use_h3() ? (h <= 64 ? 2 : ((h <= 256 || tgt->n_cap >= 32768) ? 4 : 8))
                          : (h <= 64 ? 2 : (h <= 128 ? 4 : (h <= 224 ? 7 : 8)));
  p.tiles_m = rk_cdiv(B, 128);
  const int tiles = p.tiles_m * rk_cdiv(h, 32 * tn);   // x 64 splits: a multiple of 8
#define LAUNCH(TN)                                                                              \
  do {                                                                                          \
    if (use_h3())                                                                          \
      RK_LAUNCH((gemm_kernel<4, 1, 1, TN, 0, 1, EPI_SPLITK, true, 32, PREC_H3>),               \
                dim3(tiles, splits), dim3(256), 0, stream, p);                                  \
    else                                                                                        \
      RK_LAUNCH((gemm_kernel<4, 1, 1, TN, 0, 1, EPI_SPLITK, true>), dim3(tiles, splits),        \
                dim3(256), 0, stream, p);                                                       \
  } while (0)
  if (tn == 2) LAUNCH(2); else if (tn == 4) LAUNCH(4); else if (tn == 7) LAUNCH(7); else LAUNCH(8);
#undef LAUNCH
  RK_CHECK_LAUNCH("decode_bwd_dz");
  const int grid = rk_cdiv((int64_t)B * h / 4, 64);
  RK_LAUNCH(splitk_reduce_kernel, dim3(grid), dim3(RED_W * 64), 0, stream, workspace, B, h,
                     tgt->counts, kchunk, splits, Zact, act, dZ);
  RK_CHECK_LAUNCH("splitk_reduce");
  return 0;
}

// G_de[n_t,h] = dO^T . Z   (M = n_t, N = h, K = B); gb_de = colsum(dO) if asked
extern "C" int rk_decode_bwd_dw(const float *dO, const float *Z, int32_t B, int32_t h,
                                const rk_block_t *tgt, float *G_de, float *gb_de,
                                void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RK_REQUIRE(h % 4 == 0, "h must be a multiple of 4");
  RK_REQUIRE(aligned16(dO) && aligned16(Z) && aligned16(G_de), "operands must be 16-byte aligned");
  if (B == 0) return 0;
  GemmP p = {};
  p.probe = g_gemm_probe;
  p.A = dO; p.lda_dev = tgt->counts + 2;
  p.Bm = Z; p.ldb = h;
  p.a_scale = SCALE_DO; p.b_scale = SCALE_Z;     // (dW runs on the fp32 MFMA: unused)
  p.M = tgt->n_cap; p.Mdev = tgt->counts; p.N = h; p.K = B;
  p.kchunk = B;
  p.C = G_de; p.ldc = h; p.act = RK_ACT_NONE;
  {
    // 32 x 128 tiles, BK = 32 (two workgroups per CU at h = 200).  Larger tiles (64x64 ...
    // 128x128) were probed at B = 500 and at item-parallel shapes (B = 4000, n_b = 2.3k):
    // none is faster -- the contraction has too few output tiles, split-K is what helps.
    p.n_fastest = 1;   // the h/128 column tiles of one dO panel stay on one XCD
    p.tiles_m = rk_cdiv(tgt->n_cap, 32);
    const int tiles = rk_cdiv(p.tiles_m * rk_cdiv(h, 128), 8) * 8;
    // (stays on the fp32 MFMA: Z would be re-split by every one of the ~500 workgroups, and the
    // split-fp16 variant measured 31 vs 30 us alone and 53 vs 38 us fused with the encoder backward)
    RK_LAUNCH((gemm_kernel<1, 4, 1, 1, 1, 1, EPI_STORE, true, 32>), dim3(tiles, 1), dim3(256), 0,
              stream, p);
  }
  RK_CHECK_LAUNCH("decode_bwd_dw");
  if (gb_de) return rk_colsum(dO, B, tgt->n_cap, 0, tgt->counts, gb_de, stream_);
  return 0;
}

// rk_decode_bwd_dw + rk_ae_encode_bwd (untied weights, same block) in one launch
int rk_decode_bwd_dw_encode_bwd(const float *dO, const float *Z, int32_t B, int32_t h,
                                           const rk_block_t *blk, float *G_de, int32_t row_off,
                                           const float *dZ0pre, float *G_en, float *gb_en,
                                           float *workspace, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RK_REQUIRE(h > 0 && h % 4 == 0 && h <= 1024, "h must be a multiple of 4, <= 1024");
  RK_REQUIRE(aligned16(dO) && aligned16(Z) && aligned16(G_de) && aligned16(workspace),
             "operands must be 16-byte aligned");
  RK_REQUIRE(row_off >= 0 && B >= 0 && row_off + B <= blk->S_cap, "row slice out of range");
  RK_REQUIRE(blk->bits_cr != nullptr && blk->pref_rc != nullptr,
             "block was built without the transposed bitmap / prefix index");
  RK_REQUIRE(G_de != nullptr || (workspace != nullptr && dw_splits(B) > 1),
             "G_de == NULL (leave the split-K slabs in the workspace) needs rk_dw_splits(B) > 1");
  if (B == 0) return 0;
  // large batches: split K (= B) so that the few dW tiles still fill the chip; the slabs go to
  // `workspace` (rk_dw_workspace_bytes) and are summed in split order by slab_sum_kernel
  const int splits = workspace ? dw_splits(B) : 1;
  GemmP p = {};
  p.probe = g_gemm_probe;
  p.A = dO; p.lda_dev = blk->counts + 2;
  p.Bm = Z; p.ldb = h;
  p.a_scale = SCALE_DO; p.b_scale = SCALE_Z;     // (dW runs on the fp32 MFMA: unused)
  p.M = blk->n_cap; p.Mdev = blk->counts; p.N = h; p.K = B;
  p.kchunk = splits > 1 ? ((rk_cdiv(B, splits) + 31) & ~31) : B;
  p.C = splits > 1 ? workspace : G_de; p.ldc = h; p.act = RK_ACT_NONE;
  p.tiles_m = rk_cdiv(blk->n_cap, 32);
  p.n_fastest = 1;
  const int n_dw = rk_cdiv(p.tiles_m * rk_cdiv(h, 128), 8) * 8 * splits;
  const int n_seg = rk_encode_bwd_segments(B);
  const int n_gb = gb_en ? rk_cdiv(h, 64) * n_seg : 0;
  const int64_t seg_stride = (int64_t)blk->n_cap * h;
  const int grid = n_dw + blk->n_cap * n_seg + n_gb;
  const int hv = rk_cdiv(h, 256);
#define LAUNCH(HV, SPLIT)                                                                       \
  RK_LAUNCH((dw_encode_bwd_kernel<HV, SPLIT>), dim3(grid), dim3(256), 0, stream, p, n_dw, splits, \
            *blk, row_off, B, dZ0pre, h, G_en, gb_en, n_gb, n_seg, seg_stride)
  if (splits > 1) {
    if (hv == 1) LAUNCH(1, true); else if (hv == 2) LAUNCH(2, true); else LAUNCH(4, true);
  } else {
    if (hv == 1) LAUNCH(1, false); else if (hv == 2) LAUNCH(2, false); else LAUNCH(4, false);
  }
#undef LAUNCH
  RK_CHECK_LAUNCH("decode_bwd_dw_encode_bwd");
  if (splits > 1 && G_de != nullptr) {
    RK_LAUNCH(slab_sum_kernel, dim3(rk_cdiv((int64_t)blk->n_cap * h / 4, 256)), dim3(256), 0, stream,
              workspace, blk->n_cap, h, blk->counts, splits, G_de);
    RK_CHECK_LAUNCH("slab_sum");
  }
  return 0;
}

namespace {
template <int AMODE, int BMODE>
void launch_small(const GemmP &p, int tiles, bool vec, hipStream_t stream) {
  if (vec)
    RK_LAUNCH((gemm_kernel<2, 2, 1, 1, AMODE, BMODE, EPI_STORE, true>), dim3(tiles, 1),
                       dim3(256), 0, stream, p);
  else
    RK_LAUNCH((gemm_kernel<2, 2, 1, 1, AMODE, BMODE, EPI_STORE, false>), dim3(tiles, 1),
                       dim3(256), 0, stream, p);
}
}  // namespace

// Y[B,N] = act(X[B,K] . W^T + b);  W is [N,K] (nn.Linear) or [K,N] if w_transposed
extern "C" int rk_linear_fwd(const float *X, const float *W, const float *b, int32_t B,
                             int32_t N, int32_t K, int32_t w_transposed, int32_t act, float *Y,
                             void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B == 0) return 0;
  if (rk_small_gemm_fits(B, N, K) && g_gemm_probe == nullptr) {
    rk_small_gemm_t g = {};
    g.A = X; g.lda = K; g.amode = 0;
    g.B = W; g.ldb = w_transposed ? N : K; g.bmode = w_transposed ? 1 : 0;
    g.M = B; g.N = N; g.K = K; g.C = Y; g.ldc = N; g.bias = b; g.act = act;
    return rk_small_gemm(&g, stream_);
  }
  GemmP p = {};
  p.probe = g_gemm_probe;
  p.A = X; p.lda = K;
  p.Bm = W; p.ldb = w_transposed ? N : K;
  p.M = B; p.N = N; p.K = K; p.kchunk = K;
  const bool vec = aligned16(X) && aligned16(W) && (K % 4 == 0) && (p.ldb % 4 == 0);
  p.C = Y; p.ldc = N; p.bias = b; p.act = act;
  p.tiles_m = rk_cdiv(B, 64);
  const int tiles = rk_cdiv(p.tiles_m * rk_cdiv(N, 64), 8) * 8;
  if (!w_transposed) launch_small<0, 0>(p, tiles, vec, stream);
  else launch_small<0, 1>(p, tiles, vec, stream);
  RK_CHECK_LAUNCH("linear_fwd");
  return 0;
}

static int linear_bwd_impl(float *dY, const float *Y, const float *X, const float *W, int32_t B,
                           int32_t N, int32_t K, int32_t w_transposed, int32_t act, float *dX,
                           float *dW, int32_t dw_accumulate, float *db, const float *dx_act_y, void *stream_,
                           bool pre = false);


extern "C" int rk_linear_bwd(float *dY, const float *Y, const float *X, const float *W, int32_t B,
                             int32_t N, int32_t K, int32_t w_transposed, int32_t act, float *dX,
                             float *dW, int32_t dw_accumulate, float *db, void *stream_) {
  return linear_bwd_impl(dY, Y, X, W, B, N, K, w_transposed, act, dX, dW, dw_accumulate, db, nullptr, stream_);
}

extern "C" int rk_linear_bwd_dact(float *dY, const float *Y, const float *X, const float *W, int32_t B,
                                  int32_t N, int32_t K, int32_t w_transposed, int32_t act, float *dX,
                                  float *dW, int32_t dw_accumulate, float *db, const float *dx_act_y,
                                  void *stream_) {
  RK_REQUIRE(dX != nullptr || dx_act_y == nullptr, "dx_act_y needs dX");
  return linear_bwd_impl(dY, Y, X, W, B, N, K, w_transposed, act, dX, dW, dw_accumulate, db, dx_act_y, stream_);
}

extern "C" int rk_linear_bwd_pre(const float *dYpre, const float *X, const float *W, int32_t B, int32_t N,
                                 int32_t K, int32_t w_transposed, int32_t act, float *dX, float *dW,
                                 int32_t dw_accumulate, float *db, const float *dx_act_y, void *stream_) {
  RK_REQUIRE(dX != nullptr || dx_act_y == nullptr, "dx_act_y needs dX");
  return linear_bwd_impl(const_cast<float *>(dYpre), nullptr, X, W, B, N, K, w_transposed, act, dX, dW,
                         dw_accumulate, db, dx_act_y, stream_, true);
}

static int linear_bwd_impl(float *dY, const float *Y, const float *X, const float *W, int32_t B,
                           int32_t N, int32_t K, int32_t w_transposed, int32_t act, float *dX,
                           float *dW, int32_t dw_accumulate, float *db, const float *dx_act_y, void *stream_,
                           bool pre) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B == 0) return 0;
  int rc = 0;
  const int ldw0 = w_transposed ? N : K;
  const bool g_linear_pair = rk_tune_get(RK_TUNE_LINEAR_PAIR) != 0;
  // pre: dY already IS dYpre (its producer multiplied act' in) -- no pass over it; the bias gradient's
  // column sums ride on the dX / dW launch where that is one launch, else they are an rk_colsum
  const bool small0 = g_gemm_probe == nullptr && rk_small_gemm_fits(B, K, N) &&
                      rk_small_gemm_fits(w_transposed ? K : N, w_transposed ? N : K, B);
  const bool cs_in_pair = pre && db && small0 && dX && dW && g_linear_pair;
  if (!pre)
    rc = db ? rk_act_grad_colsum(dY, Y, B, N, act, db, stream_)
            : rk_act_grad(dY, Y, (int64_t)B * N, act, stream_);
  else if (db && !cs_in_pair)
    rc = rk_colsum(dY, B, N, N, nullptr, db, stream_);
  if (rc) return rc;
  const int ldw = w_transposed ? N : K;
  const bool small = g_gemm_probe == nullptr && rk_small_gemm_fits(B, K, N) &&
                     rk_small_gemm_fits(w_transposed ? K : N, w_transposed ? N : K, B);
  if (small) {
    rk_small_gemm_t gx = {}, gw = {};
    if (dX) {  // dX[B,K] = dY[B,N] . Weff[N,K]: reduction over N
      gx.A = dY; gx.lda = N; gx.amode = 0;
      gx.B = W; gx.ldb = ldw; gx.bmode = w_transposed ? 0 : 1;   // W[N,K]: k-major; Wst[K,N]: N contiguous
      gx.M = B; gx.N = K; gx.K = N; gx.C = dX; gx.ldc = K; gx.act = RK_ACT_NONE;
      gx.dact_y = dx_act_y; gx.dact = act;
    }
    if (dW) {  // reduction over the B rows: both operands k-major
      rk_small_gemm_t &g = gw;
      g.amode = 1; g.bmode = 1; g.K = B; g.act = RK_ACT_NONE; g.accumulate = dw_accumulate; g.C = dW;
      if (!w_transposed) { g.A = dY; g.lda = N; g.B = X; g.ldb = K; g.M = N; g.N = K; g.ldc = K; }   // dW[N,K] = dY^T . X
      else               { g.A = X; g.lda = K; g.B = dY; g.ldb = N; g.M = K; g.N = N; g.ldc = N; }   // dWst[K,N] = X^T . dY
    }
    // both read dYpre only and write disjoint outputs: ONE launch of two workgroup ranges
    // (rk_small_gemm_pair: 7.2 us against 6.6 + 8.6 one behind the other at 500 x 200 x 200,
    // tools/probes/linear_bwd_probe.py 13.1 vs 17.7 us per call with the act' pass; C3 0.251 vs 0.264 ms
    // per step).  rk_tune(RK_TUNE_LINEAR_PAIR, 0): two launches (same tiles, same sums)
    if (cs_in_pair) return rk_small_gemm_pair_colsum(&gx, &gw, dY, B, N, db, stream_);
    if (dX && dW && g_linear_pair) return rk_small_gemm_pair(&gx, &gw, stream_);
    if (dX) { rc = rk_small_gemm(&gx, stream_); if (rc) return rc; }
    if (dW) { rc = rk_small_gemm(&gw, stream_); if (rc) return rc; }
    return 0;
  }
  if (dX) {  // dX[B,K] = dY[B,N] . Weff[N,K]
    GemmP p = {};
  p.probe = g_gemm_probe;
    p.A = dY; p.lda = N;
    p.Bm = W; p.ldb = ldw;
    p.M = B; p.N = K; p.K = N; p.kchunk = N;
    const bool vec = aligned16(dY) && aligned16(W) && (N % 4 == 0) && (ldw % 4 == 0);
    p.C = dX; p.ldc = K; p.act = RK_ACT_NONE;
    p.tiles_m = rk_cdiv(B, 64);
    const int tiles = rk_cdiv(p.tiles_m * rk_cdiv(K, 64), 8) * 8;
    if (!w_transposed) launch_small<0, 1>(p, tiles, vec, stream);   // W[N,K]: k-major
    else launch_small<0, 0>(p, tiles, vec, stream);                 // Wst[K,N]: reduction contiguous
    RK_CHECK_LAUNCH("linear_bwd_dx");
    if (dx_act_y) {
      rc = rk_act_grad(dX, dx_act_y, (int64_t)B * K, act, stream_);
      if (rc) return rc;
    }
  }
  if (dW) {
    GemmP p = {};
  p.probe = g_gemm_probe;
    p.K = B; p.kchunk = B; p.act = RK_ACT_NONE; p.accumulate = dw_accumulate; p.C = dW;
    if (!w_transposed) {  // dW[N,K] = dY^T . X
      p.A = dY; p.lda = N; p.Bm = X; p.ldb = K; p.M = N; p.N = K; p.ldc = K;
    } else {              // dWst[K,N] = X^T . dY
      p.A = X; p.lda = K; p.Bm = dY; p.ldb = N; p.M = K; p.N = N; p.ldc = N;
    }
    const bool vec = aligned16(p.A) && aligned16(p.Bm) && (p.lda % 4 == 0) && (p.ldb % 4 == 0);
    p.tiles_m = rk_cdiv(p.M, 64);
    const int tiles = rk_cdiv(p.tiles_m * rk_cdiv(p.N, 64), 8) * 8;
    launch_small<1, 1>(p, tiles, vec, stream);
    RK_CHECK_LAUNCH("linear_bwd_dw");
  }
  return 0;
}
