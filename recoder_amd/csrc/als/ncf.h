#pragma once
#include "ugcn.h"

namespace {

// ------------------------------------------------------------------------ ncf
// NeuMF (He et al. 2017): s(u, i) = w[:dg] . (Pg[u] o Qg[i]) + w[dg:] . phi_L + b0 with phi_0 = [Pm[u] ; Qm[i]] and
// phi_l = relu(W_l phi_{l-1} + c_l), 1 <= L <= 3 layers, every width a multiple of 4 in [4, 128].
//
// The dense parameters travel as ONE f32 vector theta = [W_1, c_1, ..., W_L, c_L, w, b0] (W_l row-major [d_l, d_{l-1}],
// d_0 = 2 dm); a tile's partial dense gradients are a slab of the same layout with the tile's loss sum behind it.
//
// Every matrix product below is a 16 x 16 tile of v_mfma_f32_16x16x4_f32 (lane l: A[l & 15][l >> 4], B[l >> 4][l & 15],
// C[4 (l >> 4) + r][l & 15]): an exact f32 fmaf chain over k ascending from +0.  A workgroup is 4 waves and a tile of
// NCF_TILE = 32 entries (the step) or items (the scores); the weights wait in LDS at a row pitch of d + 1 floats, the
// activations beside them.  32 and not 64: W_1 at dm = d_1 = 128 is 128.5 KB of the 160 KB, and a tile of 64 rows of
// phi_1 does not fit beside it.
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int NCF_TILE = RK_ALS_NCF_TILE, NCF_MAX_W = RK_ALS_NCF_MAX_WIDTH, NCF_MAX_L = RK_ALS_NCF_MAX_LAYERS;
constexpr int64_t NCF_LDS_LIMIT = 160 * 1024;
constexpr int NCF_SCORE_GY = 4;                   // user groups of the scores grid: a workgroup stages the weights once

struct NcfDims {
  int dg, dm, L;
  int d[NCF_MAX_L + 1];                           // d[0] = 2 dm, d[l] the width of layer l (0 past L)
  int woff[NCF_MAX_L + 1], coff[NCF_MAX_L + 1];   // [1 .. L]: where W_l and c_l start in theta
  int w_off, b0_off, n;                           // w, b0 and the number of dense parameters
};

bool ncf_width(int v) { return v >= 4 && v <= NCF_MAX_W && v % 4 == 0; }

bool ncf_dims(int dg, int dm, int L, int d1, int d2, int d3, NcfDims &D) {
  if (!ncf_width(dg) || !ncf_width(dm) || L < 1 || L > NCF_MAX_L) return false;
  const int dl[NCF_MAX_L] = {d1, d2, d3};
  D.dg = dg, D.dm = dm, D.L = L, D.d[0] = 2 * dm;
  int off = 0;
  for (int l = 1; l <= NCF_MAX_L; ++l) {
    D.d[l] = 0, D.woff[l] = D.coff[l] = 0;
    if (l > L) continue;
    if (!ncf_width(dl[l - 1])) return false;
    D.d[l] = dl[l - 1];
    D.woff[l] = off, off += D.d[l] * D.d[l - 1];
    D.coff[l] = off, off += D.d[l];
  }
  D.woff[0] = D.coff[0] = 0;
  D.w_off = off, off += dg + D.d[L];
  D.b0_off = off, D.n = off + 1;
  return true;
}

// floats of LDS: the step holds every W_l (pitch d_{l-1} + 1), the biases, w, b0, phi_1 .. phi_L of the tile and the
// tile's ids, g and loss terms; the scores hold W_2 .., the biases from c_2, w, b0, the tile's rows of A and Qg, two
// activation buffers of the widest layer, the user's half of layer 1 and the user's GMF row.
int64_t ncf_step_lds_floats(const NcfDims &D) {
  int64_t f = D.dg + D.d[D.L] + 1 + 4 * NCF_TILE;
  for (int l = 1; l <= D.L; ++l) f += (int64_t)D.d[l] * (D.d[l - 1] + 1) + D.d[l] + NCF_TILE * (D.d[l] + 1);
  return f;
}
int64_t ncf_scores_lds_floats(const NcfDims &D) {
  int dmax = 0;
  for (int l = 1; l <= D.L; ++l) dmax = std::max(dmax, D.d[l]);
  int64_t f = D.dg + D.d[D.L] + 1 + NCF_TILE * (D.d[1] + 1) + NCF_TILE * (D.dg + 1) + 2 * NCF_TILE * (dmax + 1) +
              D.d[1] + D.dg;
  for (int l = 2; l <= D.L; ++l) f += (int64_t)D.d[l] * (D.d[l - 1] + 1) + D.d[l];
  return f;
}

// C = A B over the workgroup: M = 16 mt_n rows, N = 16 nt_n columns, K a multiple of 4.  A unit is a row tile and two
// column tiles (one read of A serves both); wave w takes the units w, w + 4, ...  A(row, k), B(k, col) give the
// operands (+0 outside the matrices), S(row, col, value) takes the results.  Wave-uniform throughout.
template <class FA, class FB, class FS>
__device__ __forceinline__ void ncf_gemm(int mt_n, int nt_n, int K, int wv, int lane, FA A, FB B, FS S) {
  const int li = lane & 15, lk = lane >> 4;
  const int ng = (nt_n + 1) >> 1;
  for (int unit = wv; unit < mt_n * ng; unit += 4) {
    const int m0 = (unit / ng) * 16, n0 = (unit % ng) * 32;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k += 4) {
      const float a = A(m0 + li, k + lk);
      const float b0 = B(k + lk, n0 + li), b1 = B(k + lk, n0 + 16 + li);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      S(m0 + 4 * lk + r, n0 + li, acc0[r]);
      S(m0 + 4 * lk + r, n0 + 16 + li, acc1[r]);
    }
  }
}

// out[r, j] = relu(c[j] + sum_k A(r, k) W[j, k]) for the tile's rows r and j < N; W [N, K] in LDS at pitch K + 1
template <class FA>
__device__ __forceinline__ void ncf_layer(FA A, int K, const float *W, const float *c, int N, float *out, int wv,
                                          int lane) {
  ncf_gemm(NCF_TILE / 16, (N + 15) >> 4, K, wv, lane, A,
           [&](int k, int j) { return j < N ? W[j * (K + 1) + k] : 0.f; },
           [&](int r, int j, float v) {
             if (j < N) out[r * (N + 1) + j] = fmaxf(v + c[j], 0.f);
           });
}

// a weight matrix [rows, cols] of theta into LDS at pitch cols + 1
__device__ __forceinline__ void ncf_stage(const float *__restrict__ src, int rows, int cols, float *dst, int tid) {
  for (int x = tid; x < rows * cols; x += 256) dst[(x / cols) * (cols + 1) + x % cols] = src[x];
}

// One workgroup per tile of NCF_TILE entries e = t (1 + R) + c: slot t's user with its positive (c = 0, label 1) or
// its negative c - 1 (entry_draw of ugcn.h for (seed, step, t R + c - 1): uniform over the items, nothing rejected;
// label 0).  An entry whose ids lie outside the tables is invalid: g = 0, no loss, sentinel keys.
__global__ __launch_bounds__(256) void als_ncf_step_kernel(
    const int32_t *__restrict__ users, const int32_t *__restrict__ pos, int T, int R, uint64_t seed_key, uint32_t step,
    int n_users, int n_items, const float *__restrict__ Pg, int ldpg, const float *__restrict__ Qg, int ldqg,
    const float *__restrict__ Pm, int ldpm, const float *__restrict__ Qm, int ldqm, const float *__restrict__ theta,
    const NcfDims D, int32_t *__restrict__ ukey, int32_t *__restrict__ ikey, float *__restrict__ GU,
    float *__restrict__ GI, float *__restrict__ slabs) {
  extern __shared__ float ncf_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int E1 = 1 + R, En = T * E1, e0 = blockIdx.x * NCF_TILE;
  const int dg = D.dg, dm = D.dm, L = D.L, h = dg + dm;
  const int d0 = D.d[0], d1 = D.d[1], d2 = D.d[2], d3 = D.d[3], dL = D.d[L];
  float *slab = slabs + (int64_t)blockIdx.x * (D.n + 1);
  // ---- the LDS layout (ncf_step_lds_floats)
  float *p = ncf_lds;
  float *W1 = p; p += d1 * (d0 + 1);
  float *W2 = p; p += L >= 2 ? d2 * (d1 + 1) : 0;
  float *W3 = p; p += L >= 3 ? d3 * (d2 + 1) : 0;
  float *c1 = p; p += d1;
  float *c2 = p; p += d2;
  float *c3 = p; p += d3;
  float *w = p; p += dg + dL;
  float *b0 = p; p += 1;
  float *a1 = p; p += NCF_TILE * (d1 + 1);
  float *a2 = p; p += L >= 2 ? NCF_TILE * (d2 + 1) : 0;
  float *a3 = p; p += L >= 3 ? NCF_TILE * (d3 + 1) : 0;
  int *su = (int *)p; p += NCF_TILE;
  int *si = (int *)p; p += NCF_TILE;
  float *sg = p; p += NCF_TILE;
  float *sl = p;
  float *aL = L == 1 ? a1 : (L == 2 ? a2 : a3);
  ncf_stage(theta + D.woff[1], d1, d0, W1, tid);
  if (L >= 2) ncf_stage(theta + D.woff[2], d2, d1, W2, tid);
  if (L >= 3) ncf_stage(theta + D.woff[3], d3, d2, W3, tid);
  for (int x = tid; x < d1; x += 256) c1[x] = theta[D.coff[1] + x];
  for (int x = tid; x < d2; x += 256) c2[x] = theta[D.coff[2] + x];
  for (int x = tid; x < d3; x += 256) c3[x] = theta[D.coff[3] + x];
  for (int x = tid; x < dg + dL; x += 256) w[x] = theta[D.w_off + x];
  if (tid == 0) b0[0] = theta[D.b0_off];
  if (tid < NCF_TILE) {
    const int e = e0 + tid;
    int u = -1, i = -1;
    if (e < En) {
      const int t = e / E1, c = e - t * E1;
      u = users[t];
      i = c == 0 ? pos[t] : entry_draw(seed_key, step, (uint32_t)t * (uint32_t)R, c, n_items);
      if (u < 0 || u >= n_users || i < 0 || i >= n_items) u = i = -1;
      ukey[e] = u < 0 ? n_users : u;
      ikey[e] = i < 0 ? n_items : i;
    }
    su[tid] = u, si[tid] = i;
  }
  __syncthreads();
  // ---- forward
  auto phi0 = [&](int r, int k) {
    const int u = su[r];
    if (u < 0) return 0.f;
    return k < dm ? Pm[(int64_t)u * ldpm + k] : Qm[(int64_t)si[r] * ldqm + (k - dm)];
  };
  ncf_layer(phi0, d0, W1, c1, d1, a1, wv, lane);
  __syncthreads();
  if (L >= 2) {
    ncf_layer([&](int r, int k) { return a1[r * (d1 + 1) + k]; }, d1, W2, c2, d2, a2, wv, lane);
    __syncthreads();
  }
  if (L >= 3) {
    ncf_layer([&](int r, int k) { return a2[r * (d2 + 1) + k]; }, d2, W3, c3, d3, a3, wv, lane);
    __syncthreads();
  }
  // ---- the logit, eight lanes an entry: lane s takes the dimensions s, s + 8, ... of the GMF term and then of phi_L
  // in one fmaf chain from +0; the eight chains by an xor butterfly (4, 2, 1)
  {
    const int r = tid >> 3, s = tid & 7;
    const int u = su[r], i = si[r];
    float z = 0.f;
    if (u >= 0) {
      for (int k = s; k < dg; k += 8) z = fmaf(w[k], Pg[(int64_t)u * ldpg + k] * Qg[(int64_t)i * ldqg + k], z);
      for (int j = s; j < dL; j += 8) z = fmaf(w[dg + j], aL[r * (dL + 1) + j], z);
    }
    z += __shfl_xor(z, 4, 64);
    z += __shfl_xor(z, 2, 64);
    z += __shfl_xor(z, 1, 64);
    if (s == 0) {
      z += b0[0];
      const bool positive = (e0 + r) % E1 == 0;
      sg[r] = u >= 0 ? ug_sigmoid(z) - (positive ? 1.f : 0.f) : 0.f;
      sl[r] = u >= 0 ? ug_softplus(z) - (positive ? z : 0.f) : 0.f;
    }
  }
  __syncthreads();
  // ---- backward: the GMF rows, dw, db0 and the loss, every sum over the tile's entries in ascending order from +0
  for (int x = tid; x < NCF_TILE * dg; x += 256) {
    const int r = x / dg, k = x - r * dg, e = e0 + r;
    if (e < En) {
      const int u = su[r];
      const float gw = sg[r] * w[k];
      GU[(int64_t)e * h + k] = u >= 0 ? gw * Qg[(int64_t)si[r] * ldqg + k] : 0.f;
      GI[(int64_t)e * h + k] = u >= 0 ? gw * Pg[(int64_t)u * ldpg + k] : 0.f;
    }
  }
  if (tid < dg) {
    float s = 0.f;
    for (int r = 0; r < NCF_TILE; ++r)
      if (su[r] >= 0) s = fmaf(sg[r], Pg[(int64_t)su[r] * ldpg + tid] * Qg[(int64_t)si[r] * ldqg + tid], s);
    slab[D.w_off + tid] = s;
  }
  if (tid >= 128 && tid - 128 < dL) {
    const int j = tid - 128;
    float s = 0.f;
    for (int r = 0; r < NCF_TILE; ++r) s = fmaf(sg[r], aL[r * (dL + 1) + j], s);
    slab[D.w_off + dg + j] = s;
  }
  if (tid == 64) {
    float s = 0.f, ls = 0.f;
    for (int r = 0; r < NCF_TILE; ++r) s += sg[r], ls += sl[r];
    slab[D.b0_off] = s;
    slab[D.n] = ls;
  }
  __syncthreads();
  // dz_L = g w[dg:] where phi_L > 0, in place of phi_L
  for (int x = tid; x < NCF_TILE * dL; x += 256) {
    const int r = x / dL, j = x - r * dL;
    float *a = aL + r * (dL + 1) + j;
    *a = *a > 0.f ? sg[r] * w[dg + j] : 0.f;
  }
  __syncthreads();
  // layer l, from the last: dc_l and dW_l = dz_l^T phi_{l-1} into the slab, then dz_{l-1} = (dz_l W_l) where
  // phi_{l-1} > 0 in place of phi_{l-1} -- or, at l = 1, the MLP halves of the entries' gradient rows
  auto dense_grads = [&](const float *dz, int N, int K, int woff, int coff, auto prev) {
    if (tid < N) {
      float s = 0.f;
      for (int r = 0; r < NCF_TILE; ++r) s += dz[r * (N + 1) + tid];
      slab[coff + tid] = s;
    }
    ncf_gemm((N + 15) >> 4, (K + 15) >> 4, NCF_TILE, wv, lane,
             [&](int j, int r) { return j < N ? dz[r * (N + 1) + j] : 0.f; },
             [&](int r, int k) { return k < K ? prev(r, k) : 0.f; },
             [&](int j, int k, float v) {
               if (j < N && k < K) slab[woff + j * K + k] = v;
             });
  };
  auto back = [&](const float *dz, int N, const float *W, int K, float *prev) {
    ncf_gemm(NCF_TILE / 16, (K + 15) >> 4, N, wv, lane, [&](int r, int j) { return dz[r * (N + 1) + j]; },
             [&](int j, int k) { return k < K ? W[j * (K + 1) + k] : 0.f; },
             [&](int r, int k, float v) {
               if (k < K) {
                 float *a = prev + r * (K + 1) + k;
                 *a = *a > 0.f ? v : 0.f;
               }
             });
  };
  if (L >= 3) {
    dense_grads(a3, d3, d2, D.woff[3], D.coff[3], [&](int r, int k) { return a2[r * (d2 + 1) + k]; });
    __syncthreads();
    back(a3, d3, W3, d2, a2);
    __syncthreads();
  }
  if (L >= 2) {
    dense_grads(a2, d2, d1, D.woff[2], D.coff[2], [&](int r, int k) { return a1[r * (d1 + 1) + k]; });
    __syncthreads();
    back(a2, d2, W2, d1, a1);
    __syncthreads();
  }
  dense_grads(a1, d1, d0, D.woff[1], D.coff[1], phi0);
  ncf_gemm(NCF_TILE / 16, (d0 + 15) >> 4, d1, wv, lane, [&](int r, int j) { return a1[r * (d1 + 1) + j]; },
           [&](int j, int k) { return k < d0 ? W1[j * (d0 + 1) + k] : 0.f; },
           [&](int r, int k, float v) {
             const int e = e0 + r;
             if (e < En && k < d0) {
               if (k < dm) GU[(int64_t)e * h + dg + k] = v;
               else GI[(int64_t)e * h + dg + (k - dm)] = v;
             }
           });
}

// theta -= Adam(the slabs' sum in tile order / entries + reg theta on W_l and w); element n: the loss sum
__global__ __launch_bounds__(256) void als_ncf_dense_adam_kernel(float *__restrict__ theta, float *__restrict__ M,
                                                                 float *__restrict__ V,
                                                                 const float *__restrict__ slabs, int tiles,
                                                                 const NcfDims D, float inv_entries, float reg,
                                                                 float beta1, float beta2, float omb1, float omb2,
                                                                 float eps, float step, float isb2,
                                                                 float *__restrict__ loss) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x > D.n) return;
  float s = 0.f;
  for (int t = 0; t < tiles; ++t) s += slabs[(int64_t)t * (D.n + 1) + x];
  if (x == D.n) {
    loss[0] = s;
    return;
  }
  bool weight = x >= D.w_off && x < D.b0_off;
#pragma unroll
  for (int l = 1; l <= NCF_MAX_L; ++l) weight = weight || (l <= D.L && x >= D.woff[l] && x < D.coff[l]);
  const float e = theta[x];
  float grad = s * inv_entries;
  if (weight) grad = fmaf(reg, e, grad);
  const float m = fmaf(beta1, M[x], omb1 * grad);
  const float v = fmaf(beta2, V[x], (omb2 * grad) * grad);
  M[x] = m;
  V[x] = v;
  theta[x] = fmaf(-step, m / fmaf(sqrtf(v), isb2, eps), e);
}

// A[i, j] = sum_k Qm[i, k] W_1[j, dm + k]: one fmaf chain over k ascending from +0 per element
__global__ __launch_bounds__(256) void als_ncf_item_part_kernel(const float *__restrict__ Qm, int ldqm, int n_items,
                                                                const float *__restrict__ W1, int dm, int d1,
                                                                float *__restrict__ A) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= (int64_t)n_items * d1) return;
  const int64_t i = x / d1;
  const int j = (int)(x - i * d1);
  float s = 0.f;
  for (int k = 0; k < dm; ++k) s = fmaf(Qm[i * ldqm + k], W1[j * 2 * dm + dm + k], s);
  A[x] = s;
}

// UH[b, j] = c_1[j] + sum_k W_1[j, k] Pm[users[b], k] (the chain from +0, then the bias); +0 for an id that is no user
__global__ __launch_bounds__(256) void als_ncf_user_part_kernel(const int32_t *__restrict__ users, int B, int n_users,
                                                                const float *__restrict__ Pm, int ldpm,
                                                                const float *__restrict__ W1,
                                                                const float *__restrict__ c1, int dm, int d1,
                                                                float *__restrict__ UH) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= B * d1) return;
  const int b = x / d1, j = x - b * d1;
  const int u = users[b];
  float s = 0.f;
  if (u >= 0 && u < n_users) {
    for (int k = 0; k < dm; ++k) s = fmaf(W1[j * 2 * dm + k], Pm[(int64_t)u * ldpm + k], s);
    s += c1[j];
  }
  UH[x] = s;
}

// out[b, c] = s(users[b], lo + c): workgroup (tile of NCF_TILE items, user group y) keeps the tile's rows of A and Qg
// and the weights from layer 2 in LDS and walks the users b = y, y + gridDim.y, ...
__global__ __launch_bounds__(256) void als_ncf_scores_kernel(
    const int32_t *__restrict__ users, int B, int n_users, int lo, int hi, const float *__restrict__ Pg, int ldpg,
    const float *__restrict__ Qg, int ldqg, const float *__restrict__ A, const float *__restrict__ UH,
    const float *__restrict__ theta, const NcfDims D, float *__restrict__ out, int64_t ld) {
  extern __shared__ float ncf_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int dg = D.dg, L = D.L, d1 = D.d[1], d2 = D.d[2], d3 = D.d[3], dL = D.d[L];
  const int dmax = max(d1, max(d2, d3));
  const int i0 = lo + blockIdx.x * NCF_TILE;
  float *p = ncf_lds;
  float *W2 = p; p += L >= 2 ? d2 * (d1 + 1) : 0;
  float *W3 = p; p += L >= 3 ? d3 * (d2 + 1) : 0;
  float *c2 = p; p += d2;
  float *c3 = p; p += d3;
  float *w = p; p += dg + dL;
  float *b0 = p; p += 1;
  float *At = p; p += NCF_TILE * (d1 + 1);
  float *Qt = p; p += NCF_TILE * (dg + 1);
  float *buf0 = p; p += NCF_TILE * (dmax + 1);
  float *buf1 = p; p += NCF_TILE * (dmax + 1);
  float *uh = p; p += d1;
  float *pw = p;
  if (L >= 2) ncf_stage(theta + D.woff[2], d2, d1, W2, tid);
  if (L >= 3) ncf_stage(theta + D.woff[3], d3, d2, W3, tid);
  for (int x = tid; x < d2; x += 256) c2[x] = theta[D.coff[2] + x];
  for (int x = tid; x < d3; x += 256) c3[x] = theta[D.coff[3] + x];
  for (int x = tid; x < dg + dL; x += 256) w[x] = theta[D.w_off + x];
  if (tid == 0) b0[0] = theta[D.b0_off];
  for (int x = tid; x < NCF_TILE * d1; x += 256) {
    const int r = x / d1, j = x - r * d1;
    At[r * (d1 + 1) + j] = i0 + r < hi ? A[(int64_t)(i0 + r) * d1 + j] : 0.f;
  }
  for (int x = tid; x < NCF_TILE * dg; x += 256) {
    const int r = x / dg, k = x - r * dg;
    Qt[r * (dg + 1) + k] = i0 + r < hi ? Qg[(int64_t)(i0 + r) * ldqg + k] : 0.f;
  }
  float *last = L == 2 ? buf1 : buf0;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int u = users[b];
    const bool ok = u >= 0 && u < n_users;
    __syncthreads();                                // (the last user's readers are done; the first: the tile is staged)
    for (int x = tid; x < d1; x += 256) uh[x] = UH[(int64_t)b * d1 + x];
    for (int x = tid; x < dg; x += 256) pw[x] = ok ? Pg[(int64_t)u * ldpg + x] * w[x] : 0.f;
    __syncthreads();
    for (int x = tid; x < NCF_TILE * d1; x += 256) {
      const int r = x / d1, j = x - r * d1;
      buf0[r * (d1 + 1) + j] = fmaxf(uh[j] + At[r * (d1 + 1) + j], 0.f);
    }
    __syncthreads();
    if (L >= 2) {
      ncf_layer([&](int r, int k) { return buf0[r * (d1 + 1) + k]; }, d1, W2, c2, d2, buf1, wv, lane);
      __syncthreads();
    }
    if (L >= 3) {
      ncf_layer([&](int r, int k) { return buf1[r * (d2 + 1) + k]; }, d2, W3, c3, d3, buf0, wv, lane);
      __syncthreads();
    }
    const int r = tid >> 3, s = tid & 7;
    float z = 0.f;
    for (int k = s; k < dg; k += 8) z = fmaf(pw[k], Qt[r * (dg + 1) + k], z);
    for (int j = s; j < dL; j += 8) z = fmaf(w[dg + j], last[r * (dL + 1) + j], z);
    z += __shfl_xor(z, 4, 64);
    z += __shfl_xor(z, 2, 64);
    z += __shfl_xor(z, 1, 64);
    if (s == 0 && i0 + r < hi) out[(int64_t)b * ld + (i0 + r - lo)] = ok ? z + b0[0] : 0.f;
  }
}

// both LDS kernels may ask for more than the 64 KB a launch gets by default: raised once, to the most a launch uses
int ncf_lds_attributes() {
  static const int rc = [] {
    const hipError_t a = hipFuncSetAttribute((const void *)als_ncf_step_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)NCF_LDS_LIMIT);
    const hipError_t b = hipFuncSetAttribute((const void *)als_ncf_scores_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)NCF_LDS_LIMIT);
    return a == hipSuccess && b == hipSuccess ? 0 : -1;
  }();
  return rc;
}

}  // namespace

#define NCF_DIMS_MSG "1 <= L <= 3; dg, dm and d_1 .. d_L multiples of 4 in [4, 128]; the layers must fit the LDS"

extern "C" int64_t rk_als_ncf_dense_count(int32_t dg, int32_t dm, int32_t L, int32_t d1, int32_t d2, int32_t d3) {
  NcfDims D;
  return ncf_dims(dg, dm, L, d1, d2, d3, D) ? D.n : -2;
}

extern "C" int64_t rk_als_ncf_lds_bytes(int32_t dg, int32_t dm, int32_t L, int32_t d1, int32_t d2, int32_t d3,
                                        int32_t scores) {
  NcfDims D;
  if (!ncf_dims(dg, dm, L, d1, d2, d3, D)) return -2;
  return 4 * (scores ? ncf_scores_lds_floats(D) : ncf_step_lds_floats(D));
}

extern "C" int64_t rk_als_ncf_workspace_bytes(int32_t T, int32_t R, int32_t dg, int32_t dm, int32_t L, int32_t d1,
                                              int32_t d2, int32_t d3) {
  NcfDims D;
  if (!ncf_dims(dg, dm, L, d1, d2, d3, D)) return -2;
  if (T < 1 || T > RK_ALS_CCL_MAX_BATCH || R < 1 || R > RK_ALS_CCL_MAX_NEGATIVES) return -2;
  const int64_t n = (int64_t)T * (1 + R);
  if (n > RK_ALS_CCL_MAX_ENTRIES) return -2;
  const int64_t tiles = (n + NCF_TILE - 1) / NCF_TILE;
  return 2 * round256(4 * n) + 2 * round256(4 * n * (dg + dm)) + round256(4 * tiles * (D.n + 1)) + round256(4);
}

static int ncf_fit_dims(int32_t dg, int32_t dm, int32_t L, int32_t d1, int32_t d2, int32_t d3, NcfDims &D) {
  if (!ncf_dims(dg, dm, L, d1, d2, d3, D)) return -2;
  if (4 * ncf_step_lds_floats(D) > NCF_LDS_LIMIT || 4 * ncf_scores_lds_floats(D) > NCF_LDS_LIMIT) return -2;
  return 0;
}

extern "C" int rk_als_ncf_step(const int32_t *users, const int32_t *pos, int32_t T, int32_t R, int64_t seed,
                               int32_t step, int32_t n_users, int32_t n_items, const float *Pg, int32_t ldpg,
                               const float *Qg, int32_t ldqg, const float *Pm, int32_t ldpm, const float *Qm,
                               int32_t ldqm, const float *theta, int32_t dg, int32_t dm, int32_t L, int32_t d1,
                               int32_t d2, int32_t d3, int32_t *ukey, int32_t *ikey, float *GU, float *GI,
                               float *slabs, void *stream) {
  NcfDims D;
  RK_SIDE_REQUIRE(ncf_fit_dims(dg, dm, L, d1, d2, d3, D) == 0, NCF_DIMS_MSG);
  RK_SIDE_REQUIRE(rk_als_ncf_workspace_bytes(T, R, dg, dm, L, d1, d2, d3) > 0,
                  "1 <= T <= 4096, 1 <= R <= 1024, T (1 + R) <= 2^22");
  RK_SIDE_REQUIRE(n_users >= 1 && n_items >= 1 && step >= 0, "n_users, n_items >= 1, step >= 0");
  RK_SIDE_REQUIRE(ldpg >= dg && ldqg >= dg && ldpm >= dm && ldqm >= dm, "ldpg, ldqg >= dg; ldpm, ldqm >= dm");
  RK_SIDE_REQUIRE(users && pos && Pg && Qg && Pm && Qm && theta && ukey && ikey && GU && GI && slabs, "null pointer");
  RK_SIDE_REQUIRE(ncf_lds_attributes() == 0, "the LDS attribute could not be set");
  const int tiles = (T * (1 + R) + NCF_TILE - 1) / NCF_TILE;
  hipLaunchKernelGGL(als_ncf_step_kernel, dim3((unsigned)tiles), dim3(256), (size_t)(4 * ncf_step_lds_floats(D)),
                     (hipStream_t)stream, users, pos, T, R, mix64((uint64_t)seed), (uint32_t)step, n_users, n_items, Pg,
                     ldpg, Qg, ldqg, Pm, ldpm, Qm, ldqm, theta, D, ukey, ikey, GU, GI, slabs);
  RK_SIDE_CHECK_LAUNCH("als_ncf_step");
  return 0;
}

extern "C" int rk_als_ncf_dense_adam(float *theta, float *M, float *V, const float *slabs, int32_t tiles,
                                     int32_t entries, int32_t dg, int32_t dm, int32_t L, int32_t d1, int32_t d2,
                                     int32_t d3, float lr, float reg, float beta1, float beta2, float eps, int32_t t,
                                     float *loss, void *stream) {
  NcfDims D;
  RK_SIDE_REQUIRE(ncf_fit_dims(dg, dm, L, d1, d2, d3, D) == 0, NCF_DIMS_MSG);
  RK_SIDE_REQUIRE(entries >= 1 && entries <= RK_ALS_CCL_MAX_ENTRIES && tiles == (entries + NCF_TILE - 1) / NCF_TILE,
                  "1 <= entries <= 2^22, tiles = ceil(entries / 32)");
  RK_SIDE_REQUIRE(t >= 1 && reg >= 0.f && reg < INFINITY, "t >= 1, reg finite and >= 0");
  RK_SIDE_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f,
                  "0 <= beta1, beta2 < 1, eps > 0");
  RK_SIDE_REQUIRE(theta && M && V && slabs && loss, "null pointer");
  const float step = (float)((double)lr / (1.0 - pow((double)beta1, (double)t)));
  const float isb2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)t)));
  hipLaunchKernelGGL(als_ncf_dense_adam_kernel, dim3((unsigned)((D.n + 1 + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, theta, M, V, slabs, tiles, D, 1.f / (float)entries, reg, beta1, beta2,
                     1.f - beta1, 1.f - beta2, eps, step, isb2, loss);
  RK_SIDE_CHECK_LAUNCH("als_ncf_dense_adam");
  return 0;
}

extern "C" int rk_als_ncf_item_part(const float *Qm, int32_t ldqm, int32_t n_items, const float *theta, int32_t dm,
                                    int32_t d1, float *A, void *stream) {
  RK_SIDE_REQUIRE(ncf_width(dm) && ncf_width(d1) && ldqm >= dm, "dm, d1 multiples of 4 in [4, 128], ldqm >= dm");
  RK_SIDE_REQUIRE(n_items >= 1, "n_items >= 1");
  RK_SIDE_REQUIRE(Qm && theta && A, "null pointer");
  const int64_t n = (int64_t)n_items * d1;
  hipLaunchKernelGGL(als_ncf_item_part_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Qm,
                     ldqm, n_items, theta, dm, d1, A);
  RK_SIDE_CHECK_LAUNCH("als_ncf_item_part");
  return 0;
}

extern "C" int rk_als_ncf_scores(const int32_t *users, int32_t B, int32_t n_users, int32_t lo, int32_t hi,
                                 int32_t n_items, const float *Pg, int32_t ldpg, const float *Qg, int32_t ldqg,
                                 const float *Pm, int32_t ldpm, const float *A, const float *theta, int32_t dg,
                                 int32_t dm, int32_t L, int32_t d1, int32_t d2, int32_t d3, float *UH, float *out,
                                 int64_t ld, void *stream) {
  NcfDims D;
  RK_SIDE_REQUIRE(ncf_fit_dims(dg, dm, L, d1, d2, d3, D) == 0, NCF_DIMS_MSG);
  RK_SIDE_REQUIRE(B >= 1 && B <= (1 << 20) && n_users >= 1, "1 <= B <= 2^20, n_users >= 1");
  RK_SIDE_REQUIRE(lo >= 0 && hi > lo && hi <= n_items && ld >= hi - lo, "0 <= lo < hi <= n_items, ld >= hi - lo");
  RK_SIDE_REQUIRE(ldpg >= dg && ldqg >= dg && ldpm >= dm, "ldpg, ldqg >= dg; ldpm >= dm");
  RK_SIDE_REQUIRE(users && Pg && Qg && Pm && A && theta && UH && out, "null pointer");
  RK_SIDE_REQUIRE(ncf_lds_attributes() == 0, "the LDS attribute could not be set");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(als_ncf_user_part_kernel, dim3((unsigned)((B * d1 + 255) / 256)), dim3(256), 0, st, users, B,
                     n_users, Pm, ldpm, theta + D.woff[1], theta + D.coff[1], dm, d1, UH);
  const dim3 grid((unsigned)((hi - lo + NCF_TILE - 1) / NCF_TILE), (unsigned)std::min(B, NCF_SCORE_GY));
  hipLaunchKernelGGL(als_ncf_scores_kernel, grid, dim3(256), (size_t)(4 * ncf_scores_lds_floats(D)), st, users, B,
                     n_users, lo, hi, Pg, ldpg, Qg, ldqg, A, UH, theta, D, out, ld);
  RK_SIDE_CHECK_LAUNCH("als_ncf_scores");
  return 0;
}
