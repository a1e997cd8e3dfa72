#pragma once
#include "foldin.h"
#include "../side_explain.h"

namespace {

// --------------------------------------------------------------------- explanations
// rk_als_explain: per-entry contributions to the folded-in user's score of J targets.  The workgroup and the group of
// TPR threads a row are rk_als_foldin's; A_u and its factor come from the same fi_form_factor, the solves from the
// same fi_solve, so z below is what rk_als_foldin would return for the right-hand side y_j.  A group's LDS is the
// fold-in's, then XP_LDS_WORDS words of selection slots.  Every barrier is reached by the whole workgroup: all rows
// have J targets, and what differs between rows (the entry loops, the selection) holds no barrier.
//
// Per target j of a row, in order (f32, fused operations written as fmaf):
//   z         thread k < h starts from y_j[k]; fi_solve
//   baseline  d = fmaf(z[k], v[k], d) over k ascending from +0;  baseline = b_j - d   (b_j = +0 without a bias)
//   c_e       d = fmaf(z[k], y_e[k], d) over k ascending from +0;  c_e = coef_e * d, coef_e = fi_coef's
//   total     t = baseline; t = t + c_e over the entries in CSR order
//   the m best c_e by side_explain.h's order, taken by the group's first wave from the workspace, where c lies at its
//   entry's own index
// A row with a pivot that is not positive: status 1, every c_e = +0, baseline = total = +0.
template <int TPR, int TB>
__global__ __launch_bounds__(256) void als_explain_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const float *__restrict__ data, int rows,
    const float *__restrict__ Y, int ldy, int n_items, int h, const float *__restrict__ G,
    const float *__restrict__ v, const float *__restrict__ bias, float alpha, const int64_t *__restrict__ items, int J,
    int m, float *ws, int64_t *__restrict__ contributors, float *__restrict__ contributions,
    float *__restrict__ baseline, float *__restrict__ total, int32_t *__restrict__ status, int gfloats) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float fi_lds[];
  const int g = threadIdx.x / TPR, t = threadIdx.x % TPR;
  const int hp = (h + TB - 1) / TB * TB;
  float *base = fi_lds + (int64_t)g * gfloats;
  const FiLds L = fi_lds_of(base, hp);
  float *sv = base + gfloats - XP_LDS_WORDS;
  int *sp = (int *)(sv + 128);
  const int64_t row = (int64_t)blockIdx.x * (256 / TPR) + g;
  float r;
  bool live;
  int64_t e0;
  int n;
  const bool bad = fi_form_factor<TPR, TB>(L, indptr, indices, data, rows, Y, ldy, h, G, v, bias, alpha, g, t, r, live,
                                           e0, n);
  if (live && t == 0) status[row] = bad ? 1 : 0;

  for (int q = 0; q < J; ++q) {
    int64_t j = -1;
    if (live) {
      j = items[row * J + q];
      if (j >= n_items) j = -1;
    }
    const bool real = j >= 0, act = real && !bad;
    float z = (act && t < h) ? Y[j * ldy + t] : 0.f;
    fi_solve(L, h, t, !act, z);
    if (real)
      for (int e = t; e < n; e += TPR) {
        float c = 0.f;
        if (act) {
          const int col = indices[e0 + e];
          float a;
          const float cf = fi_coef(entry_value(data, e0 + e), alpha, bias ? bias[col] : 0.f, a);
          const float *y = Y + (int64_t)col * ldy;
          float d = 0.f;
          for (int k = 0; k < h; ++k) d = fmaf(L.zs[k], y[k], d);
          c = cf * d;
        }
        ws[e0 + e] = c;
      }
    __syncthreads();
    if (live && t < 64) {                           // (the group's first wave, whole)
      float b0 = 0.f;
      if (act) {
        float d = 0.f;
        for (int k = 0; k < h; ++k) d = fmaf(L.zs[k], v[k], d);
        b0 = (bias ? bias[j] : 0.f) - d;
      }
      float tot = b0;
      xp_init(sv, sp, t);
      const int len = real ? n : 0;
      for (int c0 = 0; c0 < len; c0 += 64) {
        const int cnt = min(64, len - c0);
        const float c = t < cnt ? ws[e0 + c0 + t] : 0.f;
        tot = xp_chain_add(tot, c, cnt);
        xp_merge(sv, sp, t, c, t < cnt ? c0 + t : -1);
      }
      const int64_t pair = row * J + q;
      xp_write(sv, sp, t, m, indices + e0, contributors + pair * m, contributions + pair * m);
      if (t == 0) {
        baseline[pair] = b0;
        total[pair] = tot;
      }
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int64_t rk_als_explain_workspace_bytes(int64_t nnz) {
  if (nnz < 0) {
    rk_side_set_error("%s: nnz must be >= 0", __func__);
    return -2;
  }
  return ((nnz > 0 ? nnz : 1) * 4 + 255) & ~(int64_t)255;
}

extern "C" int rk_als_explain(const int64_t *indptr, const int32_t *indices, const float *data, int32_t rows,
                              int64_t nnz, const float *Y, int32_t ldy, int32_t n_items, int32_t h, const float *G,
                              const float *v, const float *bias, float alpha, const int64_t *items, int32_t J, int32_t m,
                              int64_t *contributors, float *contributions, float *baseline, float *total,
                              int32_t *status, void *ws, int64_t ws_bytes, void *stream) {
  RK_SIDE_REQUIRE(h >= 1 && h <= FI_MAX_H && ldy >= h, "1 <= h <= 128, ldy >= h");
  RK_SIDE_REQUIRE(rows >= 0 && n_items >= 1 && nnz >= 0, "rows >= 0, n_items >= 1, nnz >= 0");
  RK_SIDE_REQUIRE(alpha >= 0.f && alpha <= FLT_MAX, "alpha must be finite and >= 0");
  RK_SIDE_REQUIRE(J >= 1 && m >= 1 && m <= XP_MAX_M, "J >= 1, 1 <= m <= 64");
  RK_SIDE_REQUIRE(ws_bytes >= rk_als_explain_workspace_bytes(nnz), "workspace too small");
  if (rows == 0) return 0;
  RK_SIDE_REQUIRE(indptr && indices && Y && G && v && items && contributors && contributions && baseline && total &&
                  status && ws, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto kernel, int tpr, int tb) {
    const int per = 256 / tpr, gfloats = fi_group_floats(h, tb) + XP_LDS_WORDS;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(256),
                       (size_t)per * gfloats * sizeof(float), st, indptr, indices, data, rows, Y, ldy, n_items, h, G, v,
                       bias, alpha, items, J, m, (float *)ws, contributors, contributions, baseline, total, status,
                       gfloats);
  };
  if (h <= 32) launch(als_explain_kernel<64, 4>, 64, 4);
  else if (h <= 64) launch(als_explain_kernel<64, 8>, 64, 8);
  else launch(als_explain_kernel<256, 8>, 256, 8);
  RK_SIDE_CHECK_LAUNCH("als_explain");
  return 0;
}
