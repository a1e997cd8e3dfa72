// The stochastic bottleneck of the variational autoencoder (include/recoder_vae.h, librecoder_vae.so).
//
//   rk_vae_sample      z = mu + eps * exp(0.5 lv) (or z = mu), eps injected or from the counter RNG,
//                      the row's beta * KL into its own loss partial
//   rk_vae_sample_bwd  dE = [dz + beta inv mu | 0.5 (dz eps sigma + beta inv (exp(lv) - 1))]
//
// Both are elementwise passes over 2 B d floats (200 k at B = 500, d = 200): their cost is the launch.
// One wave per row, 4 rows per workgroup; lane l takes columns l, l + 64, ...  The float operations of
// a row are spelled the same way in both kernels (sigma = expf(0.5f * lv), ev = expf(lv)), with the
// same code in eager and replayed steps, so a row's outputs depend on its own inputs alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "../../include/recoder_vae.h"
#include "side_error.h"

namespace {

constexpr int ROWS_PER_WG = 4;        // one wave per row

// eps of (user, column) at RNG step `step`: Box-Muller on two 24-bit uniforms of one 64-bit draw
__device__ __forceinline__ float vae_normal(uint64_t seed, uint64_t step, uint64_t uid, uint64_t col) {
  uint64_t k = rk_mix64((seed ^ RK_VAE_SEED_XOR) + 0x9e3779b97f4a7c15ULL * (step + 1));
  k = rk_mix64(k ^ (uid * 0xd1342543de82ef95ULL + col + 0x632be59bd9b4e019ULL));
  const float u1 = (float)((k >> 40) + 1) * (1.0f / 16777216.0f);          // (0, 1]
  const float u2 = (float)((k >> 16) & 0xffffffULL) * (1.0f / 16777216.0f); // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

__device__ __forceinline__ float vae_beta(const rk_cur_t &cur, const float *beta_table, float beta) {
  return (cur.cursor && beta_table) ? beta_table[rk_cur_local(cur)] : beta;
}

__global__ __launch_bounds__(256) void vae_sample_kernel(const float *__restrict__ E, int B, int d, int train,
                                                         const float *__restrict__ eps_in, uint64_t seed,
                                                         uint64_t rng_step, const int64_t *__restrict__ users,
                                                         int row_off, rk_cur_t cur, const float *beta_table,
                                                         float beta, float *__restrict__ z,
                                                         float *__restrict__ eps_out, float *__restrict__ kl_part) {
  const int r = (int)blockIdx.x * ROWS_PER_WG + ((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  if (r >= B) return;                  // (whole waves: the shuffle tree below stays inside one row)
  if (cur.cursor) {
    rng_step = (uint64_t)(rk_cur_global(cur) + 1);
    if (users) users += rk_cur_local(cur) * B;     // (replayed steps are whole batches)
  }
  const float b = vae_beta(cur, beta_table, beta);
  const uint64_t uid = users ? (uint64_t)users[row_off + r] : (uint64_t)(row_off + r);
  const float *e = E + (int64_t)r * 2 * d;
  float kl = 0.f;
  for (int j = lane; j < d; j += 64) {
    const float mu = e[j], lv = e[d + j];
    const int64_t o = (int64_t)r * d + j;
    if (train) {
      const float ep = eps_in ? eps_in[o] : vae_normal(seed, rng_step, uid, (uint64_t)j);
      const float sigma = expf(0.5f * lv);
      z[o] = fmaf(ep, sigma, mu);
      if (eps_out) eps_out[o] = ep;
    } else {
      z[o] = mu;
    }
    if (kl_part) {
      const float ev = expf(lv);
      kl += fmaf(mu, mu, ev - 1.0f) - lv;
    }
  }
  if (kl_part) {
    kl = rk_wave_sum(kl);
    if (lane == 0) kl_part[r] = b * (0.5f * kl);
  }
}

__global__ __launch_bounds__(256) void vae_sample_bwd_kernel(const float *__restrict__ E,
                                                             const float *__restrict__ eps,
                                                             const float *__restrict__ dz, int B, int d, float inv,
                                                             rk_cur_t cur, const float *beta_table, float beta,
                                                             float *__restrict__ dE) {
  const int r = (int)blockIdx.x * ROWS_PER_WG + ((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  if (r >= B) return;
  const float bi = vae_beta(cur, beta_table, beta) * inv;
  const float *e = E + (int64_t)r * 2 * d;
  float *de = dE + (int64_t)r * 2 * d;
  for (int j = lane; j < d; j += 64) {
    const float mu = e[j], lv = e[d + j];
    const int64_t o = (int64_t)r * d + j;
    const float g = dz[o];
    const float sigma = expf(0.5f * lv);
    const float ev = expf(lv);
    de[j] = fmaf(bi, mu, g);
    de[d + j] = 0.5f * fmaf(g * eps[o], sigma, bi * (ev - 1.0f));
  }
}

}  // namespace

extern "C" int rk_vae_version(void) { return 100; }

extern "C" const char *rk_vae_last_error(void) { return g_rk_side_err; }

extern "C" int rk_vae_sample(const float *E, int32_t B, int32_t d, int32_t train, const float *eps_in, uint64_t seed,
                             uint64_t rng_step, const int64_t *users, int32_t row_off, const int64_t *cursor,
                             int32_t cursor_off, const float *beta_table, float beta, float *z, float *eps_out,
                             float *kl_part, void *stream_) {
  RK_SIDE_REQUIRE(B >= 0 && d >= 1 && row_off >= 0, "B >= 0, d >= 1 and row_off >= 0");
  RK_SIDE_REQUIRE(E != nullptr && z != nullptr, "E and z are required");
  RK_SIDE_REQUIRE(!train || eps_out != nullptr, "training mode needs eps_out (the backward reads it)");
  if (B == 0) return 0;
  const rk_cur_t cur = {cursor, cursor_off};
  hipLaunchKernelGGL(vae_sample_kernel, dim3(rk_cdiv(B, ROWS_PER_WG)), dim3(64 * ROWS_PER_WG), 0,
                     (hipStream_t)stream_, E, B, d, train, eps_in, seed, rng_step, users, row_off, cur, beta_table,
                     beta, z, eps_out, kl_part);
  RK_SIDE_CHECK_LAUNCH("vae_sample");
  return 0;
}

extern "C" int rk_vae_sample_bwd(const float *E, const float *eps, const float *dz, int32_t B, int32_t d, float inv,
                                 const int64_t *cursor, int32_t cursor_off, const float *beta_table, float beta,
                                 float *dE, void *stream_) {
  RK_SIDE_REQUIRE(B >= 0 && d >= 1, "B >= 0 and d >= 1");
  RK_SIDE_REQUIRE(E != nullptr && eps != nullptr && dz != nullptr && dE != nullptr, "E, eps, dz and dE are required");
  if (B == 0) return 0;
  const rk_cur_t cur = {cursor, cursor_off};
  hipLaunchKernelGGL(vae_sample_bwd_kernel, dim3(rk_cdiv(B, ROWS_PER_WG)), dim3(64 * ROWS_PER_WG), 0,
                     (hipStream_t)stream_, E, eps, dz, B, d, inv, cur, beta_table, beta, dE);
  RK_SIDE_CHECK_LAUNCH("vae_sample_bwd");
  return 0;
}
