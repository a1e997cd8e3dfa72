/*
 * recoder_vae.h -- C ABI of librecoder_vae.so (MI355X / gfx950 only).
 *
 * The stochastic bottleneck of the variational autoencoder for collaborative filtering (Liang et al.
 * 2018, Mult-VAE; recoder_amd.nn.VariationalAutoencoder).  The encoder's last Linear (no activation)
 * gives E = [mu | logvar] ([B, 2d], mu in columns 0..d-1, logvar in columns d..2d-1); the decoder
 * reads z [B, d]:
 *   training:   z = mu + eps * exp(0.5 logvar),  eps ~ N(0, 1)
 *   evaluation: z = mu
 * and the step's loss gains beta * KL_u / rows per user, KL_u = 0.5 sum_j (exp(lv_j) + mu_j^2 - 1 - lv_j).
 * A library of its own, beside librecoder_hip.so, librecoder_index.so and librecoder_als.so, so that none
 * of their symbol sets changes; the Python binding is recoder_amd/_vae_lib.py, the sequencing
 * recoder_amd/engine.py (FusedEngine._vae_sample / the entry-by-entry step).
 *
 * Conventions (those of recoder_hip.h)
 *   - every function returns 0 on success, <0 on error; rk_vae_last_error() gives a thread-local message.
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is retained past the call.
 *   - every launch goes on the caller's hipStream_t (passed as void*); no call synchronises the host;
 *     no call allocates.
 *   - row-major fp32, rows contiguous: E [B, 2d], z / eps / dz [B, d], dE [B, 2d].
 *
 * Graph replay (recoder_amd/graph.py).  cursor (nullable) is the step cursor of csrc/common.h rk_cur_t:
 * cursor[0] = global index of the step group's first step, cursor[1] = that of the epoch's first step,
 * cursor_off = the step's position in the group.  With a cursor the kernels take
 *   rng_step = cursor[0] + cursor_off + 1,  users += (cursor[0] - cursor[1] + cursor_off) * B,
 *   beta = beta_table[cursor[0] - cursor[1] + cursor_off]   (when beta_table is not NULL)
 * and ignore the host-given rng_step / beta -- as rk_dropout does.  cursor == NULL: the host values.
 *
 * Numerics.  One wave per row; a row's outputs depend only on that row's inputs (and its user id /
 * the step for the counter RNG), so they are bitwise the same whatever the row's position or the
 * batch size, eager or replayed.  The per-row KL sum runs in a fixed order (lane strides, then a
 * fixed shuffle tree).  logvar is NOT clamped (as in the paper): exp(lv) overflows to +inf for
 * lv > ~88.7 (the KL partial and the loss become +inf), exp(0.5 lv) for lv > ~177 (z becomes +inf or
 * NaN); the gradients then carry inf / NaN into the Adam update and Recoder.train warns on the
 * non-finite loss.  Nothing is clipped or replaced.
 *
 * Counter RNG (eps == NULL in training mode): Box-Muller on two 24-bit uniforms of one rk_mix64 draw
 * keyed on (seed ^ RK_VAE_SEED_XOR, rng_step, user id, column): u1 in (0, 1] (log finite),
 * u2 in [0, 1), eps = sqrt(-2 log u1) cos(2 pi u2).
 */
#ifndef RECODER_VAE_H
#define RECODER_VAE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* (the library is built with -fvisibility=hidden: what this header declares is what it exports) */
#pragma GCC visibility push(default)

#define RK_VAE_SEED_XOR 0x7ae5a3c1b2d4e6f8ULL

int rk_vae_version(void);
const char *rk_vae_last_error(void);

/*
 * z = mu + eps * exp(0.5 lv) (train != 0) or z = mu (train == 0) for rows [0, B) of E.
 *   eps_in   [B, d] nullable: injected eps (parity tests); NULL: the counter RNG
 *   users    [>= row_off + B] int64 nullable: row r's user id is users[row_off + r] (NULL: row_off + r)
 *   eps_out  [B, d] nullable (training: required): the eps used, for rk_vae_sample_bwd
 *   kl_part  [B] nullable: kl_part[r] = beta * KL_r (unscaled: the loss reduction divides by rows), in
 *            eval mode too (validation loss).  Overwritten, not accumulated.
 * d >= 1, B >= 0.
 */
int rk_vae_sample(const float *E, int32_t B, int32_t d, int32_t train, const float *eps_in, uint64_t seed,
                  uint64_t rng_step, const int64_t *users, int32_t row_off, const int64_t *cursor,
                  int32_t cursor_off, const float *beta_table, float beta, float *z, float *eps_out,
                  float *kl_part, void *stream);

/*
 * dE [B, 2d] from dz [B, d] (the gradient at the decoder input, already 1/rows-scaled), E and the eps
 * rk_vae_sample used; inv = 1 / rows (fp32), sigma = exp(0.5 lv):
 *   dmu = dz + beta inv mu
 *   dlv = 0.5 (dz eps sigma + beta inv (exp(lv) - 1))
 * cursor / cursor_off / beta_table as rk_vae_sample (beta must be the forward's).
 */
int rk_vae_sample_bwd(const float *E, const float *eps, const float *dz, int32_t B, int32_t d, float inv,
                      const int64_t *cursor, int32_t cursor_off, const float *beta_table, float beta, float *dE,
                      void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif /* RECODER_VAE_H */
