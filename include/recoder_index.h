/*
 * recoder_index.h -- C ABI of librecoder_index.so (MI355X / gfx950 only).
 *
 * The item-embedding side of the reference's public API (recoder/embedding.py, the
 * SimilarityRecommender of recoder/recommender.py): exact cosine similarity over an item table.
 * A library of its own, beside librecoder_hip.so, so that the training library's boundary keeps
 * its symbol set; the Python binding is recoder_amd/_index_lib.py.  Selection is not part of
 * this library: the caller ranks the score strips with rk_topk_masked of librecoder_hip.so.
 *
 * Conventions (those of recoder_hip.h)
 *   - every function returns 0 on success, <0 on error; rk_ix_last_error() gives a
 *     thread-local message.
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is retained past the call.
 *   - every launch goes on the caller's hipStream_t (passed as void*); no call synchronises
 *     the host; no call allocates.
 *   - matrices are row-major fp32 with an explicit leading dimension (in elements).
 *
 * Numerics.  Every dot product of this library is ONE f32 chain: acc = +0, then
 * acc = fmaf(a[k], b[k], acc) for k = 0, 1, ..., h-1 (the f32-input MFMA computes exactly that
 * chain).  A score therefore does not depend on the tile, the batch position or the strip it is
 * computed in, and rk_ix_pool_scores reproduces rk_ix_scores bit for bit.
 */
#ifndef RECODER_INDEX_H
#define RECODER_INDEX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* (the library is built with -fvisibility=hidden: what this header declares is what it exports) */
#pragma GCC visibility push(default)

int rk_ix_version(void);
const char *rk_ix_last_error(void);

/*
 * Y[r, :] = X[r, :] / ||X[r, :]||_2 for r < rows (X: [rows, ldx], Y: [rows, ldy], ld >= h; X == Y
 * allowed when ldx == ldy).  The sum of squares is taken in f32 in an order fixed by h alone, so the
 * output is a pure function of the row: a table row and the same vector passed as a query come out
 * bitwise equal.  A zero row stays zero (cosine 0 against everything, itself included).
 */
int rk_ix_normalize(const float *X, int32_t rows, int32_t h, int32_t ldx, float *Y, int32_t ldy,
                    void *stream);

/*
 * out[q, c] = sum_k Qn[q, k] * En[lo + c, k] for q < Q, c < hi - lo (the k-ascending f32 chain).
 * Qn: [Q, ldq], En: [>= hi, lde], out: [Q, ldo] with ldo >= hi - lo.  Any h >= 1, any Q >= 0.
 */
int rk_ix_scores(const float *Qn, int32_t Q, int32_t ldq, const float *En, int32_t lde, int32_t h,
                 int32_t lo, int32_t hi, float *out, int32_t ldo, void *stream);

/*
 * The SimilarityRecommender's scores (reference recommender.py, Aiolli 2013) for U users:
 *   out[u, j] = sum over t in hist(u), ascending, of ((cos(pool[u, j], t) + 1) / 2) ^ scale
 * for j < pool_cnt[u], and -inf for pool_cnt[u] <= j < pool_ld.  En: the NORMALISED table
 * [rows, lde]; hist_ptr [U + 1] / hist_idx: the histories as CSR (row indices of En); pool_idx
 * [U, pool_ld], pool_cnt [U]: the padded pools (row indices of En); out [U, pool_ld].  cos is the
 * chain of rk_ix_scores, so a one-item history at scale 1 gives bitwise (s + 1) / 2 of its s.  An
 * integral scale in [0, 64] is applied by repeated multiplication, any other value with powf.
 */
int rk_ix_pool_scores(const float *En, int32_t lde, int32_t h, const int64_t *hist_ptr,
                      const int64_t *hist_idx, int32_t U, const int64_t *pool_idx,
                      const int64_t *pool_cnt, int32_t pool_ld, float scale, float *out, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif /* RECODER_INDEX_H */
