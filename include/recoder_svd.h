/*
 * recoder_svd.h -- C ABI of librecoder_svd.so (MI355X / gfx950 only).
 *
 * The kernels of PureSVD (Cremonesi, Koren & Turrin 2010) for a MatrixFactorization: a randomized
 * truncated SVD of the user x item CSR A (Halko, Martinsson & Tropp 2011, algorithms 4.4 + 5.1):
 *   Q = orth(A Omega), Z = orth(A^T Q), q times (Q = orth(A Z), Z = orth(A^T Q)), W = A Z,
 *   T = W^T W = S diag(lambda) S^T on the host, V = Z S (items), U = W S = A V (users).
 * orth(Y) is Cholesky-QR, twice: G = Y^T Y (rk_als_gram of librecoder_als.so), R = chol(G), Y <- Y R^-1.
 * A library of its own, beside the other five, so that none of their symbol sets changes; the Python
 * binding is recoder_amd/_svd_lib.py, the driver recoder_amd/svd.py.
 *
 * Conventions (those of recoder_als.h)
 *   - every function returns 0 on success, <0 on error; rk_svd_last_error() gives a thread-local
 *     message.
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is retained past the call.
 *   - every launch goes on the caller's hipStream_t (passed as void*); no call synchronises the
 *     host; no call allocates (scratch comes from a workspace the caller sizes with the
 *     *_workspace_bytes query).
 *   - dense matrices are row-major fp32 with an explicit leading dimension (in elements).  CSR: int64
 *     indptr [rows + 1], int32 column indices, fp32 values (NULL: every value is 1.0).
 *
 * Numerics (f32 unless said otherwise; every call is bitwise repeatable; no atomics on data)
 *   - rk_svd_spmm: lane group g of an entry owns columns 4g .. 4g + 3; with P = the power of two at or
 *     above min(ceil(l / 4), 64), a wave takes E = 64 / P entries per step.  A piece of a row (the whole
 *     row below RK_SVD_LONG_ROW entries; one of 16 contiguous pieces, one per wave, at or above it) is
 *     E interleaved fmaf chains in entry order, added by a butterfly over the slots; the 16 pieces of a
 *     long row are added in wave order.  The order depends on the row's length and l alone: any
 *     [row_lo, row_hi) gives bitwise the rows of the full call, whatever the alignment of F and Y.
 *   - rk_svd_rotate: every output element is one k-ascending fmaf chain on v_mfma_f32_32x32x2_f32.
 *   - rk_svd_chol_inverse: float64 throughout, rounded to f32 once on the way out.
 */
#ifndef RECODER_SVD_H
#define RECODER_SVD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* (the library is built with -fvisibility=hidden: what this header declares is what it exports) */
#pragma GCC visibility push(default)

int rk_svd_version(void);
const char *rk_svd_last_error(void);

/* largest sketch width l = h + oversample the kernels take */
int rk_svd_max_l(void);

/* rows of this many stored entries or more take the 16-wave path of the sparse product */
#define RK_SVD_LONG_ROW 512

/*
 * out[r, c] (r < rows, c < l; leading dimension ld) = a standard normal from the counter RNG keyed on
 * (seed, r, c): Box-Muller on two 24-bit uniforms of one 64-bit draw.  The matrix does not depend on
 * the launch shape or on ld.
 */
int rk_svd_gaussian(float *out, int32_t rows, int32_t l, int32_t ld, uint64_t seed, void *stream);

/*
 * Y[r, :l] = sum_j a_rj F[col_j, :l] over the stored entries of CSR row r, for r in [row_lo, row_hi);
 * rows without entries give zeros.  F [> every column index, ldf], Y [>= row_hi, ldy], 1 <= l <=
 * the maximum.  16-byte loads and stores are used when l, ldf and ldy are multiples of 4 and both
 * pointers are 16-byte aligned; the result is bitwise the same either way.
 */
int rk_svd_spmm(const int64_t *indptr, const int32_t *indices, const float *data, int32_t row_lo, int32_t row_hi,
                const float *F, int32_t ldf, int32_t l, float *Y, int32_t ldy, void *stream);

/* bytes of workspace rk_svd_chol_inverse needs for an [l, l] matrix (>= 0; < 0 on bad arguments) */
int64_t rk_svd_chol_inverse_workspace_bytes(int32_t l);

/*
 * Rinv ([l, l] f32, leading dimension l, upper triangular, zeros below the diagonal) = R^-1 with
 * G = R^T R the Cholesky factorisation of the symmetric G ([l, l] f32, leading dimension l; its upper
 * triangle is read).  One workgroup, float64: the matrix lives in LDS when it fits, in the workspace
 * otherwise (16-byte aligned).  A pivot that is not finite, or not above l 2^-23 G[k][k] (in
 * particular one that is <= 0: below that share the f32 Gram cannot tell it from zero), is replaced by
 * 1 and reported: *status, if it is 0, becomes k + 1 (the first wins).  *status is never cleared here,
 * so one word collects the breakdowns of a whole sequence of calls.
 */
int rk_svd_chol_inverse(const float *G, int32_t l, float *Rinv, void *ws, int64_t ws_bytes, int32_t *status,
                        void *stream);

/*
 * Out[r, :l2] = Y[r, :l] M ([l, l2], leading dimension ldm), r < rows, out of place (Out must not
 * overlap Y), 1 <= l, l2 <= the maximum.  K = l is never split.
 */
int rk_svd_rotate(const float *Y, int32_t rows, int32_t l, int32_t ldy, const float *M, int32_t l2, int32_t ldm,
                  float *Out, int32_t ldo, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif /* RECODER_SVD_H */
