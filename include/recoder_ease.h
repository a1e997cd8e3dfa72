/*
 * recoder_ease.h -- C ABI of librecoder_ease.so (MI355X / gfx950 only).
 *
 * EASE (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", WWW 2019): a linear
 * item-item autoencoder with a zero diagonal and a closed-form solution.  For the user x item
 * matrix X (values as stored), reg > 0 and n items:
 *   G = X^T X                      [n, n]
 *   P = (G + reg I)^-1
 *   B[i][j] = -P[i][j] / P[j][j]   (i != j),   B[j][j] = 0
 *   scores(u, :) = X[u, :] . B
 * A library of its own, beside the training, index, ALS and VAE libraries, so that none of their
 * symbol sets changes; the Python binding is recoder_amd/_ease_lib.py, the driver recoder_amd/ease.py.
 *
 * Conventions (those of recoder_als.h)
 *   - every function returns 0 on success, <0 on error; rk_ease_last_error() gives a
 *     thread-local message.
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is retained past the call.
 *   - every launch goes on the caller's hipStream_t (passed as void*); no call synchronises
 *     the host; no call allocates (scratch comes from a workspace the caller sizes with the
 *     *_workspace_bytes query).
 *   - matrices are row-major fp32 with an explicit leading dimension (in elements).  CSR: int64
 *     indptr [rows + 1], int32 column indices ascending inside a row, fp32 values (NULL: every
 *     value is 1.0).
 *
 * Numerics (all f32 in memory; every call is bitwise repeatable, whatever the values)
 *   - rk_ease_gram: A[i][j] is ONE f32 fmaf chain  fma(x_ui, x_uj, .)  over the users u of item i in
 *     ascending order, from 0, then + reg on the diagonal.  No atomics: a column belongs to one
 *     wave, a wave takes the users one after the other.  x_ui x_uj == x_uj x_ui and the users of i
 *     that also hold j are the users of j that also hold i, so A[i][j] and A[j][i] are the same chain:
 *     bitwise symmetric.  Integer-valued interactions with every sum below 2^24 give the exact Gram.
 *   - rk_ease_spd_inverse: blocked Gauss-Jordan (the sweep operator) without pivoting, block width
 *     64, on the whole matrix (2 n^3 flop; the symmetry is not used).  The 64 x 64 pivot block is
 *     inverted in float64 and kept in float64 for the two panels (float64 fma chains, rounded to f32
 *     once); the rank-64 update is one k-ascending f32 chain on v_mfma_f32_32x32x2_f32 subtracted
 *     from the stored value with a compensated (Kahan) subtraction whose carries live in a second
 *     n x n image in the workspace and are folded in at the end: the many updates that are below half
 *     an ulp of a large diagonal are not lost.  The result is symmetric up to rounding, not bitwise.
 *   - rk_ease_finalize: one correctly rounded f32 divide per element.
 *   - rk_ease_scores: one ascending f32 fmaf chain per output, from 0, over the user's stored
 *     entries: a score depends neither on the strip nor on the user's position in the batch.
 *   - rk_ease_lowrank_add: dot = ONE k-ascending f32 fmaf chain  fma(V[i][t], V[j][t], .)  over t = 0 .. k - 1,
 *     from 0, on v_mfma_f32_32x32x2_f32 (k is never split over waves or workgroups, there are no atomics);
 *     then  s = alpha * row_scale[i],  p = s * dot  (two f32 multiplies, in this order) and
 *     A[i][j] = fma(p, col_scale[j], A[i][j]): three roundings after the chain's k.  An element depends on
 *     neither the tile it falls in nor the row range: a row range gives bitwise the rows of the full call.  A
 *     scale (or alpha) that is exactly 0 adds +-0: the element keeps its value.
 *   - rk_ease_gemm: dot = ONE k-ascending f32 fmaf chain  fma(A[i][t], B[t][j], .)  over t = 0 .. k - 1, from +0, on
 *     v_mfma_f32_32x32x2_f32 (k is never split over waves or workgroups, there are no atomics, no workspace); then
 *     p = alpha * dot (one f32 multiply) and  D[i][j] = p  (E NULL: beta is not read)  or  D[i][j] = fma(beta, E[i][j], p):
 *     one or two roundings after the chain's k.  An element depends on neither the tile it falls in nor the row
 *     range: a row range gives bitwise the rows of the full call.
 *   - rk_ease_admm_update, per element, every operation one f32 rounding in this order (fma: a fused multiply-add):
 *       gamma_j = (T[j][j] + 1) / P[j][j]             an add, then a correctly rounded divide
 *       B  = fma(-P[i][j], gamma_j, T[i][j])          fma (the negation is exact)
 *       V  = B + U[i][j]                              add
 *       w  = V - theta (nonneg)  or  |V| - theta      subtract
 *       Cn = w > 0 ? w : +0 (nonneg)  or  w > 0 ? copysign(w, V) : +0       (exact; theta = 0 gives Cn = V, or max(V, 0))
 *       Un = V - Cn,   Mn = Cn - Un                   two subtracts
 *     and on the diagonal B = Cn = Un = Mn = +0 whatever is stored.  The row statistics: d1 = B - Cn and
 *     d2 = Cn - C[i][j] (the value before the call) as f32 subtracts, their squares summed in float64 (fma chains:
 *     thread t of 256 takes the columns t, t + 256, ... ascending, then a pairwise tree over the threads), rounded
 *     once to f32; the count of Cn != 0 is exact.  No atomics: a fixed order, bitwise repeatable, and a row does
 *     not depend on the row range.
 *   - the ELSA calls (recoder_amd/elsa.py).  A "wave sum" of 64 float64 values is the butterfly s += s[lane ^ d] for
 *     d = 32, 16, 8, 4, 2, 1; a "row dot" <x, y> of two rows of h columns is: lane l of 64 takes the float64 fma chain of
 *     x[k] y[k] (exact products) over k = l, l + 64, .. ascending, from 0, then the wave sum of the 64 chains.
 *       rk_ease_elsa_normalize: ss = (float)(row dot <W_j, W_j>) (the float64 sum rounded once), norm_j = sqrt(ss)
 *         (correctly rounded f32), d = max(norm_j, 1e-12f), A[j][k] = W[j][k] / d (a correctly rounded f32 divide).  Against
 *         the exact value that is (1/2 + 1 + 1) 2^-24 relative: ss within 2^-24 (halved by the root), the root, the divide.
 *         A zero row gives norm 0 and a row of +-0.  At is a copy: bitwise the transpose of A.
 *       rk_ease_elsa_rows, all in float64: z2 = row dot <Z_u, Z_u>, q = row dot <Z_u, Q_u>, t = t2[u],
 *         p2 = (q - 2 z2) + t, live = t > 0 and 0 < p2 < inf; for a live row c = (z2 - t) / (sqrt(p2) sqrt(t)),
 *         a = -2 / (B n sqrt(p2) sqrt(t)), b = 2 c / (B n p2), E[u][k] = (float)fma(2 (a - b), Z[u][k], b Q[u][k]),
 *         F[u][k] = (float)(b Z[u][k]) (one rounding to f32 each) and row_loss[u] = 2 - 2 c; a dead row writes E = F = +0
 *         and row_loss[u] = (t > 0 ? 1 : 0), whatever Z and Q hold; a row whose float64 E or F holds a NaN or a value
 *         beyond the f32 range (a p2 next to nothing) is dead in the same way: nothing written is ever not finite.  Then loss_acc[0] += (sum of row_loss) / (B n), the sum
 *         in float64 in a fixed order: thread v of 256 adds the rows v, v + 256, .. ascending from 0, then the pairwise
 *         tree s[v] += s[v + d] for d = 128, 64, .. 1.
 *       rk_ease_elsa_scatter: G[j][k] is ONE f32 fmaf chain fma(x_uj, E[u - lo][k], .) from +0 over the positions u of row
 *         j inside [lo, hi), ascending.  An item with RK_EASE_ELSA_LONG or more such positions is summed by a workgroup
 *         that splits the COLUMNS, not the positions: the chain of an output is the same on either path, and a row
 *         depends on nothing outside the range.  No atomics.
 *       rk_ease_elsa_project: dot = (float)(row dot <dA_j, A_j>), d = max(norm_j, 1e-12f),
 *         dW[j][k] = fma(-dot, A[j][k], dA[j][k]) / d: an fmaf and a correctly rounded divide.
 *       rk_ease_elsa_adam, per element, every operation one f32 rounding: g = rk_ease_elsa_project's dW[j][k];
 *         m = fma(beta1, m, (1 - beta1) * g); v = fma(beta2, v, ((1 - beta2) * g) * g);
 *         W = fma(-step, m / fma(sqrt(v), isb2, eps), W) (sqrt and / correctly rounded; 1 - beta one f32 subtract on the
 *         host; step = lr / (1 - beta1^t) and isb2 = 1 / sqrt(1 - beta2^t) come from the caller, who forms them in
 *         float64 and rounds once); then norm_j and A[j] from the new W[j] exactly as rk_ease_elsa_normalize does.
 *       rk_ease_csr_sub: one f32 subtract per stored entry of the strip.
 */
#ifndef RECODER_EASE_H
#define RECODER_EASE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* (the library is built with -fvisibility=hidden: what this header declares is what it exports) */
#pragma GCC visibility push(default)

int rk_ease_version(void);
const char *rk_ease_last_error(void);

/*
 * A = X^T X + reg I, dense [n_items, lda], written once, every element of the n_items x n_items
 * square.  (t_*): the item-major CSR (X^T, n_items rows, columns = users); (u_*): the user-major
 * CSR (X, n_users rows, columns = items) of the SAME matrix; t_data and u_data are both NULL or
 * both given.  n_users >= 0, n_items >= 1.
 */
int rk_ease_gram(const int64_t *t_indptr, const int32_t *t_indices, const float *t_data,
                 const int64_t *u_indptr, const int32_t *u_indices, const float *u_data, int32_t n_users,
                 int32_t n_items, float reg, float *A, int64_t lda, void *stream);

/* bytes of workspace rk_ease_spd_inverse needs for an [n, n] matrix: n * n * 4 for the carries plus the
 * panels (> 0; < 0 on bad arguments) */
int64_t rk_ease_spd_inverse_workspace_bytes(int32_t n);

/*
 * A <- A^-1 in place for a symmetric positive-definite A [n, lda], n >= 1.  status: one int32 the
 * call first sets to 0, then to 1 + (index of the first pivot that was not > 0, or not finite) if
 * there is one; such a pivot is replaced by 1 and the call runs to its end without a fault (A is
 * then garbage).  The caller reads status after synchronising the stream.
 */
int rk_ease_spd_inverse(float *A, int32_t n, int64_t lda, void *ws, int64_t ws_bytes, int32_t *status,
                        void *stream);

/*
 * B[i][j] = P[i][j] / (-P[j][j]) for i != j, B[j][j] = +0; diag [n] receives diag(P) (always
 * written: the leave-one-out diagnostics use it).  B may be P (in place) or a second buffer that
 * does not overlap it.
 */
int rk_ease_finalize(const float *P, int32_t n, int64_t ldp, float *B, int64_t ldb, float *diag,
                     void *stream);

/*
 * out[u][c] = sum over the entries (j, x_uj) of CSR row u, ascending, of x_uj * W[j][lo + c], for
 * u in [0, n_rows) and c in [0, hi - lo); 0 <= lo < hi, every j is a row of W [>, ldw] and W has at
 * least hi columns.  out [n_rows, ldo], ldo >= hi - lo; columns past hi - lo are left as they are.
 * Workgroups that share a column tile run next to one another, so that the rows of W a batch
 * shares are read from L2 / MALL.
 */
int rk_ease_scores(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows,
                   const float *W, int64_t ldw, int32_t lo, int32_t hi, float *out, int64_t ldo,
                   void *stream);

/*
 * A[i][j] += (alpha * row_scale[i]) * (sum over t < k of V[i][t] * V[j][t]) * col_scale[j] for i in
 * [row_lo, row_hi) and j in [0, n): a dense rank-k update with diagonal scalings (GF-CF's ideal low-pass
 * filter, recoder_amd/gfcf.py).  A [n, lda], lda >= n, columns at or past n are not touched; V [n, ldv],
 * 1 <= k <= 512, ldv >= k, k a multiple of nothing; row_scale, col_scale [n]; 0 <= row_lo <= row_hi <= n (an
 * empty range does nothing).  No workspace.
 */
int rk_ease_lowrank_add(float *A, int32_t n, int64_t lda, const float *V, int32_t k, int64_t ldv,
                        const float *row_scale, const float *col_scale, float alpha, int32_t row_lo, int32_t row_hi,
                        void *stream);

/*
 * D[i][j] = alpha * (sum over t < k of A[i][t] * B[t][j]) + beta * E[i][j] for i in [row_lo, row_hi) and j in
 * [0, n): a general dense product.  A [m, lda], lda >= k; B [k, ldb], ldb >= n; D [m, ldd], ldd >= n, columns at or
 * past n and rows outside the range are not touched; m, n, k >= 1 and multiples of nothing.  E is NULL (beta is
 * ignored), or D itself (lde == ldd: an in-place accumulate), or an [m, lde] buffer, lde >= n, that does not overlap
 * D; it may be A or B.  D must not overlap A or B.  0 <= row_lo <= row_hi <= m (an empty range does nothing).  No
 * workspace.
 */
int rk_ease_gemm(const float *A, int64_t lda, const float *B, int64_t ldb, const float *E, int64_t lde, float *D,
                 int64_t ldd, int32_t m, int32_t n, int32_t k, float alpha, float beta, int32_t row_lo, int32_t row_hi,
                 void *stream);

/*
 * The element-wise pass of one ADMM-SLIM iteration (Steck et al., WSDM 2020; recoder_amd/admm.py) over the rows
 * [row_lo, row_hi) of five [n, n] matrices that do not overlap: with P = (G + (l2 + rho) I)^-1 and
 * T = rho P M - (l2 + rho) P, it forms the ridge step's B = T - P diag(gamma) (zero diagonal), V = B + U, the
 * soft-thresholded C_new (theta = l1 / rho >= 0, finite; nonneg 1: clipped at 0, 0: two-sided), the scaled dual
 * U = V - C_new and the next product's operand M = C_new - U.  T and P are read (all n rows of their diagonals); C and
 * U are read and written; M is written.  gamma [n] receives gamma_j for every j, whatever the range.  For the rows of
 * the range, row_primal[i] = sum_j (B - C_new)^2, row_dual[i] = sum_j (C_new - C)^2 and row_nnz[i] = the count of
 * C_new != 0; entries of rows outside the range are not touched (an empty range does nothing at all).
 */
int rk_ease_admm_update(const float *T, int64_t ldt, const float *P, int64_t ldp, float *C, int64_t ldc, float *U,
                        int64_t ldu, float *M, int64_t ldm, int32_t n, float theta, int32_t nonneg, float *gamma,
                        float *row_primal, float *row_dual, int32_t *row_nnz, int32_t row_lo, int32_t row_hi,
                        void *stream);

/* ---- ELSA: the low-rank shallow autoencoder scores = x (A A^T - I) (recoder_amd/elsa.py; Vancura et al., RecSys 2022) ---- */

/* items with at least this many positions inside the batch's range get a workgroup each in rk_ease_elsa_scatter */
#define RK_EASE_ELSA_LONG 128

/*
 * A[j] = W[j] / max(|W[j]|, 1e-12) and norms[j] = |W[j]| for j in [0, n): W [n, ldw], A [n, lda], 1 <= h <= 512 columns,
 * ldw, lda >= h.  At NULL, or [h, ldt], ldt >= n: At[k][j] = A[j][k].  A must not overlap W.
 */
int rk_ease_elsa_normalize(const float *W, int64_t ldw, int32_t n, int32_t h, float *A, int64_t lda, float *norms,
                           float *At, int64_t ldt, void *stream);

/*
 * The per-row pass of one ELSA step over B batch rows (B >= 0: none does nothing) of a catalogue of n items: from
 * Z = X_b A [B, ldz], Q = Z (A^T A) [B, ldq] and t2[u] = |X_u|^2 it writes the gradient's two row factors E [B, lde] and
 * F [B, ldf] (dA = X_b^T E + A (Z^T F)) and row_loss [B] (float64), and adds the batch's loss
 * mse_loss(normalize(Z A^T - X_b), normalize(X_b)) to loss_acc[0] (float64; NULL: not wanted).  E and F may not overlap
 * Z or Q.
 */
int rk_ease_elsa_rows(const float *Z, int64_t ldz, const float *Q, int64_t ldq, const float *t2, int32_t B, int32_t h,
                      int32_t n, float *E, int64_t lde, float *F, int64_t ldf, double *row_loss, double *loss_acc,
                      void *stream);

/*
 * G[j] = sum over the entries (u, x_uj) of row j of the item-major CSR with lo <= u < hi, ascending, of x_uj * E[u - lo],
 * for every j in [0, n): all n rows of G [n, ldg] are written, zeros where the range holds no entry.  (t_*): n rows,
 * the column indices (positions of users) STRICTLY ascending inside a row (a position held twice is not supported: the
 * count of a row's entries inside the range is then bounded by hi - lo, which the launch relies on); E [hi - lo, lde]; 0 <= lo <= hi (lo == hi: zeros, E
 * is not read).  The cost follows the entries inside the range: each row is searched for lo and hi.
 */
int rk_ease_elsa_scatter(const int64_t *t_indptr, const int32_t *t_indices, const float *t_data, int32_t n, int32_t lo,
                         int32_t hi, const float *E, int64_t lde, int32_t h, float *G, int64_t ldg, void *stream);

/* dW[j] = (dA[j] - <dA[j], A[j]> A[j]) / max(norms[j], 1e-12): the gradient through the normalisation, j in [0, n) */
int rk_ease_elsa_project(const float *dA, int64_t ldd, const float *A, int64_t lda, const float *norms, int32_t n,
                         int32_t h, float *dW, int64_t ldw, void *stream);

/*
 * One Adam step on every row of W [n, ldw] from dA [n, ldd] (the gradient with respect to A; projected as
 * rk_ease_elsa_project does), with the moments M, V packed [n, h]; then A [n, lda] and norms [n] are taken again from
 * the new W.  0 <= beta1, beta2 < 1, eps > 0; step = lr / (1 - beta1^t) and isb2 = 1 / sqrt(1 - beta2^t) for the step
 * count t >= 1.  No weight decay.
 */
int rk_ease_elsa_adam(float *W, int64_t ldw, const float *dA, int64_t ldd, float *A, int64_t lda, float *norms,
                      float *M, float *V, int32_t n, int32_t h, float beta1, float beta2, float eps, float step,
                      float isb2, void *stream);

/*
 * out[u][j - lo] -= x_uj for the stored entries (j, x_uj) of CSR row u with lo <= j < hi, u in [0, n_rows): the
 * "- x" of a strip of ELSA's scores.  out [n_rows, ldo], ldo >= hi - lo.  The column indices of a row are distinct (an
 * entry is a lane's own read-modify-write).
 */
int rk_ease_csr_sub(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows, int32_t lo,
                    int32_t hi, float *out, int64_t ldo, void *stream);

/* the largest m of rk_ease_explain, rk_slim_explain and rk_als_explain (64) */
int rk_ease_explain_max_contributors(void);

/*
 * Explanations: which entries of a user's history carry the score of a target item.  For every row u of the batch
 * CSR (indptr [n_rows + 1] / indices / data; data NULL: all ones) and every target j = items[u][q] (int64 [n_rows, J];
 * a j outside [0, n_items) is padding, -1 by convention), with c_e = x_ue * W[i_e][j] (ONE rounded f32 product) for
 * the entries e of the row in CSR order:
 *   contributors  int64 [n_rows, J, m]  the item ids of the m best entries, best first; -1 where the row has fewer
 *                                       than m entries, or the target is padding
 *   contributions f32   [n_rows, J, m]  their c_e; +0 at padding
 *   baseline      f32   [n_rows, J]     +0 (an item-item score has no part outside the history)
 *   total         f32   [n_rows, J]     t = fmaf(x_ue, W[i_e][j], t) over ALL entries in CSR order from +0: one chain,
 *                                       not the sum of the rounded c_e; +0 for padding
 * Order, best first: the larger c_e (-0 and +0 are one value); equal values to the earlier entry of the row; a NaN
 * behind every number.  A negative c_e is an ordinary value.  A target that is in the history is explained like any
 * other.  1 <= m <= 64, J >= 1, n_rows * J < 2^31.  One wave per (user, target), one launch on `stream`; no workspace,
 * no atomics; bitwise repeatable, and a pair's result depends on its own row, target and W alone -- not on n_rows, J,
 * the other targets or the launch.  tests/explain_util.py restates it; tests/test_explain.py compares bit for bit.
 * Here W is dense [n_items, ldw], ldw >= n_items: a lane gathers W[i_e * ldw + j], four entries in flight a lane.
 */
int rk_ease_explain(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows, const float *W,
                    int64_t ldw, int32_t n_items, const int64_t *items, int32_t J, int32_t m, int64_t *contributors,
                    float *contributions, float *baseline, float *total, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif /* RECODER_EASE_H */
