/*
 * recoder_rp3.h -- C ABI of librecoder_rp3.so (MI355X / gfx950 only).
 *
 * RP3beta (Paudel, Christoffel, Newell & Bernstein 2016, "Updatable, accurate, diverse, and scalable
 * recommendations for interactive applications"; P3alpha: Cooper et al. 2014): a sparse item-item
 * model from three-step random walks on the user-item graph.  The stored non-zero entries of the
 * user x item matrix are the edges; their values play no part in the fit.  With r_v the number of
 * items of user v, d_i the number of users of item i and U(i) the users of item i:
 *   S_ij = sum over v in U(i) and U(j) of r_v^-alpha              (walk i -> v -> j)
 *   W_ij = d_i^-alpha * S_ij * d_j^-beta   (j != i),   W_ii = 0
 *   row i keeps its K largest W_ij > 0 by (W descending, j ascending); everything else is 0
 *   scores(u, :) = x_u . W                                         (x_u: the user's stored values)
 * The model is [n, K]: an n x n (or block x n) image of W never exists in device memory.
 * A library of its own, beside the training, index, ALS, VAE, EASE and SVD libraries, so that none
 * of their symbol sets changes; the Python binding is recoder_amd/_rp3_lib.py, the driver
 * recoder_amd/rp3.py.
 *
 * Conventions (those of recoder_als.h / recoder_ease.h)
 *   - every function returns 0 on success, <0 on error; rk_rp3_last_error() gives a
 *     thread-local message.
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is retained past the call.
 *   - every launch goes on the caller's hipStream_t (passed as void*); no call synchronises
 *     the host; no call allocates (scratch comes from a workspace the caller sizes with the
 *     *_workspace_bytes query).
 *   - CSR: int64 indptr [rows + 1], int32 column indices ascending inside a row, without repeats.
 *
 * The three weight vectors of rk_rp3_fit are INPUTS, made on the host: no pow runs on the device.
 * RP3beta passes user_w[v] = r_v^-alpha, row_scale[i] = d_i^-alpha, col_scale[j] = d_j^-beta.  The
 * same kernel therefore also gives P3alpha (col_scale = 1, i.e. beta = 0) and weighted cosine kNN
 * (user_w = 1, row_scale = col_scale = d^-1/2): the driver builds neither.  (That cosine is the
 * degenerate one: no shrink term, no stored values, no set similarity -- those are rk_rp3_item_fit.)
 *
 * Numerics (f32; every call is bitwise repeatable and a row's result depends on the data alone)
 *   - S_ij is ONE f32 add chain from +0 of user_w[v] over the users v of item i, ascending, that also
 *     hold j.  No atomics on data: a column belongs to one wave of the row's workgroup, and a wave
 *     takes the users one after the other.
 *   - W_ij = (row_scale[i] * S_ij) * col_scale[j]: two f32 roundings, in that order.
 *   - selection: the K-th largest value is found exactly by radix selection on the float bits, ties
 *     at that value go to the lower ids (a second radix selection on the ids), and the kept entries
 *     are sorted by id.
 *   - rk_rp3_scores: one ascending f32 fmaf chain per output, from +0, over the user's stored
 *     entries: a score depends neither on the strip nor on the user's position in the batch.
 *
 * UserKNN (rk_rp3_user_*): the user-neighbourhood model, served from the training matrix X itself.  It
 * lives in this library because it is the fit's row pass turned round: the same hand-out of rows through
 * a counter, the same LDS / workspace split of the accumulator, the same exact selection and compaction
 * (one device function in rp3.hip, shared by both kernels).  With H_v the items of training user v and
 * H_q the stored items of a query row q (values play no part in the similarity):
 *   c_qv   = |H_q and H_v|                                          (an integer, exact)
 *   sim_qv = c_qv / (qn[q] * un[v] + shrink)                        (cosine with qn = |H_q|^1/2, un = |H_v|^1/2)
 *   q keeps its N largest sim_qv > 0 by (sim descending, v ascending), stored with ascending v
 *   scores(q, j) = sum over the kept v, ascending, of sim_qv * x_vj
 * qn and un are INPUTS made on the host (float64 square roots rounded once to f32): no sqrt runs on the
 * device.  A training user whose row equals the query is a neighbour like any other (the interface
 * carries no user ids).
 *
 * Numerics of rk_rp3_user_* (bitwise repeatable; a row's result depends on the data alone)
 *   - c_qv is counted with 32-bit integer atomic adds on the workgroup's own accumulator row: integer
 *     adds commute, so the order in which the waves arrive changes nothing.
 *   - sim = c / ((qn * un) + shrink): the product, the sum and the quotient are three separate f32
 *     operations, each correctly rounded.  The product and the sum are compiled under
 *     "#pragma clang fp contract(off)" (hipcc's default would fuse them into one fma); the quotient is
 *     __fdiv_rn, and the library is built without -ffast-math and with hipcc's default
 *     -fhip-fp32-correctly-rounded-divide-sqrt, so that no approximate reciprocal stands in for it.
 *   - selection and compaction: the fit's, ties at the N-th value to the lower user ids.
 *   - rk_rp3_user_scores: one f32 fmaf chain per output, from +0, over the kept neighbours in ascending
 *     v.  The split: a workgroup takes one query and one tile of 8192 columns, each of its 8 waves owns
 *     1024 consecutive columns of the tile and walks ALL the query's neighbours in ascending order, 64 at a
 *     time (lane l finds by binary search where neighbour l's ascending row enters and leaves the wave's
 *     columns; then the wave takes the 64 one after the other).  A column's chain therefore stays inside
 *     one wave, in neighbour order, whatever lo, hi and the query's position in the batch.
 *
 * ItemKNN (rk_rp3_item_*): the shrunk item-neighbourhood model, rk_rp3_fit's row pass (the same hand-out, the
 * same LDS / workspace split with its -0 first-touch fill, the same selection and compaction) with the two
 * things rk_rp3_fit's separable scale cannot spell: stored VALUES in the dot product and a denominator that
 * is not a product of a row and a column factor.  With a_vi the stored (possibly feature-weighted) value of
 * user v for item i, and j the own item, the one whose list is built (column j of W):
 *   s_ij   = sum over the users v of item j, ascending, that also hold i, of a_vj * a_vi
 *   form 0 (product): den = own[j] * oth[i] + shrink            cosine: own = oth = |a|;
 *                                                               asymmetric: own = |a_j|^(2(1-alpha)), oth = |a_i|^(2 alpha)
 *   form 1 (sum):     den = own[j] + oth[i] + g * s_ij + shrink Tversky on binary data: own = beta d_j,
 *                                                               oth = alpha d_i, g = 1 - alpha - beta
 *                                                               (Jaccard: alpha = beta = 1; Dice: alpha = beta = 1/2)
 *   sim_ij = s_ij / den where s_ij > 0 and den > 0, +0 otherwise; sim_jj = 0
 *   column j keeps its K largest sim_ij > 0 by (sim descending, i ascending), stored with ascending i
 *   scores(u, j) = sum over the kept i of column j that u holds of x_ui * sim_ij    (rk_slim_scores: the
 *                  lists are per column, as SparseLinearModel's)
 * own and oth are INPUTS made on the host (float64, rounded once): no sqrt or pow runs on the device.
 *
 * Numerics of rk_rp3_item_fit (bitwise repeatable; a column's result depends on the data alone)
 *   - s_ij is ONE f32 fmaf(a_vj, a_vi, acc) chain from +0, users ascending; no atomics on data (a column of
 *     the accumulator has one owning wave, which takes the users one after the other).  With NULL data the
 *     chain is adds of 1.0: an exact count.  Every product must be >= +0 (values >= 0): the workspace form
 *     recognises a column's first touch from its -0 fill.
 *   - den: form 0 (own[j] * oth[i]) + shrink; form 1 ((own[j] + oth[i]) + (g * s_ij)) + shrink.  Every
 *     operation is a separately rounded f32 operation, compiled under "#pragma clang fp contract(off)"; the
 *     quotient is __fdiv_rn (see rk_rp3_user_neighbours).
 *   - selection and compaction: the fit's, ties at the K-th value to the lower ids.
 */
#ifndef RECODER_RP3_H
#define RECODER_RP3_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* (the library is built with -fvisibility=hidden: what this header declares is what it exports) */
#pragma GCC visibility push(default)

int rk_rp3_version(void);
const char *rk_rp3_last_error(void);

/* the largest K of rk_rp3_fit / rk_rp3_scores and the largest N of rk_rp3_user_* (1024) */
int rk_rp3_max_neighbours(void);

/* the largest n_items whose row accumulators live in LDS; a larger catalogue keeps one n-float row
 * (and one n-entry candidate list) per resident workgroup in the workspace */
int rk_rp3_lds_items(void);

/* bytes of workspace rk_rp3_fit needs for n_items (host arithmetic; > 0; < 0 on bad arguments) */
int64_t rk_rp3_fit_workspace_bytes(int32_t n_items);

/*
 * Rows [row_lo, row_hi) of the model: one fused pass per source item i (accumulate, scale, select,
 * compact).  (t_*): the item-major CSR (n_items rows, columns = users); (u_*): the user-major CSR
 * (n_users rows, columns = items) of the SAME matrix.  user_w [n_users], row_scale [n_items] and
 * col_scale [n_items] are >= 0.  1 <= K <= rk_rp3_max_neighbours(), 0 <= row_lo <= row_hi <= n_items.
 *   nbr_ids   int32 [n_items, K]  the kept j of row i, ascending; -1 past nbr_count[i]
 *   nbr_w     f32   [n_items, K]  their W_ij; +0 past nbr_count[i]
 *   nbr_count int32 [n_items]     how many were kept (<= K)
 * Rows outside [row_lo, row_hi) are not touched.  Rows are handed to the resident workgroups
 * through one counter in the workspace, in ascending order: a row costs sum over v in U(i) of r_v,
 * which differs by orders of magnitude, and a workgroup that finishes a light row takes the next.
 * ws must be 256-byte aligned.
 */
int rk_rp3_fit(const int64_t *t_indptr, const int32_t *t_indices, const int64_t *u_indptr,
               const int32_t *u_indices, int32_t n_users, int32_t n_items, const float *user_w,
               const float *row_scale, const float *col_scale, int32_t K, int32_t row_lo, int32_t row_hi,
               int32_t *nbr_ids, float *nbr_w, int32_t *nbr_count, void *ws, int64_t ws_bytes, void *stream);

/*
 * out[u][c] = sum over the entries (i, x_ui) of CSR row u, ascending, of x_ui * W[i][lo + c] for those
 * i whose kept row contains lo + c, for u in [0, n_rows) and c in [0, hi - lo); columns nobody reaches
 * are +0.  data NULL: every value is 1.0.  0 <= lo < hi <= n_items; an entry outside [0, n_items)
 * adds nothing.  out [n_rows, ldo], ldo >= hi - lo; columns past hi - lo are left as they are.
 * The layout is what rk_topk_masked reads.
 */
int rk_rp3_scores(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows,
                  int32_t n_items, const int32_t *nbr_ids, const float *nbr_w, const int32_t *nbr_count,
                  int32_t K, int32_t lo, int32_t hi, float *out, int64_t ldo, void *stream);

/* bytes of workspace rk_rp3_user_neighbours needs for n_users training users (host arithmetic; > 0;
 * < 0 on bad arguments): the counter alone up to rk_rp3_lds_items() users, above it one row of counts
 * and one list of touched users per resident workgroup */
int64_t rk_rp3_user_workspace_bytes(int32_t n_users);

/*
 * The neighbour lists of the query rows [row_lo, row_hi): one fused pass per row (count, scale, select,
 * compact).  (q_*): the query CSR's indptr and indices (row_hi <= its rows; an item outside [0, n_items)
 * adds nothing); (t_*): the item-major CSR of X (n_items rows, columns = training users).  un [n_users],
 * qn [query rows] as above, shrink finite and >= 0, 1 <= N <= rk_rp3_max_neighbours().
 *   nbr_ids   int32 [query rows, N]  the kept v of row q, ascending; -1 past nbr_count[q]
 *   nbr_sim   f32   [query rows, N]  their sim_qv; +0 past nbr_count[q]
 *   nbr_count int32 [query rows]     how many were kept (<= N)
 * Rows outside [row_lo, row_hi) are not touched.  Rows are handed to the resident workgroups through one
 * counter in the workspace, as in rk_rp3_fit.  ws must be 256-byte aligned.
 */
int rk_rp3_user_neighbours(const int64_t *q_indptr, const int32_t *q_indices, const int64_t *t_indptr,
                           const int32_t *t_indices, int32_t n_users, int32_t n_items, const float *un,
                           const float *qn, float shrink, int32_t N, int32_t row_lo, int32_t row_hi,
                           int32_t *nbr_ids, float *nbr_sim, int32_t *nbr_count, void *ws, int64_t ws_bytes,
                           void *stream);

/*
 * out[q][c] = sum over the kept neighbours (v, sim) of row q, ascending, of sim * X[v][lo + c] for q in
 * [0, n_rows) and c in [0, hi - lo); columns nobody reaches are +0.  (u_*): the user-major CSR of X (n_users
 * rows, columns = items ascending); u_data NULL: every value is 1.0.  A neighbour id outside [0, n_users)
 * adds nothing.  0 <= lo < hi <= n_items.  out [n_rows, ldo], ldo >= hi - lo; columns past hi - lo are
 * left as they are.  The layout is what rk_topk_masked reads.
 */
int rk_rp3_user_scores(const int32_t *nbr_ids, const float *nbr_sim, const int32_t *nbr_count, int32_t n_rows,
                       int32_t N, const int64_t *u_indptr, const int32_t *u_indices, const float *u_data,
                       int32_t n_users, int32_t n_items, int32_t lo, int32_t hi, float *out, int64_t ldo,
                       void *stream);

/* bytes of workspace rk_rp3_item_fit needs for n_items (host arithmetic; > 0; < 0 on bad arguments): what
 * rk_rp3_fit_workspace_bytes gives */
int64_t rk_rp3_item_workspace_bytes(int32_t n_items);

/*
 * Columns [col_lo, col_hi) of the ItemKNN model: one fused pass per own item j (accumulate, scale, select,
 * compact).  (t_*): the item-major CSR (n_items rows, columns = users); (u_*): the user-major CSR (n_users
 * rows, columns = items) of the SAME matrix, values included.  t_data and u_data are either both NULL (every
 * value is 1.0) or both given (finite, >= 0).  own [n_items] and oth [n_items] are >= 0; form is 0 (product)
 * or 1 (sum); g and shrink are finite, shrink >= 0.  1 <= K <= rk_rp3_max_neighbours(),
 * 0 <= col_lo <= col_hi <= n_items.
 *   nbr_ids   int32 [n_items, K]  the kept i of column j, ascending; -1 past nbr_count[j]
 *   nbr_w     f32   [n_items, K]  their sim_ij; +0 past nbr_count[j]
 *   nbr_count int32 [n_items]     how many were kept (<= K)
 * Columns outside [col_lo, col_hi) are not touched.  Columns are handed to the resident workgroups through
 * one counter in the workspace, as rk_rp3_fit's rows are: any column range, in any hand-out order, gives the
 * same bits.  ws must be 256-byte aligned.
 */
int rk_rp3_item_fit(const int64_t *t_indptr, const int32_t *t_indices, const float *t_data, const int64_t *u_indptr,
                    const int32_t *u_indices, const float *u_data, int32_t n_users, int32_t n_items,
                    const float *own, const float *oth, int32_t form, float g, float shrink, int32_t K,
                    int32_t col_lo, int32_t col_hi, int32_t *nbr_ids, float *nbr_w, int32_t *nbr_count, void *ws,
                    int64_t ws_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif /* RECODER_RP3_H */
