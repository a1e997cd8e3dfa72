/*
 * recoder_slim.h -- C ABI of librecoder_slim.so (MI355X / gfx950 only).
 *
 * SLIM (Ning & Karypis 2011, "SLIM: Sparse Linear Methods for Top-N Recommender Systems"): the learned
 * sparse item-item model.  With G = X^T X over the stored values of the user x item matrix (values >= 0),
 * column j of W solves
 *   min over w >= 0, w_j = 0 of   1/2 |x_j - X w|^2 + (l2/2) |w|^2 + l1 |w|_1
 * by cyclic coordinate descent in the covariance-update form of Friedman, Hastie & Tibshirani 2010
 * ("Regularization paths for generalized linear models via coordinate descent"), a column keeps at most
 * K entries, and scores(u, :) = x_u . W.  The model is stored by COLUMN: [n, K] ids / weights and [n]
 * counts.  A library of its own, beside the training, index, ALS, VAE, EASE, SVD and RP3beta libraries,
 * so that none of their symbol sets changes; the Python binding is recoder_amd/_slim_lib.py, the driver
 * recoder_amd/slim.py.
 *
 * Conventions (those of recoder_rp3.h)
 *   - every function returns 0 on success, <0 on error; rk_slim_last_error() gives a
 *     thread-local message.
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is retained past the call.
 *   - every launch goes on the caller's hipStream_t (passed as void*); no call synchronises
 *     the host; no call allocates (scratch comes from a workspace the caller sizes with the
 *     *_workspace_bytes query).
 *   - CSR: int64 indptr [rows + 1], int32 column indices ascending inside a row, without repeats.
 *
 * Screening (exact, not a heuristic).  The update of coordinate k of column j thresholds
 *   t_k = G_jk - sum over m != k of G_km w_m.
 * With G >= 0 (the values are >= 0) and w >= 0 (the constraint) the sum is >= 0, so t_k <= G_jk at every
 * point of every sweep.  A k with G_jk <= l1 therefore has t_k <= l1 for ever: its weight is 0 at the
 * start and no update ever moves it, and a coordinate at 0 changes nothing for the others.  The
 * candidates of column j are {k != j : G[j][k] > l1}, in ascending k; everything else is never visited,
 * and the result is the one of the sweep over all k != j.
 *
 * The algorithm (f32; no reductions anywhere; every call is bitwise repeatable and a column's result
 * depends on G, inv_denom, l1, K, max_sweeps and tol alone)
 *   state    w[c] = +0 and q[c] = G[j][cand[c]] for every candidate c      (q_c = G_jk - sum_m G_km w_m,
 *            the own term included)
 *   a sweep  for c ascending, k = cand[c]:
 *              t   = fmaf(G[k][k], w[c], q[c])
 *              new = (t > l1) ? (t - l1) * inv_denom[k] : +0        (one f32 subtraction, one f32 multiply)
 *              d   = new - w[c]
 *              d != 0:  q[c'] = fmaf(-d, G[k][cand[c']], q[c']) for every candidate c' (c included; row k
 *                       of G is read: the Gram is symmetric), then w[c] = new
 *   stop     after the first sweep whose max |d| (f32) is <= tol, or after max_sweeps sweeps; a column
 *            without candidates runs no sweep.  Every loop is bounded by max_sweeps x candidates.
 *   cut      the support is {c : w[c] > 0}; a support larger than K keeps its K largest by (w descending,
 *            id ascending), without a refit; the kept entries are stored with ascending ids.
 * inv_denom [n] is an INPUT, made on the host as 1 / (float64(G_kk) + l2) rounded once to f32: no division
 * runs on the device and l2 enters nowhere else.
 *
 * rk_slim_scores: one ascending f32 fmaf chain per output, from +0, over the kept entries of the output's
 * column: a score depends neither on the strip nor on the user's position in the batch.
 */
#ifndef RECODER_SLIM_H
#define RECODER_SLIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* (the library is built with -fvisibility=hidden: what this header declares is what it exports) */
#pragma GCC visibility push(default)

int rk_slim_version(void);
const char *rk_slim_last_error(void);

/* the largest K of rk_slim_fit / rk_slim_scores (1024) */
int rk_slim_max_neighbours(void);

/* the largest candidate count of a column whose state (cand, q, w, G_kk, inv_denom) lives in LDS; a column
 * with more candidates keeps it in its workgroup's slice of the workspace.  The result does not depend
 * on where the state lives. */
int rk_slim_lds_candidates(void);

/* bytes of workspace rk_slim_fit needs for n_items (host arithmetic; > 0; < 0 on bad arguments) */
int64_t rk_slim_fit_workspace_bytes(int32_t n_items);

/*
 * Columns [col_lo, col_hi) of the model.  G [n_items, ldg] f32 is the symmetric Gram (ldg >= n_items),
 * inv_denom [n_items] f32 as above; l1 >= 0, tol >= 0, max_sweeps >= 1, 1 <= K <= rk_slim_max_neighbours(),
 * 0 <= col_lo <= col_hi <= n_items.
 *   nbr_ids     int32 [n_items, K]  the kept k of column j, ascending; -1 past nbr_count[j]
 *   nbr_w       f32   [n_items, K]  their W[k][j]; +0 past nbr_count[j]
 *   nbr_count   int32 [n_items]     how many were kept (<= K)
 *   col_sweeps  int32 [n_items]     the sweeps run (0 without candidates).  A column that ran fewer than
 *                                   max_sweeps met the tolerance; one that ran max_sweeps may not have
 *   col_support int32 [n_items]     the entries > 0 before the cut (> K: the column was cut)
 * Columns outside [col_lo, col_hi) are not touched.  One wave solves a column; columns are handed to the
 * resident workgroups through one counter in the workspace, in ascending order: a column costs
 * sweeps x candidates^2, which differs by orders of magnitude, and a workgroup that finishes a light
 * column takes the next.  A G entry that is not > l1 (negative and NaN included) is no candidate.
 * ws must be 256-byte aligned.
 */
int rk_slim_fit(const float *G, int64_t ldg, int32_t n_items, const float *inv_denom, float l1, int32_t K,
                int32_t max_sweeps, float tol, int32_t col_lo, int32_t col_hi, int32_t *nbr_ids, float *nbr_w,
                int32_t *nbr_count, int32_t *col_sweeps, int32_t *col_support, void *ws, int64_t ws_bytes,
                void *stream);

/*
 * fsSLIM (Ning & Karypis 2011, section 4.3): rk_slim_fit with column j's regression restricted to a candidate list,
 * without the n x n Gram.  The matrix comes as both CSRs with the conventions of rk_rp3_item_fit: item-major
 * t_* [n_items + 1] / [nnz] (the users of an item, ascending), user-major u_* [n_users + 1] / [nnz] (the items of a
 * user, ascending), t_data / u_data the values in either entry order, both NULL: every value is 1.0.
 *   cand_ids   int32 [n_items, M]  the candidates of column j, ascending, -1 past cand_count[j]
 *   cand_count int32 [n_items]     how many (taken as 0 below 0 and as M above M)
 * 1 <= M <= rk_rp3_max_neighbours() (1024).  inv_denom, l1, K, max_sweeps, tol, col_lo, col_hi and the five outputs
 * are rk_slim_fit's; columns outside [col_lo, col_hi) are not touched.
 *
 * The local Gram of column j, with a_vi the value of user v for item i (f32; no atomics, no reductions):
 *   L[c][c'] = sum over the users v of a_{v, cand c} * a_{v, cand c'}     q[c] = sum over v of a_{v, cand c} * a_{v, j}
 * each entry one chain acc = fmaf(a_{v, cand c}, a_{v, other}, acc) from +0 over the users v of candidate c that hold
 * the other item, in ascending v.  L is bitwise symmetric (the product commutes), L[c][c] is the G_kk of the sweep.
 * A candidate whose q[c] is not > l1 (negative and NaN included), that is j itself or lies outside [0, n_items) is
 * screened: its weight is +0 and it is never visited.  On the others runs rk_slim_fit's sweep, stop rule and cut,
 * operation for operation (one device function serves both kernels), reading L[c][c'] where rk_slim_fit reads
 * G[cand c][cand c'].  With every item that shares a user with j among the candidates, and a Gram whose entries are
 * these chains, the result is rk_slim_fit's bit for bit.
 *
 * A workgroup of four waves solves a column; columns are handed to the resident workgroups through one counter in
 * the workspace.  A column costs about  sum over its candidates c, over the users v of c, of r_v  (r_v the entries
 * of user v) for L, then sweeps x candidates^2.  The candidate rows are handed to the four waves through a counter,
 * so the long user list of a popular candidate holds one wave while the others take the remaining rows; one
 * entry's chain is never split.  L lives in LDS for a column of up to rk_slim_sparse_lds_candidates()
 * candidates, beyond that in the workgroup's slice of the workspace; a column's result depends neither on where L
 * lives, nor on the column range, nor on the workgroup that took it.  ws must be 256-byte aligned and hold
 * rk_slim_fit_sparse_workspace_bytes(M) bytes.  col_screened int32 [n_items], or NULL: how many candidates of the
 * column passed the screen (what the sweep ran over), beside rk_slim_fit's five outputs.
 */
int rk_slim_sparse_lds_candidates(void);

/* bytes of workspace rk_slim_fit_sparse needs for lists of M candidates (host arithmetic; > 0; < 0 on a bad M) */
int64_t rk_slim_fit_sparse_workspace_bytes(int32_t M);

int rk_slim_fit_sparse(const int64_t *t_indptr, const int32_t *t_indices, const float *t_data, const int64_t *u_indptr,
                       const int32_t *u_indices, const float *u_data, int32_t n_users, int32_t n_items,
                       const int32_t *cand_ids, const int32_t *cand_count, int32_t M, const float *inv_denom, float l1,
                       int32_t K, int32_t max_sweeps, float tol, int32_t col_lo, int32_t col_hi, int32_t *nbr_ids,
                       float *nbr_w, int32_t *nbr_count, int32_t *col_sweeps, int32_t *col_support,
                       int32_t *col_screened, void *ws, int64_t ws_bytes, void *stream);

/*
 * out[u][c] = sum over the kept entries (k, w) of column lo + c, ascending, of x_uk * w for those k that CSR
 * row u stores (looked up by binary search in the row's ascending indices), for u in [0, n_rows) and c in
 * [0, hi - lo); a column nobody reaches is +0.  data NULL: every value is 1.0.  0 <= lo < hi <= n_items.
 * out [n_rows, ldo], ldo >= hi - lo; columns past hi - lo are left as they are.  The layout is what
 * rk_topk_masked reads.
 */
int rk_slim_scores(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows,
                   int32_t n_items, const int32_t *nbr_ids, const float *nbr_w, const int32_t *nbr_count,
                   int32_t K, int32_t lo, int32_t hi, float *out, int64_t ldo, void *stream);

/*
 * rk_ease_explain (include/recoder_ease.h: the same outputs, order, product and chain, from the same device code) for
 * a model stored as neighbour lists nbr_ids / nbr_w [n_items, K], nbr_count [n_items] (taken as 0 below 0 and as K
 * above K), the ids of a list ascending without repeats as every fit stores them:
 *   lists_are_columns = 1   row j of the three tensors is column j of W (rk_slim_fit, rk_rp3_item_fit): the list of the
 *                           target is searched for each history item
 *   lists_are_columns = 0   row i is row i of W (rk_rp3_fit): the list of each history item is searched for the target
 * by binary search.  A pair that the lists do not hold has W[i][j] = +0: it contributes x_ue * +0 and is a candidate
 * like any other, so a history shorter than m is not padded further.  On the dense matrix that holds the lists'
 * entries and +0 elsewhere rk_ease_explain gives the same bits.  1 <= K <= rk_slim_max_neighbours(), 1 <= m <= 64,
 * J >= 1, n_rows * J < 2^31.  No workspace, no atomics.
 */
int rk_slim_explain(const int64_t *indptr, const int32_t *indices, const float *data, int32_t n_rows, int32_t n_items,
                    const int32_t *nbr_ids, const float *nbr_w, const int32_t *nbr_count, int32_t K,
                    int32_t lists_are_columns, const int64_t *items, int32_t J, int32_t m, int64_t *contributors,
                    float *contributions, float *baseline, float *total, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif /* RECODER_SLIM_H */
