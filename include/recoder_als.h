/*
 * recoder_als.h -- C ABI of librecoder_als.so (MI355X / gfx950 only).
 *
 * Implicit-feedback alternating least squares (Hu, Koren & Volinsky 2008) for a
 * MatrixFactorization with activation "none": score s_ui = x_u . y_i + b_i, loss
 *   L = sum_{u, i} w_ui (r_ui - s_ui)^2 + reg (sum_u |x_u|^2 + sum_i |y_i|^2),  w_ui = 1 + alpha [r_ui > 0]
 * over the WHOLE user x item matrix (zeros off the support of R).  The bias b is held fixed.
 * A library of its own, beside librecoder_hip.so and librecoder_index.so, so that neither of their
 * symbol sets changes; the Python binding is recoder_amd/_als_lib.py, the driver recoder_amd/als.py.
 *
 * One half-step solves every row x_u of one table with the other table F fixed:
 *   (G + sum_{j in u} a_j f_j f_j^T) x_u = sum_{j in u} ((1 + a_j) r_j - a_j c_j) f_j - s_u v,
 *   G = F^T F + reg I,  a_j = alpha [r_j > 0],
 *   user side: c_j = b[col_j] (col_bias), s_u = 1, v = F^T b;
 *   item side: c_j = b[row] (row_bias), s_u = b[row], v = F^T 1 (column sums of the fixed table).
 *
 * Conventions (those of recoder_hip.h)
 *   - every function returns 0 on success, <0 on error; rk_als_last_error() gives a
 *     thread-local message.
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is retained past the call.
 *   - every launch goes on the caller's hipStream_t (passed as void*); no call synchronises
 *     the host; no call allocates (scratch comes from a workspace the caller sizes with the
 *     *_workspace_bytes query).
 *   - tables are row-major fp32 with an explicit leading dimension (in elements); G is [h, h]
 *     with leading dimension h.  CSR: int64 indptr [rows + 1], int32 column indices, fp32 values
 *     (NULL: every value is 1.0).
 *
 * Numerics (all f32; every call is bitwise repeatable)
 *   - rk_als_gram splits the rows into chunks fixed by (rows) alone; each chunk is one k-ascending
 *     f32 chain on v_mfma_f32_32x32x2_f32, the chunks are added in ascending order.  No atomics.
 *     G[i][j] and G[j][i] are one stored value (bitwise symmetric).
 *   - rk_als_solve: a row's result depends only on its CSR row, G, v, the fixed table, the biases
 *     and its own current value: any [row_lo, row_hi) gives bitwise the rows of the full solve,
 *     whatever path (stashed or streamed factor rows, G from LDS or from memory) a row takes.
 *     The order (tests/als_util.py restates it, tests/test_als.py compares bit for bit): lane l of the
 *     row's wave owns dimensions k = l + 64 t; a dot product is each lane's fmaf chain over t ascending
 *     from +0, then an xor butterfly over lane distances 32, 16, 8, 4, 2, 1.  G p is one fmaf chain per
 *     output k over j ascending from +0, q_k = fmaf(G[j][k], p_j, q_k).  r starts as -(s_u v) and takes
 *     the row's entries in CSR order, r = fmaf(coef_j, f_j, r), while q = G x takes q = fmaf(a_j (f_j . x),
 *     f_j, q) for the entries with a_j != 0; then r -= q.  A CG step: q = G p plus the entries as before,
 *     al = rs / (p . q), x = fmaf(al, p, x), r = fmaf(-al, q, r), p = fmaf((r . r) / rs, p, r), both
 *     divisions correctly rounded; it stops at rs == 0 and at !(p . q > 0).  A row of >= 512 entries is
 *     cut into 16 contiguous pieces of ceil(n / 16) entries: each piece's sums are chains of their own
 *     from +0, added onto r and onto G x (G p) in ascending piece order.
 *     rk_als_objective: s is that dot chain + b_i in f32; everything after it is float64.
 *
 * BPR pairwise ranking (Rendle, Freudenthaler, Gantner & Schmidt-Thieme 2009) for the same model, the
 * rk_als_bpr_* functions: a triple t = (u, i, j) scores x_t = p_u . (q_i - q_j) + b_i - b_j, its loss is
 * softplus(-x_t), its gradient weight g_t = sigma(-x_t).  One step is synchronous mini-batch SGD over T
 * triples, every gradient taken at the tables as they stand at the start of the step:
 *   p_u += lr (sum_{t: u_t = u} g_t (q_i - q_j) - reg c_u p_u)          c_u: valid triples that hold u
 *   q_i += lr (sum_{t: i_t = i} g_t p_u - sum_{t: j_t = i} g_t p_u - reg c_i q_i)   (b_i likewise, +-g_t)
 * with c_i the occurrences of item i in either role; no division by T.  sample, grad, a stable sort of
 * the keys (the caller's: T user keys, 2T item keys) and apply make one step; no floating-point atomics.
 *   - Counter RNG: mix(z) is splitmix64's output function (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) *
 *     0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31), all modulo 2^64.
 *     key(seed, step, slot) = mix(mix(seed) ^ (step << 32 | slot)); draw d is mix(key + d), and it maps
 *     to [0, range) as (high 32 bits * range) >> 32.  That map is biased: a value's probability differs
 *     from 1 / range by at most 2^-32 (nothing for a power-of-two range).
 *   - Draw 0 picks a stored entry e in [0, nnz), nnz < 2^31; the user is the row that holds e, the
 *     positive is indices[e].  Draws 1..32 pick j in [0, n_items) until j is not in the user's row (rows
 *     ascending); when all 32 are, neg[t] = -1 and the slot is invalid: it adds nothing anywhere.
 *   - rk_als_bpr_grad: lane l of the triple's wave owns dimensions k = l + 64 m.  d_k = q_ik - q_jk (one
 *     rounding); the dot is each lane's fmaf chain over m ascending from +0, then an xor butterfly over
 *     lane distances 32, 16, 8, 4, 2, 1; then + b_i, then - b_j.  With e = exp(-|x|): g = e / (1 + e) for
 *     x >= 0, 1 / (1 + e) otherwise; loss = max(-x, 0) + log1p(e).
 *   - rk_als_bpr_apply: a row's sum is one fmaf chain per element over its segment of the sorted keys in
 *     the order given (ascending slot when the sort is stable), from +0; then
 *     new = fmaf(lr, fmaf(-(reg * c), old, sum), old).  One wave owns a row; nobody else writes it.
 *
 * WARP (Weston, Bengio & Usunier 2011) and dynamic negative sampling (Zhang, Chen, Wang & Yu 2013) on the
 * same step, rk_als_rank_sample and rk_als_warp_grad: the negative of a slot is chosen by the model's scores
 * s(u, c) = p_u . q_c + b_c.  Per slot, sequentially (the kernel groups the work, its results are these):
 *   - The key and draw 0 are rk_als_bpr_sample's: users and pos are its bits for the same (seed, step, slot).
 *     Draws d = 1..max_draws map to c_d in [0, n_items) as there; a c_d the user holds is skipped, the others
 *     are the slot's candidates, in draw order.
 *   - A score is rk_als_bpr_grad's dot chain (lane l owns k = l + 64 m, fmaf over m ascending from +0, the xor
 *     butterfly over lane distances 32..1), then + b_c with one rounding.  s_pos = s(u, pos).
 *   - RK_ALS_RANK_WARP: candidate c violates when (s(u, c) - s_pos) + margin > 0, two f32 operations of one
 *     rounding each.  The first violator is neg, trials = N = the candidates scored up to and including it,
 *     s_neg its score.  No violator within max_draws draws: neg = -1, trials = 0, s_neg = +0, and the slot is
 *     invalid in BPR's sense.
 *   - RK_ALS_RANK_DNS: of the first num_candidates candidates neg is the one of the largest score (a tie stays
 *     with the earlier draw), s_neg that score, trials how many were scored; no candidate: -1, 0, +0.  The
 *     margin plays no part.  num_candidates = 1 with max_draws = 32 gives rk_als_bpr_sample's three arrays.
 *   - scores[t, d - 1] is the score of draw d where the definition above scored it, +0 where the draw is held
 *     or lies behind the stopping point.  Everything depends on (seed, step, slot, CSR, tables) alone: not on
 *     T, the launch, or how the kernel groups the draws.
 *   - rk_als_warp_grad: g = weight[trials], loss = g * ((s_neg - s_pos) + margin) with both scores recomputed
 *     by the chain above, D = q_i - q_j (one rounding), P = p_u.  The hinge's gradient has BPR's form with g the
 *     rank weight, so rk_als_bpr_apply makes the update.  weight is the caller's table, built in float64 on
 *     the host and rounded once (recoder_amd/warp.py: log(max(1, (n_items - 1) / N)) or the harmonic number
 *     of (n_items - 1) / N, the division an integer one): no logf and no harmonic loop runs on the device.
 *
 * LightGCN (He, Deng, Wang, Li, Zhang & Wang 2020) for the same model, the rk_als_lgcn_* functions: the
 * final tables are the mean over K + 1 layers of the base tables propagated over the symmetrically
 * normalised user-item graph, trained with the BPR triples above and Adam (recoder_amd/lightgcn.py).
 *   - rk_als_lgcn_propagate: a column's sum is one fmaf chain over the row's entries in ascending order
 *     from +0, acc = fmaf(col_scale[col], F[col, k], acc); then * row_scale, then + Acc, then * acc_scale,
 *     one rounding each.  A row of >= RK_ALS_LGCN_LONG_ROW entries is cut into n = 64 (h <= 128) or 16
 *     contiguous parts with the bounds e0 + p len / n; each part is such a chain and the parts are added in
 *     ascending p.  The order depends on the row's length and h alone: any [row_lo, row_hi) gives bitwise
 *     the rows of the full call, with 16-byte accesses (h, the leading dimensions and the pointers
 *     allowing) or without.
 *   - rk_als_lgcn_scatter: rk_als_bpr_apply's chain over a row's segment with the weight -g_t for a user's
 *     entry and for a positive, +g_t for a negative; then * scale.
 *   - rk_als_lgcn_adam: grad = fmaf(reg_scale * count, e, H); m = fmaf(b1, m, (1 - b1) * grad);
 *     v = fmaf(b2, v, ((1 - b2) * grad) * grad); e = fmaf(-step, m / fmaf(sqrt(v), isb2, eps), e) with
 *     step = lr / (1 - b1^t) and isb2 = 1 / sqrt(1 - b2^t) computed in float64 on the host and rounded once.
 *   No floating-point atomics anywhere.
 */
#ifndef RECODER_ALS_H
#define RECODER_ALS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* (the library is built with -fvisibility=hidden: what this header declares is what it exports) */
#pragma GCC visibility push(default)

int rk_als_version(void);
const char *rk_als_last_error(void);

/* largest embedding size the kernels take */
int rk_als_max_h(void);

/* bytes of workspace rk_als_gram needs for a [rows, h] table (>= 0; < 0 on bad arguments) */
int64_t rk_als_gram_workspace_bytes(int32_t rows, int32_t h);

/*
 * G = F^T F + reg I ([h, h]) and v = F^T w ([h]; w NULL: all ones, the column sums) for the table
 * F [rows, ldf], rows >= 0 (rows == 0 gives G = reg I, v = 0), 1 <= h <= rk_als_max_h().
 */
int rk_als_gram(const float *F, int32_t rows, int32_t h, int32_t ldf, const float *w, float reg, float *G,
                float *v, void *ws, int64_t ws_bytes, void *stream);

/* rk_als_solve flags (tests and measurements; 0 picks the paths by h and row length) */
#define RK_ALS_FORCE_STREAM 1 /* re-read every factor row from memory on every CG step */
#define RK_ALS_G_GLOBAL 2     /* read G from memory even when it fits in LDS */

/*
 * cg_steps conjugate-gradient steps, warm-started from X[r], on the normal equations above for
 * every row r in [row_lo, row_hi) of the CSR (indptr / indices / data); X [>= row_hi, ldx] is
 * updated in place.  F [>, ldf]: the fixed table (its rows indexed by the CSR's columns); G, v from
 * rk_als_gram of F; exactly one of col_bias / row_bias may be non-NULL (both NULL: b = 0).
 * A row's factor rows are gathered once into LDS and every CG step runs from there when they fit;
 * longer rows stream them from memory on every step.
 */
int rk_als_solve(const int64_t *indptr, const int32_t *indices, const float *data, int32_t row_lo,
                 int32_t row_hi, const float *F, int32_t ldf, int32_t h, const float *G, const float *v,
                 const float *col_bias, const float *row_bias, float alpha, int32_t cg_steps, float *X,
                 int32_t ldx, int32_t flags, void *stream);

/* bytes of workspace rk_als_objective needs for a CSR of `rows` rows */
int64_t rk_als_objective_workspace_bytes(int32_t rows);

/*
 * out[0] = L (float64) for X [rows, ldx] (users), Y [cols, ldy] (items), bias [cols] (NULL: 0) and
 * the user x item CSR.  Gx, sx: rk_als_gram of X with w = NULL; Gy, cy: rk_als_gram of Y with
 * w = bias; both with this reg.  The sparse part (per stored entry: w (r - s)^2 - s^2) is one row
 * per wave, the rest comes from the Grams: tr(X^T X Y^T Y) + 2 sx . cy + rows |b|^2 + reg (tr X^T X
 * + tr Y^T Y); every sum in float64 in a fixed order.
 */
int rk_als_objective(const int64_t *indptr, const int32_t *indices, const float *data, int32_t rows,
                     int32_t cols, const float *X, int32_t ldx, const float *Y, int32_t ldy, int32_t h,
                     const float *bias, float alpha, float reg, const float *Gx, const float *Gy,
                     const float *sx, const float *cy, void *ws, int64_t ws_bytes, double *out, void *stream);

/*
 * bytes of the buffers one BPR step over T triples at embedding size h needs from its caller, each
 * rounded up to 256: users, pos, neg (int32 [T]), g, loss (f32 [T]), D, P (f32 [T, h]):
 * 5 * round256(4 T) + 2 * round256(4 T h).  1 <= T <= 2^24; < 0 on bad arguments.  (The caller's sort
 * of the keys needs its own room.)
 */
int64_t rk_als_bpr_workspace_bytes(int32_t T, int32_t h);

/*
 * users[t], pos[t], neg[t] (int32 [T]) for the slots t < T of step `step` >= 0 under `seed`, from the
 * user x item CSR (int64 indptr [n_users + 1], int32 indices ascending within a row, nnz =
 * indptr[n_users], 1 <= nnz < 2^31): see the draws above.  Integer arithmetic only; stored values play
 * no part.
 */
int rk_als_bpr_sample(const int64_t *indptr, const int32_t *indices, int32_t n_users, int32_t n_items,
                      int64_t nnz, int64_t seed, int32_t step, int32_t T, int32_t *users, int32_t *pos,
                      int32_t *neg, void *stream);

/*
 * For every slot t < T: g[t] = sigma(-x_t), loss[t] = softplus(-x_t) and the staging rows D[t, :] =
 * q_i - q_j, P[t, :] = p_u (f32 [T, h], leading dimension h) from X [n_users, ldx], Y [n_items, ldy]
 * and bias [n_items].  A slot with neg[t] < 0 (or an id outside the tables) is invalid: g, loss and
 * both rows are +0.  x (f32 [T]; NULL: not wanted) receives the scores x_t, for tests and measurements.
 * One wave per triple.
 */
int rk_als_bpr_grad(const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t T, int32_t n_users,
                    int32_t n_items, const float *X, int32_t ldx, const float *Y, int32_t ldy, const float *bias,
                    int32_t h, float *g, float *loss, float *x, float *D, float *P, void *stream);

/*
 * The update of one table from the sorted keys of a step.  keys (int32 [n], ascending): the row of
 * every entry; order (int64 [n]): the entry's position before the sort, as a device sort returns it.
 * roles == 1 (users): n = T, entry t is slot t, V = D, bias NULL.  roles == 2 (items): n = 2 T, entry
 * 2 t is slot t's positive (weight +g_t) and entry 2 t + 1 its negative (weight -g_t), V = P, bias the
 * item bias, updated like a table column with V = 1.  Keys outside [0, n_rows) are skipped: give the
 * entries of an invalid slot the key n_rows.  table [n_rows, ldt] is updated in place; rows without a
 * key are not touched.  One wave per distinct key.
 */
int rk_als_bpr_apply(const int32_t *keys, const int64_t *order, int32_t n, int32_t roles, const float *g,
                     const float *V, int32_t h, float lr, float reg, int32_t n_rows, float *table, int32_t ldt,
                     float *bias, void *stream);

/* the most draws rk_als_rank_sample takes per slot, and its two modes */
#define RK_ALS_RANK_MAX_DRAWS 256
#define RK_ALS_RANK_WARP 0
#define RK_ALS_RANK_DNS 1

/*
 * The model-aware sampler of a step (see WARP / DNS above): users, pos, neg, trials (int32 [T]) for the slots
 * t < T of step `step` >= 0 under `seed`, from the CSR rk_als_bpr_sample takes and the tables X [n_users, ldx],
 * Y [n_items, ldy], bias [n_items] at embedding size h <= rk_als_max_h().  1 <= max_draws <=
 * RK_ALS_RANK_MAX_DRAWS; in DNS mode 1 <= num_candidates <= max_draws; in WARP mode margin is finite and >= 0.
 * s_pos, s_neg (f32 [T]) and scores (f32 [T, max_draws], every entry written; for tests) may be NULL: not
 * wanted.  s_pos is s(u, pos) of every slot, valid or not.  One wave per slot: 64 draws are hashed and searched
 * at a time, and the rows of several candidates are gathered before any is reduced; a score computed behind
 * the stopping point is dropped.
 */
int rk_als_rank_sample(const int64_t *indptr, const int32_t *indices, int32_t n_users, int32_t n_items,
                       int64_t nnz, int64_t seed, int32_t step, int32_t T, const float *X, int32_t ldx,
                       const float *Y, int32_t ldy, const float *bias, int32_t h, int32_t mode, int32_t max_draws,
                       int32_t num_candidates, float margin, int32_t *users, int32_t *pos, int32_t *neg,
                       int32_t *trials, float *s_pos, float *s_neg, float *scores, void *stream);

/*
 * rk_als_bpr_grad for WARP's hinge: for every slot t < T, g[t] = weight[trials[t]], loss[t] = g[t] * ((s_neg -
 * s_pos) + margin) and the staging rows D[t, :] = q_i - q_j, P[t, :] = p_u (f32 [T, h]).  weight: f32
 * [RK_ALS_RANK_MAX_DRAWS + 1], device memory.  A slot with neg[t] < 0, trials[t] outside 1..RK_ALS_RANK_MAX_DRAWS
 * or an id outside the tables is invalid: g, loss and both rows are +0.  One wave per slot.
 */
int rk_als_warp_grad(const int32_t *users, const int32_t *pos, const int32_t *neg, const int32_t *trials, int32_t T,
                     int32_t n_users, int32_t n_items, const float *X, int32_t ldx, const float *Y, int32_t ldy,
                     const float *bias, int32_t h, float margin, const float *weight, float *g, float *loss,
                     float *D, float *P, void *stream);

/* rows of at least this many stored entries get a workgroup of 16 waves each in rk_als_lgcn_propagate */
#define RK_ALS_LGCN_LONG_ROW 1024

/*
 * One propagation of a LightGCN layer over one orientation of the normalised bipartite graph.  For every
 * row r in [row_lo, row_hi) of the CSR (indptr / indices; there is no value array):
 *   Out[r, :h] = row_scale[r] * sum_j col_scale[col_j] * F[col_j, :h]     (no entries: +0)
 *   Acc[r, :h] = (Acc[r, :h] + Out[r, :h]) * acc_scale                    (Acc != NULL)
 * Out may be NULL when Acc is given (the last layer, where only the layer mean is wanted).  F [>, ldf] is
 * indexed by the CSR's columns and must not overlap Out or Acc; row_scale and col_scale hold one float per
 * row and per column.  Rows outside the range are not touched.
 */
int rk_als_lgcn_propagate(const int64_t *indptr, const int32_t *indices, const float *row_scale,
                          const float *col_scale, int32_t row_lo, int32_t row_hi, const float *F, int32_t ldf,
                          int32_t h, float *Out, int32_t ldo, float *Acc, int32_t lda, float acc_scale,
                          void *stream);

/*
 * The gradient with respect to one final table from the sorted keys of a step, in the layout of
 * rk_als_bpr_apply (keys, order, n = roles * T, roles; V = D for the users, P for the items).  For every
 * key in [0, n_rows) present: G[key, :h] = scale * sum +-g_t V[t, :h] and count[key] = its entries.
 * Rows without a key are not touched: the caller zeroes G [n_rows, ldg] and count (int32 [n_rows]) first.
 */
int rk_als_lgcn_scatter(const int32_t *keys, const int64_t *order, int32_t n, int32_t roles, const float *g,
                        const float *V, int32_t h, float scale, int32_t n_rows, float *G, int32_t ldg,
                        int32_t *count, void *stream);

/*
 * Adam step t >= 1 on the base table E0 [rows, lde] in place, from H [rows, ldh] (the propagated
 * gradient), count (int32 [rows]) and the moments M, V (f32 [rows, h], leading dimension h, in place):
 * see the numerics above.  Every row is updated: a zero gradient still decays the moments.
 */
int rk_als_lgcn_adam(float *E0, int32_t lde, const float *H, int32_t ldh, const int32_t *count, float reg_scale,
                     float *M, float *V, int32_t rows, int32_t h, float lr, float beta1, float beta2, float eps,
                     int32_t t, void *stream);

/* the largest T of rk_als_gcl_contrast (its workspace holds the T x T scores) */
#define RK_ALS_GCL_MAX_BATCH 4096

/*
 * rk_als_lgcn_propagate with SimGCL's noise in its epilogue: with x the row rk_als_lgcn_propagate gives, bit
 * for bit,
 *   Out[r, :h] = x + eps * sign(x) * u[r] / |u[r]|_2       (sign(0) = 0: a row without entries stays +0)
 * and Acc accumulates this perturbed Out.  u[r, c] in (0, 1) is a counter hash of (seed, step, view, layer,
 * side, r, c) kept apart from the sampler's draws; |u[r]| is an integer sum, so Out depends on the key, the
 * row and h alone -- not on the leading dimensions, the row range or the launch.  eps == 0 gives
 * rk_als_lgcn_propagate's bits.  step >= 0; view and layer in 0..255; side 0 (user rows) or 1 (item rows).
 */
int rk_als_gcl_propagate(const int64_t *indptr, const int32_t *indices, const float *row_scale,
                         const float *col_scale, int32_t row_lo, int32_t row_hi, const float *F, int32_t ldf,
                         int32_t h, float *Out, int32_t ldo, float *Acc, int32_t lda, float acc_scale, float eps,
                         int64_t seed, int32_t step, int32_t view, int32_t layer, int32_t side, void *stream);

/* bytes of rk_als_gcl_contrast's workspace; -2 unless 1 <= T <= RK_ALS_GCL_MAX_BATCH and 1 <= h <= 512 */
int64_t rk_als_gcl_contrast_workspace_bytes(int32_t T, int32_t h);

/*
 * SimGCL's contrast between two view tables V1 [n_rows, ld1] and V2 [n_rows, ld2] over keys (int32 [T],
 * ascending, as rk_als_lgcn_scatter takes them).  Slot t is active when keys[t] lies in [0, n_rows) and differs
 * from keys[t - 1]; with m active slots, z = v / |v| per row (0 for |v| = 0) and s_rs = z1_r . z2_s / tau,
 *   loss[0] = (1 / m) sum_r (log sum_s exp(s_rs) - s_rr)     (over active r and s; 0 when m == 0)
 *   count[0] = m
 *   G1[key_r, :h] += weight * d loss / d V1[key_r],   G2 likewise      (other rows are not touched)
 * The gradient of a row with |v| = 0 is taken as 0.  G1 and G2 may be the same table.  The workspace holds
 * the T x T scores; loss, count, G1 and G2 are device memory.  A fixed summation order: the same inputs give
 * the same bits.
 */
int rk_als_gcl_contrast(const int32_t *keys, int32_t T, int32_t n_rows, const float *V1, int32_t ld1,
                        const float *V2, int32_t ld2, int32_t h, float tau, float weight, float *G1, int32_t ldg1,
                        float *G2, int32_t ldg2, void *ws, int64_t ws_bytes, float *loss, int32_t *count,
                        void *stream);

/* bytes of rk_als_dau_grad's workspace; -2 unless 1 <= T <= RK_ALS_GCL_MAX_BATCH and 1 <= h <= 512 */
int64_t rk_als_dau_workspace_bytes(int32_t T, int32_t h);

/*
 * DirectAU's loss and its gradient rows over the T slots (users[t], items[t]) of a step, at the final tables
 * X [n_users, ldx] and Y [n_items, ldy].  Slot t is valid when both ids lie in their tables; with m valid slots,
 * a_t = X[users[t]] / |.|, b_t = Y[items[t]] / |.| (0 for a row of norm 0), and for either side's rows z
 *   e_pq = exp(-2 |z_p - z_q|^2) (|z|^2 taken as 1, or 0 for a zero row),  E = sum_{p < q} e_pq over valid slots
 * (a repeated id is a slot of its own):
 *   loss[0] = (1 / m) sum_t |a_t - b_t|^2                     (0 when m == 0)
 *   loss[1] = log(2 E / (m (m - 1))) over the a_t,  loss[2] likewise over the b_t      (0 when m < 2)
 *   count[0] = m,  valid[t] = 1.0 or 0.0
 *   DU[t, :h] = d (loss[0] + (gamma / 2) (loss[1] + loss[2])) / d X[users[t]] taken through slot t alone,
 *   DI[t, :h] likewise for Y[items[t]]: rk_als_lgcn_scatter with roles = 1 and g = valid sums them per row.
 * The rows of an invalid slot are 0, and so is the row of a table row of norm 0.  DU, DI (f32 [T, h]), valid
 * (f32 [T]), loss (f32 [3]) and count (int32 [1]) are device memory; the workspace holds one T x T tile of the
 * e_pq, used for the users and then for the items.  A fixed summation order: the same inputs give the same bits.
 */
int rk_als_dau_grad(const int32_t *users, const int32_t *items, int32_t T, int32_t n_users, int32_t n_items,
                    const float *X, int32_t ldx, const float *Y, int32_t ldy, int32_t h, float gamma, void *ws,
                    int64_t ws_bytes, float *DU, float *DI, float *valid, float *loss, int32_t *count, void *stream);

/* the largest T and S of rk_als_ssm_grad (its workspace holds the T x (T + S) scores) */
#define RK_ALS_SSM_MAX_BATCH 4096
#define RK_ALS_SSM_MAX_NEGATIVES 4096

/* bytes of rk_als_ssm_grad's workspace; -2 unless 1 <= T <= RK_ALS_SSM_MAX_BATCH, 0 <= S <=
 * RK_ALS_SSM_MAX_NEGATIVES and 1 <= h <= 512 */
int64_t rk_als_ssm_workspace_bytes(int32_t T, int32_t S, int32_t h);

/*
 * The sampled softmax of the T slots (users[t], items[t]) of a step over C = T + S candidate columns, at the final
 * tables X [n_users, ldx] and Y [n_items, ldy].  Column c < T holds items[c] (the in-batch negatives of every other
 * row); column T + n holds the n-th shared negative, drawn uniformly from [0, n_items) by the sampler's counter hash
 * of (seed, step, n) under a domain of its own, nothing rejected.  cand (int32 [C]) receives the columns' items.
 * Slot t is valid when both ids lie in their tables, column c < T when slot c is, a shared column always.  With
 *   s_tc = sim(X[users[t]], Y[cand[c]]) * inv_tau - corr[cand[c]]      (corr NULL: 0)
 * sim the cosine (cosine = 1; a row of norm 0 has z = 0) or the dot product (cosine = 0), the LIVE columns of a
 * valid row t are the valid ones except those c != t with cand[c] == items[t]; over them and the m valid slots
 *   loss[0] = (1 / m) sum_t (lse_t - s_tt),   loss[1] = (1 / m) sum_t exp(s_tt - lse_t)          (0 when m == 0)
 *   count[0] = m,  valid[t] and cvalid[c] = 1.0 or 0.0
 *   DU[t, :h] = d loss[0] / d X[users[t]] taken through slot t alone, DC[c, :h] = d loss[0] / d Y[cand[c]] taken
 *   through column c alone: rk_als_lgcn_scatter with roles = 1 sums them per row (g = valid over the T users,
 *   g = cvalid over the C candidates).
 * The rows of an invalid slot or column are +0, and so is the own row of a table row of norm 0 under the cosine.  A
 * row whose only live column is its own has the loss term 0 and zero weights exactly.  DU (f32 [T, h]), DC (f32
 * [C, h]), valid (f32 [T]), cvalid (f32 [C]), loss (f32 [2]) and count (int32 [1]) are device memory; the
 * workspace holds the T x C scores, overwritten by the weights.  The scores and both gradient products run on
 * v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32 with k ascending.  A fixed summation order: the same inputs give
 * the same bits.
 */
int rk_als_ssm_grad(const int32_t *users, const int32_t *items, int32_t T, int32_t S, int64_t seed, int32_t step,
                    int32_t n_users, int32_t n_items, const float *X, int32_t ldx, const float *Y, int32_t ldy,
                    int32_t h, float inv_tau, int32_t cosine, const float *corr, void *ws, int64_t ws_bytes,
                    int32_t *cand, float *DU, float *DC, float *valid, float *cvalid, float *loss, int32_t *count,
                    void *stream);

/* the limits of rk_als_ugcn_grad: T slots, R negatives and K neighbours a slot, T (1 + R + K) entries a step; a
 * key of rk_als_ugcn_scatter with this many entries or more is summed by a whole workgroup */
#define RK_ALS_UGCN_MAX_BATCH 4096
#define RK_ALS_UGCN_MAX_NEGATIVES 1024
#define RK_ALS_UGCN_MAX_NEIGHBOURS 64
#define RK_ALS_UGCN_MAX_ENTRIES (1 << 22)
#define RK_ALS_UGCN_LONG_KEY 1024

/* bytes of the step's buffers cand (int32 [T, E]), coef (f32 [T, E]) and loss (f32 [T, 3]), E = 1 + R + K, each
 * rounded up to 256 bytes and laid out in that order; -2 unless 1 <= T <= RK_ALS_UGCN_MAX_BATCH, 1 <= R <=
 * RK_ALS_UGCN_MAX_NEGATIVES, 0 <= K <= RK_ALS_UGCN_MAX_NEIGHBOURS, T E <= RK_ALS_UGCN_MAX_ENTRIES and 1 <= h <= 512 */
int64_t rk_als_ugcn_workspace_bytes(int32_t T, int32_t R, int32_t K, int32_t h);

/*
 * UltraGCN's constraint loss and its gradient over the T slots (users[t], items[t]) of a step, at the tables
 * X [n_users, ldx] and Y [n_items, ldy].  Slot t is valid when both ids lie in their tables.  It scores E = 1 + R + K
 * candidate items with s = X[users[t]] . Y[item] (no bias):
 *   column 0            the positive items[t]:  a = w1 + w2 bu[u] bi[i],                  term a softplus(-s)
 *   columns 1 .. R      negative r = column - 1, drawn uniformly from [0, n_items) by the sampler's counter hash of
 *                       (seed, step, t R + r) under a domain of its own, nothing rejected:
 *                       a = (negative_weight / R) (w3 + w4 bu[u] bi[j]),                  term a softplus(s)
 *   columns R + 1 ..    neighbour n of the positive, nbr_ids[i, n] with the weight nbr_w[i, n] (an id outside
 *                       [0, n_items) is an absent neighbour):  a = item_weight nbr_w[i, n],  term a softplus(-s)
 * and leaves
 *   cand [T, E]   the columns' items; n_items for an absent neighbour and for every column of an invalid slot
 *   coef [T, E]   d term / d s; +0 for an absent or invalid entry
 *   DU [T, :h]    sum_e coef[t, e] Y[cand[t, e]], over e ascending (+0 for an invalid slot)
 *   valid [T]     1.0 or 0.0
 *   loss [T, 3]   the positive's term, the sum of the negatives' terms, the sum of the neighbours' terms
 * rk_als_lgcn_scatter with roles = 1 and g = valid sums DU per user row; rk_als_ugcn_scatter sums the item side.  One
 * wave per slot; sigma and softplus through e = exp(-|x|) as in rk_als_bpr_grad.  bu (f32 [n_users]), bi (f32
 * [n_items]), nbr_ids (int32 [n_items, K]) and nbr_w (f32 [n_items, K]) may be NULL when K == 0 (the two lists).
 * A fixed summation order: the same inputs give the same bits, whatever the leading dimensions.
 */
int rk_als_ugcn_grad(const int32_t *users, const int32_t *items, int32_t T, int32_t R, int32_t K, int64_t seed,
                     int32_t step, int32_t n_users, int32_t n_items, const float *X, int32_t ldx, const float *Y,
                     int32_t ldy, int32_t h, const float *bu, const float *bi, const int32_t *nbr_ids,
                     const float *nbr_w, float w1, float w2, float w3, float w4, float negative_weight,
                     float item_weight, int32_t *cand, float *coef, float *DU, float *valid, float *loss,
                     void *stream);

/*
 * The item side of rk_als_ugcn_grad: keys (int32 [n], n = T E) are the cand entries stably sorted ascending and
 * order (int64 [n]) their positions e before the sort.  For every key in [0, n_rows) among them
 *   G[key, :h] = scale * sum coef[e] X[users[e / E], :h]     over the key's entries in ascending position
 *   count[key] = the key's entries with e % E == 0 (the slots whose positive it is)
 * The user rows are gathered from X [n_users, ldx]; an entry whose position or user lies outside its range adds
 * nothing.  Rows without a key are not touched: the caller zeroes G [n_rows, ldg] and count (int32 [n_rows]) first.
 * A key with fewer than RK_ALS_UGCN_LONG_KEY entries is one f32 fmaf chain of one wave; a longer one is cut into 16
 * equal parts, one chain each, summed in ascending part order.  No atomics.
 */
int rk_als_ugcn_scatter(const int32_t *keys, const int64_t *order, int32_t n, int32_t E, const int32_t *users,
                        const float *coef, const float *X, int32_t ldx, int32_t n_users, int32_t h, float scale,
                        int32_t n_rows, float *G, int32_t ldg, int32_t *count, void *stream);

/* the limits of rk_als_ccl_grad: T slots, R negatives a slot, T (1 + R) entries a step (UltraGCN's at K = 0) */
#define RK_ALS_CCL_MAX_BATCH 4096
#define RK_ALS_CCL_MAX_NEGATIVES 1024
#define RK_ALS_CCL_MAX_ENTRIES (1 << 22)

/* bytes of the step's buffers cand, key (int32 [T, E]), coef, self (f32 [T, E]), loss (f32 [T, 2]) and live (int32
 * [T]), E = 1 + R, each rounded up to 256 bytes and laid out in that order; -2 unless 1 <= T <= RK_ALS_CCL_MAX_BATCH,
 * 1 <= R <= RK_ALS_CCL_MAX_NEGATIVES, T E <= RK_ALS_CCL_MAX_ENTRIES and 1 <= h <= 512 */
int64_t rk_als_ccl_workspace_bytes(int32_t T, int32_t R, int32_t h);

/*
 * SimpleX's cosine contrastive loss (Mao et al. 2021) and its gradient over the T slots (users[t], items[t]) of a
 * step, at the tables X [n_users, ldx] and Y [n_items, ldy].  Slot t is valid when both ids lie in their tables.  Its
 * E = 1 + R candidates are the positive items[t] (column 0) and the R draws of rk_als_ugcn_grad for the same (seed,
 * step, t R + r) (columns 1 .. R: the same domain, uniform over [0, n_items), nothing rejected).  With p = X[users[t]],
 * a = p / |p|, y = Y[item] and c = (a . y) / |y| the cosine (a row of norm 0 normalises to the zero vector: c = 0),
 *   L_t = (1 - c_0) + (negative_weight / R) sum_r max(0, c_r - margin),
 * a negative is live when the one f32 subtraction c - margin is > 0, w = d L_t / d c is -1 for the positive,
 * negative_weight / R for a live negative and 0 for a dead one, and the call leaves
 *   cand [T, E]   the columns' items (rk_als_ugcn_grad's columns 0 .. R at K = 0); n_items in an invalid slot
 *   key [T, E]    the item where the entry carries a gradient (w != 0, |p| > 0, |y| > 0), else the sentinel n_items
 *   coef [T, E]   w / (|p| |y|); +0 under a sentinel
 *   self [T, E]   w c / |y|^2;   +0 under a sentinel      (d L_t / d Y[item] = coef p - self y)
 *   DU [T, :h]    d L_t / d p = (sum_e (w_e / |y_e|) y_e - (sum_e w_e c_e) a) / |p|   (+0 for an invalid slot)
 *   valid [T]     1.0 or 0.0
 *   loss [T, 2]   1 - c_0 and (negative_weight / R) sum_r max(0, c_r - margin)
 *   live [T]      the live negatives of the slot
 * rk_als_lgcn_scatter with roles = 1 and g = valid sums DU per user row; rk_als_ccl_scatter sums the item side.
 * Numerics, all f32.  A row is held dimension k = l + 64 q on lane l of a group of W lanes (W = 16 for h <= 16, 32 for
 * h <= 32, else 64).  |p|^2 and |y|^2 are fmaf chains over q ascending from +0, then an xor butterfly over the group
 * (offsets W / 2 .. 1); 1 / |.| = 1.f / sqrtf(.), a_k = p_k (1 / |p|); a . y is the same chain and butterfly and
 * c = (a . y) (1 / |y|).  Over the live candidates in ascending e: acc_k = fmaf(w (1 / |y|), y_k, acc_k) and
 * sc = fmaf(w, c, sc); below the wave, group g of the 64 / W takes the candidates e with e mod (64 / W) == g and the
 * groups' acc and sc are added in ascending g from +0; DU_k = fmaf(-sc, a_k, acc_k) (1 / |p|).  coef = (w (1 / |p|))
 * (1 / |y|), self = ((w c) (1 / |y|)) (1 / |y|).  The negatives' term: lane l adds c - margin of its live candidates
 * e = l + 64 j in ascending j, wave_sum's butterfly (offsets 32 .. 1), times negative_weight / R (one f32 division on
 * the host).  No atomics: the same inputs give the same bits, whatever T, the launch and the leading dimensions.
 */
int rk_als_ccl_grad(const int32_t *users, const int32_t *items, int32_t T, int32_t R, int64_t seed, int32_t step,
                    int32_t n_users, int32_t n_items, const float *X, int32_t ldx, const float *Y, int32_t ldy,
                    int32_t h, float margin, float negative_weight, int32_t *cand, int32_t *key, float *coef,
                    float *self, float *DU, float *valid, float *loss, int32_t *live, void *stream);

/*
 * The item side of rk_als_ccl_grad: keys (int32 [n], n = T E) are the key entries stably sorted ascending and order
 * (int64 [n]) their positions e before the sort.  For every key in [0, n_rows) among them
 *   G[key, :h] = scale * (sum coef[e] X[users[e / E], :h] - (sum self[e]) Y[key, :h])
 *   count[key] = the key's entries with e % E == 0 (the slots whose positive it is)
 * over the key's entries, walked as rk_als_ugcn_scatter walks them (the same device function): the coefficients' sum
 * is one f32 fmaf chain of one wave in ascending position below RK_ALS_UGCN_LONG_KEY entries, and 16 equal parts, one
 * chain each, added in ascending part order from there on.  The self sum of a chain's positions: lane l adds the
 * positions l + 64 j in ascending j, then the xor butterfly; the parts' sums in ascending part order; the row is
 * scale * fmaf(-(sum self), Y[key, k], sum_k).  The sentinels sort last and are never read: no user row is gathered
 * for a dead entry.  Y [>= n_rows, ldy] is the item table rk_als_ccl_grad read.  Rows without a key are not touched:
 * the caller zeroes G [n_rows, ldg] and count (int32 [n_rows]) first.  No atomics.
 */
int rk_als_ccl_scatter(const int32_t *keys, const int64_t *order, int32_t n, int32_t E, const int32_t *users,
                       const float *coef, const float *self, const float *X, int32_t ldx, int32_t n_users,
                       const float *Y, int32_t ldy, int32_t h, float scale, int32_t n_rows, float *G, int32_t ldg,
                       int32_t *count, void *stream);

/* the limits of rk_als_sx_forward: at most this many entries of a user's history are pooled (max_history and E); the
 * slots of rk_als_sx_backward's dW are summed in consecutive chunks of RK_ALS_SX_CHUNK */
#define RK_ALS_SX_MAX_HISTORY 1024
#define RK_ALS_SX_CHUNK 256

/* bytes of the step's buffers B, dB (f32 [T, h]), hkey (int32 [T, E]), hcoef (f32 [T, E]), part (f32 [ceil(T /
 * RK_ALS_SX_CHUNK), h, h]) and dW (f32 [h, h]), each rounded up to 256 bytes and laid out in that order; -2 unless
 * 1 <= T <= RK_ALS_CCL_MAX_BATCH, 1 <= E <= RK_ALS_SX_MAX_HISTORY, T E <= RK_ALS_CCL_MAX_ENTRIES and 1 <= h <= 512 */
int64_t rk_als_sx_workspace_bytes(int32_t T, int32_t E, int32_t h);

/*
 * SimpleX's user rows (Mao et al. 2021, average pooling) for the T slots users[t], over the user CSR indptr (int64
 * [n_users + 1]) / indices (int32, ascending within a row; the stored values play no part), the item table Q
 * [n_items, ldq], the users' own table P [n_users, ldp] (NULL: the term gamma P[u] is 0) and the map W [h, ldw].  With
 * r the stored entries of row u and L = max_history, the history H_u is the whole row when r <= L and else the entries
 * at the positions floor(j r / L), j = 0 .. L - 1 (64-bit integers), and
 *   b      = (1 / |H_u|) sum_{k in H_u} Q[k]               (the zero vector for an empty row)
 *   B[t]   = b                                             (f32 [T, h]; NULL: not stored)
 *   X[row] = gamma P[u] + (1 - gamma) W b                  row = users[t], or t when compact != 0 (X [., ldx])
 *   hkey[t, e], hcoef[t, e]   e < E: the items of H_u in ascending position with the coefficient 1 / |H_u|, then the
 *                             sentinel n_items with +0 (both NULL: not stored).  E must be at least min(L, r) for every
 *                             slot; entries past E are pooled but not listed
 * A slot whose user lies outside [0, n_users) stores b = 0 and sentinels, and no row of X (a zero row when compact).
 * Two slots of one user store the same bits to the same row.  The list is rk_als_ccl_scatter's entry layout: run on
 * (hkey, hcoef, self = 0, the table dB of rk_als_sx_backward, users = the slot index) it sums the history's gradient
 * per item.
 * Numerics, all f32.  b: one add chain per column over H_u in ascending position from +0 (the rows are gathered
 * several at a time; the order of the adds is fixed), then one multiply by 1.f / (float)|H_u|.  W b: one chain
 * s_a = fmaf(W[a, c], b_c, s_a) over c ascending from +0 per element.  X = fmaf(gamma, p, (1.f - gamma) s_a).  One wave
 * per slot, no atomics: the same inputs give the same bits, whatever T and the leading dimensions.
 */
int rk_als_sx_forward(const int32_t *users, int32_t T, const int64_t *indptr, const int32_t *indices,
                      int32_t n_users, int32_t n_items, const float *Q, int32_t ldq, const float *P, int32_t ldp,
                      const float *W, int32_t ldw, int32_t h, float gamma, int32_t max_history, int32_t E, float *B,
                      float *X, int32_t ldx, int32_t compact, int32_t *hkey, float *hcoef, void *stream);

/*
 * The backward pass of the pooling branch, from DU (f32 [T, h]: the gradient at X[users[t]], as rk_als_ccl_grad leaves
 * it), valid (f32 [T]), the pooled rows B (f32 [T, h]) and W [h, ldw]:
 *   dB[t, c] = scale sum_a W[a, c] DU[t, a]                (+0 for an invalid slot)
 *   dW[a, c] = scale sum_{t valid} DU[t, a] B[t, c]        (f32 [h, h])
 * The caller's scale carries (1 - gamma) and the mean's 1 / T.  Numerics, all f32: dB is one chain fmaf(W[a, c],
 * DU[t, a], .) over a ascending from +0, times scale.  dW is summed in consecutive chunks of RK_ALS_SX_CHUNK slots --
 * part[ch, a, c] (f32 [ceil(T / RK_ALS_SX_CHUNK), h, h]) is one chain fmaf(DU[t, a], B[t, c], .) over the chunk's
 * slots ascending from +0, an invalid slot entering with DU = +0 -- and a second launch adds the chunks in ascending
 * order and multiplies by scale: the result does not depend on the grid.  Three launches, no atomics.
 */
int rk_als_sx_backward(const float *DU, const float *valid, const float *B, int32_t T, const float *W, int32_t ldw,
                       int32_t h, float scale, float *dB, float *part, float *dW, void *stream);

/* the metric kinds of rk_als_rank_metrics and how many records one call takes */
#define RK_ALS_METRIC_RECALL 0
#define RK_ALS_METRIC_NDCG 1
#define RK_ALS_METRIC_AP 2
#define RK_ALS_RANK_METRICS_MAX 8

/*
 * Ranking metrics of B users' top-K lists, everything on the device: recs (int64 [B, K], row stride ld >= K, the ids
 * of a row distinct: what rk_topk_masked leaves) against the target CSR tgt_indptr (int64 [B + 1]) / tgt_indices
 * (int32 [tgt_nnz], ascending within a row, stored zeros dropped; may be NULL when tgt_nnz == 0).  Metric m < n_metrics
 * is (kinds[m], ks[m], normalize[m]), three host arrays; with hit_r = (recs[u, r] is a target of u), c_r = the hits
 * up to and including rank r, ny = the user's targets and k' = min(ks[m], K) ranks read:
 *   RECALL  (sum_{r < k'} hit_r) / norm                       norm = normalize ? min(ks[m], ny) : ny
 *   AP      (sum_{r < k'} hit_r c_r / (r + 1)) / norm
 *   NDCG    (sum_{r < k'} hit_r inv_w[r]) / ideal[min(ks[m], ny)]
 * inv_w (float64 [>= min(K, max k)], 1 / log2(2 + r)) and ideal (float64 [max k + 1], ideal[c] = the sequential sum
 * of inv_w[:c]) are device tables the host builds, so that a term is the very double the host arithmetic divides
 * out.  Leaves
 *   values [B, n_metrics]   float64; nan in every column for a user without targets (0 / 0)
 *   sums [n_metrics]        float64: the non-nan values of each column, user t + 256 j added to partial t in ascending
 *                           j, then the 256 partials by a halving tree (partial t += partial t + off, off = 128 .. 1)
 *   count [1]               int64: the non-nan rows (of column 0)
 * One wave per user, lanes on ranks lane + 64 j; a binary search per rank, a ballot per 64 ranks; all sums float64 in
 * ascending rank order.  Two launches on `stream`, no atomics: the same inputs give the same bits.  -2 unless B, K >= 1,
 * ld >= K, 1 <= n_metrics <= RK_ALS_RANK_METRICS_MAX, every ks[m] >= 1, every kind one of the three, no NULL pointer.
 */
int rk_als_rank_metrics(const int64_t *recs, int32_t B, int32_t K, int64_t ld, const int64_t *tgt_indptr,
                        const int32_t *tgt_indices, int64_t tgt_nnz, int32_t n_metrics, const int32_t *kinds,
                        const int32_t *ks, const int32_t *normalize, const double *inv_w, const double *ideal,
                        double *values, double *sums, int64_t *count, void *stream);

/* largest embedding size rk_als_foldin takes (128) */
int rk_als_foldin_max_h(void);

/*
 * Fold-in: the user row of a history the fit has not seen, for any MatrixFactorization state with activation "none".
 * For every row u of the batch CSR (indptr [rows + 1] / indices / data; data NULL: all ones; columns are rows of Y) it
 * solves the user-side normal equations at the head of this file EXACTLY, by a Cholesky factorisation:
 *   (G + sum_{e in u} a_e y_e y_e^T) x_u = sum_e coef_e y_e - v,   a_e = alpha [r_e > 0],
 *   coef_e = (1 + a_e) r_e - a_e b_e   (bias NULL: b = 0),
 * with G [h, h] and v [h] from rk_als_gram(Y, w = bias, reg), and writes X[u, :h] (ldx >= h) and status[u].  Only
 * the lower triangle of G is read.  One launch on `stream`; no workspace, no atomics.  -2 unless 1 <= h <=
 * rk_als_foldin_max_h(), ldy, ldx >= h, rows >= 0, alpha finite and >= 0 and (with rows > 0) no pointer but data and
 * bias is NULL: a larger h is refused, there is no other path.
 * Arithmetic (all f32, bitwise repeatable; tests/foldin_util.py restates it, tests/test_foldin.py compares bit for
 * bit).  Every fused operation is an fmaf and nothing else is contracted.
 *   - the entries are taken in CSR order, never cut into pieces; coef_e is two rounded products and their rounded
 *     difference, (1 + a_e) rounded first
 *   - r_k starts as -v_k; r_k = fmaf(coef_e, Y[j_e][k], r_k) over e ascending
 *   - the lower triangle k >= l: A[k][l] starts as G[k][l]; over the entries with a_e != 0, ascending,
 *     t = a_e Y[j_e][k] (one rounding), A[k][l] = fmaf(t, Y[j_e][l], A[k][l])
 *   - Cholesky A = L L^T: s = A[i][j], s = fmaf(-L[i][k], L[j][k], s) for k = 0 .. j - 1; L[j][j] = sqrt(s);
 *     L[i][j] = s / L[j][j]; the root and the division correctly rounded
 *   - z_i = (r_i - sum_{k < i} L[i][k] z_k) / L[i][i], the sum as fmaf(-L[i][k], z_k, .) over k ascending
 *   - x_i = (z_i - sum_{k > i} L[k][i] x_k) / L[i][i], as fmaf(-L[k][i], x_k, .) over k DESCENDING from h - 1
 *   - a pivot s that is not > 0 (nan included): X[u] = +0 and status[u] = 1; every other row has status[u] = 0
 * A row's result depends on its own entries, Y, G, v, bias and alpha alone: not on the other rows, on `rows` or on
 * the launch.
 */
int rk_als_foldin(const int64_t *indptr, const int32_t *indices, const float *data, int32_t rows, const float *Y,
                  int32_t ldy, int32_t h, const float *G, const float *v, const float *bias, float alpha, float *X,
                  int32_t ldx, int32_t *status, void *stream);

/* the limits of the iALS++ kernels: the embedding size (rk_als_ials_max_h(), 2048), the block width
 * (rk_als_ials_max_block(), 128), and the entries from which rk_als_ials_block cuts a row over a whole workgroup */
#define RK_ALS_IALS_LONG_ROW 1024
int rk_als_ials_max_h(void);
int rk_als_ials_max_block(void);

/*
 * iALS++ (Rendle, Krichene, Zhang & Koren 2021, "iALS++: Speeding up Matrix Factorization with Subspace
 * Optimization") for the same model with the bias 0, on the objective of Rendle et al. 2022: with S the stored entries
 * (their values play no part), X [n_users, ldx] and Y [n_items, ldy],
 *   L = sum_{(u,i) in S} (x_u . y_i - 1)^2 + alpha0 sum_u sum_i (x_u . y_i)^2 + sum_u lam_u |x_u|^2 + sum_i mu_i |y_i|^2
 * with per-row regularisers lam, mu the caller builds (recoder_amd/ials.py: reg (count + alpha0 n)^nu in float64,
 * rounded once).  The solver keeps c[e] = x_u . y_i for every stored entry, in the order of the user-major CSR.
 *
 * rk_als_ials_predict: c[e] = X[u_e] . Y[indices[e]] for the nnz entries of the CSR indptr (int64 [rows + 1]) / indices;
 * a wave takes 8 consecutive entries one after the other; per entry lane l runs the chain fmaf(x_k, y_k, .) over
 * k = l + 64 q ascending from +0, then an xor butterfly over lane distances 32 .. 1.  nnz == 0: nothing is launched.
 */
int rk_als_ials_predict(const int64_t *indptr, const int32_t *indices, int32_t rows, int64_t nnz, const float *X,
                        int32_t ldx, const float *Y, int32_t ldy, int32_t h, float *c, void *stream);

/*
 * One block step on the coordinates pi = [p0, p0 + k) of the rows [row_lo, row_hi) of one side.  indptr / indices is
 * that side's CSR (the user-major one, or its transpose for the items), F [., ldf] the fixed table its columns index,
 * X [., ldx] the table updated in place, P [k, ldp] the panel rk_als_ials_gram_panel(F, p0, k) = F[:, pi]^T F, reg one
 * regulariser per row, and perm (int64 [nnz]; NULL on the user side) maps entry e of this CSR to its position in the
 * cache: the cache entry of e is c[perm ? perm[e] : e].  Per row u, with S_u its entries:
 *   g = sum_{e in S_u} (c_e - 1) f_e[pi] + alpha0 P x_u + reg_u x_u[pi]
 *   A = sum_{e in S_u} f_e[pi] f_e[pi]^T + alpha0 P[:, pi] + reg_u I
 *   delta = A^-1 g (Cholesky);  x_u[pi] -= delta;  c_e -= delta . f_e[pi] for e in S_u
 * A row whose Cholesky meets a pivot that is not > 0 (nan included; possible only with reg_u = 0) is left as it is,
 * cache included, and status[0] (int32, the caller zeroes it) is raised by one: an integer atomic, the only atomic.
 * Nothing outside the rows' columns pi and the rows' own cache entries is written.
 * Arithmetic (all f32, every fused operation an fmaf, nothing else contracted; the same inputs give the same bits):
 *   - a row of fewer than RK_ALS_IALS_LONG_ROW entries is one part; a longer one is cut into NP = 8 (k <= 64) or 2
 *     contiguous parts with the bounds p n / NP.  A part takes its entries in ascending order:
 *     gp_j = fmaf(c_e - 1, f_e[j], gp_j) and, for the lower triangle, a_jl = fmaf(f_e[j], f_e[l], a_jl), from +0
 *   - A_jl = fmaf(alpha0, P[j][p0 + l], [j == l] reg_u), then the parts' a_jl added in ascending part order
 *   - g_j = fmaf(reg_u, x[p0 + j], alpha0 * d_j) with d_j = fmaf(P[j][c], x[c], .) over c = 0 .. h - 1 from +0, then
 *     the parts' gp_j added in ascending part order
 *   - Cholesky and both triangular solves as rk_als_foldin states them; x[p0 + j] = x[p0 + j] - delta_j
 *   - c_e = c_e - s_e, s_e the sum over 16 lanes (xor butterfly over distances 8 .. 1) of lane l's chain
 *     fmaf(delta_j, f_e[j], .) over j = l + 16 q ascending from +0
 * A row's result depends on its own entries, its cache entries, F, P, reg_u, alpha0 and its own value alone.
 * long_rows (int32 [n_long], or NULL): the caller's list of this CSR's rows with RK_ALS_IALS_LONG_ROW entries or more,
 * every one of them, in any order; the long rows' launch then takes one workgroup per listed row (those outside the
 * range leave at once) and none when the list is empty.  With NULL the launch takes one workgroup per row of the range
 * and the short ones leave at once: the same bits, more empty workgroups.  Two
 * launches on `stream` (the short rows, four or one a workgroup; the long rows, one workgroup of 512 threads each);
 * no workspace.  -2 unless 1 <= h <= rk_als_ials_max_h(), 1 <= k <= rk_als_ials_max_block(), 0 <= p0 <= h - k, ldf,
 * ldx, ldp >= h, 0 <= row_lo <= row_hi, alpha0 finite and >= 0 and (with rows) no pointer but perm is NULL.
 */
int rk_als_ials_block(const int64_t *indptr, const int32_t *indices, const int64_t *perm, int32_t row_lo,
                      int32_t row_hi, const int32_t *long_rows, int32_t n_long, const float *F, int32_t ldf, float *X,
                      int32_t ldx, int32_t h, const float *P, int32_t ldp, const float *reg, float alpha0, int32_t p0,
                      int32_t k, float *cache, int32_t *status, void *stream);

/* bytes of rk_als_ials_gram_panel's workspace; -2 unless rows >= 0, 1 <= k <= min(h, 128) and h <= 2048 */
int64_t rk_als_ials_panel_workspace_bytes(int32_t rows, int32_t h, int32_t k);

/*
 * P[j, c] = sum_r F[r, p0 + j] F[r, c] for j < k, c < h (P [k, ldp], f32): the k rows p0 .. p0 + k - 1 of F^T F, without
 * a ridge term.  The rows are cut into at most 64 chunks fixed by `rows` alone; a chunk is one chain fmaf(F[r, p0 + j],
 * F[r, c], .) over r ascending from +0, and the chunks are added in ascending order.  P[j, p0 + l] and P[l, p0 + j]
 * are the same bits.  rows == 0 gives zeros.  Two launches, no atomics.
 */
int rk_als_ials_gram_panel(const float *F, int32_t rows, int32_t ldf, int32_t h, int32_t p0, int32_t k, float *P,
                           int32_t ldp, void *ws, int64_t ws_bytes, void *stream);

/* bytes of rk_als_ials_objective's workspace (4 x 256 float64 partial sums) */
int64_t rk_als_ials_objective_workspace_bytes(void);

/*
 * out[0] = L (float64, device memory) from the cache (f32 [nnz]: sum (c - 1)^2), the two full Grams Gx = X^T X and
 * Gy = Y^T Y ([h, h], leading dimension h, no ridge: alpha0 <Gx, Gy>) and the weighted row norms sum_u lam_u |x_u|^2 +
 * sum_i mu_i |y_i|^2.  Every product and sum is float64: element b 256 + t + 65536 j of a sum goes to thread t of block
 * b in ascending j (for the norms: row b 4 + w + 1024 j to wave w, lanes over the columns, an xor butterfly), a block's
 * threads are added by a halving tree, the 256 blocks in ascending order, and L = ((cache + alpha0 gram) + users) +
 * items.  Two launches, no atomics.
 */
int rk_als_ials_objective(const float *cache, int64_t nnz, const float *Gx, const float *Gy, int32_t h,
                          const float *X, int32_t ldx, int32_t n_users, const float *lam, const float *Y, int32_t ldy,
                          int32_t n_items, const float *mu, float alpha0, void *ws, int64_t ws_bytes, double *out,
                          void *stream);

/*
 * NeuMF (He, Liao, Zhang, Nie, Hu & Chua 2017) for recoder_amd/ncf.py:
 *   s(u, i) = w[:dg] . (Pg[u] o Qg[i]) + w[dg:] . phi_L + b0,  phi_0 = [Pm[u] ; Qm[i]],  phi_l = relu(W_l phi_{l-1} + c_l)
 * with 1 <= L <= RK_ALS_NCF_MAX_LAYERS layers of widths d_1 .. d_L (d_l past L is ignored); dg, dm and every d_l are
 * multiples of 4 in [4, RK_ALS_NCF_MAX_WIDTH].  The dense parameters are one f32 vector
 *   theta = [W_1, c_1, ..., W_L, c_L, w, b0],  W_l row-major [d_l, d_{l-1}] (d_0 = 2 dm), w [dg + d_L],
 * of rk_als_ncf_dense_count floats.  A workgroup takes a tile of RK_ALS_NCF_TILE entries (the step) or items (the
 * scores); its matrix products are 16 x 16 tiles of the f32 MFMA over weights kept in LDS at a row pitch of d + 1.
 * rk_als_ncf_lds_bytes gives a kernel's LDS (scores == 0: the step; else the scores), in floats
 *   step    sum_l (d_l (d_{l-1} + 1) + d_l + 32 (d_l + 1)) + dg + d_L + 1 + 128
 *   scores  sum_{l >= 2} (d_l (d_{l-1} + 1) + d_l) + dg + d_L + 1 + 32 (d_1 + 1) + 32 (dg + 1) + 64 (max_l d_l + 1) + d_1 + dg
 * and a configuration fits when both are at most 160 KiB (163840 bytes); the entry points below return -2 otherwise.
 * The three queries are host arithmetic (-2 on bad sizes).
 */
#define RK_ALS_NCF_TILE 32
#define RK_ALS_NCF_MAX_WIDTH 128
#define RK_ALS_NCF_MAX_LAYERS 3
int64_t rk_als_ncf_dense_count(int32_t dg, int32_t dm, int32_t L, int32_t d1, int32_t d2, int32_t d3);
int64_t rk_als_ncf_lds_bytes(int32_t dg, int32_t dm, int32_t L, int32_t d1, int32_t d2, int32_t d3, int32_t scores);

/* bytes of the step's buffers ukey, ikey (int32 [E]), GU, GI (f32 [E, dg + dm]), slabs (f32 [ceil(E / 32), n + 1], n
 * the dense count) and loss (f32 [1]), E = T (1 + R), each rounded up to 256 bytes and laid out in that order; -2 unless
 * 1 <= T <= RK_ALS_CCL_MAX_BATCH, 1 <= R <= RK_ALS_CCL_MAX_NEGATIVES and E <= RK_ALS_CCL_MAX_ENTRIES */
int64_t rk_als_ncf_workspace_bytes(int32_t T, int32_t R, int32_t dg, int32_t dm, int32_t L, int32_t d1, int32_t d2,
                                   int32_t d3);

/*
 * Forward, loss and backward of one step in one launch.  Entry e = t (1 + R) + c of slot t (users[t], pos[t]: the
 * stored entry rk_als_bpr_sample drew): c = 0 is the pair itself with label 1, c >= 1 the user with negative c - 1,
 * label 0 -- the draw of rk_als_ugcn_grad and rk_als_ccl_grad for (seed, step, t R + c - 1), uniform over [0, n_items),
 * nothing rejected: an item the user holds can be drawn as a negative, as in those two.  An entry with an id outside
 * its table is invalid: no loss, zero gradients, the keys n_users and n_items.  With z = s(u, i):
 *   loss term  softplus(z) - y z,  g = sigma(z) - y      (through e = exp(-|z|), as rk_als_bpr_grad)
 *   ukey[e], ikey[e]  the entry's rows (to be sorted by the caller)
 *   GU[e] = [g w[:dg] o Qg[i] ; d/dPm],  GI[e] = [g w[:dg] o Pg[u] ; d/dQm]      (f32 [E, dg + dm])
 *   slabs[tile] = the tile's sums over its entries of dW_l, dc_l, dw, db0 in theta's layout, then its loss sum
 * Nothing is divided by E here.  rk_als_lgcn_scatter (roles 1, g = ones, scale -1 / E) sums GU and GI per row and
 * rk_als_lgcn_adam updates the tables [Pg | Pm] and [Qg | Qm] when each pair is one matrix of leading dimension dg + dm.
 * Every sum has a fixed order; no atomics: the same inputs give the same bits.
 */
int rk_als_ncf_step(const int32_t *users, const int32_t *pos, int32_t T, int32_t R, int64_t seed, int32_t step,
                    int32_t n_users, int32_t n_items, const float *Pg, int32_t ldpg, const float *Qg, int32_t ldqg,
                    const float *Pm, int32_t ldpm, const float *Qm, int32_t ldqm, const float *theta, int32_t dg,
                    int32_t dm, int32_t L, int32_t d1, int32_t d2, int32_t d3, int32_t *ukey, int32_t *ikey, float *GU,
                    float *GI, float *slabs, void *stream);

/*
 * One Adam step t >= 1 on theta in place (moments M, V like theta): element x's gradient is the slabs' sum over the
 * tiles in ascending order from +0, times 1.f / entries, plus reg theta[x] on W_l and w (one fmaf; not on c_l and b0);
 * the update is rk_als_lgcn_adam's.  loss[0] receives the slabs' loss sum, in the same order.  One launch.
 */
int rk_als_ncf_dense_adam(float *theta, float *M, float *V, const float *slabs, int32_t tiles, int32_t entries,
                          int32_t dg, int32_t dm, int32_t L, int32_t d1, int32_t d2, int32_t d3, float lr, float reg,
                          float beta1, float beta2, float eps, int32_t t, float *loss, void *stream);

/* A [n_items, d1] = Qm W_1[:, dm:]^T, the items' half of layer 1: one fmaf chain over k ascending per element */
int rk_als_ncf_item_part(const float *Qm, int32_t ldqm, int32_t n_items, const float *theta, int32_t dm, int32_t d1,
                         float *A, void *stream);

/*
 * out[b, c] = s(users[b], lo + c) for b < B and c < hi - lo (row stride ld; nothing else of out is written), from A of
 * rk_als_ncf_item_part at the same theta.  UH (f32 [B, d1], scratch) receives the users' half W_1[:, :dm] Pm[u] + c_1,
 * once per user; layer 1 is relu(UH[b] + A[i]), layers 2 .. L are MFMA tiles of 32 items, the GMF term is
 * (Pg[u] o w[:dg]) . Qg[i].  A user id outside [0, n_users) gives a row of +0.  Two launches.
 */
int rk_als_ncf_scores(const int32_t *users, int32_t B, int32_t n_users, int32_t lo, int32_t hi, int32_t n_items,
                      const float *Pg, int32_t ldpg, const float *Qg, int32_t ldqg, const float *Pm, int32_t ldpm,
                      const float *A, const float *theta, int32_t dg, int32_t dm, int32_t L, int32_t d1, int32_t d2,
                      int32_t d3, float *UH, float *out, int64_t ld, void *stream);

/*
 * Constrained serving (recoder_amd/serve.py): item filters, candidate reranking, scores.
 *
 * The deny bitmap of a batch: bits (uint32 [B, ldw], 32 ldw >= n_items) has bit (c & 31) of word bits[r, c >> 5] set
 * when item c is NOT eligible for row r, which is rk_block_t::bits_rc of an unsampled block with `implicit` set: what
 * rk_topk_masked masks.  Item c is eligible for row r when all of these hold:
 *   - seen_indptr is NULL, or (r, c) is not an entry of the seen CSR (int64 seen_indptr [B + 1], int32 seen_ids,
 *     f32 seen_vals or NULL for all ones) with a value > 0: a stored value <= 0 does not mask
 *   - cat_allow is NULL or has bit c set;  cat_deny is NULL or has bit c clear (uint32 [ceil(n_items / 32)] each)
 *   - ua_indptr is NULL, or c is in row r of the allow CSR (ua_indptr [B + 1], ua_ids);  c is not in row r of the
 *     deny CSR (ud_indptr, ud_ids; NULL: nobody is denied)
 * The bits of the last word past n_items are 1 and the words from ceil(n_items / 32) to ldw are all-ones.
 * eligible[r] (int32) is the number of eligible items of row r: the popcount of the complement over [0, n_items), taken
 * after every OR of the row is complete.  An id outside [0, n_items) is skipped, an indptr clamped to [0, nnz]; ids may
 * repeat and need no order.  One launch on `stream`, one workgroup a row; 32-bit integer atomicAnd / atomicOr on the
 * row's own words, whose result does not depend on their order: the same inputs give the same bits.  -2 unless B >= 0,
 * n_items >= 1, 32 ldw >= n_items, every nnz >= 0 and (with B > 0) bits and eligible are not NULL.
 */
int rk_als_serve_mask(int32_t B, int32_t n_items, int32_t ldw, const int64_t *seen_indptr, const int32_t *seen_ids,
                      const float *seen_vals, int64_t seen_nnz, const uint32_t *cat_allow, const uint32_t *cat_deny,
                      const int64_t *ua_indptr, const int32_t *ua_ids, int64_t ua_nnz, const int64_t *ud_indptr,
                      const int32_t *ud_ids, int64_t ud_nnz, uint32_t *bits, int32_t *eligible, void *stream);

/*
 * scores[e] = z[r] . Y[ids[e]] + bias[ids[e]] for every entry e of row r < B of a ragged candidate list (int64 indptr
 * [B + 1], int32 ids [nnz]); z [B, h] with row stride ldz, Y [n, h] with row stride ldy, bias [n] or NULL.  An entry
 * whose id is outside [0, n), or whose bit is set in the optional deny bitmap (rk_als_serve_mask's, row stride ldw), is
 * not gathered and scores -inf.  max_row, an upper bound of a row's length, only sizes the launch: any value gives the
 * same scores.  h is a multiple of 4 in [4, rk_als_ials_max_h()]; ldz and ldy are multiples of 4 and z, Y 16-byte
 * aligned (rows are read as float4); anything else is -2.
 * The summation order depends on h alone.  A group of W lanes takes an entry, with
 *   h <= 16: W = 4, Q = 1    h <= 32: W = 8, Q = 1    h <= 64: W = 16, Q = 1     h <= 128: W = 32, Q = 1
 *   h <= 256: W = 64, Q = 1  h <= 512: W = 64, Q = 2  h <= 1024: W = 64, Q = 4   else: W = 64, Q = 8
 * lane j < W owns the dimensions d = 4 (j + W q) + c (q < Q, c < 4, d < h): its partial is one chain from +0,
 * s = fmaf(z[d], y[d], s), over q ascending and c ascending inside q.  The W partials are added by an xor butterfly at
 * the distances W / 2, ..., 2, 1 (p_j = p_j + p_{j ^ distance}), and the bias last: score = p + bias[id], one rounded
 * add.  tests/serve_util.py restates it; tests/test_serve.py compares bit for bit.  One launch, no atomics.
 */
int rk_als_pair_scores(const int64_t *indptr, const int32_t *ids, int64_t nnz, int32_t B, int32_t max_row,
                       const float *z, int32_t ldz, const float *Y, int32_t ldy, int32_t n, int32_t h,
                       const float *bias, const uint32_t *deny, int32_t ldw, float *scores, void *stream);

/* the longest row rk_als_pairs_topk ranks (8192) */
int32_t rk_als_pairs_topk_max_row(void);

/*
 * Ragged top-k: for every row r < B of the list (indptr, ids, scores as above) the eligible entries -- id in [0, n),
 * its bit clear in the optional deny bitmap -- by (score descending, id ascending) in rk_topk_pairs' order: float32 by
 * value, -0 and +0 one value, a NaN without the sign bit above +inf.  out_idx[r, i] (int64, row stride out_ld >= k) and
 * out_val[r, i] (f32, the same stride; may be NULL) receive the first min(k, count) of them, then id -1 and score -inf
 * up to k: the padding follows count[r] (int32, may be NULL), the row's number of eligible entries, never the score
 * values.  A row with fewer than k entries, or none, is an ordinary case.  The ids of a row must be distinct.
 * max_row bounds the rows' lengths (<= rk_als_pairs_topk_max_row(); a longer row is cut at the next power of two).
 * One workgroup a row, a bitonic sort in LDS; one launch.  -2 unless 1 <= k <= 8192 and 0 <= max_row <= 8192.
 */
int rk_als_pairs_topk(const int64_t *indptr, const int32_t *ids, const float *scores, int64_t nnz, int32_t B,
                      int32_t max_row, int32_t n, const uint32_t *deny, int32_t ldw, int32_t k, int64_t *out_idx,
                      float *out_val, int32_t out_ld, int32_t *count, void *stream);

/* bytes of workspace rk_als_explain needs for a CSR whose indices array holds nnz entries (host arithmetic; > 0;
 * < 0 for nnz < 0) */
int64_t rk_als_explain_workspace_bytes(int64_t nnz);

/*
 * Explanations of the folded-in user's scores: which entries of the history carry y_j . x_u + b_j.  With A_u, coef_e
 * and v of rk_als_foldin and z = A_u^-1 y_j,
 *   s_uj = sum_e coef_e (z . y_e) + (b_j - z . v):
 * the contribution of entry e is c_e = coef_e (z . y_e), the rest is the baseline.  Arguments up to alpha are
 * rk_als_foldin's (nnz: the entries of the indices array, which sizes the workspace; n_items: the rows of Y); items
 * int64 [rows, J], a j outside [0, n_items) is padding (-1 by convention).  Outputs as rk_ease_explain's
 * (include/recoder_ease.h: contributors int64 [rows, J, m], contributions f32 [rows, J, m], baseline and total f32
 * [rows, J], the same order of the candidates from the same device code), and status int32 [rows] as rk_als_foldin's.
 * Arithmetic (all f32, bitwise repeatable; tests/explain_util.py restates it, tests/test_explain.py compares bit for
 * bit).  Every fused operation is an fmaf and nothing else is contracted.
 *   - A_u and its Cholesky factor exactly as rk_als_foldin states them: one device function forms and factorises
 *     the system for both entry points
 *   - per target: z by rk_als_foldin's two triangular solves (one device function again) from the right-hand side y_j
 *   - baseline: d = fmaf(z_k, v_k, d) over k ascending from +0; baseline = b_j - d, one rounded difference (bias NULL:
 *     b_j = +0)
 *   - c_e: d = fmaf(z_k, Y[i_e][k], d) over k ascending from +0; c_e = coef_e * d, one rounded product, coef_e as
 *     rk_als_foldin rounds it
 *   - total: t = baseline; t = t + c_e over ALL entries in CSR order, one rounded sum each
 *   - a row whose system has a pivot that is not > 0: status 1, every c_e = +0 (so the contributors are the first
 *     entries of the row), baseline = total = +0; a padding target: contributors -1, everything else +0
 * The workgroups are rk_als_foldin's (a row a workgroup at h > 64, four rows below); a row's targets are taken one
 * after the other, the c_e of a target go through the workspace at their entry's index, and the row's first wave
 * selects.  One launch on `stream`, no atomics.  A (row, target) pair's result depends on the row's entries, the
 * target, Y, G, v, bias and alpha alone: not on the other rows or targets, on rows, J or the launch.  -2 unless
 * 1 <= h <= rk_als_foldin_max_h(), ldy >= h, rows >= 0, n_items >= 1, J >= 1, 1 <= m <= 64, alpha finite and >= 0,
 * ws_bytes >= rk_als_explain_workspace_bytes(nnz) and (with rows > 0) no pointer but data and bias is NULL.
 */
int rk_als_explain(const int64_t *indptr, const int32_t *indices, const float *data, int32_t rows, int64_t nnz,
                   const float *Y, int32_t ldy, int32_t n_items, int32_t h, const float *G, const float *v,
                   const float *bias, float alpha, const int64_t *items, int32_t J, int32_t m, int64_t *contributors,
                   float *contributions, float *baseline, float *total, int32_t *status, void *ws, int64_t ws_bytes,
                   void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif /* RECODER_ALS_H */
