// Implicit-feedback ALS (include/recoder_als.h, librecoder_als.so).
//
//   rk_als_gram       G = F^T F + reg I and v = F^T w: split-K over fixed row chunks, each chunk one
//                     k-ascending chain on v_mfma_f32_32x32x2_f32 (upper tile pairs only), then the
//                     chunks added in ascending order and mirrored: bitwise symmetric, no atomics
//   rk_als_solve      one wave per row: the row's factor rows gathered once into LDS (or streamed
//                     when they do not fit), cg_steps CG steps warm-started from the row's value;
//                     G . p from LDS (small h) or from memory (L2).  Rows of >= 512 entries: one
//                     workgroup of 16 waves each, the entries split between the waves
//   rk_als_objective  the sparse part of L, one wave per row, per-row float64 partials; one
//                     workgroup adds them and the Gram terms in a fixed order
//
// BPR pairwise ranking for the same model (rk_als_bpr_*): one synchronous mini-batch SGD step is
//   rk_als_bpr_sample  one thread per slot: a stored entry and a rejected-until-unseen negative, from
//                      a counter hash of (seed, step, slot, draw); integer arithmetic only
//   rk_als_bpr_grad    one wave per triple: x, g = sigma(-x), softplus(-x), and the staging rows
//                      D[t] = q_i - q_j, P[t] = p_u (the apply step then updates the tables in place)
//   rk_als_bpr_apply   one wave per distinct row of the sorted keys: the row's segment summed in
//                      ascending slot order, one fmaf chain per element, then the row's own update.
//                      No atomics: nobody else writes the row
//
// WARP and dynamic negative sampling on the same step (rk_als_rank_sample, rk_als_warp_grad):
//   rk_als_rank_sample  one wave per slot: the sampler's draws 64 at a time, the candidates scored against p_u
//                       several rows in flight, decided in draw order (first margin violator / hardest of M)
//   rk_als_warp_grad    rk_als_bpr_grad's staging rows with g = the rank weight of the slot's trials
//
// LightGCN for the same model (rk_als_lgcn_*): the step of recoder_amd/lightgcn.py adds
//   rk_als_lgcn_propagate  one group of lanes per CSR row: the scaled sum of the row's gathered table rows,
//                          lanes own columns; long rows by a workgroup of 16 waves each, in fixed parts
//   rk_als_lgcn_scatter    the apply's segment walk, writing the gradient rows and the counts
//   rk_als_lgcn_adam       one elementwise pass: the L2 term and the Adam update of a base table
//
// SimGCL on top of it (rk_als_gcl_*): the step of recoder_amd/simgcl.py adds
//   rk_als_gcl_propagate   rk_als_lgcn_propagate's row pass (one template) with a counter-hash noise of length
//                          eps added to every row in the epilogue
//   rk_als_gcl_contrast    InfoNCE between two view tables over the distinct keys of a step: loss and gradient
//                          rows, the T x T scores tiled through LDS; fixed summation orders, no atomics
//
// DirectAU for the same model (rk_als_dau_*): the step of recoder_amd/directau.py adds
//   rk_als_dau_grad        alignment and uniformity over the slots of a step: the three losses and one gradient row
//                          per slot and side, on the contrast's tile code; the T x T weights are stored once and
//                          staged as they are by one dZ product per side
//
// Sampled softmax for the same model (rk_als_ssm_*): the step of recoder_amd/ssm.py adds
//   rk_als_ssm_grad        the softmax of every slot over the batch's positives and S shared uniform negatives: the
//                          T x (T + S) scores and both gradient products on the f32 MFMA through LDS, one expf per
//                          element; fixed summation orders, no atomics
//
// UltraGCN for the same model (rk_als_ugcn_*): the step of recoder_amd/ultragcn.py adds
//   rk_als_ugcn_grad       the constraint loss of every slot over its positive, R private uniform negatives and the
//                          positive's K neighbours: one wave per slot, the candidates' rows gathered several at a
//                          time by lane groups of 16, 32 or 64, the loss terms and DU in ascending candidate order
//   rk_als_ugcn_scatter    the item side, the entry scatter: the scatter's segment walk with the user rows gathered
//                          through the slot, a key of RK_ALS_UGCN_LONG_KEY entries or more by a workgroup of 16 waves
//                          in fixed parts
// als/ugcn.h also holds what the losses with private per-slot negatives share: the candidate round of the grad kernels
// (the draw, the round's gather, the way back to the owning lane; dispatch_group picks the lane groups) and the
// entry scatter's one pair of kernels and one launcher.
//
// SimpleX's cosine contrastive loss for the same model (rk_als_ccl_*): the step of recoder_amd/ccl.py adds
//   rk_als_ccl_grad        the hinge on the cosine of every slot over its positive and R private uniform negatives
//                          (ugcn.h's candidate round): norm and dot product from one gathered copy of a row, a dead
//                          negative dropped at once, a live row used for DU while it is in registers
//   rk_als_ccl_scatter     the entry scatter (the same kernels, SELF) over the keys of the live entries only (the dead
//                          carry a sentinel that sorts last), with the row's own -sum self Y[key] term
//
// SimpleX's history-pooled user rows under that loss (rk_als_sx_*): the step of recoder_amd/simplex.py adds
//   rk_als_sx_forward      one wave per slot: the user's history (the whole row, or max_history entries spread over it)
//                          gathered several rows at a time and averaged, the h x h map W through an LDS tile the
//                          workgroup's four slots share, the mix with the user's own row; the history's entry list in
//                          the entry scatter's layout
//   rk_als_sx_backward     dB = scale W^T DU per slot and dW = scale DU^T B in fixed chunks of 256 slots, the chunks added
//                          in ascending order by a second launch
//
// Ranking metrics on device-resident top-k lists (rk_als_rank_metrics): what recoder_amd/validation.py reads per epoch
//   rk_als_rank_metrics    one wave per user: a binary search of each rank's id in the user's target row, a ballot per
//                          64 ranks, Recall / NDCG / AP summed in float64 in ascending rank order; a second launch of
//                          one workgroup adds the users in a fixed order.  No atomics
//
// Fold-in of a user the fit has not seen (rk_als_foldin): what recoder_amd/foldin.py calls per batch of histories
//   rk_als_foldin          the user-side normal equations of a history solved exactly: A = G + the entries' outer
//                          products in register tiles of the lower triangle, a right-looking Cholesky on the packed
//                          triangle in LDS, both triangular solves by columns; one workgroup a row at h > 64, four rows
//                          a workgroup below; h <= 128.  No atomics, no workspace
//
// iALS++ for the same model (rk_als_ials_*): the sweep of recoder_amd/ials.py adds
//   rk_als_ials_predict     the prediction cache c[e] = x_u . y_i of every stored entry, a wave's dot chain per entry
//   rk_als_ials_block       one block of k <= 128 coordinates of every row solved exactly against the cache: the fold-in's
//                          register tiles, Cholesky and solves on a k x k system, a long row cut over one workgroup in
//                          fixed parts, then the row's cache entries
//   rk_als_ials_gram_panel  the k rows F[:, pi]^T F of a Gram in fixed row chunks; rk_als_ials_objective: L in float64
//
// NeuMF (rk_als_ncf_*): the step of recoder_amd/ncf.py and the scores of nn.NeuralMatrixFactorization add
//   rk_als_ncf_step         forward, loss and backward of a tile of 32 entries in one workgroup: the MLP on 16 x 16 tiles
//                           of the f32 MFMA against weights in LDS, gradient rows per entry, a slab of dense partials
//   rk_als_ncf_dense_adam   the slabs added in tile order and Adam on every dense parameter, one launch
//   rk_als_ncf_item_part    the items' half of layer 1, once per model state
//   rk_als_ncf_scores       a strip of scores for a batch of user ids: layer 1 as a sum of halves, the rest on MFMA tiles
//                           of 32 items, no [B, strip, .] intermediate
//
// Constrained serving (rk_als_serve_mask, rk_als_pair_scores, rk_als_pairs_topk): what recoder_amd/serve.py adds
//   rk_als_serve_mask       the per-row deny bitmap rk_topk_masked reads, from the seen entries, a catalogue bitmap and
//                           per-row allow / deny lists: integer atomicAnd / atomicOr on the row's words, then the count
//   rk_als_pair_scores      z_r . Y[c] + b[c] of ragged candidate lists, lane groups by h, several rows in flight
//   rk_als_pairs_topk       the ragged top-k of those lists with -1 / -inf padding from the count of eligible entries
//
// Explanations (rk_als_explain): what recoder_amd/explain.py adds for the folded-in user
//   rk_als_explain          the fold-in's system and factor, then per target z = A^-1 y_j, a dot chain per history entry
//                           and the m largest contributions, selected by the row's first wave
//
// One translation unit (one last-error buffer, one anonymous namespace), laid out by family under als/: every file
// holds its kernels, then its extern "C" entry points.
#include "als/common.h"     // the lane layout, the counter hash, the segment walk, the NT and lane-group dispatch
#include "als/solve.h"      // rk_als_gram, rk_als_solve, rk_als_objective
#include "als/pairwise.h"   // rk_als_bpr_*, rk_als_rank_sample, rk_als_warp_grad
#include "als/lgcn.h"       // rk_als_lgcn_*, rk_als_gcl_propagate
#include "als/contrast.h"   // rk_als_gcl_contrast, rk_als_dau_*
#include "als/ssm.h"        // rk_als_ssm_*
#include "als/ugcn.h"       // rk_als_ugcn_*, the candidate round, the entry scatter
#include "als/ccl.h"        // rk_als_ccl_* (on ugcn.h)
#include "als/simplex.h"    // rk_als_sx_* (beside ccl.h's loss)
#include "als/metrics.h"    // rk_als_rank_metrics
#include "als/foldin.h"     // rk_als_foldin (beside solve.h's row solves)
#include "als/ials.h"       // rk_als_ials_* (the fold-in's solve on a block of coordinates)
#include "als/ncf.h"        // rk_als_ncf_* (on ugcn.h's draw)
#include "als/serve.h"      // rk_als_serve_mask, rk_als_pair_scores, rk_als_pairs_topk
#include "als/explain.h"    // rk_als_explain (on foldin.h's system and solves)

extern "C" int rk_als_version(void) { return 100; }
extern "C" const char *rk_als_last_error(void) { return g_rk_side_err; }
extern "C" int rk_als_max_h(void) { return MAX_H; }
