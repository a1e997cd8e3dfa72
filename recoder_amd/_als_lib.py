"""ctypes binding of librecoder_als.so (the C ABI in include/recoder_als.h): implicit-feedback ALS
for recoder_amd.als, the BPR step (rk_als_bpr_*) for recoder_amd.bpr, the WARP / DNS sampler and WARP's
gradient (rk_als_rank_sample, rk_als_warp_grad) for recoder_amd.warp, the LightGCN kernels
(rk_als_lgcn_*) for recoder_amd.lightgcn, SimGCL's (rk_als_gcl_*) for recoder_amd.simgcl, DirectAU's
(rk_als_dau_*) for recoder_amd.directau, the sampled softmax's (rk_als_ssm_*) for recoder_amd.ssm, UltraGCN's (rk_als_ugcn_*) for
recoder_amd.ultragcn, the cosine contrastive loss' (rk_als_ccl_*) for recoder_amd.ccl and SimpleX's pooled user rows
(rk_als_sx_*) for recoder_amd.simplex, and the ranking metrics of device-resident top-k lists (rk_als_rank_metrics) for recoder_amd.metrics
and recoder_amd.validation, the exact fold-in of unseen users (rk_als_foldin) for recoder_amd.foldin, and the iALS++ kernels
(rk_als_ials_*) for recoder_amd.ials, and NeuMF's step and scores (rk_als_ncf_*) for recoder_amd.ncf, and the
constrained-serving kernels (rk_als_serve_mask, rk_als_pair_scores, rk_als_pairs_topk) for recoder_amd.serve.  Like _lib.py: plain pointers and sizes, no torch types across the boundary, no CPU fallback."""
import os

# PyTorch-ROCm loads its HIP runtime first (see _lib.py): one runtime instance per process
import torch  # noqa: F401

from ctypes import c_char_p, c_float, c_int32, c_int64, c_void_p

from ._lib import checker, loader

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librecoder_als.so")

_P = c_void_p

FORCE_STREAM = 1      # RK_ALS_FORCE_STREAM
G_GLOBAL = 2          # RK_ALS_G_GLOBAL
LGCN_LONG_ROW = 1024  # RK_ALS_LGCN_LONG_ROW
GCL_MAX_BATCH = 4096  # RK_ALS_GCL_MAX_BATCH
SSM_MAX_BATCH, SSM_MAX_NEGATIVES = 4096, 4096  # RK_ALS_SSM_MAX_BATCH, RK_ALS_SSM_MAX_NEGATIVES
UGCN_MAX_BATCH, UGCN_MAX_NEGATIVES, UGCN_MAX_NEIGHBOURS = 4096, 1024, 64  # RK_ALS_UGCN_MAX_BATCH, _NEGATIVES, _NEIGHBOURS
UGCN_MAX_ENTRIES, UGCN_LONG_KEY = 1 << 22, 1024  # RK_ALS_UGCN_MAX_ENTRIES, RK_ALS_UGCN_LONG_KEY
CCL_MAX_BATCH, CCL_MAX_NEGATIVES, CCL_MAX_ENTRIES = 4096, 1024, 1 << 22  # RK_ALS_CCL_MAX_BATCH, _NEGATIVES, _ENTRIES
SX_MAX_HISTORY, SX_CHUNK = 1024, 256  # RK_ALS_SX_MAX_HISTORY, RK_ALS_SX_CHUNK
RANK_MAX_DRAWS = 256  # RK_ALS_RANK_MAX_DRAWS
RANK_WARP, RANK_DNS = 0, 1  # RK_ALS_RANK_WARP, RK_ALS_RANK_DNS
METRIC_RECALL, METRIC_NDCG, METRIC_AP = 0, 1, 2  # RK_ALS_METRIC_RECALL, _NDCG, _AP
RANK_METRICS_MAX = 8  # RK_ALS_RANK_METRICS_MAX
FOLDIN_MAX_H = 128  # rk_als_foldin_max_h()
IALS_MAX_H, IALS_MAX_BLOCK, IALS_LONG_ROW = 2048, 128, 1024  # rk_als_ials_max_h(), _max_block(), RK_ALS_IALS_LONG_ROW
NCF_TILE, NCF_MAX_WIDTH, NCF_MAX_LAYERS = 32, 128, 3  # RK_ALS_NCF_TILE, _MAX_WIDTH, _MAX_LAYERS
PAIRS_TOPK_MAX_ROW = 8192  # rk_als_pairs_topk_max_row()

# name -> (restype, argtypes); every symbol include/recoder_als.h declares
SIGNATURES = {
  "rk_als_version": (c_int32, []),
  "rk_als_last_error": (c_char_p, []),
  "rk_als_max_h": (c_int32, []),
  "rk_als_gram_workspace_bytes": (c_int64, [c_int32, c_int32]),
  "rk_als_gram": (c_int32, [_P, c_int32, c_int32, c_int32, _P, c_float, _P, _P, _P, c_int64, _P]),
  "rk_als_solve": (c_int32, [_P, _P, _P, c_int32, c_int32, _P, c_int32, c_int32, _P, _P, _P, _P, c_float,
                             c_int32, _P, c_int32, c_int32, _P]),
  "rk_als_objective_workspace_bytes": (c_int64, [c_int32]),
  "rk_als_objective": (c_int32, [_P, _P, _P, c_int32, c_int32, _P, c_int32, _P, c_int32, c_int32, _P, c_float,
                                 c_float, _P, _P, _P, _P, _P, c_int64, _P, _P]),
  "rk_als_bpr_workspace_bytes": (c_int64, [c_int32, c_int32]),
  "rk_als_bpr_sample": (c_int32, [_P, _P, c_int32, c_int32, c_int64, c_int64, c_int32, c_int32, _P, _P, _P, _P]),
  "rk_als_bpr_grad": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, _P, c_int32, _P, c_int32, _P, c_int32,
                                _P, _P, _P, _P, _P, _P]),
  "rk_als_bpr_apply": (c_int32, [_P, _P, c_int32, c_int32, _P, _P, c_int32, c_float, c_float, c_int32, _P,
                                 c_int32, _P, _P]),
  "rk_als_rank_sample": (c_int32, [_P, _P, c_int32, c_int32, c_int64, c_int64, c_int32, c_int32, _P, c_int32, _P,
                                   c_int32, _P, c_int32, c_int32, c_int32, c_int32, c_float, _P, _P, _P, _P, _P,
                                   _P, _P, _P]),
  "rk_als_warp_grad": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, _P, c_int32, _P, c_int32, _P, c_int32,
                                 c_float, _P, _P, _P, _P, _P, _P]),
  "rk_als_lgcn_propagate": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, _P, c_int32, c_int32, _P, c_int32, _P,
                                      c_int32, c_float, _P]),
  "rk_als_lgcn_scatter": (c_int32, [_P, _P, c_int32, c_int32, _P, _P, c_int32, c_float, c_int32, _P, c_int32, _P,
                                    _P]),
  "rk_als_lgcn_adam": (c_int32, [_P, c_int32, _P, c_int32, _P, c_float, _P, _P, c_int32, c_int32, c_float, c_float,
                                 c_float, c_float, c_int32, _P]),
  "rk_als_gcl_propagate": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, _P, c_int32, c_int32, _P, c_int32, _P,
                                     c_int32, c_float, c_float, c_int64, c_int32, c_int32, c_int32, c_int32, _P]),
  "rk_als_gcl_contrast_workspace_bytes": (c_int64, [c_int32, c_int32]),
  "rk_als_gcl_contrast": (c_int32, [_P, c_int32, c_int32, _P, c_int32, _P, c_int32, c_int32, c_float, c_float, _P,
                                    c_int32, _P, c_int32, _P, c_int64, _P, _P, _P]),
  "rk_als_dau_workspace_bytes": (c_int64, [c_int32, c_int32]),
  "rk_als_dau_grad": (c_int32, [_P, _P, c_int32, c_int32, c_int32, _P, c_int32, _P, c_int32, c_int32, c_float, _P,
                                c_int64, _P, _P, _P, _P, _P, _P]),
  "rk_als_ssm_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
  "rk_als_ssm_grad": (c_int32, [_P, _P, c_int32, c_int32, c_int64, c_int32, c_int32, c_int32, _P, c_int32, _P,
                                c_int32, c_int32, c_float, c_int32, _P, _P, c_int64, _P, _P, _P, _P, _P, _P, _P, _P]),
  "rk_als_ugcn_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
  "rk_als_ugcn_grad": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int64, c_int32, c_int32, c_int32, _P, c_int32,
                                 _P, c_int32, c_int32, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float,
                                 c_float, _P, _P, _P, _P, _P, _P]),
  "rk_als_ugcn_scatter": (c_int32, [_P, _P, c_int32, c_int32, _P, _P, _P, c_int32, c_int32, c_int32, c_float, c_int32,
                                    _P, c_int32, _P, _P]),
  "rk_als_ccl_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
  "rk_als_ccl_grad": (c_int32, [_P, _P, c_int32, c_int32, c_int64, c_int32, c_int32, c_int32, _P, c_int32, _P, c_int32,
                                c_int32, c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
  "rk_als_ccl_scatter": (c_int32, [_P, _P, c_int32, c_int32, _P, _P, _P, _P, c_int32, c_int32, _P, c_int32, c_int32,
                                   c_float, c_int32, _P, c_int32, _P, _P]),
  "rk_als_sx_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
  "rk_als_sx_forward": (c_int32, [_P, c_int32, _P, _P, c_int32, c_int32, _P, c_int32, _P, c_int32, _P, c_int32, c_int32,
                                  c_float, c_int32, c_int32, _P, _P, c_int32, c_int32, _P, _P, _P]),
  "rk_als_sx_backward": (c_int32, [_P, _P, _P, c_int32, _P, c_int32, c_int32, c_float, _P, _P, _P, _P]),
  "rk_als_rank_metrics": (c_int32, [_P, c_int32, c_int32, c_int64, _P, _P, c_int64, c_int32, _P, _P, _P, _P, _P, _P,
                                    _P, _P, _P]),
  "rk_als_foldin_max_h": (c_int32, []),
  "rk_als_foldin": (c_int32, [_P, _P, _P, c_int32, _P, c_int32, c_int32, _P, _P, _P, c_float, _P, c_int32, _P, _P]),
  "rk_als_ials_max_h": (c_int32, []),
  "rk_als_ials_max_block": (c_int32, []),
  "rk_als_ials_predict": (c_int32, [_P, _P, c_int32, c_int64, _P, c_int32, _P, c_int32, c_int32, _P, _P]),
  "rk_als_ials_block": (c_int32, [_P, _P, _P, c_int32, c_int32, _P, c_int32, _P, c_int32, _P, c_int32, c_int32, _P,
                                  c_int32, _P, c_float, c_int32, c_int32, _P, _P, _P]),
  "rk_als_ials_panel_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
  "rk_als_ials_gram_panel": (c_int32, [_P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, c_int32, _P, c_int64, _P]),
  "rk_als_ials_objective_workspace_bytes": (c_int64, []),
  "rk_als_ials_objective": (c_int32, [_P, c_int64, _P, _P, c_int32, _P, c_int32, c_int32, _P, _P, c_int32, c_int32, _P,
                                      c_float, _P, c_int64, _P, _P]),
  "rk_als_ncf_dense_count": (c_int64, [c_int32] * 6),
  "rk_als_ncf_lds_bytes": (c_int64, [c_int32] * 7),
  "rk_als_ncf_workspace_bytes": (c_int64, [c_int32] * 8),
  "rk_als_ncf_step": (c_int32, [_P, _P, c_int32, c_int32, c_int64, c_int32, c_int32, c_int32, _P, c_int32, _P, c_int32,
                                _P, c_int32, _P, c_int32, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P,
                                _P, _P, _P, _P, _P]),
  "rk_als_ncf_dense_adam": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                      c_int32, c_float, c_float, c_float, c_float, c_float, c_int32, _P, _P]),
  "rk_als_ncf_item_part": (c_int32, [_P, c_int32, c_int32, _P, c_int32, c_int32, _P, _P]),
  "rk_als_ncf_scores": (c_int32, [_P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, c_int32, _P, c_int32, _P,
                                  c_int32, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P,
                                  c_int64, _P]),
  "rk_als_serve_mask": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, c_int64, _P, _P, _P, _P, c_int64, _P, _P,
                                  c_int64, _P, _P, _P]),
  "rk_als_pair_scores": (c_int32, [_P, _P, c_int64, c_int32, c_int32, _P, c_int32, _P, c_int32, c_int32, c_int32, _P,
                                   _P, c_int32, _P, _P]),
  "rk_als_explain_workspace_bytes": (c_int64, [c_int64]),
  "rk_als_explain": (c_int32, [_P, _P, _P, c_int32, c_int64, _P, c_int32, c_int32, c_int32, _P, _P, _P, c_float, _P,
                               c_int32, c_int32, _P, _P, _P, _P, _P, _P, c_int64, _P]),
  "rk_als_pairs_topk_max_row": (c_int32, []),
  "rk_als_pairs_topk": (c_int32, [_P, _P, _P, c_int64, c_int32, c_int32, c_int32, _P, c_int32, c_int32, _P, _P,
                                  c_int32, _P, _P]),
}

load = loader(LIB_PATH, SIGNATURES)
check = checker(load, "rk_als_last_error")
