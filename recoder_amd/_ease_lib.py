"""ctypes binding of librecoder_ease.so (the C ABI in include/recoder_ease.h): the EASE kernels
for recoder_amd.ease.  Like _lib.py: plain pointers and sizes, no torch types across the boundary,
no CPU fallback."""
import os

# PyTorch-ROCm loads its HIP runtime first (see _lib.py): one runtime instance per process
import torch  # noqa: F401

from ctypes import c_char_p, c_float, c_int32, c_int64, c_void_p

from ._lib import checker, loader

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librecoder_ease.so")

_P = c_void_p

# name -> (restype, argtypes); every symbol include/recoder_ease.h declares
SIGNATURES = {
  "rk_ease_version": (c_int32, []),
  "rk_ease_last_error": (c_char_p, []),
  "rk_ease_gram": (c_int32, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_float, _P, c_int64, _P]),
  "rk_ease_spd_inverse_workspace_bytes": (c_int64, [c_int32]),
  "rk_ease_spd_inverse": (c_int32, [_P, c_int32, c_int64, _P, c_int64, _P, _P]),
  "rk_ease_finalize": (c_int32, [_P, c_int32, c_int64, _P, c_int64, _P, _P]),
  "rk_ease_scores": (c_int32, [_P, _P, _P, c_int32, _P, c_int64, c_int32, c_int32, _P, c_int64, _P]),
  "rk_ease_lowrank_add": (c_int32, [_P, c_int32, c_int64, _P, c_int32, c_int64, _P, _P, c_float, c_int32, c_int32, _P]),
  "rk_ease_gemm": (c_int32, [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32, c_int32, c_int32, c_float,
                             c_float, c_int32, c_int32, _P]),
  "rk_ease_admm_update": (c_int32, [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int32, c_float,
                                    c_int32, _P, _P, _P, _P, c_int32, c_int32, _P]),
  "rk_ease_elsa_normalize": (c_int32, [_P, c_int64, c_int32, c_int32, _P, c_int64, _P, _P, c_int64, _P]),
  "rk_ease_elsa_rows": (c_int32, [_P, c_int64, _P, c_int64, _P, c_int32, c_int32, c_int32, _P, c_int64, _P, c_int64, _P,
                                  _P, _P]),
  "rk_ease_elsa_scatter": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, _P, c_int64, c_int32, _P, c_int64, _P]),
  "rk_ease_elsa_project": (c_int32, [_P, c_int64, _P, c_int64, _P, c_int32, c_int32, _P, c_int64, _P]),
  "rk_ease_elsa_adam": (c_int32, [_P, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P, c_int32, c_int32, c_float, c_float,
                                  c_float, c_float, c_float, _P]),
  "rk_ease_csr_sub": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, _P, c_int64, _P]),
  "rk_ease_explain_max_contributors": (c_int32, []),
  "rk_ease_explain": (c_int32, [_P, _P, _P, c_int32, _P, c_int64, c_int32, _P, c_int32, c_int32, _P, _P, _P, _P, _P]),
}

load = loader(LIB_PATH, SIGNATURES)
check = checker(load, "rk_ease_last_error")
