"""ctypes binding of librecoder_slim.so (the C ABI in include/recoder_slim.h): the SLIM kernels
for recoder_amd.slim.  Like _lib.py: plain pointers and sizes, no torch types across the boundary,
no CPU fallback."""
import os

# PyTorch-ROCm loads its HIP runtime first (see _lib.py): one runtime instance per process
import torch  # noqa: F401

from ctypes import c_char_p, c_float, c_int32, c_int64, c_void_p

from ._lib import checker, loader

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librecoder_slim.so")

_P = c_void_p

# name -> (restype, argtypes); every symbol include/recoder_slim.h declares
SIGNATURES = {
  "rk_slim_version": (c_int32, []),
  "rk_slim_last_error": (c_char_p, []),
  "rk_slim_max_neighbours": (c_int32, []),
  "rk_slim_lds_candidates": (c_int32, []),
  "rk_slim_fit_workspace_bytes": (c_int64, [c_int32]),
  "rk_slim_fit": (c_int32, [_P, c_int64, c_int32, _P, c_float, c_int32, c_int32, c_float, c_int32, c_int32, _P, _P, _P,
                            _P, _P, _P, c_int64, _P]),
  "rk_slim_sparse_lds_candidates": (c_int32, []),
  "rk_slim_fit_sparse_workspace_bytes": (c_int64, [c_int32]),
  "rk_slim_fit_sparse": (c_int32, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, _P, _P, c_int32, _P, c_float, c_int32,
                                   c_int32, c_float, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, c_int64, _P]),
  "rk_slim_scores": (c_int32, [_P, _P, _P, c_int32, c_int32, _P, _P, _P, c_int32, c_int32, c_int32, _P, c_int64, _P]),
  "rk_slim_explain": (c_int32, [_P, _P, _P, c_int32, c_int32, _P, _P, _P, c_int32, c_int32, _P, c_int32, c_int32, _P, _P,
                                _P, _P, _P]),
}

load = loader(LIB_PATH, SIGNATURES)
check = checker(load, "rk_slim_last_error")
