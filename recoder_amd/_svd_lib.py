"""ctypes binding of librecoder_svd.so (the C ABI in include/recoder_svd.h): the randomized truncated
SVD behind recoder_amd.svd.  Like _als_lib.py: plain pointers and sizes, no torch types across the
boundary, no CPU fallback."""
import os

# PyTorch-ROCm loads its HIP runtime first (see _lib.py): one runtime instance per process
import torch  # noqa: F401

from ctypes import c_char_p, c_int32, c_int64, c_uint64, c_void_p

from ._lib import checker, loader

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librecoder_svd.so")

_P = c_void_p

LONG_ROW = 512        # RK_SVD_LONG_ROW

# name -> (restype, argtypes); every symbol include/recoder_svd.h declares
SIGNATURES = {
  "rk_svd_version": (c_int32, []),
  "rk_svd_last_error": (c_char_p, []),
  "rk_svd_max_l": (c_int32, []),
  "rk_svd_gaussian": (c_int32, [_P, c_int32, c_int32, c_int32, c_uint64, _P]),
  "rk_svd_spmm": (c_int32, [_P, _P, _P, c_int32, c_int32, _P, c_int32, c_int32, _P, c_int32, _P]),
  "rk_svd_chol_inverse_workspace_bytes": (c_int64, [c_int32]),
  "rk_svd_chol_inverse": (c_int32, [_P, c_int32, _P, _P, c_int64, _P, _P]),
  "rk_svd_rotate": (c_int32, [_P, c_int32, c_int32, c_int32, _P, c_int32, c_int32, _P, c_int32, _P]),
}

load = loader(LIB_PATH, SIGNATURES)
check = checker(load, "rk_svd_last_error")
