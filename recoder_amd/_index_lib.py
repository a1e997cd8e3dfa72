"""ctypes binding of librecoder_index.so (the C ABI in include/recoder_index.h): exact item
similarity for recoder_amd.embedding.  Like _lib.py: plain pointers and sizes, no torch types
across the boundary, no CPU fallback."""
import os

# PyTorch-ROCm loads its HIP runtime first (see _lib.py): one runtime instance per process
import torch  # noqa: F401

from ctypes import c_char_p, c_float, c_int32, c_void_p

from ._lib import checker, loader

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librecoder_index.so")

_P = c_void_p

# name -> (restype, argtypes); every symbol include/recoder_index.h declares
SIGNATURES = {
  "rk_ix_version": (c_int32, []),
  "rk_ix_last_error": (c_char_p, []),
  "rk_ix_normalize": (c_int32, [_P, c_int32, c_int32, c_int32, _P, c_int32, _P]),
  "rk_ix_scores": (c_int32, [_P, c_int32, c_int32, _P, c_int32, c_int32, c_int32, c_int32, _P, c_int32, _P]),
  "rk_ix_pool_scores": (c_int32, [_P, c_int32, c_int32, _P, _P, c_int32, _P, _P, c_int32, c_float, _P, _P]),
}

load = loader(LIB_PATH, SIGNATURES)
check = checker(load, "rk_ix_last_error")
