"""ctypes binding of librecoder_rp3.so (the C ABI in include/recoder_rp3.h): the RP3beta kernels
for recoder_amd.rp3, the user-neighbourhood kernels for recoder_amd.userknn and the item-neighbourhood fit for
recoder_amd.itemknn.  Like _lib.py: plain pointers and sizes, no torch types across the boundary,
no CPU fallback."""
import os

# PyTorch-ROCm loads its HIP runtime first (see _lib.py): one runtime instance per process
import torch  # noqa: F401

from ctypes import c_char_p, c_float, c_int32, c_int64, c_void_p

from ._lib import checker, loader

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librecoder_rp3.so")

_P = c_void_p

# name -> (restype, argtypes); every symbol include/recoder_rp3.h declares
SIGNATURES = {
  "rk_rp3_version": (c_int32, []),
  "rk_rp3_last_error": (c_char_p, []),
  "rk_rp3_max_neighbours": (c_int32, []),
  "rk_rp3_lds_items": (c_int32, []),
  "rk_rp3_fit_workspace_bytes": (c_int64, [c_int32]),
  "rk_rp3_fit": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, _P, _P, _P, c_int32, c_int32, c_int32, _P, _P, _P, _P,
                           c_int64, _P]),
  "rk_rp3_scores": (c_int32, [_P, _P, _P, c_int32, c_int32, _P, _P, _P, c_int32, c_int32, c_int32, _P, c_int64, _P]),
  "rk_rp3_user_workspace_bytes": (c_int64, [c_int32]),
  "rk_rp3_user_neighbours": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, _P, _P, c_float, c_int32, c_int32, c_int32, _P,
                                       _P, _P, _P, c_int64, _P]),
  "rk_rp3_user_scores": (c_int32, [_P, _P, _P, c_int32, c_int32, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P,
                                   c_int64, _P]),
  "rk_rp3_item_workspace_bytes": (c_int64, [c_int32]),
  "rk_rp3_item_fit": (c_int32, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, _P, _P, c_int32, c_float, c_float, c_int32,
                                c_int32, c_int32, _P, _P, _P, _P, c_int64, _P]),
}

load = loader(LIB_PATH, SIGNATURES)
check = checker(load, "rk_rp3_last_error")
