"""ctypes binding of librecoder_vae.so (the C ABI in include/recoder_vae.h): the stochastic bottleneck of
recoder_amd.nn.VariationalAutoencoder, sequenced by recoder_amd.engine.  Like _lib.py: plain pointers and
sizes, no torch types across the boundary, no CPU fallback."""
import os

# PyTorch-ROCm loads its HIP runtime first (see _lib.py): one runtime instance per process
import torch  # noqa: F401

from ctypes import c_char_p, c_float, c_int32, c_uint64, c_void_p

from ._lib import checker, loader

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librecoder_vae.so")

_P = c_void_p

SEED_XOR = 0x7ae5a3c1b2d4e6f8     # RK_VAE_SEED_XOR

# name -> (restype, argtypes); every symbol include/recoder_vae.h declares
SIGNATURES = {
  "rk_vae_version": (c_int32, []),
  "rk_vae_last_error": (c_char_p, []),
  "rk_vae_sample": (c_int32, [_P, c_int32, c_int32, c_int32, _P, c_uint64, c_uint64, _P, c_int32, _P, c_int32,
                              _P, c_float, _P, _P, _P, _P]),
  "rk_vae_sample_bwd": (c_int32, [_P, _P, _P, c_int32, c_int32, c_float, _P, c_int32, _P, c_float, _P, _P]),
}

load = loader(LIB_PATH, SIGNATURES)
check = checker(load, "rk_vae_last_error")
