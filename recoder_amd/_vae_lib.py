"""ctypes binding of librecoder_vae.so (the C ABI in include/recoder_vae.h): the stochastic bottleneck of
recoder_amd.nn.VariationalAutoencoder, sequenced by recoder_amd.engine.  Like _lib.py: plain pointers and
sizes, no torch types across the boundary, no CPU fallback."""
import ctypes
import os

# PyTorch-ROCm loads its HIP runtime first (see _lib.py): one runtime instance per process
import torch  # noqa: F401

from ctypes import c_char_p, c_float, c_int32, c_uint64, c_void_p

from ._lib import RecoderHipError

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

_lib = None


def load():
  """Load the VAE library (once) and bind every declared symbol."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise RecoderHipError(
        "librecoder_vae.so not found at %s -- build it with `python -m recoder_amd.build`" % LIB_PATH)
  lib = ctypes.CDLL(LIB_PATH)
  for name, (res, args) in SIGNATURES.items():
    fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
    fn.restype = res
    fn.argtypes = args
  _lib = lib
  return lib


def check(rc, what=""):
  if rc != 0:
    msg = load().rk_vae_last_error()
    raise RecoderHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))
