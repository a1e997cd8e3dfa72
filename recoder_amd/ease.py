"""EASE (Steck 2019, "Embarrassingly Shallow Autoencoders for Sparse Data") for ``ShallowAutoencoder``,
on the HIP kernels of librecoder_ease.so (include/recoder_ease.h).

For the user x item matrix X (values as stored), reg > 0 and n items:

    G = X^T X,   P = (G + reg I)^-1,   B[i, j] = -P[i, j] / P[j, j] (i != j),   B[j, j] = 0

and a user's scores are ``X[u, :] @ B``.  The fit is closed-form: one sparse Gram, one dense SPD
inverse, one element-wise pass, all in the n x n buffer that ends up holding B.

``Recoder.train_ease`` is the public entry point; the functions below are the layer under it (and what
the tests and tools/ease_bench.py drive directly).
"""
import math

import torch

from . import _ease_lib, als
from ._lib import ptr
from .device import DEVICE_HBM_BYTES, current_stream

_INV_NB, _INV_TILE = 64, 128       # (the block width and update tile of rk_ease_spd_inverse)


def check_not_distributed():
  als.check_not_distributed("train_ease runs on one GPU: a multi-GPU EASE fit is not implemented")


def check_config(model, reg):
  """The EASE contract, checked before any GPU work; returns reg."""
  from .nn import ShallowAutoencoder
  if not isinstance(model, ShallowAutoencoder):
    raise ValueError("train_ease fits a ShallowAutoencoder, not %s" % type(model).__name__)
  return check_reg(reg)


def check_reg(reg):
  reg = float(reg)
  if not (math.isfinite(reg) and reg > 0):
    raise ValueError("reg must be finite and > 0 (got %r)" % (reg,))
  return reg


def inverse_workspace_bytes(n):
  """rk_ease_spd_inverse_workspace_bytes(n), restated on the host (the memory check needs no library)."""
  ldw = -(-int(n) // _INV_TILE) * _INV_TILE
  return 2 * _INV_NB * ldw * 4 + _INV_NB * _INV_NB * 8 + int(n) * int(n) * 4


def required_bytes(n, allocate_matrix=True):
  """Device bytes a fit over n items allocates: the n x n fp32 matrix (unless the caller already holds
  it), the inverse's workspace (a second n x n image: the carries of its compensated update), diag(P) and
  the status word."""
  n = int(n)
  return (n * n * 4 if allocate_matrix else 0) + inverse_workspace_bytes(n) + n * 4 + 4


def check_memory(n, free_bytes=None, allocate_matrix=True):
  """ValueError naming n and the bytes needed when the fit cannot fit: against one device's whole HBM
  without touching a device, then (``free_bytes`` None: asked from the current device) against what
  is free."""
  n = int(n)
  if n < 1:
    raise ValueError("EASE needs at least one item (got n = %d)" % n)
  whole = required_bytes(n, True)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError("EASE over n = %d items needs %d bytes for its n x n fp32 matrix and workspace: more than "
                     "one device's memory (%d bytes); multi-device fits are not implemented"
                     % (n, whole, DEVICE_HBM_BYTES))
  if n >= 2 ** 31 // 256:
    raise ValueError("EASE over n = %d items is outside the kernels' index range" % n)
  need = required_bytes(n, allocate_matrix)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("EASE over n = %d items needs %d bytes of device memory, %d are free"
                     % (n, need, free_bytes))
  return need


# ------------------------------------------------------------------ kernels
def gram(ucsr, icsr, reg, out=None):
  """A = X^T X + reg I [n, n] f32 from the user-major and item-major CSRs of ``als.csr_pair`` (rk_ease_gram)."""
  lib = _ease_lib.load()
  n_users, n = ucsr.shape
  assert icsr.shape == (n, n_users)
  if out is None:
    out = torch.empty(n, n, dtype=torch.float32, device=ucsr.indptr.device)
  assert out.shape == (n, n) and out.dtype == torch.float32 and out.stride(1) == 1
  _ease_lib.check(lib.rk_ease_gram(ptr(icsr.indptr), ptr(icsr.indices), ptr(icsr.data), ptr(ucsr.indptr),
                                   ptr(ucsr.indices), ptr(ucsr.data), n_users, n, float(reg), ptr(out),
                                   out.stride(0), current_stream()), "rk_ease_gram")
  return out


def spd_inverse_async(A, status, ws=None):
  """A <- A^-1 in place (rk_ease_spd_inverse); ``status`` (int32 [1], device) is left for the caller to read."""
  lib = _ease_lib.load()
  n = A.shape[0]
  assert A.shape == (n, n) and A.dtype == torch.float32 and A.stride(1) == 1
  need = lib.rk_ease_spd_inverse_workspace_bytes(n)
  if ws is None or ws.numel() < need:
    ws = torch.empty(need, dtype=torch.uint8, device=A.device)
  _ease_lib.check(lib.rk_ease_spd_inverse(ptr(A), n, A.stride(0), ptr(ws), ws.numel(), ptr(status),
                                          current_stream()), "rk_ease_spd_inverse")
  return ws


def raise_on_status(status):
  """The one read-back of the fit: ValueError when a pivot was not positive."""
  s = int(status.cpu().item())
  if s:
    raise ValueError("the matrix is not positive definite: pivot %d of the elimination is not > 0 "
                     "(an item nobody touched needs reg > 0)" % (s - 1))


def spd_inverse(A):
  """In-place inverse of the SPD matrix A; ValueError when a pivot is not positive."""
  status = torch.zeros(1, dtype=torch.int32, device=A.device)
  spd_inverse_async(A, status)
  raise_on_status(status)
  return A


def finalize(P, out=None):
  """(B, diag(P)): B = -P / diag(P) by columns with a zero diagonal, in place when ``out`` is None
  (rk_ease_finalize)."""
  lib = _ease_lib.load()
  n = P.shape[0]
  out = P if out is None else out
  assert P.shape == out.shape == (n, n) and P.stride(1) == 1 and out.stride(1) == 1
  diag = torch.empty(n, dtype=torch.float32, device=P.device)
  _ease_lib.check(lib.rk_ease_finalize(ptr(P), n, P.stride(0), ptr(out), out.stride(0), ptr(diag),
                                       current_stream()), "rk_ease_finalize")
  return out, diag


def scores(csr, W, lo=0, hi=None, out=None, ld=None, n_rows=None):
  """out[u, c] = sum_j x_uj W[j, lo + c] over the stored entries of CSR row u, ascending (rk_ease_scores).
  ``csr``: anything with int64 ``indptr``, int32 ``indices`` and fp32 ``data`` (or None) on the device."""
  lib = _ease_lib.load()
  hi = W.shape[1] if hi is None else hi
  n_rows = csr.shape[0] if n_rows is None else n_rows
  assert W.dtype == torch.float32 and W.stride(1) == 1 and 0 <= lo < hi <= W.shape[1]
  assert csr.shape[1] <= W.shape[0]
  if out is None:
    ld = hi - lo if ld is None else ld
    out = torch.empty(n_rows, ld, dtype=torch.float32, device=W.device)
  ld = out.stride(0) if ld is None else ld
  _ease_lib.check(lib.rk_ease_scores(ptr(csr.indptr), ptr(csr.indices), ptr(csr.data), n_rows, ptr(W),
                                     W.stride(0), lo, hi, ptr(out), ld, current_stream()), "rk_ease_scores")
  return out


# ---------------------------------------------------------------------- fit
def fit(csr_pair, reg, out=None):
  """(B, info) for the (user-major, item-major) CSR pair of ``als.csr_pair``: Gram, inverse and
  finalize in one [n, n] buffer (``out`` when given).  One host synchronisation, at the end; ``info``
  holds n, nnz, reg, the milliseconds of each phase from HIP events and diag(P)."""
  ucsr, icsr = csr_pair
  reg = check_reg(reg)
  check_not_distributed()
  n = ucsr.shape[1]
  check_memory(n, allocate_matrix=out is None)
  dev = ucsr.indptr.device
  status = torch.zeros(1, dtype=torch.int32, device=dev)
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
  ev[0].record()
  A = gram(ucsr, icsr, reg, out)
  ev[1].record()
  spd_inverse_async(A, status)
  ev[2].record()
  B, diag = finalize(A)
  ev[3].record()
  raise_on_status(status)            # (the synchronisation)
  ev[3].synchronize()
  info = dict(n=int(n), nnz=int(ucsr.nnz), reg=reg, gram_ms=ev[0].elapsed_time(ev[1]),
              inverse_ms=ev[1].elapsed_time(ev[2]), finalize_ms=ev[2].elapsed_time(ev[3]), diag=diag)
  return B, info
