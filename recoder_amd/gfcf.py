"""GF-CF (Shen, Wang, Zhang, Shen, Han, Jiang & Gao 2021, "How Powerful is Graph Convolution for
Recommendation?") for ``GraphFilterModel``, on the HIP kernels of librecoder_ease.so (include/recoder_ease.h)
and the randomized SVD of recoder_amd/svd.py.

The stored entries of the user x item matrix are the edges of the bipartite graph LightGCN propagates over
(their values play no part in the fit, as in recoder_amd/rp3.py).  With R the binary matrix, r_u / d_i the
user / item degrees and n items:

    Rn = D_U^-1/2 R D_I^-1/2                       (0 where a degree is 0)
    V [n, rank] = the top right singular vectors of Rn
    W = Rn^T Rn + alpha * D_I^-1/2 V V^T D_I^1/2     (D_I^1/2 is 0 for an item nobody holds)

and a user's scores are ``X[u, :] @ W`` with the user's stored values: a linear filter plus an ideal low-pass
filter, no training.  The fit is one sparse Gram, one randomized SVD and one dense rank-k update, all in the
n x n buffer that ends up holding W.

``Recoder.train_gfcf`` is the public entry point; the functions below are the layer under it (and what the
tests and tools/gfcf_bench.py drive directly).
"""
import math

import numpy as np
import torch

from . import _ease_lib, als, ease, svd
from ._lib import ptr
from .device import DEVICE_HBM_BYTES, current_stream

MAX_RANK = svd.MAX_L


def check_not_distributed():
  als.check_not_distributed("train_gfcf runs on one GPU: a multi-GPU GF-CF fit is not implemented")


def check_params(rank, alpha):
  if not svd._is_int(rank) or rank < 1:
    raise ValueError("rank must be an integer >= 1 (got %r)" % (rank,))
  try:
    alpha = float(alpha)
  except (TypeError, ValueError):
    raise ValueError("alpha must be finite and >= 0 (got %r)" % (alpha,))
  if not (math.isfinite(alpha) and alpha >= 0):
    raise ValueError("alpha must be finite and >= 0 (got %r)" % (alpha,))
  return int(rank), alpha


def check_config(model, rank, alpha, oversample=16, num_power_iterations=6, seed=0):
  """The GF-CF contract, checked before any GPU work; returns (rank, alpha, l)."""
  from .nn import GraphFilterModel
  if not isinstance(model, GraphFilterModel):
    raise ValueError("train_gfcf fits a GraphFilterModel, not %s" % type(model).__name__)
  rank, alpha = check_params(rank, alpha)
  if not svd._is_int(oversample) or oversample < 0:
    raise ValueError("oversample must be an integer >= 0 (got %r)" % (oversample,))
  if rank + oversample > MAX_RANK:
    raise ValueError("rank + oversample must be at most %d (got %d + %d)" % (MAX_RANK, rank, oversample))
  if not svd._is_int(num_power_iterations) or num_power_iterations < 0:
    raise ValueError("num_power_iterations must be an integer >= 0 (got %r)" % (num_power_iterations,))
  if not svd._is_int(seed):
    raise ValueError("seed must be an integer (got %r)" % (seed,))
  return rank, alpha, int(rank + oversample)


def required_bytes(n_users, n_items, l, nnz, allocate_matrix=True):
  """Device bytes a fit allocates: the n x n fp32 matrix (unless the caller already holds it), the buffers of
  ``svd.required_bytes`` (which count both CSRs with their values: the normalised pair), the [users, rank] and
  [items, rank] tables of the SVD (counted at l), and the three scale vectors.  No second n x n image."""
  n_users, n, l, nnz = int(n_users), int(n_items), int(l), int(nnz)
  return ((n * n * 4 if allocate_matrix else 0) + svd.required_bytes(n_users, n, l, nnz, with_data=True)
          + (n_users + n) * l * 4 + (n_users + 2 * n) * 4)


def check_memory(n_users, n_items, l, nnz, free_bytes=None, allocate_matrix=True):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's whole HBM
  without touching a device, then (``free_bytes`` None: asked from the current device) against what is free."""
  n_users, n, l, nnz = int(n_users), int(n_items), int(l), int(nnz)
  if n < 1:
    raise ValueError("GF-CF needs at least one item (got n = %d)" % n)
  whole = required_bytes(n_users, n, l, nnz, True)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError("GF-CF over %d users x n = %d items at l = %d needs %d bytes for its n x n fp32 matrix and the "
                     "SVD's buffers: more than one device's memory (%d bytes); multi-device fits are not implemented"
                     % (n_users, n, l, whole, DEVICE_HBM_BYTES))
  if n >= 2 ** 31 // 256:
    raise ValueError("GF-CF over n = %d items is outside the kernels' index range" % n)
  need = required_bytes(n_users, n, l, nnz, allocate_matrix)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("GF-CF over %d users x n = %d items at l = %d needs %d bytes of device memory, %d are free"
                     % (n_users, n, l, need, free_bytes))
  return need


# ------------------------------------------------------------------ kernels
def lowrank_add(A, V, row_scale, col_scale, alpha, row_lo=0, row_hi=None):
  """A[i, j] += (alpha row_scale[i]) (V[i] . V[j]) col_scale[j] for i in [row_lo, row_hi), in place
  (rk_ease_lowrank_add); returns A."""
  lib = _ease_lib.load()
  n, k = V.shape
  row_hi = n if row_hi is None else row_hi
  assert A.shape[0] == n and A.shape[1] == n and A.dtype == V.dtype == torch.float32
  assert (A.stride(1) == 1 or n == 1) and (V.stride(1) == 1 or k == 1)
  assert row_scale.shape == col_scale.shape == (n,) and row_scale.dtype == col_scale.dtype == torch.float32
  assert row_scale.is_contiguous() and col_scale.is_contiguous()
  lda = A.stride(0) if n > 1 else max(n, A.stride(0))
  ldv = V.stride(0) if n > 1 else max(k, V.stride(0))
  _ease_lib.check(lib.rk_ease_lowrank_add(ptr(A), n, lda, ptr(V), k, ldv, ptr(row_scale), ptr(col_scale),
                                          float(alpha), row_lo, row_hi, current_stream()), "rk_ease_lowrank_add")
  return A


# ---------------------------------------------------------------------- fit
def _power(x, e):
  """x^e in float64, rounded once to f32; 0 where x is 0."""
  out = np.zeros_like(x)
  out[x > 0] = x[x > 0] ** float(e)
  return out.astype(np.float32)


def host_scales(csr_pair):
  """(r^-1/2, d^-1/2, d^1/2) from the device CSR pair of ``als.csr_pair`` (the two indptr arrays hold r and d)."""
  ucsr, icsr = csr_pair
  r = np.diff(ucsr.indptr.cpu().numpy()).astype(np.float64)
  d = np.diff(icsr.indptr.cpu().numpy()).astype(np.float64)
  return _power(r, -0.5), _power(d, -0.5), _power(d, 0.5)


class _NormCSR:
  """A CSR that shares the index arrays of an ``als.AlsCSR`` and carries values of its own."""

  def __init__(self, csr, row_w, col_w):
    self.shape, self.nnz, self.indptr, self.indices = csr.shape, csr.nnz, csr.indptr, csr.indices
    dev = csr.indptr.device
    if csr.nnz:
      rows = torch.repeat_interleave(torch.arange(csr.shape[0], device=dev), csr.indptr.diff(), output_size=csr.nnz)
      self.data = row_w[rows] * col_w[csr.indices[:csr.nnz].to(torch.int64)]
    else:
      self.data = torch.zeros(1, dtype=torch.float32, device=dev)


def normalised_pair(csr_pair, ri, di):
  """The CSR pair of Rn = D_U^-1/2 R D_I^-1/2: the index arrays of ``csr_pair``, the values ri[row] * di[col]
  (one f32 multiply; the same product in both CSRs)."""
  ucsr, icsr = csr_pair
  return _NormCSR(ucsr, ri, di), _NormCSR(icsr, di, ri)


def fit(csr_pair, rank, alpha, oversample=16, num_power_iterations=6, seed=0, out=None, omega=None):
  """(W, info) for the (user-major, item-major) CSR pair of ``als.csr_pair``: the Gram of the normalised
  matrix, its randomized SVD and the rank-k update in one [n, n] buffer (``out`` when given).  ``omega``
  ([items, rank + oversample]) replaces the SVD's seeded Gaussian.  One host synchronisation of its own (the
  SVD's small eigendecomposition, where its status word is read too) besides the degrees' read-back at the
  start; ``info`` holds n, nnz, rank, alpha, l, singular_values, ritz_residual, the milliseconds of each phase
  from HIP events and V, the [n, rank] device tensor of the singular vectors."""
  ucsr, icsr = csr_pair
  rank, alpha = check_params(rank, alpha)
  check_not_distributed()
  n_users, n = ucsr.shape
  l = rank + int(oversample)
  svd.check_rank(l, n_users, n)
  check_memory(n_users, n, l, ucsr.nnz, allocate_matrix=out is None)
  dev = ucsr.indptr.device
  ri, di, dh = (torch.from_numpy(a).to(dev) for a in host_scales(csr_pair))
  norm_u, norm_i = normalised_pair(csr_pair, ri, di)
  W = torch.empty(n, n, dtype=torch.float32, device=dev) if out is None else out
  U_tmp = torch.empty(n_users, rank, dtype=torch.float32, device=dev)
  V = torch.empty(n, rank, dtype=torch.float32, device=dev)
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
  ev[0].record()
  ease.gram(norm_u, norm_i, 0.0, out=W)
  ev[1].record()
  sinfo = svd.fit(U_tmp, V, norm_u, norm_i, int(oversample), int(num_power_iterations), int(seed), omega=omega)
  ev[2].record()
  lowrank_add(W, V, di, dh, alpha)
  ev[3].record()
  ev[3].synchronize()
  info = dict(n=int(n), nnz=int(ucsr.nnz), rank=rank, alpha=alpha, l=int(l),
              singular_values=sinfo["singular_values"], ritz_residual=sinfo["ritz_residual"],
              gram_ms=ev[0].elapsed_time(ev[1]), svd_ms=ev[1].elapsed_time(ev[2]),
              filter_ms=ev[2].elapsed_time(ev[3]), V=V)
  return W, info
