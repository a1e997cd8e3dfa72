"""RP3beta (Paudel, Christoffel, Newell & Bernstein 2016; P3alpha: Cooper et al. 2014) for
``RandomWalkItemModel``, on the HIP kernels of librecoder_rp3.so (include/recoder_rp3.h).

The stored non-zero entries of the user x item matrix are the edges of a bipartite graph (their values
play no part in the fit).  With r_v the items of user v, d_i the users of item i:

    S[i, j] = sum over the users v that hold i and j of r_v^-alpha
    W[i, j] = d_i^-alpha * S[i, j] * d_j^-beta   (j != i),   W[i, i] = 0

and every row keeps its ``neighbours`` largest entries > 0, by (W descending, j ascending).  A user's
scores are ``X[u, :] @ W`` with the user's stored values.  The model is [n, K]: no n x n matrix exists
anywhere, so catalogues ``ShallowAutoencoder`` refuses fit.

``Recoder.train_rp3beta`` is the public entry point; the functions below are the layer under it (and
what the tests and tools/rp3_bench.py drive directly).
"""
import math

import numpy as np
import torch

from . import _neighbours, _rp3_lib, als
from ._lib import ptr
from .device import DEVICE_HBM_BYTES, current_stream

MAX_NEIGHBOURS = 1024      # rk_rp3_max_neighbours()
LDS_ITEMS = 12288          # rk_rp3_lds_items()
_GROUPS, _WAVES = 512, 16  # (resident workgroups and waves per workgroup of rk_rp3_fit)


def check_not_distributed():
  als.check_not_distributed("train_rp3beta runs on one GPU: a multi-GPU RP3beta fit is not implemented")


def check_config(model, alpha, beta, neighbours):
  """The RP3beta contract, checked before any GPU work; returns (alpha, beta, neighbours)."""
  from .nn import RandomWalkItemModel
  if not isinstance(model, RandomWalkItemModel):
    raise ValueError("train_rp3beta fits a RandomWalkItemModel, not %s" % type(model).__name__)
  return check_params(alpha, beta, neighbours)


def check_params(alpha, beta, neighbours):
  for name, v in (("alpha", alpha), ("beta", beta)):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
        not (math.isfinite(float(v)) and float(v) >= 0):
      raise ValueError("%s must be finite and >= 0 (got %r)" % (name, v))
  return float(alpha), float(beta), _neighbours.check_neighbours(neighbours, MAX_NEIGHBOURS)


def _power(x, e):
  """x^-e in float64, rounded once to f32; 0 where x is 0."""
  out = np.zeros_like(x)
  out[x > 0] = x[x > 0] ** -float(e)
  return out.astype(np.float32)


def weights(ucsr, alpha, beta):
  """(user_w, row_scale, col_scale) = (r^-alpha, d^-alpha, d^-beta) of the host CSR ``ucsr`` (users x
  items): float64, rounded once to f32; 0 for users and items without entries."""
  indptr = np.asarray(ucsr.indptr, np.int64)
  r = np.diff(indptr).astype(np.float64)
  d = np.bincount(np.asarray(ucsr.indices, np.int64), minlength=ucsr.shape[1]).astype(np.float64)
  return _power(r, alpha), _power(d, alpha), _power(d, beta)


def workspace_bytes(n_items):
  """rk_rp3_fit_workspace_bytes(n_items), restated on the host (the memory check needs no library)."""
  n = int(n_items)
  if n <= LDS_ITEMS:
    return 256
  return 256 + _GROUPS * (-(-n // 64) * 64 + _WAVES * (-(-n // 1024) * 64)) * 4


def required_bytes(n_users, n_items, K, nnz, allocate_model=True):
  """Device bytes of a fit: the [n, K] ids and weights and the counts (unless the caller already holds
  them), both CSRs (int64 indptr, int32 indices), the three weight vectors and the workspace."""
  n_users, n, K, nnz = int(n_users), int(n_items), int(K), int(nnz)
  model = n * K * 8 + n * 4 if allocate_model else 0
  csrs = (n_users + 1 + n + 1) * 8 + 2 * max(1, nnz) * 4
  return model + csrs + (n_users + 2 * n) * 4 + workspace_bytes(n)


def check_memory(n_users, n_items, K, nnz, free_bytes=None, allocate_model=True):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's whole
  HBM without touching a device, then (``free_bytes`` None: asked from the current device) against
  what is free."""
  n_users, n, K, nnz = int(n_users), int(n_items), int(K), int(nnz)
  if n < 1:
    raise ValueError("RP3beta needs at least one item (got n = %d)" % n)
  whole = required_bytes(n_users, n, K, nnz, True)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError("RP3beta over %d users x %d items with %d neighbours and %d entries needs %d bytes: more "
                     "than one device's memory (%d bytes); multi-device fits are not implemented"
                     % (n_users, n, K, nnz, whole, DEVICE_HBM_BYTES))
  if n * K >= 2 ** 40:
    raise ValueError("RP3beta over n = %d items with %d neighbours is outside the kernels' index range" % (n, K))
  need = required_bytes(n_users, n, K, nnz, allocate_model)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("RP3beta over %d users x %d items with %d neighbours and %d entries needs %d bytes of "
                     "device memory, %d are free" % (n_users, n, K, nnz, need, free_bytes))
  return need


# ------------------------------------------------------------------ kernels
def fit_rows(ucsr, icsr, user_w, row_scale, col_scale, ids, w, count, row_lo=0, row_hi=None, ws=None):
  """Rows [row_lo, row_hi) of the model into ``ids`` / ``w`` / ``count`` (rk_rp3_fit); returns the workspace."""
  lib = _rp3_lib.load()
  n_users, n = ucsr.shape
  assert icsr.shape == (n, n_users)
  K = ids.shape[1]
  row_hi = n if row_hi is None else row_hi
  assert ids.shape == (n, K) and ids.dtype == torch.int32 and ids.is_contiguous()
  assert w.shape == (n, K) and w.dtype == torch.float32 and w.is_contiguous()
  assert count.shape == (n,) and count.dtype == torch.int32
  assert user_w.shape == (n_users,) and row_scale.shape == (n,) and col_scale.shape == (n,)
  need = lib.rk_rp3_fit_workspace_bytes(n)
  if ws is None or ws.numel() < need:
    ws = torch.empty(need, dtype=torch.uint8, device=ids.device)
  _rp3_lib.check(lib.rk_rp3_fit(ptr(icsr.indptr), ptr(icsr.indices), ptr(ucsr.indptr), ptr(ucsr.indices),
                                n_users, n, ptr(user_w), ptr(row_scale), ptr(col_scale), K, row_lo, row_hi,
                                ptr(ids), ptr(w), ptr(count), ptr(ws), ws.numel(), current_stream()),
                 "rk_rp3_fit")
  return ws


def scores(csr, ids, w, count, lo=0, hi=None, out=None, ld=None, n_rows=None):
  """out[u, c] = sum_i x_ui W[i, lo + c] over the stored entries of CSR row u, ascending, W the sparse
  matrix the kept neighbours spell (rk_rp3_scores).  ``csr``: anything with int64 ``indptr``, int32
  ``indices`` and fp32 ``data`` (or None) on the device."""
  return _neighbours.scores(_rp3_lib, "rk_rp3_scores", csr, ids, w, count, lo, hi, out, ld, n_rows)


# ---------------------------------------------------------------------- fit
def host_weights(csr_pair, alpha, beta):
  """``weights`` from the device CSR pair of ``als.csr_pair`` (the two indptr arrays hold r and d)."""
  ucsr, icsr = csr_pair
  r = np.diff(ucsr.indptr.cpu().numpy()).astype(np.float64)
  d = np.diff(icsr.indptr.cpu().numpy()).astype(np.float64)
  return _power(r, alpha), _power(d, alpha), _power(d, beta)


def fit(csr_pair, alpha, beta, neighbours, out=None):
  """(nbr_ids, nbr_w, nbr_count, info) for the (user-major, item-major) CSR pair of ``als.csr_pair``
  (``out``: the three tensors to fill, when the caller holds them).  One host synchronisation, at the
  end; ``info`` holds n, nnz, alpha, beta, neighbours, kept (the total of nbr_count) and fit_ms (HIP
  events)."""
  ucsr, icsr = csr_pair
  alpha, beta, K = check_params(alpha, beta, neighbours)
  check_not_distributed()
  n_users, n = ucsr.shape
  check_memory(n_users, n, K, ucsr.nnz, allocate_model=out is None)
  dev = ucsr.indptr.device
  uw, rs, cs = (torch.from_numpy(a).to(dev) for a in host_weights(csr_pair, alpha, beta))
  if out is None:
    out = (torch.empty(n, K, dtype=torch.int32, device=dev), torch.empty(n, K, dtype=torch.float32, device=dev),
           torch.empty(n, dtype=torch.int32, device=dev))
  ids, w, count = out
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
  ev[0].record()
  fit_rows(ucsr, icsr, uw, rs, cs, ids, w, count)
  ev[1].record()
  kept = int(count.sum(dtype=torch.int64).item())      # (the synchronisation)
  ev[1].synchronize()
  info = dict(n=int(n), nnz=int(ucsr.nnz), alpha=alpha, beta=beta, neighbours=K, kept=kept,
              fit_ms=ev[0].elapsed_time(ev[1]))
  return ids, w, count, info
