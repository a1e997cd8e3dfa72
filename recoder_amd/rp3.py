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
import numpy as np
import torch

from . import _neighbours, _rp3_lib, als
from ._lib import ptr
from .device import DEVICE_HBM_BYTES, current_stream  # noqa: F401 (the bound of check_memory, for callers)

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
  return (_neighbours.check_number("alpha", alpha), _neighbours.check_number("beta", beta),
          _neighbours.check_neighbours(neighbours, MAX_NEIGHBOURS))


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
  what = "RP3beta over %(users)d users x %(n)d items with %(K)d neighbours and %(nnz)d entries needs %(need)d bytes"
  return _neighbours.check_memory(
      lambda allocate: required_bytes(n_users, n, K, nnz, allocate), dict(users=n_users, n=n, K=K, nnz=nnz),
      what + ": more than one device's memory (%(hbm)d bytes); multi-device fits are not implemented",
      what + " of device memory, %(free)d are free", free_bytes, allocate_model,
      "RP3beta over n = %(n)d items with %(K)d neighbours is outside the kernels' index range")


# ------------------------------------------------------------------ kernels
def fit_rows(ucsr, icsr, user_w, row_scale, col_scale, ids, w, count, row_lo=0, row_hi=None, ws=None):
  """Rows [row_lo, row_hi) of the model into ``ids`` / ``w`` / ``count`` (rk_rp3_fit); returns the workspace."""
  lib = _rp3_lib.load()
  n_users, n = ucsr.shape
  assert icsr.shape == (n, n_users)
  K = ids.shape[1]
  row_hi = n if row_hi is None else row_hi
  _neighbours.lists(n, K, ids.device, (ids, w, count))
  assert user_w.shape == (n_users,) and row_scale.shape == (n,) and col_scale.shape == (n,)
  ws = _neighbours.workspace(ws, lib.rk_rp3_fit_workspace_bytes(n), ids.device)
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
  ids, w, count = _neighbours.lists(n, K, dev, out)
  kept, fit_ms = _neighbours.timed_fit(lambda: fit_rows(ucsr, icsr, uw, rs, cs, ids, w, count), count)
  info = dict(n=int(n), nnz=int(ucsr.nnz), alpha=alpha, beta=beta, neighbours=K, kept=kept, fit_ms=fit_ms)
  return ids, w, count, info
