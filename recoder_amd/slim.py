"""SLIM (Ning & Karypis 2011, "SLIM: Sparse Linear Methods for Top-N Recommender Systems") for
``SparseLinearModel``, on the HIP kernels of librecoder_slim.so (include/recoder_slim.h).

With G = X^T X over the stored values of the user x item matrix (values >= 0), column j of W solves

    min over w >= 0, w_j = 0 of   1/2 |x_j - X w|^2 + (l2_reg/2) |w|^2 + l1_reg |w|_1

by cyclic coordinate descent on the Gram (the covariance updates of Friedman, Hastie & Tibshirani 2010),
over the candidates {k != j : G[j, k] > l1_reg} only (exact: every other weight stays 0), and keeps at
most ``neighbours`` entries.  A user's scores are ``X[u, :] @ W``.  The model is stored by column,
[n, K]; the fit needs the n x n Gram on the device, which is EASE's limit on the catalogue.

scikit-learn's ``ElasticNet(alpha, l1_ratio, positive=True)`` over U users minimises the same objective
divided by U:  l1_reg = U * alpha * l1_ratio,  l2_reg = U * alpha * (1 - l1_ratio).

``Recoder.train_slim`` is the public entry point; the functions below are the layer under it (and what
the tests and tools/slim_bench.py drive directly).
"""
import numpy as np
import torch

from . import _neighbours, _slim_lib, als
from ._lib import ptr
from .device import current_stream

MAX_NEIGHBOURS = 1024      # rk_slim_max_neighbours()
LDS_CANDIDATES = 960       # rk_slim_lds_candidates()
_GROUPS, _ARRAYS = 2048, 5  # (resident workgroups of rk_slim_fit and the state arrays of a column)


def check_not_distributed():
  als.check_not_distributed("train_slim runs on one GPU: a multi-GPU SLIM fit is not implemented")


def check_config(model, l1_reg, l2_reg, neighbours, max_sweeps=50, tol=1e-5):
  """The SLIM contract, checked before any GPU work; returns (l1_reg, l2_reg, neighbours, max_sweeps, tol)."""
  from .nn import SparseLinearModel
  if not isinstance(model, SparseLinearModel):
    raise ValueError("train_slim fits a SparseLinearModel, not %s" % type(model).__name__)
  return check_params(l1_reg, l2_reg, neighbours, max_sweeps, tol)


def check_params(l1_reg, l2_reg, neighbours, max_sweeps=50, tol=1e-5):
  l1_reg, l2_reg, tol = (_neighbours.check_number(name, v) for name, v in
                         (("l1_reg", l1_reg), ("l2_reg", l2_reg), ("tol", tol)))
  neighbours = _neighbours.check_neighbours(neighbours, MAX_NEIGHBOURS)
  if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, (int, np.integer)) or not 1 <= max_sweeps < 2 ** 31:
    raise ValueError("max_sweeps must be an integer >= 1 (got %r)" % (max_sweeps,))
  return l1_reg, l2_reg, neighbours, int(max_sweeps), tol


def check_values(host):
  """ValueError when a stored value is negative (or NaN): the screening of the candidates needs G >= 0."""
  data = np.asarray(host.data)
  if data.size and not bool(np.all(data >= 0)):
    raise ValueError("SLIM needs interaction values >= 0 (the candidate screening relies on a Gram >= 0): "
                     "%d of the %d stored values are negative or NaN" % (int((~(data >= 0)).sum()), data.size))


def inv_denom(diag, l2_reg):
  """1 / (float64(G_kk) + l2_reg) rounded once to f32; 0 where the denominator is 0 (an item nobody holds
  with l2_reg = 0: it is never a candidate)."""
  d = np.asarray(diag, np.float64) + float(l2_reg)
  out = np.zeros_like(d)
  out[d > 0] = 1.0 / d[d > 0]
  return out.astype(np.float32)


def workspace_bytes(n_items):
  """rk_slim_fit_workspace_bytes(n_items), restated on the host (the memory check needs no library)."""
  n = int(n_items)
  if n <= LDS_CANDIDATES:
    return 256
  return 256 + _GROUPS * _ARRAYS * (-(-n // 64) * 64) * 4


def required_bytes(n_users, n_items, K, nnz, allocate_model=True):
  """Device bytes of a fit: the n x n f32 Gram, the [n, K] ids and weights and the counts (unless the
  caller already holds them), the sweeps and supports, both CSRs (int64 indptr, int32 indices, f32
  values), inv_denom and the workspace."""
  n_users, n, K, nnz = int(n_users), int(n_items), int(K), int(nnz)
  model = n * K * 8 + n * 4 if allocate_model else 0
  csrs = (n_users + 1 + n + 1) * 8 + 2 * max(1, nnz) * 8
  return n * n * 4 + model + csrs + 3 * n * 4 + workspace_bytes(n)


def check_memory(n_users, n_items, K, nnz, free_bytes=None, allocate_model=True):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's whole
  HBM without touching a device, then (``free_bytes`` None: asked from the current device) against
  what is free.  The n x n Gram dominates: this is EASE's limit on the catalogue."""
  n_users, n, K, nnz = int(n_users), int(n_items), int(K), int(nnz)
  if n < 1:
    raise ValueError("SLIM needs at least one item (got n = %d)" % n)
  what = "SLIM over %(users)d users x %(n)d items with %(K)d neighbours and %(nnz)d entries needs %(need)d bytes"
  return _neighbours.check_memory(
      lambda allocate: required_bytes(n_users, n, K, nnz, allocate),
      dict(users=n_users, n=n, K=K, nnz=nnz, gram=n * n * 4),
      what + ", %(gram)d of them for its n x n fp32 Gram (the limit EASE has): more than one device's memory "
      "(%(hbm)d bytes); multi-device fits are not implemented",
      what + " of device memory (%(gram)d for the n x n Gram), %(free)d are free", free_bytes, allocate_model)


# ------------------------------------------------------------------ kernels
def fit_columns(G, inv, l1_reg, ids, w, count, sweeps, support, max_sweeps=50, tol=1e-5, col_lo=0, col_hi=None,
                ws=None):
  """Columns [col_lo, col_hi) of the model into ``ids`` / ``w`` / ``count`` / ``sweeps`` / ``support``
  from the Gram ``G`` [n, n] f32 and ``inv`` [n] f32 (rk_slim_fit); returns the workspace."""
  lib = _slim_lib.load()
  n = G.shape[0]
  K = ids.shape[1]
  col_hi = n if col_hi is None else col_hi
  assert G.shape == (n, n) and G.dtype == torch.float32 and G.stride(1) == 1
  assert inv.shape == (n,) and inv.dtype == torch.float32
  _neighbours.lists(n, K, ids.device, (ids, w, count))
  for t in (sweeps, support):
    assert t.shape == (n,) and t.dtype == torch.int32
  ws = _neighbours.workspace(ws, lib.rk_slim_fit_workspace_bytes(n), ids.device)
  _slim_lib.check(lib.rk_slim_fit(ptr(G), G.stride(0), n, ptr(inv), float(l1_reg), K, int(max_sweeps), float(tol),
                                  col_lo, col_hi, ptr(ids), ptr(w), ptr(count), ptr(sweeps), ptr(support),
                                  ptr(ws), ws.numel(), current_stream()), "rk_slim_fit")
  return ws


def scores(csr, ids, w, count, lo=0, hi=None, out=None, ld=None, n_rows=None):
  """out[u, c] = sum_k x_uk W[k, lo + c] over the kept entries of column lo + c, ascending, that CSR row u
  stores (rk_slim_scores).  ``csr``: anything with int64 ``indptr``, int32 ``indices`` and fp32 ``data``
  (or None) on the device."""
  return _neighbours.scores(_slim_lib, "rk_slim_scores", csr, ids, w, count, lo, hi, out, ld, n_rows)


# ---------------------------------------------------------------------- fit
def fit(csr_pair, l1_reg, l2_reg, neighbours, max_sweeps=50, tol=1e-5, out=None):
  """(nbr_ids, nbr_w, nbr_count, info) for the (user-major, item-major) CSR pair of ``als.csr_pair``
  (``out``: the three tensors to fill, when the caller holds them).  The Gram comes from ``ease.gram``
  with reg 0 (bitwise symmetric, exact for binary data), its diagonal is read back for ``inv_denom``,
  and G is freed at the end, after the one host synchronisation.  The stored values must be >= 0 (the
  caller checks: ``check_values``).  ``info`` holds n, nnz, l1_reg, l2_reg, neighbours, kept (the total of
  nbr_count), cut_columns (support > neighbours), unconverged_columns (columns that ran all max_sweeps
  sweeps), max_sweeps_run, gram_ms and fit_ms (HIP events)."""
  from . import ease
  ucsr, icsr = csr_pair
  l1, l2, K, max_sweeps, tol = check_params(l1_reg, l2_reg, neighbours, max_sweeps, tol)
  check_not_distributed()
  n_users, n = ucsr.shape
  check_memory(n_users, n, K, ucsr.nnz, allocate_model=out is None)
  dev = ucsr.indptr.device
  ids, w, count = _neighbours.lists(n, K, dev, out)
  sweeps = torch.empty(n, dtype=torch.int32, device=dev)
  support = torch.empty(n, dtype=torch.int32, device=dev)
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
  ev[0].record()
  G = ease.gram(ucsr, icsr, 0.0)
  ev[1].record()
  # (the read-back of the n diagonal entries waits for the Gram alone; the fit itself is enqueued behind it
  # and waited for once, at the end)
  inv = torch.from_numpy(inv_denom(torch.diagonal(G).cpu().numpy(), l2)).to(dev)
  ev[2].record()
  fit_columns(G, inv, l1, ids, w, count, sweeps, support, max_sweeps, tol)
  ev[3].record()
  stats = torch.stack([count.sum(dtype=torch.int64), (support > K).sum(dtype=torch.int64),
                       (sweeps >= max_sweeps).sum(dtype=torch.int64),
                       sweeps.max().to(torch.int64)]).cpu().numpy()                # (the synchronisation)
  ev[3].synchronize()
  del G
  info = dict(n=int(n), nnz=int(ucsr.nnz), l1_reg=l1, l2_reg=l2, neighbours=K, kept=int(stats[0]),
              cut_columns=int(stats[1]), unconverged_columns=int(stats[2]), max_sweeps_run=int(stats[3]),
              gram_ms=ev[0].elapsed_time(ev[1]), fit_ms=ev[2].elapsed_time(ev[3]))
  return ids, w, count, info
