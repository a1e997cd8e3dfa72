"""SLIM (Ning & Karypis 2011, "SLIM: Sparse Linear Methods for Top-N Recommender Systems") for
``SparseLinearModel``, on the HIP kernels of librecoder_slim.so (include/recoder_slim.h).

With G = X^T X over the stored values of the user x item matrix (values >= 0), column j of W solves

    min over w >= 0, w_j = 0 of   1/2 |x_j - X w|^2 + (l2_reg/2) |w|^2 + l1_reg |w|_1

by cyclic coordinate descent on the Gram (the covariance updates of Friedman, Hastie & Tibshirani 2010),
over the candidates {k != j : G[j, k] > l1_reg} only (exact: every other weight stays 0), and keeps at
most ``neighbours`` entries.  A user's scores are ``X[u, :] @ W``.  The model is stored by column,
[n, K].  The plain fit needs the n x n Gram on the device, which is EASE's limit on the catalogue.

fsSLIM (section 4.3 of the paper; ``candidates=M``) lifts that limit: column j is regressed on the M items most
similar to j only, found by an ItemKNN fit (recoder_amd/itemknn.py), and rk_slim_fit_sparse forms the column's
M x M block of the Gram from the two CSRs on the fly and runs the same sweep on it.  No n x n buffer exists.

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
MAX_CANDIDATES = 1024      # rk_rp3_max_neighbours(): the longest list the ItemKNN fit makes
SPARSE_LDS_CANDIDATES = 104  # rk_slim_sparse_lds_candidates()
_SPARSE_GROUPS, _SPARSE_ARRAYS = 768, 7  # (those of rk_slim_fit_sparse)


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


def check_candidates(candidates, candidate_similarity="cosine", candidate_shrink=0.0):
  """(candidates, candidate_similarity, candidate_shrink) of an fsSLIM fit, checked; ``candidates`` None: the
  plain fit, the other two are checked all the same."""
  from . import itemknn
  if candidates is not None and (isinstance(candidates, bool) or not isinstance(candidates, (int, np.integer)) or
                                 not 1 <= candidates <= MAX_CANDIDATES):
    raise ValueError("candidates must be None or an integer in [1, %d] (got %r)" % (MAX_CANDIDATES, candidates))
  if candidate_similarity not in itemknn.SIMILARITIES:
    raise ValueError("candidate_similarity must be one of %s (got %r)"
                     % (", ".join(itemknn.SIMILARITIES), candidate_similarity))
  shrink = _neighbours.check_number("candidate_shrink", candidate_shrink)
  return (None if candidates is None else int(candidates)), candidate_similarity, shrink


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


def sparse_workspace_bytes(candidates):
  """rk_slim_fit_sparse_workspace_bytes(candidates), restated on the host."""
  M = check_candidates(candidates)[0]
  if M is None:
    raise ValueError("candidates must be an integer in [1, %d] (got None)" % MAX_CANDIDATES)
  if M <= SPARSE_LDS_CANDIDATES:
    return 256
  pad = -(-M // 64) * 64
  return 256 + _SPARSE_GROUPS * (pad * pad + _SPARSE_ARRAYS * pad) * 4


def required_bytes(n_users, n_items, K, nnz, allocate_model=True, candidates=None):
  """Device bytes of a fit: the n x n f32 Gram, the [n, K] ids and weights and the counts (unless the
  caller already holds them), the sweeps and supports, both CSRs (int64 indptr, int32 indices, f32
  values), inv_denom and the workspace.  With ``candidates`` = M, instead of the Gram and that workspace: the
  [n, M] candidate ids and similarities and their counts, the screened counts, what the ItemKNN fit adds to the
  CSRs (its two vectors and its workspace) and rk_slim_fit_sparse's workspace."""
  n_users, n, K, nnz = int(n_users), int(n_items), int(K), int(nnz)
  model = n * K * 8 + n * 4 if allocate_model else 0
  csrs = (n_users + 1 + n + 1) * 8 + 2 * max(1, nnz) * 8
  if candidates is None:
    return n * n * 4 + model + csrs + 3 * n * 4 + workspace_bytes(n)
  from . import itemknn
  M = int(candidates)
  lists = n * M * 8 + n * 4
  return lists + model + csrs + 4 * n * 4 + 2 * n * 4 + itemknn.workspace_bytes(n) + sparse_workspace_bytes(M)


def check_memory(n_users, n_items, K, nnz, free_bytes=None, allocate_model=True, candidates=None):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's whole
  HBM without touching a device, then (``free_bytes`` None: asked from the current device) against
  what is free.  The n x n Gram dominates: this is EASE's limit on the catalogue.  With ``candidates`` = M
  (fsSLIM) there is no Gram: the [n, M] candidate lists and the workspace are counted instead."""
  n_users, n, K, nnz = int(n_users), int(n_items), int(K), int(nnz)
  if n < 1:
    raise ValueError("SLIM needs at least one item (got n = %d)" % n)
  if candidates is not None:
    M = check_candidates(candidates)[0]
    what = ("SLIM over %(users)d users x %(n)d items with %(K)d neighbours, %(M)d candidates and %(nnz)d entries "
            "needs %(need)d bytes")
    return _neighbours.check_memory(
        lambda allocate: required_bytes(n_users, n, K, nnz, allocate, M), dict(users=n_users, n=n, K=K, nnz=nnz, M=M),
        what + ": more than one device's memory (%(hbm)d bytes); multi-device fits are not implemented",
        what + " of device memory, %(free)d are free", free_bytes, allocate_model,
        "SLIM over n = %(n)d items with %(K)d neighbours is outside the kernels' index range")
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


def fit_columns_sparse(ucsr, icsr, cand_ids, cand_count, inv, l1_reg, ids, w, count, sweeps, support, max_sweeps=50,
                       tol=1e-5, col_lo=0, col_hi=None, ws=None, screened=None):
  """Columns [col_lo, col_hi) of the model from the (user-major, item-major) CSR pair and the candidate lists
  ``cand_ids`` int32 [n, M] (ascending, -1 behind ``cand_count``) (rk_slim_fit_sparse); ``screened`` int32 [n] or
  None: the candidates that passed the l1 screen.  Returns the workspace."""
  lib = _slim_lib.load()
  n_users, n = ucsr.shape
  assert icsr.shape == (n, n_users)
  K = ids.shape[1]
  M = cand_ids.shape[1]
  col_hi = n if col_hi is None else col_hi
  assert cand_ids.shape == (n, M) and cand_ids.dtype == torch.int32 and cand_ids.is_contiguous()
  assert cand_count.shape == (n,) and cand_count.dtype == torch.int32
  assert inv.shape == (n,) and inv.dtype == torch.float32
  assert (ucsr.data is None) == (icsr.data is None)
  _neighbours.lists(n, K, ids.device, (ids, w, count))
  for t in (sweeps, support) + (() if screened is None else (screened,)):
    assert t.shape == (n,) and t.dtype == torch.int32
  ws = _neighbours.workspace(ws, lib.rk_slim_fit_sparse_workspace_bytes(M), ids.device)
  _slim_lib.check(lib.rk_slim_fit_sparse(
      ptr(icsr.indptr), ptr(icsr.indices), ptr(icsr.data), ptr(ucsr.indptr), ptr(ucsr.indices), ptr(ucsr.data), n_users,
      n, ptr(cand_ids), ptr(cand_count), M, ptr(inv), float(l1_reg), K, int(max_sweeps), float(tol), col_lo, col_hi,
      ptr(ids), ptr(w), ptr(count), ptr(sweeps), ptr(support), ptr(screened), ptr(ws), ws.numel(), current_stream()),
      "rk_slim_fit_sparse")
  return ws


def _fmaf32(a, b, c):
  """f32 fused multiply-add on the host, element-wise: the product is exact in float64; where the float64 sum sits
  on an f32 rounding midpoint without being exact (TwoSum gives its error) it is moved one ulp towards the true
  value before the one rounding to f32."""
  a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
  p = a * b
  s = p + c
  bb = s - p
  err = (p - (s - bb)) + (c - bb)
  fix = ((np.ascontiguousarray(s).view(np.int64) & 0x1FFFFFFF) == 0x10000000) & (err != 0)
  return np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s).astype(np.float32)


def diagonal(icsr):
  """G_kk f32 [n] per item from the item-major CSR: the chain acc = fmaf(a, a, acc) from +0 over the item's users
  in ascending order, which is rk_slim_fit_sparse's L[c][c] (binary data: the item's degree, exact below 2^24)."""
  indptr = icsr.indptr.cpu().numpy()
  deg = np.diff(indptr)
  if icsr.data is None:
    return deg.astype(np.float32)
  data = icsr.data.cpu().numpy()
  acc = np.zeros(len(deg), np.float32)
  order = np.argsort(-deg, kind="stable")            # (the items with more than s users are a prefix of it)
  sdeg = deg[order]
  for s in range(int(sdeg[0]) if len(sdeg) else 0):
    live = order[:int(np.searchsorted(-sdeg, -s, side="left"))]       # deg > s
    a = data[indptr[live] + s]
    acc[live] = _fmaf32(a, a, acc[live])
  return acc


def scores(csr, ids, w, count, lo=0, hi=None, out=None, ld=None, n_rows=None):
  """out[u, c] = sum_k x_uk W[k, lo + c] over the kept entries of column lo + c, ascending, that CSR row u
  stores (rk_slim_scores).  ``csr``: anything with int64 ``indptr``, int32 ``indices`` and fp32 ``data``
  (or None) on the device."""
  return _neighbours.scores(_slim_lib, "rk_slim_scores", csr, ids, w, count, lo, hi, out, ld, n_rows)


# ---------------------------------------------------------------------- fit
def candidate_lists(csr_pair, candidates, candidate_similarity="cosine", candidate_shrink=0.0):
  """(cand_ids int32 [n, M], cand_count int32 [n], ms) of fsSLIM: every column's M most similar items by
  ``itemknn.fit`` over the stored values (ties to the lower id), ascending inside a column with -1 behind the count:
  what rk_slim_fit_sparse reads."""
  from . import itemknn
  ids, _, count, info = itemknn.fit(csr_pair, candidates, candidate_shrink, candidate_similarity)
  return ids, count, info["fit_ms"]


def _fit_sparse(csr_pair, l1, l2, K, max_sweeps, tol, M, similarity, shrink, out):
  """``fit`` with ``candidates`` = M: the ItemKNN lists, the diagonal, rk_slim_fit_sparse."""
  ucsr, icsr = csr_pair
  n_users, n = ucsr.shape
  check_memory(n_users, n, K, ucsr.nnz, allocate_model=out is None, candidates=M)
  dev = ucsr.indptr.device
  cand_ids, cand_count, candidate_ms = candidate_lists(csr_pair, M, similarity, shrink)
  ids, w, count = _neighbours.lists(n, K, dev, out)
  sweeps, support, screened = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
  inv = torch.from_numpy(inv_denom(diagonal(icsr), l2)).to(dev)
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
  ev[0].record()
  fit_columns_sparse(ucsr, icsr, cand_ids, cand_count, inv, l1, ids, w, count, sweeps, support, max_sweeps, tol,
                     screened=screened)
  ev[1].record()
  stats = torch.stack([count.sum(dtype=torch.int64), (support > K).sum(dtype=torch.int64),
                       (sweeps >= max_sweeps).sum(dtype=torch.int64), sweeps.max().to(torch.int64),
                       screened.sum(dtype=torch.int64)]).cpu().numpy()             # (the synchronisation)
  ev[1].synchronize()
  info = dict(n=int(n), nnz=int(ucsr.nnz), l1_reg=l1, l2_reg=l2, neighbours=K, kept=int(stats[0]),
              cut_columns=int(stats[1]), unconverged_columns=int(stats[2]), max_sweeps_run=int(stats[3]),
              gram_ms=0.0, fit_ms=ev[0].elapsed_time(ev[1]), candidates=M, candidate_ms=candidate_ms,
              mean_candidates=float(stats[4]) / n)
  return ids, w, count, info


def fit(csr_pair, l1_reg, l2_reg, neighbours, max_sweeps=50, tol=1e-5, candidates=None, candidate_similarity="cosine",
        candidate_shrink=0.0, out=None):
  """(nbr_ids, nbr_w, nbr_count, info) for the (user-major, item-major) CSR pair of ``als.csr_pair``
  (``out``: the three tensors to fill, when the caller holds them).  The Gram comes from ``ease.gram``
  with reg 0 (bitwise symmetric, exact for binary data), its diagonal is read back for ``inv_denom``,
  and G is freed at the end, after the one host synchronisation.  The stored values must be >= 0 (the
  caller checks: ``check_values``).  ``info`` holds n, nnz, l1_reg, l2_reg, neighbours, kept (the total of
  nbr_count), cut_columns (support > neighbours), unconverged_columns (columns that ran all max_sweeps
  sweeps), max_sweeps_run, gram_ms and fit_ms (HIP events).

  ``candidates`` = M (fsSLIM): ``itemknn.fit`` with ``candidate_similarity`` and ``candidate_shrink`` over the stored
  values gives every column its M most similar items; ``inv_denom`` comes from ``diagonal``; rk_slim_fit_sparse
  fills the model.  ``ease.gram`` is not called and no n x n buffer is allocated.  ``info`` then also holds
  candidates, candidate_ms (the ItemKNN fit) and mean_candidates (the mean number of candidates of a column that
  passed the l1 screen); gram_ms is 0 (the local Grams are formed inside fit_ms)."""
  from . import ease
  ucsr, icsr = csr_pair
  l1, l2, K, max_sweeps, tol = check_params(l1_reg, l2_reg, neighbours, max_sweeps, tol)
  M, similarity, shrink = check_candidates(candidates, candidate_similarity, candidate_shrink)
  check_not_distributed()
  if M is not None:
    return _fit_sparse(csr_pair, l1, l2, K, max_sweeps, tol, M, similarity, shrink, out)
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
