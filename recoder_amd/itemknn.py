"""ItemKNN (the shrunk item-neighbourhood baseline of Dacrema et al. 2019) for ``ItemNeighbourhoodModel``, fitted
by rk_rp3_item_fit of librecoder_rp3.so (include/recoder_rp3.h) and served by rk_slim_scores.

With a_vi the (feature-weighted) value of user v for item i, d_i the users of item i, and j the own item:

    s[i, j]   = sum over the users v that hold i and j of a_vj * a_vi
    cosine      sim[i, j] = s / (|a_j| |a_i| + shrink)
    asymmetric  sim[i, j] = s / (|a_j|^(2(1 - alpha)) |a_i|^(2 alpha) + shrink)              (Aiolli 2013)
    tversky     sim[i, j] = s / (beta d_j + alpha d_i + (1 - alpha - beta) s + shrink)   on the binary matrix;
                jaccard is alpha = beta = 1, dice alpha = beta = 1/2
    sim[j, j] = 0, and column j keeps its ``neighbours`` largest sim > 0 by (sim descending, i ascending)

A user's scores are ``X[u, :] @ W`` with the user's stored values, W[i, j] = sim[i, j].  The shrink term is what
rk_rp3_fit's separable scale cannot spell, and it matters: without it the slice ranks far below popularity.
The model is [n, K], stored per column as ``SparseLinearModel``'s: no n x n matrix exists anywhere.

Feature weighting (Dacrema's, over the items x users matrix; r_v the stored entries of user v) is made on the
host in float64 and rounded once to f32, and so are the two vectors of the denominator: no sqrt, pow or log
runs on the device.

    tfidf  a_vi = sqrt(x_vi) max(0, log(n_items / (1 + r_v)))
    bm25   a_vi = x_vi (k1 + 1) / (k1 ((1 - b) + b len_i / mean len) + x_vi) max(0, log(n_items / (1 + r_v)))
           len_i = sum_v x_vi, k1 = 1.2, b = 0.75

``Recoder.train_itemknn`` is the public entry point; the functions below are the layer under it (and what the
tests and tools/itemknn_bench.py drive directly).
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _neighbours, _rp3_lib, _slim_lib, als
from ._lib import ptr
from .device import current_stream
from .rp3 import LDS_ITEMS, MAX_NEIGHBOURS      # rk_rp3_lds_items(), rk_rp3_max_neighbours()
from .rp3 import workspace_bytes                # (rk_rp3_item_workspace_bytes is rk_rp3_fit_workspace_bytes)

SIMILARITIES = ("cosine", "asymmetric", "jaccard", "dice", "tversky")
SET_SIMILARITIES = ("jaccard", "dice", "tversky")       # (on the binary matrix: the stored values play no part)
FEATURE_WEIGHTINGS = ("none", "tfidf", "bm25")
BM25_K1, BM25_B = 1.2, 0.75


def check_not_distributed():
  als.check_not_distributed("train_itemknn runs on one GPU: a multi-GPU ItemKNN fit is not implemented")


def check_config(model, neighbours, shrink, similarity, feature_weighting):
  """The ItemKNN contract, checked before any GPU work; returns what ``check_params`` returns, the three
  alpha / beta values being the model's."""
  from .nn import ItemNeighbourhoodModel
  if not isinstance(model, ItemNeighbourhoodModel):
    raise ValueError("train_itemknn fits an ItemNeighbourhoodModel, not %s" % type(model).__name__)
  return check_params(neighbours, shrink, similarity, feature_weighting, model.asymmetric_alpha,
                      model.tversky_alpha, model.tversky_beta)


def check_params(neighbours, shrink, similarity="cosine", feature_weighting="none", asymmetric_alpha=0.5,
                 tversky_alpha=1.0, tversky_beta=1.0):
  """(neighbours, shrink, similarity, feature_weighting, asymmetric_alpha, tversky_alpha, tversky_beta), checked."""
  K = _neighbours.check_neighbours(neighbours, MAX_NEIGHBOURS)
  number = _neighbours.check_number
  shrink = number("shrink", shrink)
  if similarity not in SIMILARITIES:
    raise ValueError("similarity must be one of %s (got %r)" % (", ".join(SIMILARITIES), similarity))
  if feature_weighting not in FEATURE_WEIGHTINGS:
    raise ValueError("feature_weighting must be one of %s (got %r)"
                     % (", ".join(FEATURE_WEIGHTINGS), feature_weighting))
  if similarity in SET_SIMILARITIES and feature_weighting != "none":
    raise ValueError("the %s similarity is over item sets, on the binary matrix: feature_weighting %r has nothing "
                     "to weigh (use \"none\")" % (similarity, feature_weighting))
  return (K, shrink, similarity, feature_weighting, number("asymmetric_alpha", asymmetric_alpha, 0.0, 1.0),
          number("tversky_alpha", tversky_alpha), number("tversky_beta", tversky_beta))


def check_values(host):
  """ValueError when a stored value is negative, NaN or infinite: the first-touch fill of the fit's workspace
  form needs every product >= +0."""
  data = np.asarray(host.data)
  ok = np.isfinite(data) & (data >= 0)
  if data.size and not bool(ok.all()):
    raise ValueError("ItemKNN needs finite interaction values >= 0: %d of the %d stored values are negative, NaN "
                     "or infinite" % (int((~ok).sum()), data.size))


# ------------------------------------------------------------- host arithmetic
def feature_weighted(X, feature_weighting):
  """The stored values of the host CSR ``X`` (users x items) after the weighting, as f32 in X's entry order:
  float64 arithmetic, rounded once.  An entry whose weight is 0 (a user who holds about every item) stays
  stored, as 0."""
  X = sp.csr_matrix(X)
  x = np.asarray(X.data, np.float64)
  if feature_weighting == "none":
    return x.astype(np.float32)
  n_users, n = X.shape
  lens = np.diff(X.indptr)
  idf = np.maximum(0.0, np.log(n / (1.0 + lens.astype(np.float64))))
  idf = np.repeat(idf, lens)
  if feature_weighting == "tfidf":
    return (np.sqrt(x) * idf).astype(np.float32)
  length = np.bincount(X.indices, weights=x, minlength=n)
  norm = (1.0 - BM25_B) + BM25_B * length / length.mean()
  return (x * (BM25_K1 + 1.0) / (BM25_K1 * norm[X.indices] + x) * idf).astype(np.float32)


def vectors(indices, values, n_items, similarity, asymmetric_alpha=0.5, tversky_alpha=1.0, tversky_beta=1.0):
  """(form, own f32 [n], oth f32 [n], g) of the denominator for the entries (``indices``: their items;
  ``values``: their f32 values as the kernel gets them, None for all 1.0): float64, rounded once.

      cosine      form 0  own = oth = |a|
      asymmetric  form 0  own = |a|^(2(1 - alpha))   oth = |a|^(2 alpha)
      tversky     form 1  own = beta d               oth = alpha d        g = 1 - alpha - beta"""
  indices = np.asarray(indices, np.int64)
  if similarity in SET_SIMILARITIES:
    ta, tb = {"jaccard": (1.0, 1.0), "dice": (0.5, 0.5)}.get(similarity, (float(tversky_alpha), float(tversky_beta)))
    d = np.bincount(indices, minlength=n_items).astype(np.float64)
    return 1, (tb * d).astype(np.float32), (ta * d).astype(np.float32), float(np.float32(1.0 - ta - tb))
  sq = np.bincount(indices, weights=None if values is None else np.asarray(values, np.float64) ** 2,
                   minlength=n_items).astype(np.float64)
  al = 0.5 if similarity == "cosine" else float(asymmetric_alpha)
  return 0, (sq ** (1.0 - al)).astype(np.float32), (sq ** al).astype(np.float32), 0.0


def required_bytes(n_users, n_items, K, nnz, allocate_model=True):
  """Device bytes of a fit: the [n, K] ids and weights and the counts (unless the caller already holds them),
  both CSRs (int64 indptr, int32 indices), the two value arrays, the two vectors and the workspace."""
  n_users, n, K, nnz = int(n_users), int(n_items), int(K), int(nnz)
  model = n * K * 8 + n * 4 if allocate_model else 0
  csrs = (n_users + 1 + n + 1) * 8 + 2 * max(1, nnz) * 4
  return model + csrs + 2 * max(1, nnz) * 4 + 2 * n * 4 + workspace_bytes(n)


def check_memory(n_users, n_items, K, nnz, free_bytes=None, allocate_model=True):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's whole
  HBM without touching a device, then (``free_bytes`` None: asked from the current device) against
  what is free."""
  n_users, n, K, nnz = int(n_users), int(n_items), int(K), int(nnz)
  if n < 1:
    raise ValueError("ItemKNN needs at least one item (got n = %d)" % n)
  what = "ItemKNN over %(users)d users x %(n)d items with %(K)d neighbours and %(nnz)d entries needs %(need)d bytes"
  return _neighbours.check_memory(
      lambda allocate: required_bytes(n_users, n, K, nnz, allocate), dict(users=n_users, n=n, K=K, nnz=nnz),
      what + ": more than one device's memory (%(hbm)d bytes); multi-device fits are not implemented",
      what + " of device memory, %(free)d are free", free_bytes, allocate_model,
      "ItemKNN over n = %(n)d items with %(K)d neighbours is outside the kernels' index range")


# ------------------------------------------------------------------ kernels
def fit_columns(ucsr, icsr, u_data, t_data, own, oth, form, g, shrink, ids, w, count, col_lo=0, col_hi=None, ws=None):
  """Columns [col_lo, col_hi) of the model into ``ids`` / ``w`` / ``count`` (rk_rp3_item_fit); ``u_data`` /
  ``t_data``: the values in the entry order of the user-major / item-major CSR, or both None (all 1.0).
  Returns the workspace."""
  lib = _rp3_lib.load()
  n_users, n = ucsr.shape
  assert icsr.shape == (n, n_users)
  K = ids.shape[1]
  col_hi = n if col_hi is None else col_hi
  _neighbours.lists(n, K, ids.device, (ids, w, count))
  assert own.shape == (n,) and oth.shape == (n,) and own.dtype == oth.dtype == torch.float32
  for d in (u_data, t_data):
    assert d is None or (d.dtype == torch.float32 and d.numel() >= ucsr.nnz and d.is_contiguous())
  ws = _neighbours.workspace(ws, lib.rk_rp3_item_workspace_bytes(n), ids.device)
  _rp3_lib.check(lib.rk_rp3_item_fit(ptr(icsr.indptr), ptr(icsr.indices), ptr(t_data), ptr(ucsr.indptr),
                                     ptr(ucsr.indices), ptr(u_data), n_users, n, ptr(own), ptr(oth), int(form),
                                     float(g), float(shrink), K, col_lo, col_hi, ptr(ids), ptr(w), ptr(count),
                                     ptr(ws), ws.numel(), current_stream()), "rk_rp3_item_fit")
  return ws


def scores(csr, ids, w, count, lo=0, hi=None, out=None, ld=None, n_rows=None):
  """out[u, c] = sum_i x_ui sim[i, lo + c] over the kept entries of column lo + c, ascending, that CSR row u
  stores: the lists are per column as ``SparseLinearModel``'s, so rk_slim_scores is the gather kernel."""
  return _neighbours.scores(_slim_lib, "rk_slim_scores", csr, ids, w, count, lo, hi, out, ld, n_rows)


# ---------------------------------------------------------------------- fit
def host_inputs(csr_pair, similarity, feature_weighting, asymmetric_alpha=0.5, tversky_alpha=1.0, tversky_beta=1.0):
  """(u_data, t_data, form, own, oth, g) on the host from the device CSR pair of ``als.csr_pair``: the
  weighted f32 values in the entry order of either CSR (both None: the kernel's all-1.0 path) and ``vectors``."""
  ucsr, icsr = csr_pair
  n_users, n = ucsr.shape
  nnz = int(ucsr.nnz)
  indptr = ucsr.indptr.cpu().numpy()
  indices = ucsr.indices.cpu().numpy()[:nnz]
  data = np.ones(nnz, np.float32) if ucsr.data is None else ucsr.data.cpu().numpy()[:nnz]
  X = sp.csr_matrix((data, indices, indptr), shape=(n_users, n))
  check_values(X)
  if similarity in SET_SIMILARITIES or (feature_weighting == "none" and ucsr.data is None):
    return (None, None) + vectors(indices, None, n, similarity, asymmetric_alpha, tversky_alpha, tversky_beta)
  a = feature_weighted(X, feature_weighting)
  # (the item-major order: the transpose of the entry numbers, as als.csr_pair transposes the matrix)
  order = sp.csr_matrix((np.arange(1, nnz + 1, dtype=np.int64), indices, indptr), shape=(n_users, n)).T.tocsr()
  order.sort_indices()
  assert np.array_equal(order.indptr, icsr.indptr.cpu().numpy())
  return (a, a[order.data - 1]) + vectors(indices, a, n, similarity, asymmetric_alpha, tversky_alpha, tversky_beta)


def fit(csr_pair, neighbours, shrink, similarity="cosine", feature_weighting="none", asymmetric_alpha=0.5,
        tversky_alpha=1.0, tversky_beta=1.0, out=None):
  """(nbr_ids, nbr_w, nbr_count, info) for the (user-major, item-major) CSR pair of ``als.csr_pair``
  (``out``: the three tensors to fill, when the caller holds them).  One host synchronisation, at the
  end; ``info`` holds n, nnz, neighbours, shrink, similarity, feature_weighting, kept (the total of
  nbr_count) and fit_ms (HIP events)."""
  ucsr, icsr = csr_pair
  K, shrink, similarity, feature_weighting, aa, ta, tb = check_params(
      neighbours, shrink, similarity, feature_weighting, asymmetric_alpha, tversky_alpha, tversky_beta)
  check_not_distributed()
  n_users, n = ucsr.shape
  check_memory(n_users, n, K, ucsr.nnz, allocate_model=out is None)
  dev = ucsr.indptr.device
  u_data, t_data, form, own, oth, g = host_inputs(csr_pair, similarity, feature_weighting, aa, ta, tb)
  if u_data is not None:
    u_data, t_data = torch.from_numpy(u_data).to(dev), torch.from_numpy(t_data).to(dev)
  own, oth = torch.from_numpy(own).to(dev), torch.from_numpy(oth).to(dev)
  ids, w, count = _neighbours.lists(n, K, dev, out)
  kept, fit_ms = _neighbours.timed_fit(
      lambda: fit_columns(ucsr, icsr, u_data, t_data, own, oth, form, g, shrink, ids, w, count), count)
  info = dict(n=int(n), nnz=int(ucsr.nnz), neighbours=K, shrink=shrink, similarity=similarity,
              feature_weighting=feature_weighting, kept=kept, fit_ms=fit_ms)
  return ids, w, count, info
