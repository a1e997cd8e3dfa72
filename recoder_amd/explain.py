"""Explanations: which items of a user's history carry the score of a served item, for the two score families that
are linear in the history, on rk_ease_explain (librecoder_ease.so), rk_slim_explain (librecoder_slim.so) and
rk_als_explain (librecoder_als.so).  Nothing is approximated.

  item-item models   s_uj = sum_{i in u} x_ui W[i, j]: the contribution of history item i to target j is the one
                     product x_ui W[i, j], and nothing is left over (the baseline is +0).  ``ShallowAutoencoder``,
                     ``GraphFilterModel`` and ``AdmmSlimModel`` store W dense; every ``_NeighbourListModel`` stores
                     lists, by rows (``RandomWalkItemModel``) or by columns (SLIM, fsSLIM, ItemKNN).
  MatrixFactorization, activation "none", embedding size <= ``foldin.MAX_H``.  The user is the FOLDED-IN one
                     (recoder_amd/foldin.py), whether a fit has seen the history or not:
                       A_u = G + sum_e a_e y_e y_e^T,   x_u = A_u^-1 (sum_e coef_e y_e - v),
                       s_uj = y_j . x_u + b_j = sum_e coef_e (z_uj . y_e) + (b_j - z_uj . v),   z_uj = A_u^-1 y_j:
                     entry e contributes coef_e (z_uj . y_e), the rest is the baseline.  ``total`` is therefore the
                     score ``recommend_folded`` ranks by, NOT the score of the trained user row.

For B users and targets ``items`` [B, J] the result holds, per (user, target), the ``num_contributors`` = m history
items with the largest contributions (ties to the smaller item id, a NaN behind every number; a negative contribution
is an ordinary value and is kept when fewer than m larger ones exist), their values, the baseline, and ``total``: all
of the history's contributions -- not only the kept m -- plus the baseline.  A target of -1 (the padding of
``recommend_filtered``) gives -1 / 0 everywhere; a user with an empty history gets -1 / 0 and total = baseline.

``Recoder.explain`` is the public entry point.  ``check`` runs on the host before any GPU work.
"""
import collections
import numbers
import warnings

import numpy as np
import torch

from . import _als_lib, _ease_lib, _slim_lib, foldin
from ._lib import ptr
from .device import current_stream
from .nn import (AdmmSlimModel, GraphFilterModel, MatrixFactorization, ShallowAutoencoder, _NeighbourListModel)

MAX_CONTRIBUTORS = 64                              # rk_ease_explain_max_contributors()
DENSE_MODELS = (ShallowAutoencoder, GraphFilterModel, AdmmSlimModel)

Explanation = collections.namedtuple("Explanation", ["contributors", "contributions", "baseline", "total"])
Explanation.__doc__ = """Host numpy arrays: ``contributors`` int64 [B, J, m] (history item ids, best first, -1 padding),
``contributions`` f32 [B, J, m] (0.0 at padding), ``baseline`` f32 [B, J], ``total`` f32 [B, J]."""


def check(recoder, matrix, items, num_contributors, alpha, reg):
  """The contract of ``explain``, checked before any GPU work; returns (items int64 [B, J], m, alpha, reg)."""
  model = recoder.model
  name = type(model).__name__
  if isinstance(model, MatrixFactorization):
    try:
      alpha, reg = foldin.check_config(model, alpha, reg)
    except ValueError as e:
      raise ValueError("explain: %s: %s" % (name, str(e).replace("fold_in", "the folded-in user of explain"))) from None
    n_items = int(model.item_embedding_layer.weight.shape[0])
  elif isinstance(model, DENSE_MODELS + (_NeighbourListModel,)):
    if model.item_weights is None:
      raise ValueError("explain needs a fitted %s: call %s first or load a checkpoint" % (name, model.fit_method))
    n_items = int(model.item_weights.shape[0])
  else:
    raise ValueError("explain serves the item-item models and a MatrixFactorization with activation_type='none', "
                     "not %s: its score is not a sum over the history's items" % name)
  try:
    foldin.check_not_distributed()
  except ValueError:
    raise ValueError("explain runs on one GPU: multi-GPU explanation of a %s is not implemented" % name) from None
  m = num_contributors
  if isinstance(m, bool) or not isinstance(m, numbers.Integral) or not 1 <= m <= MAX_CONTRIBUTORS:
    raise ValueError("num_contributors must be an integer in [1, %d] (got %r)" % (MAX_CONTRIBUTORS, m))
  B = int(matrix.shape[0])
  if matrix.shape[1] > n_items:
    raise ValueError("interactions_matrix has %d columns, the %s has %d items" % (matrix.shape[1], name, n_items))
  a = np.asarray(items)
  if a.ndim != 2 or not (np.issubdtype(a.dtype, np.integer) and a.dtype != np.bool_):
    raise ValueError("items must be an integer array [users, targets] for %s.explain (got dtype %s, shape %r)"
                     % (name, a.dtype, a.shape))
  if a.shape[0] != B:
    raise ValueError("items has %d rows, the batch has %d users (%s.explain takes one row of targets a user)"
                     % (a.shape[0], B, name))
  if a.shape[1] < 1:
    raise ValueError("items needs at least one target a user for %s.explain (got shape %r)" % (name, a.shape))
  if a.size and (a.min() < -1 or a.max() >= n_items):
    raise ValueError("items holds an id outside [-1, %d) for %s.explain (got %d .. %d)"
                     % (n_items, name, a.min(), a.max()))
  if B * a.shape[1] >= 2 ** 31:
    raise ValueError("explain takes fewer than 2^31 (user, target) pairs a call for %s (got %d)"
                     % (name, B * a.shape[1]))
  return np.ascontiguousarray(a, dtype=np.int64), int(m), alpha, reg


def _outputs(B, J, m, device):
  return (torch.empty((B, J, m), dtype=torch.int64, device=device),
          torch.empty((B, J, m), dtype=torch.float32, device=device),
          torch.empty((B, J), dtype=torch.float32, device=device),
          torch.empty((B, J), dtype=torch.float32, device=device))


def _rows(csr, row_lo, row_hi):
  row_hi = csr.shape[0] if row_hi is None else row_hi
  assert 0 <= row_lo <= row_hi <= csr.shape[0]
  return row_hi - row_lo, csr.indptr.data_ptr() + 8 * row_lo


def _check_items(items, rows, n):
  assert items.dtype == torch.int64 and items.dim() == 2 and items.shape[0] == rows and items.is_contiguous()
  assert items.shape[1] >= 1 and n >= 1


def dense(csr, W, items, m, row_lo=0, row_hi=None):
  """rk_ease_explain on the rows [row_lo, row_hi) of the device CSR ``csr`` (an ``als.AlsCSR`` over W's rows) against
  the dense W [n, >= n] f32 (row stride W.stride(0)) and ``items`` int64 [rows, J] on the device: the four outputs on
  the device, nothing synchronised."""
  rows, indptr = _rows(csr, row_lo, row_hi)
  n = int(W.shape[0])
  _check_items(items, rows, n)
  assert W.dtype == torch.float32 and W.stride(1) == 1 and W.shape[1] >= n and csr.shape[1] <= n
  out = _outputs(rows, items.shape[1], m, W.device)
  lib = _ease_lib.load()
  _ease_lib.check(lib.rk_ease_explain(indptr, ptr(csr.indices), ptr(csr.data), rows, ptr(W), W.stride(0), n,
                                      ptr(items), items.shape[1], int(m), *(ptr(o) for o in out), current_stream()),
                  "rk_ease_explain")
  return out


def lists(csr, ids, w, count, columns, items, m, row_lo=0, row_hi=None):
  """rk_slim_explain: ``dense`` for a model stored as neighbour lists (``ids`` int32 [n, K], ``w`` f32 [n, K],
  ``count`` int32 [n]); ``columns``: row j of the tensors is column j of W, else row j."""
  rows, indptr = _rows(csr, row_lo, row_hi)
  n, K = ids.shape
  _check_items(items, rows, n)
  assert ids.dtype == torch.int32 and w.dtype == torch.float32 and count.dtype == torch.int32
  assert ids.is_contiguous() and w.is_contiguous() and w.shape == (n, K) and count.shape == (n,) and csr.shape[1] <= n
  out = _outputs(rows, items.shape[1], m, ids.device)
  lib = _slim_lib.load()
  _slim_lib.check(lib.rk_slim_explain(indptr, ptr(csr.indices), ptr(csr.data), rows, n, ptr(ids), ptr(w), ptr(count),
                                      K, 1 if columns else 0, ptr(items), items.shape[1], int(m),
                                      *(ptr(o) for o in out), current_stream()), "rk_slim_explain")
  return out


def folded(csr, Y, G, v, bias, alpha, items, m, row_lo=0, row_hi=None, ws=None):
  """rk_als_explain on the rows [row_lo, row_hi) of ``csr`` with ``foldin.solve``'s Y, G, v, bias and alpha: the four
  outputs and status int32 [rows] on the device."""
  rows, indptr = _rows(csr, row_lo, row_hi)
  n, h = int(Y.shape[0]), int(Y.shape[1])
  if h > foldin.MAX_H:
    raise ValueError("rk_als_explain takes h <= %d (got %d)" % (foldin.MAX_H, h))
  _check_items(items, rows, n)
  assert Y.dtype == torch.float32 and Y.stride(1) == 1 and tuple(G.shape) == (h, h) and G.is_contiguous()
  assert csr.shape[1] <= n
  out = _outputs(rows, items.shape[1], m, Y.device)
  status = torch.empty(max(rows, 1), dtype=torch.int32, device=Y.device)
  lib = _als_lib.load()
  nnz = int(csr.indices.numel())
  need = lib.rk_als_explain_workspace_bytes(nnz)
  if ws is None or ws.numel() < need:
    ws = torch.empty(need, dtype=torch.uint8, device=Y.device)
  _als_lib.check(lib.rk_als_explain(indptr, ptr(csr.indices), ptr(csr.data), rows, nnz, ptr(Y), Y.stride(0), n, h,
                                    ptr(G), ptr(v), ptr(bias), float(alpha), ptr(items), items.shape[1], int(m),
                                    *(ptr(o) for o in out), ptr(status), ptr(ws), ws.numel(), current_stream()),
                 "rk_als_explain")
  return out + (status[:rows],)


def explain(recoder, users_interactions, items, num_contributors=5, alpha=foldin.DEFAULT_ALPHA,
            reg=foldin.DEFAULT_REG):
  """``Recoder.explain``: an ``Explanation`` of host arrays."""
  from . import als
  matrix = users_interactions.interactions_matrix
  items, m, alpha, reg = check(recoder, matrix, items, num_contributors, alpha, reg)
  model = recoder.model
  if isinstance(model, MatrixFactorization):
    Y = model.item_embedding_layer.weight.data
    bias = model.bias.data
    csr = foldin.batch_csr(matrix, Y.shape[0], Y.device)
    dev_items = torch.from_numpy(items).to(Y.device)
    G, v = als.gram(Y, reg, bias)
    *out, status = folded(csr, Y, G, v, bias, alpha, dev_items, m)
    failed = int(status.sum().item()) if csr.shape[0] else 0
    if failed:
      warnings.warn("explain: %d of %d rows had a system that is not positive definite and were left as zero vectors "
                    "(raise reg)" % (failed, csr.shape[0]), RuntimeWarning, stacklevel=3)
  else:
    W = model.item_weights.data
    csr = foldin.batch_csr(matrix, W.shape[0], W.device)
    dev_items = torch.from_numpy(items).to(W.device)
    if isinstance(model, _NeighbourListModel):
      out = lists(csr, model.item_neighbours, W, model.neighbour_counts, model.lists_spell_columns, dev_items, m)
    else:
      out = dense(csr, W, dev_items, m)
  return Explanation(*(o.cpu().numpy().copy() for o in out))
