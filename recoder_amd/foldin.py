"""Fold-in: the user row of a history the fit has not seen, for any ``MatrixFactorization`` state with
``activation_type="none"``, on rk_als_foldin of librecoder_als.so (include/recoder_als.h).

Whatever trainer left the item table Y and the bias b, a user with the history r (a sparse row over the model's
items) is given the row that minimises the ALS user objective with Y and b held fixed,

    x = argmin_x sum_i w_i (r_i - x . y_i - b_i)^2 + reg |x|^2,   w_i = 1 + alpha [r_i > 0],

over ALL items (zeros off the history's support): the user half-step of ``recoder_amd/als.py`` solved exactly, by a
Cholesky factorisation of the h x h normal equations, instead of by a few conjugate-gradient steps from the row's
current value -- a new user has no current value.  With alpha = 0 and reg = 0 on a PureSVD state (Y orthonormal,
b = 0) this is the projection x = V^T r, the model's own user row; on an ALS state at the fit's confidence and reg it
is the exact minimiser of the user half-step.  For the other trainers (BPR, WARP, LightGCN, SimGCL, DirectAU, SSM,
UltraGCN, CCL, SimpleX) it is a least-squares projection onto the item table as it stands: their own loss plays no
part, and LightGCN's graph is not propagated again.

G = Y^T Y + reg I and v = Y^T b are recomputed on every call (rk_als_gram): a cache would go stale after any trainer.
The kernel takes h <= ``MAX_H``; a larger state is refused, there is no other path.

``Recoder.fold_in``, ``Recoder.recommend_folded`` and ``recommender.FoldInRecommender`` are the public entry points.
"""
import math
import numbers
import warnings

import scipy.sparse as sp
import torch

from . import _als_lib, als
from ._lib import ptr
from .device import current_stream
from .nn import MatrixFactorization

MAX_H = _als_lib.FOLDIN_MAX_H          # rk_als_foldin_max_h()
# the best Recall@20 cell of tools/foldin_bench.py --cpu-grid for the ALS state (profiles/foldin_quality.jsonl)
DEFAULT_ALPHA = 30.0
DEFAULT_REG = 100.0


def _number(name, value):
  if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value) or value < 0:
    raise ValueError("%s must be a finite number >= 0 (got %r)" % (name, value))
  return float(value)


def check_config(model, alpha, reg):
  """The contract of ``fold_in``, checked before any GPU work; returns (alpha, reg) as floats."""
  if not isinstance(model, MatrixFactorization):
    raise ValueError("fold_in serves a MatrixFactorization, not %s" % type(model).__name__)
  if model.activation_type != "none":
    raise ValueError("fold_in needs activation_type='none' (got %r)" % (model.activation_type,))
  h = model.embedding_size
  if isinstance(h, bool) or not isinstance(h, numbers.Integral) or not 1 <= h <= MAX_H:
    raise ValueError("fold_in supports embedding sizes 1..%d (got %r): a larger state serves known users only"
                     % (MAX_H, h))
  alpha, reg = _number("alpha", alpha), _number("reg", reg)
  if model.item_embedding_layer is None:
    raise ValueError("fold_in needs an initialised model: train it or load a checkpoint first")
  return alpha, reg


def check_not_distributed():
  """ValueError under more than one rank."""
  try:
    als.check_not_distributed("fold_in runs on one GPU: multi-GPU fold-in is not implemented")
  except NotImplementedError as e:
    raise ValueError(str(e)) from None


def solve(csr, Y, G, v, bias, alpha, X=None, status=None, row_lo=0, row_hi=None):
  """rk_als_foldin on the rows [row_lo, row_hi) of the device CSR ``csr`` (an ``als.AlsCSR``): (X, status), the
  rows' vectors [rows, h] f32 and 1 where a pivot was not positive (that row is zero), else 0."""
  h = Y.shape[1]
  if h > MAX_H:
    raise ValueError("rk_als_foldin takes h <= %d (got %d)" % (MAX_H, h))
  row_hi = csr.shape[0] if row_hi is None else row_hi
  rows = row_hi - row_lo
  assert 0 <= row_lo <= row_hi <= csr.shape[0] and Y.shape[0] >= csr.shape[1]
  assert Y.dtype == torch.float32 and Y.stride(1) == 1 and tuple(G.shape) == (h, h) and G.is_contiguous()
  X = torch.empty((rows, h), dtype=torch.float32, device=Y.device) if X is None else X
  status = torch.empty(rows, dtype=torch.int32, device=Y.device) if status is None else status
  assert X.shape[0] >= rows and X.shape[1] == h and X.stride(1) == 1 and status.numel() >= rows
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_foldin(csr.indptr.data_ptr() + 8 * row_lo, ptr(csr.indices), ptr(csr.data), rows, ptr(Y),
                                   Y.stride(0), h, ptr(G), ptr(v), ptr(bias), float(alpha), ptr(X),
                                   X.stride(0) if rows else h, ptr(status), current_stream()), "rk_als_foldin")
  return X, status


def batch_csr(matrix, n_items, device):
  """The histories as the kernel's CSR: canonical (sorted, no duplicates, no explicit zeros), its columns padded to
  the model's ``n_items``; more columns than that is a ValueError."""
  m = als.canonical_csr(matrix)
  if m.shape[1] > n_items:
    raise ValueError("interactions_matrix has %d columns, the model has %d items" % (m.shape[1], n_items))
  m = sp.csr_matrix((m.data, m.indices, m.indptr), shape=(m.shape[0], n_items))
  return als.AlsCSR(m, device)


def fold_in(recoder, matrix, alpha=DEFAULT_ALPHA, reg=DEFAULT_REG):
  """[B, h] f32 on the device: the folded-in rows of the B histories ``matrix`` (a scipy matrix over the model's
  items) against ``recoder``'s item table and bias as they stand.  A row whose system is not positive definite
  (possible only at reg = 0) comes back as zeros; one warning per call gives their count."""
  alpha, reg = check_config(recoder.model, alpha, reg)
  check_not_distributed()
  Y = recoder.model.item_embedding_layer.weight.data
  bias = recoder.model.bias.data
  csr = batch_csr(matrix, Y.shape[0], Y.device)
  G, v = als.gram(Y, reg, bias)
  X, status = solve(csr, Y, G, v, bias, alpha)
  failed = int(status.sum().item()) if csr.shape[0] else 0
  if failed:
    warnings.warn("fold_in: %d of %d rows had a system that is not positive definite and were left as zero vectors "
                  "(raise reg)" % (failed, csr.shape[0]), RuntimeWarning, stacklevel=2)
  return X
