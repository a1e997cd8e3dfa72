"""Implicit-feedback alternating least squares for ``MatrixFactorization`` (Hu, Koren & Volinsky 2008,
with the conjugate-gradient row solves of Takacs et al.), on the HIP kernels of librecoder_als.so
(include/recoder_als.h).

The model is a ``MatrixFactorization`` with ``activation_type="none"``: s_ui = x_u . y_i + b_i, with
x = ``user_embedding_layer.weight``, y = ``item_embedding_layer.weight`` and b = ``bias``.  ALS
minimises, over the WHOLE user x item matrix R (zeros off its support),

    L = sum_{u, i} w_ui (r_ui - s_ui)^2 + reg (sum_u |x_u|^2 + sum_i |y_i|^2),  w_ui = 1 + alpha [r_ui > 0]

which is ``MSELoss(confidence=alpha, reduction="sum")`` on the dense output plus the reg term.  b is
held fixed.  One iteration solves every user row with the items fixed, then every item row with the
users fixed, each row with ``cg_steps`` CG steps warm-started from its current value.

``Recoder.train_als`` is the public entry point; the functions below are the layer under it (and what
the tests and tools/als_bench.py drive directly).
"""
import math

import numpy as np
import scipy.sparse as sp
import torch

from . import _als_lib
from ._lib import ptr
from .device import canonical_csr, current_stream
from .losses import MSELoss
from .nn import MatrixFactorization

MAX_H = 512          # rk_als_max_h()


# ------------------------------------------------------------------ config
def check_config(model, loss, loss_params, num_iterations, reg, cg_steps):
  """The ALS contract, checked before any GPU work; returns alpha (the MSE confidence)."""
  if not isinstance(model, MatrixFactorization):
    raise ValueError("train_als trains a MatrixFactorization, not %s" % type(model).__name__)
  if model.activation_type != "none":
    raise ValueError("train_als needs activation_type='none' (got %r)" % (model.activation_type,))
  if model.dropout_prob and model.dropout_prob > 0:
    raise ValueError("train_als needs dropout_prob == 0 (got %r)" % (model.dropout_prob,))
  h = model.embedding_size
  if not isinstance(h, (int, np.integer)) or not 1 <= h <= MAX_H:
    raise ValueError("train_als supports embedding sizes 1..%d (got %r)" % (MAX_H, h))
  if isinstance(loss, str):
    params = loss_params or {}
    if loss != "mse" or set(params) - {"confidence"}:
      raise ValueError("train_als minimises the 'mse' loss with at most a 'confidence' parameter "
                       "(got loss %r, loss_params %r)" % (loss, params))
    alpha = params.get("confidence", 0)
  elif isinstance(loss, MSELoss):
    if loss.reduction != "sum":
      raise ValueError("train_als needs MSELoss(reduction='sum') (got reduction %r)" % (loss.reduction,))
    alpha = loss.confidence
  else:
    raise ValueError("train_als minimises the 'mse' loss (got %r)" % (loss,))
  alpha = float(alpha)
  if not (math.isfinite(alpha) and alpha >= 0):
    raise ValueError("confidence must be finite and >= 0 (got %r)" % (alpha,))
  if isinstance(num_iterations, bool) or not isinstance(num_iterations, (int, np.integer)) or num_iterations < 0:
    raise ValueError("num_iterations must be an integer >= 0 (got %r)" % (num_iterations,))
  if isinstance(cg_steps, bool) or not isinstance(cg_steps, (int, np.integer)) or cg_steps < 1:
    raise ValueError("cg_steps must be an integer >= 1 (got %r)" % (cg_steps,))
  reg = float(reg)
  if not (math.isfinite(reg) and reg >= 0):
    raise ValueError("reg must be finite and >= 0 (got %r)" % (reg,))
  return alpha


def check_not_distributed(message="train_als runs on one GPU: multi-GPU ALS is not implemented"):
  import torch.distributed as dist
  if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
    raise NotImplementedError(message)


# --------------------------------------------------------------------- CSR
class AlsCSR:
  """A CSR in HBM in the layout rk_als_solve reads: int64 indptr, int32 indices, fp32 data (None when
  every value is 1.0)."""

  def __init__(self, m, device):
    m = sp.csr_matrix(m)
    self.shape = m.shape
    self.nnz = int(m.nnz)
    self.indptr = torch.from_numpy(m.indptr.astype(np.int64)).to(device)
    self.indices = torch.from_numpy(np.ascontiguousarray(m.indices, dtype=np.int32)).to(device) if self.nnz \
        else torch.zeros(1, dtype=torch.int32, device=device)
    data = np.asarray(m.data, dtype=np.float32)
    self.data = None if bool((data == 1.0).all()) else torch.from_numpy(data).to(device)


def host_matrix(dataset):
  """The training dataset's interaction matrix on the host (canonical: sorted, no duplicates, no
  explicit zeros), from the scipy matrix or, for a device-only dataset, from its device CSR."""
  if getattr(dataset, "interactions_matrix", None) is not None:
    return canonical_csr(dataset.interactions_matrix)
  d = dataset.device_csr()
  nnz = d.nnz
  indptr = d.indptr.cpu().numpy()
  indices = d.indices[:nnz].cpu().numpy() if nnz else np.zeros(0, np.int32)
  data = d.data[:nnz].cpu().numpy() if d.data is not None else np.ones(nnz, np.float32)
  return sp.csr_matrix((data, indices, indptr), shape=d.shape)


def csr_pair(m, n_users, n_items, device):
  """(user x item CSR, its transpose) padded to the tables' row counts, uploaded once."""
  m = sp.csr_matrix(m)
  if m.shape[0] > n_users or m.shape[1] > n_items:
    raise ValueError("interaction matrix %s larger than the tables (%d users, %d items)"
                     % (m.shape, n_users, n_items))
  indptr = np.concatenate([m.indptr, np.full(n_users - m.shape[0], m.indptr[-1], m.indptr.dtype)])
  m = sp.csr_matrix((m.data, m.indices, indptr), shape=(n_users, n_items))
  mt = m.T.tocsr()
  mt.sort_indices()
  return AlsCSR(m, device), AlsCSR(mt, device)


# ------------------------------------------------------------------ kernels
def gram(F, reg, w=None, ws=None):
  """(G, v): G = F^T F + reg I [h, h], v = F^T w (w None: the column sums), f32 (rk_als_gram)."""
  lib = _als_lib.load()
  rows, h = F.shape
  need = lib.rk_als_gram_workspace_bytes(rows, h)
  if ws is None or ws.numel() < need:
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=F.device)
  G = torch.empty(h, h, dtype=torch.float32, device=F.device)
  v = torch.empty(h, dtype=torch.float32, device=F.device)
  ldf = F.stride(0) if rows else h              # (an empty table's stride is arbitrary)
  _als_lib.check(lib.rk_als_gram(ptr(F), rows, h, ldf, ptr(w), float(reg), ptr(G), ptr(v), ptr(ws),
                                 ws.numel(), current_stream()), "rk_als_gram")
  return G, v


def solve(csr, F, G, v, X, alpha, cg_steps, col_bias=None, row_bias=None, row_lo=0, row_hi=None, flags=0):
  """cg_steps CG steps on rows [row_lo, row_hi) of X (in place) with F fixed (rk_als_solve)."""
  row_hi = csr.shape[0] if row_hi is None else row_hi
  assert 0 <= row_lo <= row_hi <= min(csr.shape[0], X.shape[0]) and F.shape[0] >= csr.shape[1]
  assert X.shape[1] == F.shape[1] == G.shape[0] and X.stride(1) == 1 and F.stride(1) == 1
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_solve(ptr(csr.indptr), ptr(csr.indices), ptr(csr.data), row_lo, row_hi, ptr(F),
                                  F.stride(0), F.shape[1], ptr(G), ptr(v), ptr(col_bias), ptr(row_bias),
                                  float(alpha), int(cg_steps), ptr(X), X.stride(0), int(flags),
                                  current_stream()), "rk_als_solve")


def objective(csr, X, Y, bias, alpha, reg, Gx, sx, Gy, cy, out, ws=None):
  """out[0] = L (float64, on the device) for the user x item CSR (rk_als_objective); Gx, sx from
  gram(X, reg), Gy, cy from gram(Y, reg, bias)."""
  lib = _als_lib.load()
  rows, h = X.shape
  need = lib.rk_als_objective_workspace_bytes(rows)
  if ws is None or ws.numel() < need:
    ws = torch.empty(need, dtype=torch.uint8, device=X.device)
  _als_lib.check(lib.rk_als_objective(ptr(csr.indptr), ptr(csr.indices), ptr(csr.data), rows, Y.shape[0],
                                      ptr(X), X.stride(0), ptr(Y), Y.stride(0), h, ptr(bias), float(alpha),
                                      float(reg), ptr(Gx), ptr(Gy), ptr(sx), ptr(cy), ptr(ws), ws.numel(),
                                      ptr(out), current_stream()), "rk_als_objective")


# ---------------------------------------------------------------------- fit
def fit(X, Y, bias, ucsr, icsr, alpha, reg, cg_steps, num_iterations):
  """num_iterations ALS iterations on the tables X [users, h], Y [items, h] (in place, f32, row-major);
  returns L after each iteration (floats).  One host synchronisation, at the end."""
  lib = _als_lib.load()
  dev = X.device
  gws_bytes = max(lib.rk_als_gram_workspace_bytes(X.shape[0], X.shape[1]),
                  lib.rk_als_gram_workspace_bytes(Y.shape[0], Y.shape[1]), 4)
  gws = torch.empty(gws_bytes, dtype=torch.uint8, device=dev)
  ows = torch.empty(lib.rk_als_objective_workspace_bytes(X.shape[0]), dtype=torch.uint8, device=dev)
  hist = torch.zeros(max(num_iterations, 1), dtype=torch.float64, device=dev)
  if num_iterations == 0:
    return []
  Gy, cy = gram(Y, reg, bias, gws)
  for it in range(num_iterations):
    solve(ucsr, Y, Gy, cy, X, alpha, cg_steps, col_bias=bias)
    Gx, sx = gram(X, reg, None, gws)
    solve(icsr, X, Gx, sx, Y, alpha, cg_steps, row_bias=bias)
    Gy, cy = gram(Y, reg, bias, gws)
    objective(ucsr, X, Y, bias, alpha, reg, Gx, sx, Gy, cy, hist[it:], ows)
  return hist[:num_iterations].cpu().tolist()
