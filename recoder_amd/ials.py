"""iALS++ (Rendle, Krichene, Zhang & Koren 2021, "iALS++: Speeding up Matrix Factorization with Subspace
Optimization") for ``MatrixFactorization``, on the objective of Rendle, Krichene, Zhang & Koren 2022 ("Revisiting the
Performance of iALS on Item Recommendation Benchmarks"), on the rk_als_ials_* kernels of librecoder_als.so
(include/recoder_als.h).

The model is a ``MatrixFactorization`` with ``activation_type="none"`` and the bias 0; the stored values play no part.
With S the stored entries, r_u and d_i the row and column counts, X the user table and Y the item table,

    L = sum_{(u,i) in S} (x_u . y_i - 1)^2 + alpha0 sum_u sum_i (x_u . y_i)^2 + sum_u lam_u |x_u|^2 + sum_i mu_i |y_i|^2
    lam_u = reg (r_u + alpha0 n_items)^nu        mu_i = reg (d_i + alpha0 n_users)^nu

(lam and mu in float64 on the host, rounded once to f32).  A sweep visits the blocks of ``block_size`` coordinates in
ascending order -- all users for a block, then all items for it -- and solves each row's block exactly by one
Cholesky against a cache of the stored entries' predictions, so that a block step costs O(r k^2 + k^3) instead of
O(r h^2 + h^3); ``block_size = h`` is exact ALS.  The cache is recomputed from the tables at the start of every sweep.

``Recoder.train_ials`` is the public entry point; the functions below are the layer under it (and what the tests and
tools/ials_bench.py drive directly).
"""
import math
import numbers
import warnings

import numpy as np
import scipy.sparse as sp
import torch

from . import _als_lib, als
from ._lib import ptr
from .bpr import DEVICE_HBM_BYTES
from .device import current_stream
from .nn import MatrixFactorization

MAX_H = _als_lib.IALS_MAX_H                # rk_als_ials_max_h()
MAX_BLOCK = _als_lib.IALS_MAX_BLOCK        # rk_als_ials_max_block()
LONG_ROW = _als_lib.IALS_LONG_ROW          # RK_ALS_IALS_LONG_ROW
GRAM_MAX_H = als.MAX_H                     # rk_als_gram's limit: above it the full Grams are stacked from panels
# the best Recall@20 cell of tools/ials_bench.py --cpu-grid (profiles/ials_quality.jsonl)
DEFAULT_ALPHA0 = 0.03
DEFAULT_REG = 0.03

check_not_distributed = als.check_not_distributed


# ------------------------------------------------------------------ config
def _number(name, value):
  if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value) or value < 0:
    raise ValueError("%s must be a finite number >= 0 (got %r)" % (name, value))
  return float(value)


def _count(name, value, lo, hi=None):
  if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value < lo or (hi is not None and value > hi):
    raise ValueError("%s must be an integer in %d..%s (got %r)" % (name, lo, "" if hi is None else hi, value))
  return int(value)


def check_config(model, num_sweeps, block_size, alpha0, reg, nu, init_std=None, seed=0):
  """The contract of ``train_ials``, checked before any GPU work; returns (num_sweeps, block_size, alpha0, reg, nu,
  init_std, seed) with ``block_size`` cut to h."""
  if not isinstance(model, MatrixFactorization):
    raise ValueError("train_ials trains a MatrixFactorization, not %s" % type(model).__name__)
  if model.activation_type != "none":
    raise ValueError("train_ials needs activation_type='none' (got %r)" % (model.activation_type,))
  if model.dropout_prob and model.dropout_prob > 0:
    raise ValueError("train_ials needs dropout_prob == 0 (got %r)" % (model.dropout_prob,))
  h = model.embedding_size
  if isinstance(h, bool) or not isinstance(h, numbers.Integral) or not 1 <= h <= MAX_H:
    raise ValueError("train_ials supports embedding sizes 1..%d (got %r)" % (MAX_H, h))
  num_sweeps = _count("num_sweeps", num_sweeps, 0)
  block_size = min(_count("block_size", block_size, 1, MAX_BLOCK), int(h))
  alpha0, reg, nu = _number("alpha0", alpha0), _number("reg", reg), _number("nu", nu)
  if init_std is not None:
    init_std = _number("init_std", init_std)
  if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not -2 ** 63 <= seed < 2 ** 63:
    raise ValueError("seed must be an integer that fits 64 bits (got %r)" % (seed,))
  return num_sweeps, block_size, alpha0, reg, nu, init_std, int(seed)


def regularisers(row_counts, col_counts, alpha0, reg, nu):
  """(lam, mu) in float64: reg (r_u + alpha0 n_items)^nu per user, reg (d_i + alpha0 n_users)^nu per item.  nu = 0 is
  ``reg`` for every row, a row without entries at alpha0 = 0 included."""
  r, d = np.asarray(row_counts, np.float64), np.asarray(col_counts, np.float64)
  if nu == 0:
    return np.full(r.shape, float(reg)), np.full(d.shape, float(reg))
  return reg * (r + alpha0 * d.shape[0]) ** nu, reg * (d + alpha0 * r.shape[0]) ** nu


def blocks(h, block_size):
  """[(p0, k)] of a sweep: ascending, the last one narrower when ``block_size`` does not divide h."""
  return [(p0, min(int(block_size), h - p0)) for p0 in range(0, h, int(block_size))]


# --------------------------------------------------------------------- CSR
def transpose_permutation(m):
  """(mt, perm): the item-major CSR of the canonical user-major CSR ``m`` (rows ascending) and, for each of its
  entries, the position of the same (user, item) pair in ``m``'s entry order (int64)."""
  m = sp.csr_matrix(m)
  tagged = sp.csr_matrix((np.arange(1, m.nnz + 1, dtype=np.int64), m.indices, m.indptr), shape=m.shape)
  mt = tagged.T.tocsr()
  mt.sort_indices()
  perm = np.asarray(mt.data, np.int64) - 1
  return sp.csr_matrix((np.ones(mt.nnz, np.float32), mt.indices, mt.indptr), shape=mt.shape), perm


class Pair:
  """What a fit reads of the matrix, uploaded once: the user-major CSR, its transpose, the permutation from the
  transpose's entries to the user-major cache, and the row and column counts (host)."""

  def __init__(self, m, n_users, n_items, device):
    m = sp.csr_matrix(m)
    if m.shape[0] > n_users or m.shape[1] > n_items:
      raise ValueError("interaction matrix %s larger than the tables (%d users, %d items)"
                       % (m.shape, n_users, n_items))
    if not m.has_sorted_indices:
      m = m.copy()
      m.sort_indices()
    indptr = np.concatenate([m.indptr, np.full(n_users - m.shape[0], m.indptr[-1], m.indptr.dtype)])
    m = sp.csr_matrix((np.ones(m.nnz, np.float32), m.indices, indptr), shape=(n_users, n_items))
    mt, perm = transpose_permutation(m)
    self.nnz = int(m.nnz)
    self.ucsr, self.icsr = als.AlsCSR(m, device), als.AlsCSR(mt, device)
    self.perm = torch.from_numpy(perm).to(device) if self.nnz else torch.zeros(1, dtype=torch.int64, device=device)
    self.row_counts, self.col_counts = np.diff(m.indptr), np.diff(mt.indptr)
    # the rows rk_als_ials_block cuts over a workgroup, listed once (an empty list: that launch is skipped)
    for csr, counts in ((self.ucsr, self.row_counts), (self.icsr, self.col_counts)):
      rows = np.flatnonzero(counts >= LONG_ROW).astype(np.int32)
      csr.n_long = int(rows.shape[0])
      csr.long_rows = torch.from_numpy(rows if csr.n_long else np.zeros(1, np.int32)).to(device)


def csr_pair(m, n_users, n_items, device):
  return Pair(m, n_users, n_items, device)


# ------------------------------------------------------------------ memory
def required_bytes(n_users, n_items, h, nnz, block_size, allocate_model=True, snapshot=False):
  """Device bytes of a fit: the tables and the bias (unless the caller already holds them; ``snapshot``: and the
  copy validation with ``restore_best`` keeps), both CSRs, the permutation, the cache, lam and mu, the panel with its
  chunk workspace, both full Grams and rk_als_gram's workspace or the panels they are stacked from."""
  n_users, n_items, h, nnz, k = int(n_users), int(n_items), int(h), int(nnz), min(int(block_size), int(h))
  model = ((n_users + n_items) * h * 4 + n_items * 4) * (int(bool(allocate_model)) + int(bool(snapshot)))
  csr = (n_users + n_items + 2) * 8 + 2 * max(1, nnz) * 4 + max(1, nnz) * 8
  chunks = max(1, min(64, -(-max(n_users, n_items) // 1024)))
  panel = (chunks + 1) * k * h * 4
  grams = 2 * h * h * 4 + (2 * h * h * 4 + 256 * (h * h + h) * 4 if h <= GRAM_MAX_H else 0)
  return model + csr + max(1, nnz) * 4 + (n_users + n_items) * 4 + panel + grams + 8192


def check_memory(n_users, n_items, h, nnz, block_size, free_bytes=None, allocate_model=True, snapshot=False):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's whole HBM without
  touching a device, then (``free_bytes`` None: asked from the current device) against what is free."""
  args = (int(n_users), int(n_items), int(h), int(nnz), int(block_size))
  whole = required_bytes(*args, True, snapshot)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError("iALS++ over %d users x %d items at h = %d with %d entries and blocks of %d needs %d bytes: more "
                     "than one device's memory (%d bytes); multi-device fits are not implemented"
                     % (args + (whole, DEVICE_HBM_BYTES)))
  need = required_bytes(*args, allocate_model, snapshot)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("iALS++ over %d users x %d items at h = %d with %d entries and blocks of %d needs %d bytes of "
                     "device memory, %d are free" % (args + (need, free_bytes)))
  return need


# ------------------------------------------------------------------ kernels
def _table(T):
  assert T.dtype == torch.float32 and T.dim() == 2 and T.stride(1) == 1, (T.dtype, T.shape, T.stride())
  return T.stride(0) if T.shape[0] > 1 else max(T.stride(0), T.shape[1])


def predict(ucsr, X, Y, cache=None):
  """cache[e] = x_u . y_i for every stored entry of the user-major CSR (rk_als_ials_predict)."""
  h = X.shape[1]
  assert Y.shape[1] == h and X.shape[0] >= ucsr.shape[0] and Y.shape[0] >= ucsr.shape[1]
  if cache is None:
    cache = torch.empty(max(ucsr.nnz, 1), dtype=torch.float32, device=X.device)
  assert cache.dtype == torch.float32 and cache.is_contiguous() and cache.numel() >= ucsr.nnz
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_ials_predict(ptr(ucsr.indptr), ptr(ucsr.indices), ucsr.shape[0], ucsr.nnz, ptr(X),
                                         _table(X), ptr(Y), _table(Y), h, ptr(cache), current_stream()),
                 "rk_als_ials_predict")
  return cache


def panel_workspace(rows, h, k, device):
  need = _als_lib.load().rk_als_ials_panel_workspace_bytes(int(rows), int(h), int(k))
  assert need > 0, (rows, h, k)
  return torch.empty(need, dtype=torch.uint8, device=device)


def gram_panel(F, p0, k, out=None, ws=None):
  """P = F[:, p0 : p0 + k]^T F, [k, h] f32 (rk_als_ials_gram_panel)."""
  rows, h = F.shape
  lib = _als_lib.load()
  if ws is None or ws.numel() < lib.rk_als_ials_panel_workspace_bytes(rows, h, k):
    ws = panel_workspace(rows, h, k, F.device)
  if out is None:
    out = torch.empty(k, h, dtype=torch.float32, device=F.device)
  assert out.dtype == torch.float32 and out.shape[0] >= k and out.shape[1] == h and out.stride(1) == 1
  _als_lib.check(lib.rk_als_ials_gram_panel(ptr(F), rows, _table(F) if rows else h, h, int(p0), int(k), ptr(out),
                                            _table(out), ptr(ws), ws.numel(), current_stream()),
                 "rk_als_ials_gram_panel")
  return out[:k]


def block(csr, perm, F, X, P, reg, alpha0, p0, k, cache, status, row_lo=0, row_hi=None):
  """One block step on the rows [row_lo, row_hi) of ``csr``'s side: X and ``cache`` in place (rk_als_ials_block);
  ``perm`` None on the user side; ``status`` (int32 [1]) counts the rows left unchanged."""
  row_hi = csr.shape[0] if row_hi is None else row_hi
  h = X.shape[1]
  assert 0 <= row_lo <= row_hi <= min(csr.shape[0], X.shape[0]) and F.shape[0] >= csr.shape[1] and F.shape[1] == h
  assert reg.dtype == torch.float32 and reg.is_contiguous() and reg.numel() >= row_hi
  assert status.dtype == torch.int32 and cache.dtype == torch.float32 and cache.numel() >= csr.nnz
  assert perm is None or (perm.dtype == torch.int64 and perm.numel() >= csr.nnz)
  assert P.shape[0] >= k and P.shape[1] == h and P.dtype == torch.float32
  lib = _als_lib.load()
  # (a CSR without the list -- a plain als.AlsCSR -- has every row of the range looked at by the long rows' launch)
  long_rows, n_long = getattr(csr, "long_rows", None), getattr(csr, "n_long", 0)
  _als_lib.check(lib.rk_als_ials_block(ptr(csr.indptr), ptr(csr.indices), ptr(perm), int(row_lo), int(row_hi),
                                       ptr(long_rows), n_long, ptr(F), _table(F), ptr(X), _table(X), h, ptr(P), _table(P), ptr(reg), float(alpha0),
                                       int(p0), int(k), ptr(cache), ptr(status), current_stream()),
                 "rk_als_ials_block")


def full_gram(F, block_size, out=None, ws=None, gws=None):
  """F^T F [h, h] without a ridge: rk_als_gram at reg = 0 while it takes h, the panels stacked above it."""
  h = F.shape[1]
  if h <= GRAM_MAX_H:
    return als.gram(F, 0.0, None, gws)[0]
  out = torch.empty(h, h, dtype=torch.float32, device=F.device) if out is None else out
  for p0, k in blocks(h, block_size):
    gram_panel(F, p0, k, out[p0:p0 + k], ws)
  return out


def objective(cache, nnz, Gx, Gy, X, lam, Y, mu, alpha0, out, ws=None):
  """out[0] = L (float64, on the device) from the cache, the full Grams and the weighted row norms
  (rk_als_ials_objective)."""
  lib = _als_lib.load()
  need = lib.rk_als_ials_objective_workspace_bytes()
  if ws is None or ws.numel() < need:
    ws = torch.empty(need, dtype=torch.uint8, device=X.device)
  h = X.shape[1]
  assert tuple(Gx.shape) == tuple(Gy.shape) == (h, h) and Gx.is_contiguous() and Gy.is_contiguous()
  assert out.dtype == torch.float64
  _als_lib.check(lib.rk_als_ials_objective(ptr(cache), int(nnz), ptr(Gx), ptr(Gy), h, ptr(X), _table(X), X.shape[0],
                                           ptr(lam), ptr(Y), _table(Y), Y.shape[0], ptr(mu), float(alpha0), ptr(ws),
                                           ws.numel(), ptr(out), current_stream()), "rk_als_ials_objective")


# ---------------------------------------------------------------------- fit
def init_tables(X, Y, init_std, seed):
  """Both tables from N(0, init_std^2 / h), from a generator of its own seeded with ``seed`` (torch's global one is
  not touched): X first, then Y, drawn on the host."""
  gen = torch.Generator(device="cpu")
  gen.manual_seed(int(seed) % (2 ** 63))
  scale = float(init_std) / math.sqrt(X.shape[1])
  for T in (X, Y):
    T.copy_(torch.randn(tuple(T.shape), generator=gen, dtype=torch.float32) * scale)


def sweep(X, Y, pair, lam, mu, alpha0, block_size, cache, status, P, ws):
  """One sweep on the tables in place: the cache from the tables, then for every block all users and all items."""
  predict(pair.ucsr, X, Y, cache)
  for p0, k in blocks(X.shape[1], block_size):
    block(pair.ucsr, None, Y, X, gram_panel(Y, p0, k, P, ws), lam, alpha0, p0, k, cache, status)
    block(pair.icsr, pair.perm, X, Y, gram_panel(X, p0, k, P, ws), mu, alpha0, p0, k, cache, status)


def fit(X, Y, pair, alpha0, reg, nu, block_size, num_sweeps, monitor=None):
  """num_sweeps sweeps on the tables X [users, h], Y [items, h] (in place, f32, row-major); returns L after each sweep
  (floats).  One host synchronisation, at the end (validation adds its own per evaluation).  ``monitor`` (a
  ``validation.Monitor``) scores the tables after every sweep that is due, may stop the fit and at the end puts the
  best sweep's tables back; the history keeps every sweep that ran."""
  dev, h = X.device, X.shape[1]
  k = min(int(block_size), h)
  if num_sweeps == 0:
    return []
  check_memory(X.shape[0], Y.shape[0], h, pair.nnz, k, allocate_model=False,
               snapshot=monitor is not None and monitor.restore_best)
  lam64, mu64 = regularisers(pair.row_counts, pair.col_counts, alpha0, reg, nu)
  lam = torch.from_numpy(lam64.astype(np.float32)).to(dev)
  mu = torch.from_numpy(mu64.astype(np.float32)).to(dev)
  cache = torch.empty(max(pair.nnz, 1), dtype=torch.float32, device=dev)
  status = torch.zeros(1, dtype=torch.int32, device=dev)
  P = torch.empty(k, h, dtype=torch.float32, device=dev)
  ws = panel_workspace(max(X.shape[0], Y.shape[0]), h, k, dev)
  ows = torch.empty(_als_lib.load().rk_als_ials_objective_workspace_bytes(), dtype=torch.uint8, device=dev)
  gws = None
  if h <= GRAM_MAX_H:
    lib = _als_lib.load()
    gws = torch.empty(max(lib.rk_als_gram_workspace_bytes(X.shape[0], h), lib.rk_als_gram_workspace_bytes(Y.shape[0], h),
                          4), dtype=torch.uint8, device=dev)
  Gx = Gy = None
  if h > GRAM_MAX_H:
    Gx, Gy = (torch.empty(h, h, dtype=torch.float32, device=dev) for _ in range(2))
  hist = torch.zeros(num_sweeps, dtype=torch.float64, device=dev)
  ran = 0
  for s in range(num_sweeps):
    sweep(X, Y, pair, lam, mu, alpha0, k, cache, status, P, ws)
    objective(cache, pair.nnz, full_gram(X, k, Gx, ws, gws), full_gram(Y, k, Gy, ws, gws), X, lam, Y, mu, alpha0,
              hist[s:], ows)
    ran = s + 1
    if monitor is not None and monitor.due(s) and monitor.epoch_end(s, (X, Y)):
      break
  if monitor is not None:
    monitor.finish((X, Y), ran)
  out = torch.cat([hist[:ran], status.double()]).cpu().tolist()       # (the synchronisation)
  if out[-1]:
    warnings.warn("train_ials: %d block solves met a system that is not positive definite and left their rows "
                  "unchanged (raise reg)" % int(out[-1]), RuntimeWarning, stacklevel=2)
  return out[:-1]
