"""Numpy restatements of SLIM (Ning & Karypis 2011) fitted by cyclic coordinate descent in the
covariance-update form of Friedman, Hastie & Tibshirani 2010, written from the formulas:

    G = X^T X (values >= 0);  column j of W solves
      min over w >= 0, w_j = 0 of  1/2 |x_j - X w|^2 + l2/2 |w|^2 + l1 |w|_1
    candidates of column j: {k != j : G[j, k] > l1}, ascending (with G >= 0 and w >= 0 every other k stays 0)
    state: w[c] = +0, q[c] = G[j, cand[c]]          (q = G_jk - sum_m G_km w_m, own term included)
    sweep, c ascending, k = cand[c]:
      t = fma(G[k, k], w[c], q[c]);  new = (t - l1) * inv_denom[k] if t > l1 else +0;  d = new - w[c]
      d != 0:  q[c'] = fma(-d, G[k, cand[c']], q[c']) for every c' (c included);  w[c] = new
    stop after the first sweep whose max |d| <= tol, or after max_sweeps sweeps
    cut: a support (w > 0) larger than K keeps its K largest by (w descending, id ascending)
    scores = X W

``cd_f32`` restates the f32 chains the kernels promise (``ease_util.fmaf`` for the fused steps), ``cd_f64``
runs the same sweeps in float64.  They are the comparators of the SLIM tests and never the code under test."""
import numpy as np
import scipy.sparse as sp

from tests import ease_util

SLICE = ease_util.SLICE


def gram_f64(X):
  X = sp.csr_matrix(X).astype(np.float64)
  return np.asarray((X.T @ X).todense())


def inv_denom_f64(G, l2):
  """1 / (G_kk + l2) in float64; 0 where the denominator is 0 (such a k is never a candidate)."""
  d = np.diag(np.asarray(G)).astype(np.float64) + float(l2)
  out = np.zeros_like(d)
  out[d > 0] = 1.0 / d[d > 0]
  return out


def candidates(G, j, l1, screen=True):
  row = np.asarray(G[j])
  keep = (row > l1) if screen else np.ones(len(row), bool)
  keep[j] = False
  return np.flatnonzero(keep)


def cd_column_f32(G, j, inv_denom, l1, max_sweeps, tol):
  """(cand, w f32, sweeps) of column j: the f32 chains, one coordinate after the other."""
  G = np.asarray(G, np.float32)
  inv_denom = np.asarray(inv_denom, np.float32)
  l1, tol = np.float32(l1), np.float32(tol)
  cand = candidates(G, j, l1)
  C = len(cand)
  w = np.zeros(C, np.float32)
  if C == 0:
    return cand, w, 0
  q = G[j, cand].copy()
  sub = np.ascontiguousarray(G[np.ix_(cand, cand)])      # sub[c, c'] = G[cand[c], cand[c']]
  diag = sub.diagonal().copy()
  inv = inv_denom[cand]
  sweeps = 0
  for _ in range(int(max_sweeps)):
    sweeps += 1
    maxd = np.float32(0.0)
    for c in range(C):
      t = ease_util.fmaf(diag[c:c + 1], w[c:c + 1], q[c:c + 1])[0]
      new = np.float32(np.float32(t - l1) * inv[c]) if t > l1 else np.float32(0.0)
      d = np.float32(new - w[c])
      if d != 0:
        q = ease_util.fmaf(-d, sub[c], q)
        w[c] = new
        maxd = max(maxd, np.float32(abs(d)))
    if maxd <= tol:
      break
  return cand, w, sweeps


def cd_column_f64(G, j, l1, l2, max_sweeps, tol, sweeps=None, screen=True):
  """(cand, w float64, sweeps run) of column j in float64: exactly ``sweeps`` sweeps when given, otherwise
  the stop rule.  ``screen`` False sweeps every k != j."""
  G = np.asarray(G, np.float64)
  cand = candidates(G, j, l1, screen)
  C = len(cand)
  w = np.zeros(C)
  if C == 0:
    return cand, w, 0
  q = G[j, cand].copy()
  sub = np.ascontiguousarray(G[np.ix_(cand, cand)])
  diag = sub.diagonal().copy()
  denom = diag + float(l2)
  run = 0
  for _ in range(int(max_sweeps) if sweeps is None else int(sweeps)):
    run += 1
    maxd = 0.0
    for c in range(C):
      t = diag[c] * w[c] + q[c]
      new = (t - l1) / denom[c] if t > l1 and denom[c] > 0 else 0.0
      d = new - w[c]
      if d != 0:
        q -= d * sub[c]
        w[c] = new
        maxd = max(maxd, abs(d))
    if sweeps is None and maxd <= tol:
      break
  return cand, w, run


def cut(ids, w, K):
  """The entries > 0 of (ids ascending, w) cut to the K largest by (w descending, id ascending), ids ascending."""
  live = w > 0
  ids, w = ids[live], w[live]
  if len(ids) > K:
    top = np.sort(np.argsort(-w, kind="stable")[:K])       # (ids ascending: a stable sort keeps the lower ids)
    ids, w = ids[top], w[top]
  return ids, w


def cd_f32(G, inv_denom, l1, K, max_sweeps, tol, cols=None):
  """(ids int32 [n, K], w f32 [n, K], count int32 [n], sweeps int32 [n], support int32 [n]) of the f32
  restatement: column j's kept entries with ascending ids, -1 / +0 behind them; ``support`` is the number of
  entries > 0 before the cut.  ``cols``: only these columns (the others stay empty)."""
  n = np.asarray(G).shape[0]
  ids = np.full((n, K), -1, np.int32)
  w = np.zeros((n, K), np.float32)
  count, sweeps, support = (np.zeros(n, np.int32) for _ in range(3))
  for j in (range(n) if cols is None else cols):
    cand, wj, sweeps[j] = cd_column_f32(G, j, inv_denom, l1, max_sweeps, tol)
    support[j] = int((wj > 0).sum())
    kid, kw = cut(cand, wj, K)
    count[j] = len(kid)
    ids[j, :len(kid)] = kid
    w[j, :len(kid)] = kw
  return ids, w, count, sweeps, support


def cd_f64(G, l1, l2, max_sweeps, tol, sweeps=None, screen=True, cols=None):
  """The uncut float64 W [n, n] (column j = the solution of problem j) and the sweeps run per column."""
  n = np.asarray(G).shape[0]
  W = np.zeros((n, n))
  run = np.zeros(n, np.int32)
  for j in (range(n) if cols is None else cols):
    cand, wj, run[j] = cd_column_f64(G, j, l1, l2, max_sweeps, tol, None if sweeps is None else sweeps[j], screen)
    W[cand, j] = wj
  return W, run


def dense(ids, w, count):
  """W [n, n] of the column-stored model: W[ids[j, s], j] = w[j, s]."""
  n, K = ids.shape
  W = np.zeros((n, n), w.dtype)
  live = np.arange(K)[None, :] < count[:, None]
  cols = np.broadcast_to(np.arange(n)[:, None], (n, K))
  W[ids[live], cols[live]] = w[live]
  return W


def scores_f32(X, ids, w, count, lo=0, hi=None):
  """out[u, c]: one ascending f32 fmaf chain from +0 over the kept entries (k, w) of column lo + c whose k
  row u stores, of x_uk * w.  Step s of every (user, column) at once."""
  X = sp.csr_matrix(X).astype(np.float32)
  X.sort_indices()
  n, K = ids.shape
  hi = n if hi is None else hi
  D = np.asarray(X.todense())
  stored = np.zeros(D.shape, bool)
  stored[np.repeat(np.arange(X.shape[0]), np.diff(X.indptr)), X.indices] = True
  out = np.zeros((X.shape[0], hi - lo), np.float32)
  for s in range(K):
    cols = np.flatnonzero(count[lo:hi] > s)
    if not len(cols):
      break
    k = ids[lo + cols, s]
    hit = stored[:, k]                                       # [users, cols]
    step = ease_util.fmaf(D[:, k], w[lo + cols, s][None, :], out[:, cols])
    out[:, cols] = np.where(hit, step, out[:, cols])
  return out


def kkt_residual(G, W, l1, l2, cols):
  """The largest violation of the optimality conditions of columns ``cols`` of W (float64): with
  r = G[:, j] - G w_j,  |r_k - l1 - l2 w_k| on the support,  max(0, r_k - l1) off it (k != j)."""
  G = np.asarray(G, np.float64)
  worst = 0.0
  for j in cols:
    wj = np.asarray(W[:, j], np.float64)
    r = G[:, j] - G @ wj
    on = wj > 0
    off = ~on
    off[j] = False
    if on.any():
      worst = max(worst, float(np.abs(r[on] - l1 - l2 * wj[on]).max()))
    if off.any():
      worst = max(worst, float(np.maximum(r[off] - l1, 0.0).max()))
  return worst
