"""rk_ease_explain, rk_slim_explain and rk_als_explain (include/recoder_ease.h, recoder_slim.h, recoder_als.h) restated
in numpy in their own order of f32 operations, bit for bit, the same definitions in plain float64, and the cases
tests/test_explain_host.py and tests/test_explain.py share.

The Cholesky is tests/foldin_util.foldin_row32's, statement for statement, split so that the factor can be kept and
solved against several right-hand sides; test_explain_host.py holds ``factor32`` + ``solve32`` to ``foldin_row32`` bit
for bit."""
import functools

import numpy as np
import scipy.sparse as sp

from .als_util import _fma
from . import foldin_util as FU

F32 = np.float32
MAX_M = 64


# ------------------------------------------------------------------------------------------------ order and selection
def order(c):
  """The positions of the contributions ``c`` best first: numbers before NaNs, the larger value first (-0 and +0 one
  value), equal values to the earlier position."""
  c = np.asarray(c)
  nan = np.isnan(c)
  return np.lexsort((np.arange(len(c)), np.where(nan, 0, -c), nan))


def select(cols, c, m):
  """(contributors int64 [m], contributions [m]) of a pair: the m best, -1 / 0 where the row has fewer."""
  ids = np.full(m, -1, np.int64)
  vals = np.zeros(m, np.asarray(c).dtype)
  o = order(c)[:m]
  ids[:len(o)] = np.asarray(cols, np.int64)[o]
  vals[:len(o)] = np.asarray(c)[o]
  return ids, vals


def _scalar(x):
  return np.asarray(x, F32).reshape(-1)[0]


def _pad(m, dtype):
  return np.full(m, -1, np.int64), np.zeros(m, dtype), dtype(0), dtype(0)


# ------------------------------------------------------------------------------------------------ item-item models
def item_pair32(cols, vals, wcol, m):
  """One (user, target) of the item-item kernels: ``wcol`` = W[cols, j] f32.  c_e one rounded product, total one
  fmaf chain in CSR order from +0.  Returns (contributors, contributions, baseline, total)."""
  n = len(cols)
  x = np.ones(n, F32) if vals is None else np.asarray(vals, F32)
  w = np.asarray(wcol, F32)
  with np.errstate(invalid="ignore", over="ignore"):
    c = x * w
    t = F32(0)
    for e in range(n):
      t = _scalar(_fma(x[e], w[e], t, F32))
  assert c.dtype == F32
  ids, kept = select(cols, c, m)
  return ids, kept, F32(0), t


def item_pair64(cols, vals, wcol, m):
  n = len(cols)
  x = np.ones(n) if vals is None else np.asarray(vals, F32).astype(np.float64)
  c = x * np.asarray(wcol, F32).astype(np.float64)
  ids, kept = select(cols, c, m)
  return ids, kept, 0.0, float(c.sum())


def _rows(csr, use_data):
  csr = sp.csr_matrix(csr)
  for u in range(csr.shape[0]):
    lo, hi = csr.indptr[u], csr.indptr[u + 1]
    yield csr.indices[lo:hi], (csr.data[lo:hi] if use_data else None)


def item_explain(csr, W, items, m, use_data=True, pair=item_pair32):
  """The four arrays of rk_ease_explain / rk_slim_explain for a dense W [n, n]."""
  dt = F32 if pair is item_pair32 else np.float64
  B, J = items.shape
  out = (np.empty((B, J, m), np.int64), np.empty((B, J, m), dt), np.empty((B, J), dt), np.empty((B, J), dt))
  for u, (cols, vals) in enumerate(_rows(csr, use_data)):
    for q in range(J):
      j = items[u, q]
      r = _pad(m, dt) if j < 0 else pair(cols, vals, W[cols, j], m)
      for o, x in zip(out, r):
        o[u, q] = x
  return out


def lists_to_dense(ids, w, count, columns):
  """``_NeighbourListModel.dense_weights`` on the host."""
  n, K = ids.shape
  W = np.zeros((n, n), F32)
  for r in range(n):
    for s in range(min(max(int(count[r]), 0), K)):
      if columns:
        W[ids[r, s], r] = w[r, s]
      else:
        W[r, ids[r, s]] = w[r, s]
  return W


# ------------------------------------------------------------------------------------------------ folded-in MF
def factor32(cols, vals, Y, G, alpha):
  """(L, dg, status): A_u and its Cholesky factor as ``foldin_row32`` forms them (L's strict lower triangle and the
  roots dg); status 1 and None factors where a pivot is not > 0."""
  h = np.asarray(G).shape[0]
  cols = np.asarray(cols, np.int64)
  n = len(cols)
  y = np.asarray(Y, F32)[cols, :h].reshape(n, h)
  vals = np.ones(n, F32) if vals is None else np.asarray(vals, F32)
  a = np.where(vals > 0, F32(alpha), F32(0)).astype(F32)
  with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
    A = np.tril(np.asarray(G, F32)[:h, :h])
    for e in np.flatnonzero(a != 0):
      t = a[e] * y[e]
      A = _fma(t[:, None], y[e][None, :], A, F32)
    dg = np.zeros(h, F32)
    for j in range(h):
      d = A[j, j]
      if not d > 0:
        return None, None, 1
      dg[j] = np.sqrt(d)
      A[j + 1:, j] = A[j + 1:, j] / dg[j]
      col = A[j + 1:, j]
      A[j + 1:, j + 1:] = _fma(-col[:, None], col[None, :], A[j + 1:, j + 1:], F32)
  assert A.dtype == F32
  return A, dg, 0


def solve32(L, dg, rhs):
  """A^-1 rhs by ``foldin_row32``'s two triangular solves."""
  r = np.array(rhs, F32)
  h = len(r)
  with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
    for k in range(h):
      r[k] = r[k] / dg[k]
      r[k + 1:] = _fma(-L[k + 1:, k], r[k], r[k + 1:], F32)
    for k in range(h - 1, -1, -1):
      r[k] = r[k] / dg[k]
      r[:k] = _fma(-L[k, :k], r[k], r[:k], F32)
  return r


def coef32(cols, vals, bias, alpha):
  n = len(cols)
  vals = np.ones(n, F32) if vals is None else np.asarray(vals, F32)
  a = np.where(vals > 0, F32(alpha), F32(0)).astype(F32)
  b = np.asarray(bias, F32)[np.asarray(cols, np.int64)] if bias is not None else np.zeros(n, F32)
  coef = (F32(1) + a) * vals - a * b
  assert coef.dtype == F32
  return coef


def _dot32(z, y):
  """d = fmaf(z_k, y[..., k], d) over k ascending from +0; y [h] or [n, h]."""
  y = np.asarray(y, F32)
  d = np.zeros(y.shape[:-1], F32)
  for k in range(len(z)):
    d = _fma(z[k], y[..., k], d, F32).astype(F32)
  return d


def mf_row32(cols, vals, Y, G, v, bias, alpha, targets, m):
  """rk_als_explain for one row: (contributors [J, m], contributions [J, m], baseline [J], total [J], status)."""
  h = np.asarray(G).shape[0]
  cols = np.asarray(cols, np.int64)
  J = len(targets)
  out = (np.empty((J, m), np.int64), np.empty((J, m), F32), np.empty(J, F32), np.empty(J, F32))
  L, dg, status = factor32(cols, vals, Y, G, alpha)
  Yh = np.asarray(Y, F32)[:, :h]
  coef = coef32(cols, vals, bias, alpha)
  for q, j in enumerate(targets):
    if j < 0:
      r = _pad(m, F32)
    elif status:
      r = select(cols, np.zeros(len(cols), F32), m) + (F32(0), F32(0))
    else:
      with np.errstate(invalid="ignore", over="ignore"):
        z = solve32(L, dg, Yh[j])
        base = (F32(bias[j]) if bias is not None else F32(0)) - _scalar(_dot32(z, np.asarray(v, F32)[:h]))
        c = coef * _dot32(z, Yh[cols].reshape(len(cols), h))
        t = F32(base)
        for e in range(len(cols)):
          t = F32(t + c[e])
      assert c.dtype == F32 and np.asarray(base).dtype == F32
      r = select(cols, c, m) + (F32(base), t)
    for o, x in zip(out, r):
      o[q] = x
  return out + (status,)


def mf_row64(cols, vals, Y, G, v, bias, alpha, targets, m):
  """The same definitions in float64 from the same f32 inputs: A_u and the right-hand side are ``foldin_util``'s
  ``normal_equations64``.  Also returns the score y_j . x_u + b_j with x_u the float64 fold-in, per target."""
  h = np.asarray(G).shape[0]
  cols = np.asarray(cols, np.int64)
  J = len(targets)
  A, rhs = FU.normal_equations64(cols, vals, Y, G, v, bias, alpha)
  x = np.linalg.solve(A, rhs)
  Y64 = np.asarray(Y, F32)[:, :h].astype(np.float64)
  n = len(cols)
  val = np.ones(n) if vals is None else np.asarray(vals, F32).astype(np.float64)
  a = np.where(val > 0, float(F32(alpha)), 0.0)
  b = np.asarray(bias, F32).astype(np.float64) if bias is not None else np.zeros(Y64.shape[0])
  coef = (1 + a) * val - a * b[cols]
  out = (np.empty((J, m), np.int64), np.empty((J, m)), np.empty(J), np.empty(J))
  score = np.zeros(J)
  sums = np.zeros(J)                                          # sum |c_e| + |baseline|: the scale of a pair
  for q, j in enumerate(targets):
    if j < 0:
      r = _pad(m, np.float64)
    else:
      z = np.linalg.solve(A, Y64[j])
      base = b[j] - z @ np.asarray(v, F32)[:h].astype(np.float64)
      c = coef * (Y64[cols].reshape(n, h) @ z)
      r = select(cols, c, m) + (base, base + c.sum())
      score[q] = Y64[j] @ x + b[j]
      sums[q] = np.abs(c).sum() + abs(base)
    for o, x_ in zip(out, r):
      o[q] = x_
  return out + (score, sums)


def mf_explain32(csr, Y, G, v, bias, alpha, items, m, use_data=True):
  """(contributors, contributions, baseline, total, status) of rk_als_explain."""
  rows = [mf_row32(cols, vals, Y, G, v, bias, alpha, items[u], m) for u, (cols, vals) in enumerate(_rows(csr, use_data))]
  return tuple(np.stack([r[i] for r in rows]) for i in range(4)) + (np.array([r[4] for r in rows], np.int32),)


# ---------------------------------------------------------------------------------------------------------------------
# The cases.  Ten users over 300 items whose history lengths are {0, 1, m - 1, m, m + 1, 63, 64, 65, 300} for every m of
# MS; the tests run them as the two batches of B = 7, users [0, 7) and [3, 10), which is also the sub-range check.
N_ITEMS = 300
B = 7
LENGTHS = (0, 1, 2, 4, 5, 6, 63, 64, 65, 300)
BATCHES = ((0, 7), (3, 10))
MS = (1, 5, 64)
JS = (1, 3)
KS = (1, 10, 64)
HS = (1, 3, 64, 65, 128)
ABSENT = 7                    # a target that no neighbour list holds and whose own list is empty
# (name, alpha, CSR values given, bias given): fold-in's
VARIANTS = (("values", 30.0, True, True), ("ones", 30.0, False, True), ("alpha 0", 0.0, True, True),
            ("no bias", 30.0, True, False))


@functools.lru_cache(maxsize=None)
def histories():
  """(csr with non-unit values, items [10, 3]): targets with -1 among them, a duplicate, one that is in the history,
  ABSENT, and a -1 in the first column (what J = 1 reads)."""
  rng = np.random.RandomState(41)
  lens = list(LENGTHS)
  indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  indices = np.concatenate([np.sort(rng.choice(N_ITEMS, n, replace=False)) for n in lens]).astype(np.int32)
  nnz = len(indices)
  vals = np.where(rng.rand(nnz) < 0.75, rng.randint(1, 17, nnz), rng.randint(-16, 0, nnz)) / 2.0
  csr = sp.csr_matrix((vals.astype(F32), indices, indptr), shape=(len(lens), N_ITEMS))
  items = rng.randint(0, N_ITEMS, (len(lens), 3)).astype(np.int64)
  for u in range(len(lens)):
    row = csr.indices[csr.indptr[u]:csr.indptr[u + 1]]
    if u % 3 == 0:
      items[u, 1] = -1
    if u % 3 == 1:
      items[u, 2] = items[u, 0]                               # a duplicate
    if len(row):
      items[u, u % 2] = row[len(row) // 2]                    # a target that is in the history
  items[4, 0] = -1
  items[6, 2] = items[9, 0] = ABSENT
  items[8, 0] = items[5, 1] = 0                               # an even column: quantised weights, ties
  assert (items == -1).any() and (items[:, 0] == -1).any()
  csr.data.setflags(write=False), items.setflags(write=False)
  return csr, items


@functools.lru_cache(maxsize=None)
def dense_w():
  """W [300, 300] f32 with negative entries; the even columns hold multiples of 1/4 in [-1, 1], so that with all-ones
  values many history items tie exactly; zero diagonal."""
  rng = np.random.RandomState(42)
  W = rng.randn(N_ITEMS, N_ITEMS).astype(F32)
  W[:, ::2] = (rng.randint(-4, 5, (N_ITEMS, N_ITEMS // 2)) / 4.0).astype(F32)
  np.fill_diagonal(W, 0)
  W.setflags(write=False)
  return W


@functools.lru_cache(maxsize=None)
def neighbour_lists(K):
  """(ids int32 [n, K] ascending, -1 behind the count; w f32 [n, K]; count int32 [n]) with empty lists among them and
  ABSENT in none; every third list holds multiples of 1/4."""
  rng = np.random.RandomState(43 + K)
  pool = np.array([i for i in range(N_ITEMS) if i != ABSENT])
  count = rng.randint(0, K + 1, N_ITEMS).astype(np.int32)
  count[::11] = 0
  count[ABSENT] = 0
  count[1] = K
  ids = np.full((N_ITEMS, K), -1, np.int32)
  w = np.zeros((N_ITEMS, K), F32)
  for r in range(N_ITEMS):
    ids[r, :count[r]] = np.sort(rng.choice(pool, count[r], replace=False))
    w[r, :count[r]] = rng.randn(count[r]) if r % 3 else rng.randint(-4, 5, count[r]) / 4.0
  assert (count == 0).sum() > 1 and not (ids == ABSENT).any()
  for a in (ids, w, count):
    a.setflags(write=False)
  return ids, w, count


@functools.lru_cache(maxsize=None)
def want_items(which, m, use_data):
  """The restatement's four arrays for all ten users and J = 3 against ``which``: "dense" or (K, columns)."""
  csr, items = histories()
  W = dense_w() if which == "dense" else lists_to_dense(*neighbour_lists(which[0]), which[1])
  out = item_explain(csr, W, items, m, use_data)
  for o in out:
    o.setflags(write=False)
  return out


@functools.lru_cache(maxsize=None)
def mf_problem(h):
  """Y, G, v, bias over the 300 items at embedding size h; reg = 1e-2 tr(Y^T Y) / h (``foldin_util.problem``'s)."""
  rng = np.random.RandomState(3000 + h)
  Y = (0.1 * rng.randn(N_ITEMS, h)).astype(F32)
  Y64 = Y.astype(np.float64)
  G = Y64.T @ Y64
  reg = 1e-2 * np.trace(G) / h
  G = (0.5 * (G + G.T) + reg * np.eye(h)).astype(F32)
  bias = (rng.randint(-255, 256, N_ITEMS) / 256.0).astype(F32)
  v = (Y64.T @ bias.astype(np.float64)).astype(F32)
  return dict(Y=Y, G=G, v=v, bias=bias)


def variant_inputs(p, bias_given):
  return (p["v"], p["bias"]) if bias_given else (np.zeros_like(p["v"]), None)


@functools.lru_cache(maxsize=None)
def want_mf(h, variant):
  """The restatement's arrays at m = 64 and J = 3 for all ten users (a smaller m is their first m columns)."""
  csr, items = histories()
  p = mf_problem(h)
  _, alpha, use_data, bias_given = VARIANTS[variant]
  v, bias = variant_inputs(p, bias_given)
  out = mf_explain32(csr, p["Y"], p["G"], v, bias, alpha, items, MAX_M, use_data)
  for o in out:
    o.setflags(write=False)
  return out


def cut(out, lo, hi, J, m):
  """Users [lo, hi), the first J targets and the first m contributors of the arrays of a full restatement."""
  ids, c, base, tot = out[:4]
  return ids[lo:hi, :J, :m], c[lo:hi, :J, :m], base[lo:hi, :J], tot[lo:hi, :J]


@functools.lru_cache(maxsize=None)
def mf_error(h, variant):
  """The largest error of the f32 restatement against float64 over the case's pairs, relative to the pair's scale
  sum |c_e| + |baseline| (float64): of any contribution, of the baseline and of the total."""
  csr, items = histories()
  p = mf_problem(h)
  _, alpha, use_data, bias_given = VARIANTS[variant]
  v, bias = variant_inputs(p, bias_given)
  worst = 0.0
  for u, (cols, vals) in enumerate(_rows(csr, use_data)):
    got = mf_row32(cols, vals, p["Y"], p["G"], v, bias, alpha, items[u], len(cols) or 1)
    ref = mf_row64(cols, vals, p["Y"], p["G"], v, bias, alpha, items[u], len(cols) or 1)
    for q, j in enumerate(items[u]):
      if j < 0 or ref[5][q] == 0:
        continue
      # the kept lists are permutations of the whole row at m = len: compare by item id
      c32 = dict(zip(got[0][q], got[1][q].astype(np.float64)))
      err = max([abs(c32[i] - c) for i, c in zip(ref[0][q], ref[1][q])] +
                [abs(float(got[2][q]) - ref[2][q]), abs(float(got[3][q]) - ref[3][q])])
      worst = max(worst, err / ref[5][q])
  return worst


def item_error():
  """The same figure for the item-item restatement on the dense case: |total32 - total64| / sum |c_e| (a contribution
  is one rounded product, at most 2^-24 relative)."""
  csr, items = histories()
  W = dense_w()
  worst = 0.0
  for use_data in (True, False):
    t32 = item_explain(csr, W, items, 1, use_data)[3]
    for u, (cols, vals) in enumerate(_rows(csr, use_data)):
      for q, j in enumerate(items[u]):
        if j < 0 or not len(cols):
          continue
        x = np.ones(len(cols)) if vals is None else vals.astype(np.float64)
        c = x * W[cols, j].astype(np.float64)
        if np.abs(c).sum():
          worst = max(worst, abs(float(t32[u, q]) - c.sum()) / np.abs(c).sum())
  return worst


def singular_case():
  """``foldin_util.singular_problem`` with a history: alpha = 0 leaves A_u = G, whose second pivot is exactly 0."""
  s = FU.singular_problem()
  csr = sp.csr_matrix(np.array([[2.0, 0, 1.0, 0]], F32))
  return dict(s, csr=csr, items=np.array([[1, -1, 2]], np.int64), alpha=0.0)
