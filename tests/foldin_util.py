"""rk_als_foldin (include/recoder_als.h, recoder_amd/csrc/als/foldin.h) restated in numpy in its own order of f32
operations, bit for bit, and the float64 solve of the same f32 inputs with the bound the restatement must keep to it.

The bound is counted, not measured: with u = 2^-24 and A the float64 matrix of the row,
    |x - x64| / |x64| <= u (4 h (3 h + 1) + 2 (len + 2)) cond_2(A),
Cholesky's backward-error bound for the factorisation and both triangular solves (Higham 2002, Accuracy and Stability
of Numerical Algorithms, Thm 10.4: |dA| <= 4 h (3 h + 1) u |A| at first order) plus the error of forming A and the
right-hand side: a chain of len fused operations, the product a_e y_k and the rounding of coef_e."""
import functools

import numpy as np
import scipy.sparse as sp

from .als_util import _fma

F32 = np.float32
U = 2.0 ** -24
CHUNK = 16                    # FI_CHUNK: the item rows staged at a time
MAX_H = 128                   # rk_als_foldin_max_h()


def foldin_row32(cols, vals, Y, G, v, bias, alpha):
  """(x [h] f32, status) of one row: ``cols``, ``vals`` its CSR entries in order (vals None: all ones), Y [>, >= h],
  G [h, h] (only its lower triangle is read), v [h], bias [items] or None."""
  h = np.asarray(G).shape[0]
  cols = np.asarray(cols, np.int64)
  n = len(cols)
  y = np.asarray(Y, F32)[cols, :h].reshape(n, h)
  vals = np.ones(n, F32) if vals is None else np.asarray(vals, F32)
  a = np.where(vals > 0, F32(alpha), F32(0)).astype(F32)
  b = np.asarray(bias, F32)[cols] if bias is not None else np.zeros(n, F32)
  with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
    coef = (F32(1) + a) * vals - a * b
    assert coef.dtype == F32
    r = -np.asarray(v, F32)[:h]
    for e in range(n):
      r = _fma(coef[e], y[e], r, F32)
    A = np.tril(np.asarray(G, F32)[:h, :h])                  # (the strict upper triangle below is never meaningful)
    for e in np.flatnonzero(a != 0):
      t = a[e] * y[e]
      A = _fma(t[:, None], y[e][None, :], A, F32)
    dg = np.zeros(h, F32)
    for j in range(h):
      d = A[j, j]
      if not d > 0:
        return np.zeros(h, F32), 1
      dg[j] = np.sqrt(d)
      A[j + 1:, j] = A[j + 1:, j] / dg[j]
      col = A[j + 1:, j]
      A[j + 1:, j + 1:] = _fma(-col[:, None], col[None, :], A[j + 1:, j + 1:], F32)
    for k in range(h):
      r[k] = r[k] / dg[k]
      r[k + 1:] = _fma(-A[k + 1:, k], r[k], r[k + 1:], F32)
    for k in range(h - 1, -1, -1):
      r[k] = r[k] / dg[k]
      r[:k] = _fma(-A[k, :k], r[k], r[:k], F32)
  assert r.dtype == F32 and A.dtype == F32
  return r, 0


def foldin32(csr, Y, G, v, bias, alpha, use_data=True, rows=None):
  """(X [B, h], status [B] int32) of rk_als_foldin on the rows of ``csr`` (``rows``: those only)."""
  csr = sp.csr_matrix(csr)
  rows = range(csr.shape[0]) if rows is None else rows
  out = [foldin_row32(csr.indices[csr.indptr[u]:csr.indptr[u + 1]],
                      csr.data[csr.indptr[u]:csr.indptr[u + 1]] if use_data else None, Y, G, v, bias, alpha)
         for u in rows]
  h = np.asarray(G).shape[0]
  return (np.stack([x for x, _ in out]) if out else np.zeros((0, h), F32)), np.array([s for _, s in out], np.int32)


def normal_equations64(cols, vals, Y, G, v, bias, alpha):
  """(A, rhs) of the row in float64 from the same f32 inputs (G symmetrised from its lower triangle)."""
  h = np.asarray(G).shape[0]
  cols = np.asarray(cols, np.int64)
  n = len(cols)
  y = np.asarray(Y, F32)[cols, :h].reshape(n, h).astype(np.float64)
  vals = np.ones(n) if vals is None else np.asarray(vals, F32).astype(np.float64)
  al = float(F32(alpha))
  a = np.where(vals > 0, al, 0.0)
  b = np.asarray(bias, F32)[cols].astype(np.float64) if bias is not None else np.zeros(n)
  G64 = np.tril(np.asarray(G, F32)[:h, :h].astype(np.float64))
  G64 = G64 + np.tril(G64, -1).T
  A = G64 + (y * a[:, None]).T @ y
  rhs = y.T @ ((1 + a) * vals - a * b) - np.asarray(v, F32)[:h].astype(np.float64)
  return A, rhs


def solve64(cols, vals, Y, G, v, bias, alpha):
  """(x64, bound): the float64 solve of the row and the relative error the f32 restatement may have against it."""
  A, rhs = normal_equations64(cols, vals, Y, G, v, bias, alpha)
  h = A.shape[0]
  return np.linalg.solve(A, rhs), bound(h, len(cols), np.linalg.cond(A, 2))


def bound(h, length, cond):
  return U * (4 * h * (3 * h + 1) + 2 * (length + 2)) * cond


# ---------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_foldin.py and tests/test_foldin_host.py.  alpha, the CSR values and the bias carry few
# bits, so coef is exact however it is rounded; Y, G and v are generic f32.
N_ITEMS = 900
ALPHA = 10.0
HS = (1, 3, 33, 64, 128)
# 37 rows: empty, one entry, 5, one longer than any staging chunk, lengths around CHUNK and its multiples
LENGTHS = (0, 1, 5, 700, 15, 16, 17, 31, 32, 33, 0, 2, 3, 4, 7, 8, 9, 12, 20, 24, 40, 48, 49, 64, 65, 100, 6, 10, 11, 13,
           14, 18, 19, 21, 22, 23, 1)
# (name, alpha, CSR values given, bias given)
VARIANTS = (("values", ALPHA, True, True), ("ones", ALPHA, False, True), ("alpha 0", 0.0, True, True),
            ("no bias", ALPHA, True, False))


@functools.lru_cache(maxsize=None)
def problem(h):
  """A batch of len(LENGTHS) histories over N_ITEMS items at embedding size h; reg = 1e-2 tr(Y^T Y) / h."""
  rng = np.random.RandomState(2000 + h)
  lens = list(LENGTHS)
  indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  indices = np.concatenate([np.sort(rng.choice(N_ITEMS, n, replace=False)) for n in lens]).astype(np.int32)
  nnz = len(indices)
  vals = np.where(rng.rand(nnz) < 0.75, rng.randint(1, 17, nnz), rng.randint(-16, 1, nnz)) / 2.0    # (stored zeros too)
  assert (vals == 0).any() and (vals != 1).any()
  csr = sp.csr_matrix((vals.astype(F32), indices, indptr), shape=(len(lens), N_ITEMS))
  Y = (0.1 * rng.randn(N_ITEMS, h)).astype(F32)
  Y64 = Y.astype(np.float64)
  G = Y64.T @ Y64
  reg = 1e-2 * np.trace(G) / h
  G = (0.5 * (G + G.T) + reg * np.eye(h)).astype(F32)
  bias = (rng.randint(-255, 256, N_ITEMS) / 256.0).astype(F32)
  v = (Y64.T @ bias.astype(np.float64)).astype(F32)
  return dict(lens=lens, csr=csr, Y=Y, G=G, v=v, bias=bias, reg=reg)


def variant_inputs(p, bias_given):
  """(v, bias) of a variant: without a bias v = Y^T 0 = 0."""
  return (p["v"], p["bias"]) if bias_given else (np.zeros_like(p["v"]), None)


@functools.lru_cache(maxsize=None)
def want(h, variant):
  """(X, status) of the restatement for a variant of ``problem(h)`` (computed once, shared by the tests)."""
  p = problem(h)
  _, alpha, use_data, bias_given = VARIANTS[variant]
  v, bias = variant_inputs(p, bias_given)
  X, st = foldin32(p["csr"], p["Y"], p["G"], v, bias, alpha, use_data)
  X.setflags(write=False), st.setflags(write=False)
  return X, st


def singular_problem():
  """reg = 0 and a rank-deficient Y: four copies of one item row, h = 3, one history with no entries.  G = 4 y y^T is
  exact in f32, the first pivot 4 has the exact root 2, and the second pivot is 16 - 4 * 4 = 0: not > 0."""
  Y = np.tile(np.array([[1.0, 2.0, 3.0]], F32), (4, 1))
  G = (Y.astype(np.float64).T @ Y.astype(np.float64)).astype(F32)
  bias = np.array([0.5, -0.25, 1.0, 0.125], F32)
  v = (Y.astype(np.float64).T @ bias.astype(np.float64)).astype(F32)
  csr = sp.csr_matrix((1, 4), dtype=F32)
  return dict(csr=csr, Y=Y, G=G, v=v, bias=bias)


# ---------------------------------------------------------------------------------------------------------------------
# The property tests through Recoder: a 300 x 200 random matrix.
PROP_USERS, PROP_ITEMS, PROP_K = 300, 200, 10
PROP_SEED = 1                 # (of seeds 1..8 the one that leaves the fewest positions undecided: test_foldin_host)


def prop_matrix(seed=PROP_SEED):
  """300 x 200, binary, density 0.1, no empty row."""
  rng = np.random.RandomState(seed)
  m = (rng.rand(PROP_USERS, PROP_ITEMS) < 0.1).astype(F32)
  m[np.arange(PROP_USERS), rng.randint(0, PROP_ITEMS, PROP_USERS)] = 1.0
  return sp.csr_matrix(m)


def decided(S, seen, k, thr):
  """(ids [B, k], sure [B, k]): the top-k unseen ids of the float64 scores S by (score descending, id ascending) and
  whether each position stands clear of both its neighbours in that order (the k + 1-th included) by more than
  thr [B]: two score rows that differ by at most thr / 2 in every element put the same id there."""
  S = np.array(S, np.float64)
  seen = sp.csr_matrix(seen)
  for u in range(S.shape[0]):
    S[u, seen.indices[seen.indptr[u]:seen.indptr[u + 1]]] = -np.inf
  order = np.argsort(-S, axis=1, kind="stable")[:, :k + 1]
  top = np.take_along_axis(S, order, 1)
  gap = top[:, :-1] - top[:, 1:]                             # gap[p]: between positions p and p + 1
  thr = np.asarray(thr, np.float64)[:, None]
  below = gap > thr
  above = np.concatenate([np.ones((S.shape[0], 1), bool), below[:, :-1]], axis=1)
  return order[:, :k], below & above
