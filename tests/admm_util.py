"""Numpy restatements of ADMM-SLIM (Steck, Dimakis, Riabov & Jebara 2020), written from the loop that
recoder_amd/admm.py states:

    P = (X^T X + kappa I)^-1,  kappa = l2 + rho,  theta = l1 / rho,  C = U = M = 0
    T = rho P M - kappa P;  gamma = (diag T + 1) / diag P;  B = T - P diag(gamma), diag B = 0;  V = B + U
    C_new = max(V - theta, 0) (nonneg)  or  sign(V) max(|V| - theta, 0);  U = V - C_new;  M = C_new - U

``fit`` runs it in one dtype (float64: the comparator; float32 with BLAS sgemm: the yardstick of what an f32 chain in
another order costs), ``update_f32`` restates rk_ease_admm_update rounding by rounding (include/recoder_ease.h), and
``kkt_violation`` checks a returned point against the objective's sub-gradient condition.  They are the comparators
of the ADMM-SLIM tests and of tools/admm_bench.py --cpu-grid and never the code under test."""
import numpy as np
import scipy.sparse as sp

from tests import ease_util

SLICE = ease_util.SLICE


def zipf_matrix(n_users=600, n_items=257, seed=0, per_user=12):
  """Binary users x items with Zipf item popularity (every item held by somebody is not promised)."""
  rng = np.random.RandomState(seed)
  p = 1.0 / np.arange(1, n_items + 1) ** 0.8
  p /= p.sum()
  rows, cols = [], []
  for u in range(n_users):
    k = 1 + rng.poisson(per_user - 1)
    c = np.unique(rng.choice(n_items, size=min(k, n_items), p=p))
    rows += [u] * len(c)
    cols += list(c)
  X = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_users, n_items))
  X.sort_indices()
  return X


def threshold(V, theta, nonneg):
  V = np.asarray(V)
  if nonneg:
    return np.maximum(V - theta, 0)
  return np.sign(V) * np.maximum(np.abs(V) - theta, 0)


def fit(X, l1, l2, rho, iterations, nonneg, dtype=np.float64, trace=None):
  """(C, info) of the loop, every step in ``dtype``: the Gram (exact for integer data) rounded to it, LAPACK's inverse
  and BLAS's product in it.  ``info``: primal / dual residual lists, density, and B, U, V of the last iteration.
  ``trace(it, C)`` is called after each iteration (1-based)."""
  dt = np.dtype(dtype).type
  kappa, theta = dt(l2 + rho), dt(l1 / rho)
  P = np.linalg.inv(ease_util.gram(X, float(l2) + float(rho)).astype(dtype))
  assert P.dtype == np.dtype(dtype)
  n = P.shape[0]
  dP = np.diag(P).copy()
  C, U, M = (np.zeros((n, n), dtype) for _ in range(3))
  primal, dual = [], []
  B = V = None
  for it in range(iterations):
    T = dt(rho) * (P @ M) - kappa * P
    gamma = (np.diag(T) + dt(1)) / dP
    B = T - P * gamma[None, :]
    B[np.diag_indices(n)] = 0
    V = B + U
    Cn = threshold(V, theta, nonneg).astype(dtype)
    U = V - Cn
    M = Cn - U
    primal.append(float(np.sqrt(((B - Cn).astype(np.float64) ** 2).sum())))
    dual.append(float(rho) * float(np.sqrt(((Cn - C).astype(np.float64) ** 2).sum())))
    C = Cn
    assert C.dtype == np.dtype(dtype)
    if trace is not None:
      trace(it + 1, C)
  info = dict(primal_residual=primal, dual_residual=dual, density=float((C != 0).mean()), B=B, U=U, V=V)
  return C, info


def update_f32(T, P, C, U, theta, nonneg, row_lo=0, row_hi=None):
  """rk_ease_admm_update, rounding by rounding, on f32 arrays: returns (C, U, M, gamma, primal, dual, nnz) with the
  rows outside the range of C and U as given, of M zero, and the three row statistics in float64 (exact sums of the
  squares of the f32 differences: what the kernel's float64 sums approximate)."""
  T, P, C, U = (np.asarray(a, np.float32) for a in (T, P, C, U))
  n = T.shape[0]
  row_hi = n if row_hi is None else row_hi
  theta = np.float32(theta)
  gamma = ((np.diag(T) + np.float32(1)) / np.diag(P)).astype(np.float32)
  r = slice(row_lo, row_hi)
  diag = np.arange(n)[r, None] == np.arange(n)[None, :]
  B = ease_util.fmaf(-P[r], gamma[None, :], T[r])
  B[diag] = np.float32(0)
  V = B + U[r]
  V[diag] = np.float32(0)
  w = (V if nonneg else np.abs(V)) - theta
  Cn = np.where(w > 0, w if nonneg else np.copysign(w, V), np.float32(0)).astype(np.float32)
  Un = V - Cn
  Mn = Cn - Un
  for a in (B, V, w, Cn, Un, Mn):
    assert a.dtype == np.float32
  d1 = (B - Cn).astype(np.float64)
  d2 = (Cn - C[r]).astype(np.float64)
  Co, Uo, Mo = C.copy(), U.copy(), np.zeros_like(C)
  Co[r], Uo[r], Mo[r] = Cn, Un, Mn
  return Co, Uo, Mo, gamma, (d1 * d1).sum(1), (d2 * d2).sum(1), (Cn != 0).sum(1)


def objective_gradient(X, C, l2):
  """The gradient of the smooth part 1/2 |X - X C|^2 + l2/2 |C|^2 at C: G C - G + l2 C, float64."""
  G = ease_util.gram(X, 0.0)
  C = np.asarray(C, np.float64)
  return G @ C - G + l2 * C


def kkt_violation(X, C, l1, l2, nonneg):
  """max over the off-diagonal entries with C != 0 of |grad_ij + l1 sign(C_ij)|: zero at a minimiser (the diagonal
  carries the multiplier of diag = 0 and is exempt; where C = 0 the condition is an inequality the sparse iterate of
  a truncated run need not meet).  The caller bounds it by what the run's residuals allow."""
  C = np.asarray(C, np.float64)
  g = objective_gradient(X, C, l2) + l1 * np.sign(C)
  mask = C != 0
  mask[np.diag_indices_from(mask)] = False
  return float(np.abs(g[mask]).max()) if mask.any() else 0.0
