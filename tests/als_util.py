"""Float64 numpy restatement of implicit-feedback ALS (recoder_amd/als.py, include/recoder_als.h):
the same normal equations, the same warm-started CG with the same stopping rules, row by row."""
import os

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))


def normal_equations(csr, r, F, bias, alpha, reg, side):
  """(A, rhs) of row r: A = F^T F + reg I + sum a_j f_j f_j^T, rhs as in include/recoder_als.h."""
  F = np.asarray(F, np.float64)
  h = F.shape[1]
  b = np.zeros(csr.shape[1] if side == "user" else csr.shape[0]) if bias is None else np.asarray(bias, np.float64)
  A = F.T @ F + reg * np.eye(h)
  lo, hi = csr.indptr[r], csr.indptr[r + 1]
  cols, vals = csr.indices[lo:hi], np.asarray(csr.data[lo:hi], np.float64)
  a = np.where(vals > 0, alpha, 0.0)
  f = F[cols]
  if side == "user":
    rhs = -(F.T @ b) + f.T @ ((1 + a) * vals - a * b[cols])
  else:
    rhs = -b[r] * F.sum(0) + f.T @ ((1 + a) * vals - a * b[r])
  A = A + (f * a[:, None]).T @ f
  return A, rhs


def cg(A, rhs, x, steps):
  x = np.array(x, np.float64)
  r = rhs - A @ x
  p = r.copy()
  rs = r @ r
  for _ in range(steps):
    if not rs > 0:
      break
    q = A @ p
    pq = p @ q
    if not pq > 0:
      break
    al = rs / pq
    x += al * p
    r -= al * q
    rsn = r @ r
    p = r + (rsn / rs) * p
    rs = rsn
  return x


def half_step(csr, F, X, bias, alpha, reg, cg_steps, side, exact=False):
  """Every row of X solved with F fixed (a new array); side 'user' (bias per column) or 'item'."""
  X = np.array(X, np.float64)
  for r in range(csr.shape[0]):
    A, rhs = normal_equations(csr, r, F, bias, alpha, reg, side)
    X[r] = np.linalg.solve(A, rhs) if exact else cg(A, rhs, X[r], cg_steps)
  return X


def objective(csr, X, Y, bias, alpha, reg):
  R = np.asarray(csr.todense(), np.float64)
  S = np.asarray(X, np.float64) @ np.asarray(Y, np.float64).T
  if bias is not None:
    S = S + np.asarray(bias, np.float64)[None, :]
  W = 1 + alpha * (R > 0)
  return float((W * (R - S) ** 2).sum() + reg * ((np.asarray(X, np.float64) ** 2).sum()
                                                   + (np.asarray(Y, np.float64) ** 2).sum()))


def fit(csr, X, Y, bias, alpha, reg, cg_steps, num_iterations):
  csr = sp.csr_matrix(csr)
  csc = csr.T.tocsr()
  X, Y = np.array(X, np.float64), np.array(Y, np.float64)
  hist = []
  for _ in range(num_iterations):
    X = half_step(csr, Y, X, bias, alpha, reg, cg_steps, "user")
    Y = half_step(csc, X, Y, bias, alpha, reg, cg_steps, "item")
    hist.append(objective(csr, X, Y, bias, alpha, reg))
  return X, Y, hist


def random_csr(n_rows, n_cols, density, seed, values="binary", empty_rows=()):
  rng = np.random.RandomState(seed)
  m = sp.random(n_rows, n_cols, density=density, random_state=rng, format="csr", dtype=np.float64)
  if values == "binary":
    m.data[:] = 1.0
  else:                     # counts and a few non-positive values (weight 1, as in MSELoss)
    m.data = np.round(m.data * 5, 1) - 0.5
    m.data[m.data == 0] = 2.0
  m = m.tolil()
  for r in empty_rows:
    m.rows[r] = []
    m.data[r] = []
  m = m.tocsr().astype(np.float32)
  m.sort_indices()
  return m
