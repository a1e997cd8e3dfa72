"""Float64 numpy restatement of EASE (Steck 2019), written from the paper's formulas:

    G = X^T X,   P = (G + reg I)^-1,   B[i, j] = -P[i, j] / P[j, j] (i != j),   B[j, j] = 0,
    scores = X B

It is the comparator of the EASE tests and never the code under test."""
import os

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
SLICE = os.path.join(HERE, "golden", "real_ml20m_slice.npz")


def gram(X, reg):
  X = sp.csr_matrix(X).astype(np.float64)
  return np.asarray((X.T @ X).todense()) + reg * np.eye(X.shape[1])


def inverse(A):
  return np.linalg.inv(np.asarray(A, np.float64))


def weights(P):
  P = np.asarray(P, np.float64)
  B = P / (-np.diag(P))[None, :]
  B[np.diag_indices_from(B)] = 0.0
  return B


def fit(X, reg):
  """(B, P), float64."""
  P = inverse(gram(X, reg))
  return weights(P), P


def scores(X, B):
  return np.asarray(sp.csr_matrix(X).astype(np.float64) @ np.asarray(B, np.float64))


def finalize_f32(P32):
  """The f32 element-wise formula: one correctly rounded divide per element, diagonal +0."""
  P32 = np.asarray(P32, np.float32)
  B = P32 / (-np.diag(P32))[None, :]
  B[np.diag_indices_from(B)] = np.float32(0.0)
  assert B.dtype == np.float32
  return B


def fmaf(a, b, c):
  """f32 fused multiply-add, element-wise and exact: the product of two f32 is exact in float64; the
  float64 sum is rounded once more to f32, which can differ from the single rounding of an fma only
  when the float64 sum sits exactly on an f32 rounding midpoint while the true sum does not.  TwoSum
  gives the float64 sum's error; on a midpoint with a non-zero error the sum is moved one float64 ulp
  towards the true value before the final rounding.  (Normal f32 range; checked against exact
  rational arithmetic in tests/test_ease_host.py.)"""
  a = np.asarray(a, np.float32).astype(np.float64)
  b = np.asarray(b, np.float32).astype(np.float64)
  c = np.asarray(c, np.float32).astype(np.float64)
  a, b, c = np.broadcast_arrays(a, b, c)
  p = a * b
  s = p + c
  bb = s - p
  err = (p - (s - bb)) + (c - bb)
  mid = (np.ascontiguousarray(s).view(np.int64) & 0x1FFFFFFF) == 0x10000000
  fix = mid & (err != 0)
  s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
  return s.astype(np.float32)


def scores_chain_f32(csr, W, lo=0, hi=None):
  """out[u, c] = the ascending f32 fmaf chain over the stored entries of row u, from 0, item by item."""
  csr = sp.csr_matrix(csr)
  W = np.asarray(W, np.float32)
  hi = W.shape[1] if hi is None else hi
  out = np.zeros((csr.shape[0], hi - lo), np.float32)
  for u in range(csr.shape[0]):
    acc = np.zeros(hi - lo, np.float32)
    for e in range(csr.indptr[u], csr.indptr[u + 1]):
      acc = fmaf(np.float32(csr.data[e]), W[csr.indices[e], lo:hi], acc)
    out[u] = acc
  return out


def rel_err(P, P64):
  """e(P) = max|P - P64| / max|P64|."""
  return float(np.abs(np.asarray(P, np.float64) - P64).max() / np.abs(P64).max())


def residual(A, P):
  """max|A P - I| in float64."""
  A = np.asarray(A, np.float64)
  return float(np.abs(A @ np.asarray(P, np.float64) - np.eye(A.shape[0])).max())


def top_k(S, seen, k):
  """Top-k unseen ids by (score descending, id ascending)."""
  S = np.array(S, np.float64)
  seen = sp.csr_matrix(seen)
  for u in range(S.shape[0]):
    S[u, seen.indices[seen.indptr[u]:seen.indptr[u + 1]]] = -np.inf
  order = np.argsort(-S, axis=1, kind="stable")[:, :k]
  return order
