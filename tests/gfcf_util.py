"""Numpy / scipy restatement of GF-CF (Shen et al., "How Powerful is Graph Convolution for Recommendation?",
CIKM 2021) in float64, written from the formulas:

    R = the binary user x item matrix of the stored entries, r_u / d_i its user / item degrees
    Rn = D_U^-1/2 R D_I^-1/2                 (0 where a degree is 0)
    V [n, k] = the top-k right singular vectors of Rn (eigenvectors of Rn^T Rn)
    W = Rn^T Rn + alpha * D_I^-1/2 V V^T D_I^1/2     (D_I^1/2 is 0, not 1/0, for an item nobody holds)
    scores = X W                              (the user's values as stored)

It is the comparator of the GF-CF tests and of tools/gfcf_bench.py --cpu-grid and never the code under test;
the two error bounds the tests assert on are here too."""
import numpy as np
import scipy.sparse as sp

from tests import rp3_util, svd_util

SLICE = svd_util.SLICE
load_slice = svd_util.load_slice


def scales_f64(X):
  """(r^-1/2, d^-1/2, d^1/2) in float64, all 0 where the degree is 0."""
  r, d = rp3_util.degrees(X)

  def power(x, e):
    out = np.zeros_like(x)
    out[x > 0] = x[x > 0] ** e
    return out
  return power(r, -0.5), power(d, -0.5), power(d, 0.5)


def normalised(X):
  """Rn as a float64 CSR with X's pattern."""
  B = sp.csr_matrix(X).astype(np.float64)
  B.data[:] = 1.0
  ri, di, _ = scales_f64(X)
  Rn = (sp.diags(ri) @ B @ sp.diags(di)).tocsr()
  Rn.sort_indices()
  return Rn


def gram_f64(X):
  Rn = normalised(X)
  return np.asarray((Rn.T @ Rn).todense())


def top_eigenvectors(G, rank):
  """(sigma [rank] descending, V [n, rank]): the exact top eigenpairs of the symmetric G, float64 eigh."""
  lam, E = np.linalg.eigh((G + G.T) / 2)
  order = np.argsort(-lam, kind="stable")[:rank]
  return np.sqrt(np.maximum(lam[order], 0.0)), E[:, order]


def weights_f64(X, rank, alpha, V=None):
  """W [n, n] in float64; ``V`` None: the exact eigenvectors of the Gram, else the given [n, rank] basis."""
  G = gram_f64(X)
  _, di, dh = scales_f64(X)
  if V is None:
    _, V = top_eigenvectors(G, rank)
  V = np.asarray(V, np.float64)
  assert V.shape == (G.shape[0], rank)
  return G + float(alpha) * ((di[:, None] * V) @ (V.T * dh[None, :]))


def scores_f64(X, W):
  return np.asarray(sp.csr_matrix(X).astype(np.float64) @ W)


def quality(X, Y, W=None, S=None):
  """[Recall@20, NDCG@100] of the scores ``S`` (or ``X W``) with the seen items masked: the evaluation of
  tests/rp3_util.py.  ``S`` is modified."""
  S = scores_f64(X, W) if S is None else S
  return rp3_util.metric_means(rp3_util.top_k(S, sp.csr_matrix(X), 100), sp.csr_matrix(Y))


def rsvd_basis(X, rank, oversample, q, seed):
  """V [n, rank] of the float64 randomized SVD of Rn (tests/svd_util.py) with the seeded Omega of the tests."""
  Rn = normalised(X)
  return svd_util.rsvd(Rn, rank, oversample, q, svd_util.omega(Rn.shape[1], rank + oversample, seed), np.float64)[1]


# ------------------------------------------------------------------ bounds
EPS = 2.0 ** -23


def lowrank_bound(A, V, row_scale, col_scale, alpha):
  """Per element, for rk_ease_lowrank_add: (k + 4) 2^-23 (|A_ij| + |alpha a_i b_j| sum_t |V_it V_jt|).
  Derived: the dot product is one chain of k roundings (each product enters the chain exactly; the MFMA
  takes two products per instruction and rounds after each of them, so k roundings, not k / 2), the two
  scalings and the final add are three more; each is half an ulp, 2^-24 relative to a magnitude that
  sum|terms| (or |A| + that) bounds to first order.  (k + 3) 2^-24 to first order; the factor 2 to
  (k + 4) 2^-23 covers the higher-order terms and operands (scales) that were themselves rounded once."""
  A, V = np.asarray(A, np.float64), np.abs(np.asarray(V, np.float64))
  a, b = np.abs(np.asarray(row_scale, np.float64)), np.abs(np.asarray(col_scale, np.float64))
  k = V.shape[1]
  return (k + 4) * EPS * (np.abs(A) + abs(float(alpha)) * a[:, None] * (V @ V.T) * b[None, :])


def gram_bound(X):
  """Per element, for rk_ease_gram over the normalised values: d_max 2^-23 sum|terms|.  G_ij is an fmaf
  chain over the users that hold i and j, at most d_max = the largest item degree of them: d_max roundings of
  2^-24.  Every term is > 0, so sum|terms| is the float64 G_ij itself.  The factor 2 to 2^-23 covers the six
  roundings inside a term's two values (r^-1/2, d^-1/2 and their product, each rounded to f32 once) as
  soon as d_max >= 6, and the higher-order terms."""
  _, d = rp3_util.degrees(X)
  assert d.max() >= 6
  return float(d.max()) * EPS * gram_f64(X)
