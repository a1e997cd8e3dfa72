"""Numpy restatement of the randomized truncated SVD behind PureSVD (recoder_amd/svd.py), written from
Halko, Martinsson & Tropp 2011 (algorithms 4.4 + 5.1) in float64 or float32: Cholesky-QR done twice after
every product, Rayleigh-Ritz on T = W^T W with a float64 eigh, the same sign rule, Omega injected.  It is
the comparator of the SVD tests and never the code under test; the statistics the tests assert on are
here too."""
import os

import numpy as np
import scipy.linalg
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
SLICE = os.path.join(HERE, "golden", "real_ml20m_slice.npz")


def load_slice():
  z = np.load(SLICE)
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


def planted(n_users=600, n_items=400, groups=8, inside=0.5, outside=0.02, seed=1):
  """A binary matrix with `groups` user and item groups: density `inside` within a group's block,
  `outside` elsewhere.  Its first `groups` singular values stand clear of the rest."""
  rng = np.random.RandomState(seed)
  gu = np.arange(n_users) * groups // n_users
  gi = np.arange(n_items) * groups // n_items
  p = np.where(gu[:, None] == gi[None, :], inside, outside)
  m = sp.csr_matrix((rng.rand(n_users, n_items) < p).astype(np.float32))
  m.sort_indices()
  return m


def orth(Y):
  """Cholesky-QR, twice, in Y's dtype."""
  for _ in range(2):
    G = Y.T @ Y
    R = np.linalg.cholesky(G).T                    # G = R^T R, R upper
    Y = scipy.linalg.solve_triangular(R, Y.T, trans="T", lower=False).T.astype(Y.dtype)   # Y R^-1
  return Y


def fix_signs(S):
  big = np.abs(S).argmax(axis=0)
  return S * np.where(S[big, np.arange(S.shape[1])] < 0, -1.0, 1.0)[None, :]


def rsvd(A, h, oversample, q, omega, dtype=np.float64):
  """(sigma [h], V [items, h], U [users, h]) in `dtype` (the eigendecomposition always in float64)."""
  A = sp.csr_matrix(A).astype(dtype)
  At = A.T.tocsr()
  l = h + oversample
  Z = np.asarray(omega, dtype).reshape(A.shape[1], l)
  Q = orth(np.asarray(A @ Z, dtype))
  Z = orth(np.asarray(At @ Q, dtype))
  for _ in range(q):
    Q = orth(np.asarray(A @ Z, dtype))
    Z = orth(np.asarray(At @ Q, dtype))
  W = np.asarray(A @ Z, dtype)
  T = (W.T @ W).astype(np.float64)
  lam, S = np.linalg.eigh((T + T.T) / 2)
  order = np.argsort(-lam, kind="stable")[:h]
  lam, S = lam[order], fix_signs(S[:, order])
  S = S.astype(dtype)
  return np.sqrt(np.maximum(lam, 0.0)), (Z @ S).astype(dtype), (W @ S).astype(dtype)


def omega(n_items, l, seed):
  return np.random.RandomState(seed).randn(n_items, l).astype(np.float32)


# ------------------------------------------------------------------ statistics
def stats(A, result, ref64):
  """e_sigma, e_orth, e_sub, e_U of `result` = (sigma, V, U) against the float64 restatement `ref64`."""
  sigma, V, U = (np.asarray(x, np.float64) for x in result)
  s64, V64, _ = ref64
  A = sp.csr_matrix(A).astype(np.float64)
  h = V.shape[1]
  return dict(
      e_sigma=float(np.abs(sigma - s64).max() / s64[0]),
      e_orth=float(np.abs(V.T @ V - np.eye(h)).max()),
      e_sub=float(np.linalg.norm(V - V64 @ (V64.T @ V))),
      e_U=float(np.linalg.norm(U - np.asarray(A @ V)) / np.linalg.norm(U)))


def top_k(S, seen, k):
  """Top-k unseen ids by (score descending, id ascending)."""
  S = np.array(S, np.float64)
  seen = sp.csr_matrix(seen)
  for u in range(S.shape[0]):
    S[u, seen.indices[seen.indptr[u]:seen.indptr[u + 1]]] = -np.inf
  return np.argsort(-S, axis=1, kind="stable")[:, :k]


def scores(result):
  _, V, U = result
  return np.asarray(U, np.float64) @ np.asarray(V, np.float64).T


def top20_differ(lists_a, lists_b):
  """Share of users whose top-20 SETS differ."""
  return float(np.mean([set(a) != set(b) for a, b in zip(lists_a, lists_b)]))


def recall_at(lists, y, k=20):
  """Mean normalised Recall@k over the users with held-out items."""
  y = sp.csr_matrix(y)
  out = []
  for u in range(y.shape[0]):
    t = y.indices[y.indptr[u]:y.indptr[u + 1]]
    if len(t):
      out.append(len(np.intersect1d(lists[u][:k], t)) / min(k, len(t)))
  return float(np.mean(out))


def popularity_recall(x, y, k=20):
  x = sp.csr_matrix(x)
  pop = np.asarray(x.sum(axis=0)).ravel().astype(np.float64)
  S = np.broadcast_to(pop, x.shape)
  return recall_at(top_k(S, x, k), y, k)
