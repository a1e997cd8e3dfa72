"""Shared helpers of the item-similarity tests: the golden fixtures of make_golden_similarity.py,
float64 cosines, and the near-tie comparison of ranked lists."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = ("h64", "h200", "h37")
COS_TOL = 2e-6          # |cosine - float64 cosine|
TIE_TOL = 4e-6          # scores this close may come in either order


def load_fixture(name):
  z = np.load(os.path.join(HERE, "golden", "similarity_%s.npz" % name))
  emb = z["emb_q"].astype(np.float32) / np.float32(z["emb_scale"])
  ids = z["ids"]
  id_map = {int(ids[r]): r for r in range(len(ids))}
  return z, emb, ids, id_map


def unit64(x):
  x = np.asarray(x, dtype=np.float64)
  nrm = np.linalg.norm(x, axis=-1, keepdims=True)
  return np.divide(x, nrm, out=np.zeros_like(x), where=nrm > 0)


def assert_same_ranking(got, want, score, tol=TIE_TOL, what=""):
  """``got`` and ``want`` rank keys by ``score`` (float64) descending: equal up to reorderings among keys whose
  scores lie within ``tol`` of each other, and up to swaps of such keys at the cut."""
  got, want = list(got), list(want)
  assert len(got) == len(want), (what, got, want)
  assert len(set(got)) == len(got), (what, got)
  sg = np.array([score(k) for k in got], dtype=np.float64)
  sw = np.array([score(k) for k in want], dtype=np.float64)
  assert np.all(np.abs(sg - sw) <= tol), (what, got, want, sg - sw)
  if want:
    cut = sw[-1]
    for k in set(got) ^ set(want):
      assert abs(score(k) - cut) <= tol, (what, k, score(k), cut)


def check_knn(idx, cos, C64, n, tol=TIE_TOL):
  """Rows of a kNN result (idx / cos [Q, n], numpy) against the float64 cosines C64 [Q, N] of the same queries."""
  Q = C64.shape[0]
  assert idx.shape == (Q, n) and cos.shape == (Q, n)
  g = np.take_along_axis(C64, idx, axis=1)
  assert np.abs(cos.astype(np.float64) - g).max() <= COS_TOL
  assert np.all(g[:, :-1] >= g[:, 1:] - tol)
  kth = -np.sort(-C64, axis=1)[:, n - 1:n]
  assert np.all(g >= kth - tol)
  for q in range(Q):
    assert len(np.unique(idx[q])) == n
    must = np.nonzero(C64[q] > kth[q, 0] + tol)[0]
    assert np.isin(must, idx[q]).all()
