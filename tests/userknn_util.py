"""Numpy restatements of UserKNN (user-based cosine neighbourhoods), written from the formulas:

    c[q, v]   = |H_q and H_v|                    (H: the stored non-zero items of a row; values play no part)
    sim[q, v] = c[q, v] / (qn[q] * un[v] + shrink),   qn = sqrt(|H_q|), un = sqrt(|H_v|)
    q keeps its N largest sim > 0 by (sim descending, v ascending)
    scores[q, j] = sum over the kept v, ascending, of sim[q, v] * X[v, j]

``neighbours_f32`` / ``scores_f32`` restate the f32 operations the kernels promise, with the same rounding
points (the norms: float64 square roots rounded once; the product, the sum and the quotient: one f32
operation each; the scores: one ascending fmaf chain per output).  ``neighbours_f64`` / ``scores_f64`` are the
float64 model.  They are the comparators of the UserKNN tests and never the code under test."""
import numpy as np
import scipy.sparse as sp

from tests import ease_util, rp3_util

SLICE = ease_util.SLICE
top_k = rp3_util.top_k
metric_means = rp3_util.metric_means


def _binary(m, n=None):
  m = sp.csr_matrix(m)
  if n is not None and m.shape[1] != n:
    m = sp.csr_matrix((m.data, m.indices, m.indptr), shape=(m.shape[0], n))
  b = m.astype(np.float64)
  b.data[:] = 1.0
  return b


def norms_f32(m):
  """sqrt(stored entries of every row): float64, rounded once to f32."""
  return np.sqrt(np.diff(sp.csr_matrix(m).indptr).astype(np.float64)).astype(np.float32)


def counts(X, Q, rows):
  """c[q, v] for the query rows ``rows``: exact integers, as a dense int64 [len(rows), U] array."""
  B = _binary(X)
  C = _binary(Q, X.shape[1])[rows] @ B.T
  return np.rint(np.asarray(C.todense())).astype(np.int64)


def _cut(sim, N):
  """(ids, values) of one row's N largest entries > 0 by (value descending, id ascending), ids ascending."""
  cand = np.flatnonzero(sim > 0)
  top = np.sort(cand[np.argsort(-sim[cand], kind="stable")[:N]])       # (a stable sort keeps the lower ids)
  return top, sim[top]


def neighbours_f32(X, Q, N, shrink, un=None, qn=None, block=500):
  """(ids int32 [Q, N], sim f32 [Q, N], count int32 [Q]): -1 / +0 behind the kept entries."""
  X, Q = sp.csr_matrix(X), sp.csr_matrix(Q)
  un = norms_f32(X) if un is None else np.asarray(un, np.float32)
  qn = norms_f32(Q) if qn is None else np.asarray(qn, np.float32)
  shrink = np.float32(shrink)
  nq = Q.shape[0]
  ids = np.full((nq, N), -1, np.int32)
  sim = np.zeros((nq, N), np.float32)
  count = np.zeros(nq, np.int32)
  for b0 in range(0, nq, block):
    rows = np.arange(b0, min(nq, b0 + block))
    C = counts(X, Q, rows)
    for r, q in enumerate(rows):
      c = C[r]
      den = qn[q] * un                     # f32 * f32: one rounding
      den = den + shrink                   # one rounding
      assert den.dtype == np.float32
      s = np.zeros(len(c), np.float32)
      hit = c > 0
      s[hit] = c[hit].astype(np.float32) / den[hit]          # (counts < 2^24 are exact; one rounding)
      top, val = _cut(s, N)
      count[q] = len(top)
      ids[q, :len(top)] = top
      sim[q, :len(top)] = val
  return ids, sim, count


def scores_f32(X, ids, sim, count, lo=0, hi=None):
  """out[q, c]: the f32 fmaf chain from +0 over the kept neighbours of q, ascending, of sim * X[v, lo + c].
  Neighbour s of every query at once: the items of one row of X are distinct, so a fancy-indexed update
  is one chain step per output."""
  X = sp.csr_matrix(X).astype(np.float32)
  X.sort_indices()
  hi = X.shape[1] if hi is None else hi
  nq, N = ids.shape
  out = np.zeros((nq, hi - lo), np.float32)
  for s in range(N):
    qs = np.flatnonzero(count > s)
    if not len(qs):
      break
    R = X[ids[qs, s]].tocoo()
    live = (R.col >= lo) & (R.col < hi)
    qq, jj, x = qs[R.row[live]], R.col[live] - lo, R.data[live]
    out[qq, jj] = ease_util.fmaf(sim[qq, s], x, out[qq, jj])
  return out


def neighbours_f64(X, Q, N, shrink, un=None, qn=None, rows=None):
  """(kept, S): per query row the kept ids (ascending) and the dense float64 similarity row they were cut
  from.  ``un`` / ``qn``: the norms to use (default: float64 square roots)."""
  X, Q = sp.csr_matrix(X), sp.csr_matrix(Q)
  un = np.sqrt(np.diff(X.indptr).astype(np.float64)) if un is None else np.asarray(un, np.float64)
  qn = np.sqrt(np.diff(Q.indptr).astype(np.float64)) if qn is None else np.asarray(qn, np.float64)
  rows = np.arange(Q.shape[0]) if rows is None else np.asarray(rows)
  C = counts(X, Q, rows)
  S = np.zeros(C.shape, np.float64)
  den = qn[rows][:, None] * un[None, :] + float(shrink)
  S[C > 0] = C[C > 0] / den[C > 0]
  return [_cut(S[r], N)[0] for r in range(len(rows))], S


def scores_f64(X, kept, S):
  """Dense float64 scores [len(kept), n] of the neighbour sets ``kept`` with the similarities ``S``."""
  X = sp.csr_matrix(X).astype(np.float64)
  W = np.zeros_like(S)
  for r, ids in enumerate(kept):
    W[r, ids] = S[r, ids]
  return (sp.csr_matrix(W) @ X).toarray()


def load_slice():
  z = np.load(SLICE)
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


def quality_f64(X, Y, N, shrink, block=1000, ks=((20, "recall"), (100, "ndcg"))):
  """Mean Recall@20 / NDCG@100 of the float64 model with the training users as queries (every query finds
  its own row among its neighbours: not excluded), seen items masked."""
  lists = []
  k = max(k for k, _ in ks)
  for b0 in range(0, X.shape[0], block):
    rows = np.arange(b0, min(X.shape[0], b0 + block))
    kept, S = neighbours_f64(X, X, N, shrink, rows=rows)
    lists.append(top_k(scores_f64(X, kept, S), X[rows], k))
  return metric_means(np.concatenate(lists), Y, ks)


def random_matrix(n_users, n, density, seed, values=False):
  rng = np.random.RandomState(seed)
  m = (rng.rand(n_users, n) < density).astype(np.float32)
  if values:
    m *= rng.choice(np.array([0.5, 1.0, 2.0, 3.5, -1.5], np.float32), m.shape)
  m = sp.csr_matrix(m)
  m.eliminate_zeros()
  m.sort_indices()
  return m
