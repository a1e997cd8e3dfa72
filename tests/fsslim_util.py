"""Numpy restatement of fsSLIM (Ning & Karypis 2011, section 4.3): SLIM's column j regressed on the M items most
similar to j only, written from the formulas.

    candidates of column j: the M largest ItemKNN similarities sim[i, j] > 0 by (sim descending, i ascending),
      stored with ascending ids (``itemknn_util.fit_f32``: the f32 chains of the ItemKNN kernel)
    the local problem: the Gram masked to the items {candidates of j} + {j}; on it column j is plain SLIM:
      ``slim_util.cd_column_f32`` / ``cd_column_f64`` with its screen (G[j, k] > l1), its sweep, its stop rule,
      and ``slim_util.cut``

The masked Gram is a sub-matrix of the Gram it is given: for data whose products and sums are exact in f32 (binary,
or values in {0.5, 1, 2}) that is the kernel's ascending fmaf chain whatever the order.  With M >= n - 1 every
co-occurring item is a candidate and the restatement is ``slim_util.cd_f32`` on the full Gram.  These are the
comparators of the fsSLIM tests and never the code under test."""
import numpy as np
import scipy.sparse as sp

from tests import ease_util, itemknn_util, slim_util


def select(X, M, similarity="cosine", shrink=0.0):
  """(cand_ids int32 [n, M] ascending with -1 behind, cand_count int32 [n]): every column's M most similar items
  over the stored values of X, ties to the lower id."""
  A = sp.csr_matrix(X).astype(np.float32)
  A.sort_indices()
  form, own, oth, g, binary = itemknn_util.vectors_f64(A, similarity)
  ids, _, count = itemknn_util.fit_f32(A, form, own.astype(np.float32), oth.astype(np.float32), g, shrink, int(M),
                                       binary)
  return ids, count


def all_candidates(n, M=None):
  """Every other item as a candidate of every column (M = n - 1 unless given larger)."""
  M = max(1, n - 1) if M is None else M
  ids = np.full((n, M), -1, np.int32)
  count = np.full(n, n - 1, np.int32)
  for j in range(n):
    ids[j, :n - 1] = np.delete(np.arange(n, dtype=np.int32), j)
  return ids, count


def local(G, j, cand):
  """(items ascending = cand + {j}, the position of j among them, the Gram masked to them as a dense array)."""
  items = np.union1d(np.asarray(cand, np.int64), [j])
  if sp.issparse(G):
    sub = np.asarray(G[items][:, items].todense())
  else:
    sub = np.asarray(G)[np.ix_(items, items)]
  return items, int(np.searchsorted(items, j)), sub


class chains:
  """X and its transpose as f32 CSRs with ascending indices, and the rows of the Gram made as the header of
  rk_slim_fit_sparse promises, whatever the values: G[k][i] is one chain acc = fmaf(a_vk, a_vi, acc) from +0 over the
  users v of item k that hold i, in ascending v.  A row is made once (small catalogues: it has n entries)."""

  def __init__(self, X):
    self.X = sp.csr_matrix(X).astype(np.float32)
    self.X.sort_indices()
    self.Xt = self.X.T.tocsr()
    self.Xt.sort_indices()
    self.shape = (self.X.shape[1],) * 2
    self.rows = {}

  def row(self, k):
    if k not in self.rows:
      X, Xt = self.X, self.Xt
      acc = np.zeros(X.shape[1], np.float32)
      for e in range(Xt.indptr[k], Xt.indptr[k + 1]):           # the users of item k, ascending
        v = Xt.indices[e]
        cols = X.indices[X.indptr[v]:X.indptr[v + 1]]
        acc[cols] = ease_util.fmaf(Xt.data[e], X.data[X.indptr[v]:X.indptr[v + 1]], acc[cols])
      self.rows[k] = acc
    return self.rows[k]


def local_chain_f32(ch, j, cand):
  """``local`` from the chains of ``ch``: row c of L and q[c] (the entry at j's place) come from the walk over the
  users of candidate c; the sweep reads q as row j of the masked Gram, and never reads (j, j)."""
  items = np.union1d(np.asarray(cand, np.int64), [j])
  jl = int(np.searchsorted(items, j))
  sub = np.stack([ch.row(int(k))[items] for k in items])
  sub[jl, :] = sub[:, jl]
  sub[jl, jl] = 0.0
  return items, jl, sub


def cd_f32(G, inv_denom, cand_ids, cand_count, l1, K, max_sweeps, tol, cols=None):
  """``slim_util.cd_f32``'s five arrays with column j fitted on its masked Gram; ``G`` dense or scipy sparse, or
  ``chains(X)``: then the masked Gram is made by ``local_chain_f32``."""
  chain = isinstance(G, chains)
  n = G.shape[0]
  inv_denom = np.asarray(inv_denom, np.float32)
  ids = np.full((n, K), -1, np.int32)
  w = np.zeros((n, K), np.float32)
  count, sweeps, support = (np.zeros(n, np.int32) for _ in range(3))
  for j in (range(n) if cols is None else cols):
    items, jl, sub = (local_chain_f32 if chain else local)(G, j, cand_ids[j, :cand_count[j]])
    cand, wj, sweeps[j] = slim_util.cd_column_f32(sub.astype(np.float32), jl, inv_denom[items], l1, max_sweeps, tol)
    support[j] = int((wj > 0).sum())
    kid, kw = slim_util.cut(items[cand], wj, K)
    count[j] = len(kid)
    ids[j, :len(kid)] = kid
    w[j, :len(kid)] = kw
  return ids, w, count, sweeps, support


def cd_f64(G, cand_ids, cand_count, l1, l2, max_sweeps, tol, K=None, cols=None):
  """(W as a scipy CSC [n, n] in float64, column j = the solution of the masked problem j, cut to its K largest
  when K is given; the sweeps run per column)."""
  n = G.shape[0]
  rows, cs, vals = [], [], []
  run = np.zeros(n, np.int32)
  for j in (range(n) if cols is None else cols):
    items, jl, sub = local(G, j, cand_ids[j, :cand_count[j]])
    cand, wj, run[j] = slim_util.cd_column_f64(sub, jl, l1, l2, max_sweeps, tol)
    kid, kw = (items[cand], wj) if K is None else slim_util.cut(items[cand], wj, K)
    live = kw > 0
    rows.append(kid[live])
    cs.append(np.full(int(live.sum()), j))
    vals.append(kw[live])
  W = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cs))), shape=(n, n)) \
      if rows else sp.csc_matrix((n, n))
  return W, run


def screened(G, cand_ids, cand_count, l1):
  """How many candidates of every column pass the l1 screen (G[j, k] > l1, k != j)."""
  out = np.zeros(G.shape[0], np.int64)
  for j in range(G.shape[0]):
    items, jl, sub = local(G, j, cand_ids[j, :cand_count[j]])
    out[j] = len(slim_util.candidates(sub, jl, l1))
  return out


def kkt_residual(G, cand_ids, cand_count, W, l1, l2, cols):
  """``slim_util.kkt_residual`` of the masked problems: the largest violation of column j's optimality conditions
  over its candidates, for j in ``cols``; W [n, n] dense (float64)."""
  worst = 0.0
  for j in cols:
    items, jl, sub = local(G, j, cand_ids[j, :cand_count[j]])
    assert not np.delete(np.asarray(W[:, j]), items).any(), "column %d has a weight outside its candidates" % j
    worst = max(worst, slim_util.kkt_residual(sub, np.asarray(W)[np.ix_(items, [j])].repeat(len(items), axis=1),
                                              l1, l2, [jl]))
  return worst


def dense_model(ids, w, count):
  return slim_util.dense(ids, w, count)
