"""Numpy restatements of RP3beta (Paudel et al. 2016), written from the formulas:

    S[i, j] = sum over the users v that hold i and j of r_v^-alpha
    W[i, j] = d_i^-alpha * S[i, j] * d_j^-beta (j != i),   W[i, i] = 0
    row i keeps its K largest W[i, j] > 0 by (W descending, j ascending)
    scores = X W

(r_v: items of user v, d_i: users of item i; the stored entries are edges, their values play no part
in the fit.)  ``fit_f64`` is the float64 model; ``fit_f32`` restates the two f32 chains the kernels
promise, row by row and without an n x n array.  They are the comparators of the RP3beta tests and
never the code under test."""
import numpy as np
import scipy.sparse as sp

from tests import ease_util

SLICE = ease_util.SLICE


def degrees(X):
  X = sp.csr_matrix(X)
  r = np.diff(X.indptr).astype(np.float64)
  d = np.bincount(X.indices, minlength=X.shape[1]).astype(np.float64)
  return r, d


def weights_f64(X, alpha, beta):
  """(r^-alpha, d^-alpha, d^-beta) in float64, 0 where the degree is 0."""
  r, d = degrees(X)

  def power(x, e):
    out = np.zeros_like(x)
    out[x > 0] = x[x > 0] ** -e
    return out
  return power(r, alpha), power(d, alpha), power(d, beta)


def dense_w_f64(X, user_w, row_scale, col_scale):
  """The uncut W as a scipy CSR in float64 from the three weight vectors (sparse products only)."""
  B = sp.csr_matrix(X).astype(np.float64)
  B.data[:] = 1.0
  S = (B.T @ sp.diags(np.asarray(user_w, np.float64)) @ B).tocsr()
  W = (sp.diags(np.asarray(row_scale, np.float64)) @ S @ sp.diags(np.asarray(col_scale, np.float64))).tocoo()
  off = W.row != W.col
  W = sp.csr_matrix((W.data[off], (W.row[off], W.col[off])), shape=W.shape)
  W.eliminate_zeros()
  W.sort_indices()
  return W


def cut(W, K):
  """Every row's K largest entries > 0 by (W descending, j ascending), as a CSR with ascending ids."""
  W = sp.csr_matrix(W)
  rows, cols, vals = [], [], []
  for i in range(W.shape[0]):
    j = W.indices[W.indptr[i]:W.indptr[i + 1]]
    v = W.data[W.indptr[i]:W.indptr[i + 1]]
    keep = v > 0
    j, v = j[keep], v[keep]
    top = np.sort(j[np.argsort(-v, kind="stable")[:K]])       # (j ascending: a stable sort keeps the lower ids)
    sel = np.isin(j, top)
    rows.append(np.full(int(sel.sum()), i))
    cols.append(j[sel])
    vals.append(v[sel])
  return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=W.shape)


def fit_f64(X, alpha, beta, K):
  """The float64 model as a CSR [n, n] with at most K entries per row."""
  return cut(dense_w_f64(X, *weights_f64(X, alpha, beta)), K)


def fit_f32(X, user_w, row_scale, col_scale, K, rows=None):
  """(ids int32 [n, K], w f32 [n, K], count int32 [n]): S[i, :] is one f32 add chain per column over the
  users of item i, ascending; W = (row_scale[i] * S) * col_scale in two f32 multiplies; a stable sort on
  (-W, j) picks the K; the kept entries are stored with ascending ids, -1 / +0 behind them.  One row of n
  floats at a time."""
  X = sp.csr_matrix(X)
  Xt = X.T.tocsr()
  Xt.sort_indices()
  n = X.shape[1]
  user_w, row_scale, col_scale = (np.asarray(a, np.float32) for a in (user_w, row_scale, col_scale))
  ids = np.full((n, K), -1, np.int32)
  w = np.zeros((n, K), np.float32)
  count = np.zeros(n, np.int32)
  for i in (range(n) if rows is None else rows):
    S = np.zeros(n, np.float32)
    for v in Xt.indices[Xt.indptr[i]:Xt.indptr[i + 1]]:
      S[X.indices[X.indptr[v]:X.indptr[v + 1]]] += user_w[v]
    Wi = (row_scale[i] * S) * col_scale
    assert Wi.dtype == np.float32
    Wi[i] = 0.0
    cand = np.flatnonzero(Wi > 0)
    top = np.sort(cand[np.argsort(-Wi[cand], kind="stable")[:K]])
    count[i] = len(top)
    ids[i, :len(top)] = top
    w[i, :len(top)] = Wi[top]
  return ids, w, count


def scores_f32(X, ids, w, count, lo=0, hi=None):
  """out[u, c]: the ascending f32 fmaf chain from +0 over the stored entries (i, x) of row u of
  x * W[i, lo + c], W the sparse matrix (ids, w, count) spell.  Entry e of every user at once: the ids of
  one neighbour row are distinct, so a fancy-indexed update is one chain step per column."""
  X = sp.csr_matrix(X).astype(np.float32)
  X.sort_indices()
  n = ids.shape[0]
  hi = n if hi is None else hi
  out = np.zeros((X.shape[0], hi - lo), np.float32)
  lens = np.diff(X.indptr)
  K = ids.shape[1]
  for e in range(int(lens.max()) if len(lens) else 0):
    users = np.flatnonzero(lens > e)
    pos = X.indptr[users] + e
    items, x = X.indices[pos], X.data[pos]
    j = ids[items]                                             # [U, K]
    live = (np.arange(K)[None, :] < count[items][:, None]) & (j >= lo) & (j < hi)
    uu = np.broadcast_to(users[:, None], j.shape)[live]
    jj = j[live] - lo
    out[uu, jj] = ease_util.fmaf(np.broadcast_to(x[:, None], j.shape)[live], w[items][live], out[uu, jj])
  return out


def top_k(S, seen, k):
  """Top-k unseen ids by (score descending, id ascending), [users, k]; S is modified (seen at -inf)."""
  seen = sp.csr_matrix(seen)
  for u in range(S.shape[0]):
    S[u, seen.indices[seen.indptr[u]:seen.indptr[u + 1]]] = -np.inf
  kth = np.partition(S, S.shape[1] - k, axis=1)[:, S.shape[1] - k]
  out = np.empty((S.shape[0], k), np.int64)
  for u in range(S.shape[0]):
    idx = np.flatnonzero(S[u] >= kth[u])
    out[u] = idx[np.argsort(-S[u, idx], kind="stable")[:k]]
  return out


def metric_means(lists, y, ks=((20, "recall"), (100, "ndcg"))):
  """Mean Recall@k (normalised) / NDCG@k over the users with held-out items."""
  from recoder_amd import metrics as M
  out = []
  for k, kind in ks:
    vals = []
    for u in range(y.shape[0]):
      t = y.indices[y.indptr[u]:y.indptr[u + 1]]
      if len(t):
        vals.append(M.recall(lists[u], t, k) if kind == "recall" else M.ndcg(lists[u], t, k))
    out.append(float(np.mean(vals)))
  return out


def graph_matrix(n_users, n, density, seed, empty=(0,), full=None, none=None):
  """Random binary CSR with empty users, one item every other user holds (``full``) and one item nobody
  holds (``none``)."""
  rng = np.random.RandomState(seed)
  m = (rng.rand(n_users, n) < density).astype(np.float32)
  if full is not None:
    m[:, full] = 1.0
  if none is not None:
    m[:, none] = 0.0
  for r in empty:
    m[r, :] = 0.0
  m = sp.csr_matrix(m)
  m.eliminate_zeros()
  m.sort_indices()
  return m
