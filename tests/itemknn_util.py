"""Numpy restatements of ItemKNN (the shrunk item-neighbourhood baseline of Dacrema et al. 2019), written from
the formulas.  With a_vi the (feature-weighted) value of user v for item i and j the own item (column j of W):

    s[i, j]   = sum over the users v that hold i and j of a_vj * a_vi
    cosine:     sim = s / (|a_j| |a_i| + shrink)
    asymmetric: sim = s / (|a_j|^(2(1 - alpha)) |a_i|^(2 alpha) + shrink)                 (Aiolli 2013)
    tversky:    sim = s / (beta d_j + alpha d_i + (1 - alpha - beta) s + shrink)  on the binary matrix, i.e.
                s / (s + alpha |i \\ j| + beta |j \\ i| + shrink); jaccard: alpha = beta = 1, dice: alpha = beta = 1/2
    sim[j, j] = 0; column j keeps its K largest sim > 0 by (sim descending, i ascending)
    scores = X W

    tfidf: a_vi = sqrt(x_vi) max(0, log(n_items / (1 + r_v)))
    bm25:  a_vi = x_vi (k1 + 1) / (k1 ((1 - b) + b len_i / mean len) + x_vi) max(0, log(n_items / (1 + r_v))),
           len_i = sum_v x_vi, k1 = 1.2, b = 0.75

``fit_f64`` is the float64 model; ``fit_f32`` restates the f32 chains include/recoder_rp3.h promises for
rk_rp3_item_fit, column by column.  They are the comparators of the ItemKNN tests and never the code under test."""
import numpy as np
import scipy.sparse as sp

from tests import ease_util, rp3_util

SLICE = ease_util.SLICE
K1, B = 1.2, 0.75
SET_KINDS = {"jaccard": (1.0, 1.0), "dice": (0.5, 0.5)}


def weighted_f64(X, kind):
  """The feature-weighted matrix (users x items, the structure of X) in float64."""
  X = sp.csr_matrix(X).astype(np.float64)
  X.sort_indices()
  if kind == "none":
    return X
  n_users, n = X.shape
  r = np.diff(X.indptr).astype(np.float64)
  idf = np.maximum(0.0, np.log(n / (1.0 + r)))
  rows = np.repeat(np.arange(n_users), np.diff(X.indptr))
  if kind == "tfidf":
    data = np.sqrt(X.data) * idf[rows]
  elif kind == "bm25":
    length = np.asarray(X.sum(axis=0)).ravel()
    norm = (1.0 - B) + B * length / length.mean()
    data = X.data * (K1 + 1.0) / (K1 * norm[X.indices] + X.data) * idf[rows]
  else:
    raise ValueError(kind)
  return sp.csr_matrix((data, X.indices.copy(), X.indptr.copy()), shape=X.shape)


def vectors_f64(A, similarity, asymmetric_alpha=0.5, tversky_alpha=1.0, tversky_beta=1.0):
  """(form, own, oth, g, binary) in float64: the denominator's two vectors, and whether the dot products run on
  the binary matrix."""
  A = sp.csr_matrix(A).astype(np.float64)
  if similarity in ("cosine", "asymmetric"):
    sq = np.asarray(A.multiply(A).sum(axis=0)).ravel()
    al = 0.5 if similarity == "cosine" else float(asymmetric_alpha)
    return 0, sq ** (1.0 - al), sq ** al, 0.0, False
  ta, tb = SET_KINDS.get(similarity, (float(tversky_alpha), float(tversky_beta)))
  d = np.bincount(A.indices, minlength=A.shape[1]).astype(np.float64)
  return 1, tb * d, ta * d, 1.0 - ta - tb, True


def sims_f64(A, form, own, oth, g, shrink, binary):
  """The uncut W [n, n] as a scipy CSR in float64, W[i, j] = sim of neighbour i for the own item j."""
  A = sp.csr_matrix(A).astype(np.float64)
  if binary:
    A = A.copy()
    A.data[:] = 1.0
  S = (A.T @ A).tocoo()
  i, j, s = S.row, S.col, S.data
  den = own[j] * oth[i] + shrink if form == 0 else own[j] + oth[i] + g * s + shrink
  ok = (i != j) & (s > 0) & (den > 0)
  W = sp.csr_matrix((s[ok] / den[ok], (i[ok], j[ok])), shape=S.shape)
  W.sort_indices()
  return W


def cut_columns(W, K):
  """Every column's K largest entries > 0 by (value descending, row id ascending): rp3_util.cut on the transpose."""
  return rp3_util.cut(sp.csr_matrix(W).T.tocsr(), K).T.tocsr()


def fit_f64(X, K, shrink, similarity="cosine", feature_weighting="none", asymmetric_alpha=0.5, tversky_alpha=1.0,
            tversky_beta=1.0):
  """The float64 model as a CSR [n, n] with at most K entries per column."""
  A = weighted_f64(X, feature_weighting)
  return cut_columns(sims_f64(A, *vectors_f64(A, similarity, asymmetric_alpha, tversky_alpha, tversky_beta)[:4],
                              shrink, similarity not in ("cosine", "asymmetric")), K)


def sim_column_f32(A, At, j, form, own, oth, g, shrink, binary):
  """sim[:, j] in f32 exactly as the header promises: one fmaf(a_vj, a_vi, acc) chain per i from +0 over the
  users of item j, ascending (plain adds of 1.0 on the binary matrix); the denominator and the quotient in
  separately rounded f32 operations; +0 unless s > 0 and den > 0; the diagonal 0."""
  n = A.shape[1]
  s = np.zeros(n, np.float32)
  for e in range(At.indptr[j], At.indptr[j + 1]):
    v = At.indices[e]
    cols = A.indices[A.indptr[v]:A.indptr[v + 1]]
    if binary:
      s[cols] += np.float32(1.0)
    else:
      s[cols] = ease_util.fmaf(At.data[e], A.data[A.indptr[v]:A.indptr[v + 1]], s[cols])
  with np.errstate(all="ignore"):
    if form == 0:
      den = np.float32(own[j]) * oth + shrink
    else:
      den = ((np.float32(own[j]) + oth) + (g * s)) + shrink
    assert den.dtype == np.float32 and s.dtype == np.float32
    sim = np.where((s > 0) & (den > 0), s / np.where(den > 0, den, np.float32(1.0)), np.float32(0.0))
  sim[j] = 0.0
  assert sim.dtype == np.float32
  return sim


def ranked_f32(A, form, own, oth, g, shrink, kmax, binary, cols=None):
  """Per column j (None for a column outside ``cols``): (ids, sims) of its ``kmax`` largest sim > 0 in the order
  (sim descending, i ascending), from ``sim_column_f32``.  ``A``: the weighted matrix whose f32 values the kernel
  is given; own / oth / g / shrink are rounded to f32 as the call rounds them."""
  A = sp.csr_matrix(A).astype(np.float32)
  A.sort_indices()
  At = A.T.tocsr()
  At.sort_indices()
  own, oth = np.asarray(own, np.float32), np.asarray(oth, np.float32)
  g, shrink = np.float32(g), np.float32(shrink)
  out = [None] * A.shape[1]
  for j in (range(A.shape[1]) if cols is None else cols):
    sim = sim_column_f32(A, At, j, form, own, oth, g, shrink, binary)
    cand = np.flatnonzero(sim > 0)
    top = cand[np.argsort(-sim[cand], kind="stable")[:kmax]]      # (ids ascending: a stable sort keeps the lower ids)
    out[j] = (top, sim[top])
  return out


def cut_ranked(ranked, K):
  """(ids int32 [n, K], w f32 [n, K], count int32 [n]): every column's first K of ``ranked_f32`` stored with
  ascending ids, -1 / +0 behind them."""
  n = len(ranked)
  ids = np.full((n, K), -1, np.int32)
  w = np.zeros((n, K), np.float32)
  count = np.zeros(n, np.int32)
  for j, col in enumerate(ranked):
    if col is not None:
      top, sim = col[0][:K], col[1][:K]
      order = np.argsort(top)
      count[j] = len(top)
      ids[j, :len(top)] = top[order]
      w[j, :len(top)] = sim[order]
  return ids, w, count


def fit_f32(A, form, own, oth, g, shrink, K, binary, cols=None):
  """(ids, w, count) of the f32 restatement at K neighbours."""
  return cut_ranked(ranked_f32(A, form, own, oth, g, shrink, K, binary, cols), K)


def dense_f32(A, form, own, oth, g, shrink, binary):
  """The uncut f32 W [n, n] (small n only)."""
  A = sp.csr_matrix(A).astype(np.float32)
  A.sort_indices()
  At = A.T.tocsr()
  At.sort_indices()
  own, oth = np.asarray(own, np.float32), np.asarray(oth, np.float32)
  return np.stack([sim_column_f32(A, At, j, form, own, oth, np.float32(g), np.float32(shrink), binary)
                   for j in range(A.shape[1])], axis=1)


def scores_binary_f32(X, ids, w, count):
  """slim_util.scores_f32 for a BINARY X without its [users, n] work per neighbour slot: x = 1 makes a chain
  step fmaf(1, w, acc) = the f32 sum acc + w, and ``np.add.at`` on an f32 row adds its operands one after the
  other in the order given -- rows i of W taken in ascending i give every (user, column) its ascending chain."""
  X = sp.csr_matrix(X)
  X.sort_indices()
  assert np.all(X.data == 1.0)
  n, K = ids.shape
  live = np.arange(K)[None, :] < count[:, None]
  cols = np.broadcast_to(np.arange(n)[:, None], (n, K))
  W = sp.csr_matrix((w[live], (ids[live], cols[live])), shape=(n, n))       # W[i, j], rows i
  W.sort_indices()
  out = np.zeros((X.shape[0], n), np.float32)
  for u in range(X.shape[0]):
    items = X.indices[X.indptr[u]:X.indptr[u + 1]]
    if len(items):
      sel = np.concatenate([np.arange(W.indptr[i], W.indptr[i + 1]) for i in items])
      np.add.at(out[u], W.indices[sel], W.data[sel])
  return out


def popularity_lists(X, k):
  pop = np.tile(rp3_util.degrees(X)[1].astype(np.float32), (X.shape[0], 1))
  return rp3_util.top_k(pop, X, k)


def quality(X, y, W64):
  """(Recall@20, NDCG@100) of the float64 model W64 [n, n] on the held-out y, seen items masked."""
  S = np.asarray((sp.csr_matrix(X).astype(np.float64) @ W64).todense())
  return rp3_util.metric_means(rp3_util.top_k(S, X, 100), y)

