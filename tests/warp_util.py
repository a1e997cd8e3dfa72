"""Numpy restatement of the WARP / DNS step (recoder_amd/warp.py, rk_als_rank_sample and rk_als_warp_grad of
include/recoder_als.h) on bpr_util's counter RNG: the model-aware sampler for both modes, vectorised (float64,
or float32 for the measurement of what f32 costs) and as a literal per-slot walk written the slow way, the rank
weights, grad / step / fit on bpr_util's apply, and Recall / NDCG on the ML-20M slice."""
import math

import numpy as np
import scipy.sparse as sp

from tests import bpr_util

WARP, DNS = 0, 1
MAX_DRAWS = 256


def weight_table(n_items, rank_weight):
  """w(N), N = 0..256, as float32: one float64 value per N, each written out the long way."""
  w = [0.0]
  for N in range(1, MAX_DRAWS + 1):
    r = (n_items - 1) // N
    w.append(math.log(max(1, r)) if rank_weight == "log" else math.fsum(1.0 / k for k in range(1, r + 1)))
  return np.array(w, np.float64).astype(np.float32)


def exact_tables(n_users, n_items, h, seed, high_bias_users=(), csr=None):
  """Tables and bias drawn from {k / 8: k = -8..8}: every product is a multiple of 1/64 and every partial sum at
  h <= 512 fits 15 bits, so a score is exact in f32 in any summation order.  The items that the users
  ``high_bias_users`` hold (rows of ``csr``) get the bias 1 and those users the row 0: their positives score 1,
  no other item scores above 1, and so no candidate violates a margin of 0."""
  rng = np.random.RandomState(seed)
  X, Y = (rng.randint(-8, 9, (n, h)).astype(np.float32) / 8 for n in (n_users, n_items))
  b = rng.randint(-8, 9, n_items).astype(np.float32) / 8
  for u in high_bias_users:
    X[u] = 0
    b[csr.indices[csr.indptr[u]:csr.indptr[u + 1]]] = 1.0
  return X, Y, b


# ------------------------------------------------------------------ sampler
def decide(C, cand, S, s_pos, mode, num_candidates, margin):
  """The sequential rule, vectorised over the slots, on given scores S [T, D] (of S's dtype: float32 scores are
  compared in float32): (neg, trials, s_neg, written), ``written`` [T, D] the draws the rule scored."""
  T, D = C.shape
  rows, cols = np.arange(T), np.arange(D)[None, :]
  rank = np.cumsum(cand, axis=1)
  if mode == WARP:
    hit = cand & ((S - s_pos[:, None]) + S.dtype.type(margin) > 0)
    has, at = hit.any(1), hit.argmax(1)
    written = cand & (cols <= np.where(has, at, D)[:, None])
    trials = np.where(has, rank[rows, at], 0)
  else:
    written = cand & (rank <= num_candidates)
    has = written.any(1)
    at = np.where(written, S, -np.inf).argmax(1)          # (the first of equal maxima: the earlier draw)
    trials = written.sum(1)
  neg = np.where(has, C[rows, at], -1)
  s_neg = np.where(has, S[rows, at], 0).astype(S.dtype)
  return neg.astype(np.int32), trials.astype(np.int32), s_neg, written


class Sampler(bpr_util.Sampler):
  """bpr_util's draws, with the candidates of a slot scored against the tables."""

  def draws(self, seed, step, T, max_draws):
    """(users, pos, C, cand): draw 0's entry, the items of draws 1..max_draws [T, max_draws] and which of them
    the user does not hold."""
    keys = bpr_util.slot_keys(seed, step, T)
    e = bpr_util.draw(keys, 0, self.nnz)
    users = np.searchsorted(self.indptr, e, side="right") - 1
    pos = self.indices[e]
    C = np.stack([bpr_util.draw(keys, d, self.n_items) for d in range(1, max_draws + 1)], axis=1)
    q = users[:, None] * self.n_items + C
    at = np.minimum(np.searchsorted(self.held, q), len(self.held) - 1)
    return users, pos, C, self.held[at] != q

  def sample(self, seed, step, T, X, Y, b, mode, max_draws, num_candidates=1, margin=0.0, dtype=np.float64):
    """(users, pos, neg, trials int32 [T]; s_pos, s_neg [T] and scores [T, max_draws] of ``dtype``).  Scores are
    computed eight draws at a time, for the slots that are still open: the decisions are ``decide``'s."""
    X, Y, b = (np.asarray(a, dtype) for a in (X, Y, b))
    users, pos, C, cand = self.draws(seed, step, T, max_draws)
    s_pos = (X[users] * Y[pos]).sum(1) + b[pos]
    S = np.zeros(C.shape, dtype)
    open_ = np.ones(T, bool)
    for c0 in range(0, max_draws, 8):
      rows = np.flatnonzero(open_)
      if not len(rows):
        break
      Cc = C[rows, c0:c0 + 8]
      Sc = np.einsum("rh,rch->rc", X[users[rows]], Y[Cc]) + b[Cc]
      S[rows, c0:c0 + 8] = Sc
      if mode == WARP:
        open_[rows] = ~(cand[rows, c0:c0 + 8] & ((Sc - s_pos[rows, None]) + dtype(margin) > 0)).any(1)
      else:
        open_[rows] = cand[rows, :c0 + 8].sum(1) < num_candidates
    neg, trials, s_neg, written = decide(C, cand, S, s_pos, mode, num_candidates, margin)
    return (users.astype(np.int32), pos.astype(np.int32), neg, trials, s_pos, s_neg, np.where(written, S, 0).astype(dtype))

  def sample_literal(self, seed, step, T, X, Y, b, mode, max_draws, num_candidates=1, margin=0.0):
    """The same seven arrays in float64, one slot and one draw at a time, as the definition reads."""
    X, Y, b = (np.asarray(a, np.float64) for a in (X, Y, b))
    keys = bpr_util.slot_keys(seed, step, T)
    out = [np.zeros(T, np.int32) for _ in range(4)] + [np.zeros(T), np.zeros(T), np.zeros((T, max_draws))]
    users, pos, neg, trials, s_pos, s_neg, scores = out
    for t in range(T):
      e = int(bpr_util.draw(keys[t:t + 1], 0, self.nnz)[0])
      u = int(np.searchsorted(self.indptr, e, side="right")) - 1
      i = int(self.indices[e])
      row = set(self.indices[self.indptr[u]:self.indptr[u + 1]].tolist())
      sp_ = float(X[u] @ Y[i]) + b[i]
      users[t], pos[t], s_pos[t], neg[t] = u, i, sp_, -1
      n, best = 0, None
      for d in range(1, max_draws + 1):
        c = int(bpr_util.draw(keys[t:t + 1], d, self.n_items)[0])
        if c in row:
          continue
        s = float(X[u] @ Y[c]) + b[c]
        n += 1
        scores[t, d - 1] = s
        if mode == WARP:
          if (s - sp_) + margin > 0:
            neg[t], trials[t], s_neg[t] = c, n, s
            break
        else:
          if best is None or s > best:
            best = s
            neg[t], s_neg[t] = c, s
          trials[t] = n
          if n == num_candidates:
            break
    return tuple(out)


# --------------------------------------------------------------- grad / step
def grad(users, pos, neg, trials, X, Y, b, margin, weight, dtype=np.float64):
  """(g, loss, D, P) of WARP's hinge; invalid slots (neg < 0) give zeros everywhere."""
  X, Y, b = (np.asarray(a, dtype) for a in (X, Y, b))
  ok = neg >= 0
  u, i, j = users[ok], pos[ok], neg[ok]
  T, h = len(users), X.shape[1]
  D, P = np.zeros((T, h), dtype), np.zeros((T, h), dtype)
  D[ok], P[ok] = Y[i] - Y[j], X[u]
  g, loss = np.zeros(T, dtype), np.zeros(T, dtype)
  g[ok] = np.asarray(weight, dtype)[trials[ok]]
  s_pos, s_neg = (X[u] * Y[i]).sum(1) + b[i], (X[u] * Y[j]).sum(1) + b[j]
  loss[ok] = g[ok] * ((s_neg - s_pos) + dtype(margin))
  return g, loss, D, P


def step(sampler, seed, s, T, X, Y, b, lr, reg, margin, max_draws, weight, dtype=np.float64):
  """One WARP step: (X, Y, b, summed loss, valid slots, summed trials)."""
  users, pos, neg, trials, _, _, _ = sampler.sample(seed, s, T, X, Y, b, WARP, max_draws, 1, margin, dtype)
  g, loss, D, P = grad(users, pos, neg, trials, X, Y, b, margin, weight, dtype)
  X, Y, b = bpr_util.apply(users, pos, neg, g, D, P, X, Y, b, lr, reg, dtype)
  return X, Y, b, float(loss.sum(dtype=np.float64)), int((neg >= 0).sum()), int(trials.sum())


def fit(csr, X, Y, b, num_epochs, batch_size, lr, reg, margin=1.0, max_draws=32, rank_weight="log", seed=0,
        dtype=np.float64, first_step=0):
  """(X, Y, b, history, stats): recoder_amd.warp.fit restated."""
  csr = sp.csr_matrix(csr)
  sampler = Sampler(csr)
  weight = weight_table(csr.shape[1], rank_weight)
  X, Y, b = (np.array(a, dtype) for a in (X, Y, b))
  steps = -(-csr.nnz // batch_size)
  hist, stats, s = [], [], int(first_step)
  for _ in range(num_epochs):
    total, count, drawn = 0.0, 0, 0
    for _ in range(steps):
      X, Y, b, l, c, n = step(sampler, seed, s, batch_size, X, Y, b, lr, reg, margin, max_draws, weight, dtype)
      total, count, drawn, s = total + l, count + c, drawn + n, s + 1
    hist.append(total / count if count else float("nan"))
    stats.append((count / (steps * batch_size), drawn / count if count else float("nan")))
  return X, Y, b, hist, stats


def fit_dns(csr, X, Y, b, num_epochs, batch_size, lr, reg, num_candidates, seed=0, dtype=np.float64, first_step=0):
  """(X, Y, b, history): bpr_util.fit with the negative of a slot the hardest of ``num_candidates``."""
  csr = sp.csr_matrix(csr)
  sampler = Sampler(csr)
  X, Y, b = (np.array(a, dtype) for a in (X, Y, b))
  steps = -(-csr.nnz // batch_size)
  hist, s = [], int(first_step)
  for _ in range(num_epochs):
    total, count = 0.0, 0
    for _ in range(steps):
      users, pos, neg = sampler.sample(seed, s, batch_size, X, Y, b, DNS, bpr_util.MAX_DRAWS, num_candidates,
                                       dtype=dtype)[:3]
      X, Y, b, l, c = bpr_util.step(users, pos, neg, X, Y, b, lr, reg, dtype)
      total, count, s = total + l, count + c, s + 1
    hist.append(total / count if count else float("nan"))
  return X, Y, b, hist


# ----------------------------------------------------------------- quality
def recall_ndcg(X, Y, b, x, y):
  from tests import rp3_util
  lists = []
  for b0 in range(0, x.shape[0], 1000):
    lists.append(rp3_util.top_k(X[b0:b0 + 1000] @ Y.T + b[None, :], x[b0:b0 + 1000], 100))
  return rp3_util.metric_means(np.concatenate(lists), y)


def quality_f64(x, y, h, epochs, batch_size, lr, reg, margin=1.0, max_draws=32, rank_weight="log", num_candidates=None,
                seed=0, init_seed=0):
  """[(epoch, Recall@20, NDCG@100, the epoch's loss, valid share, mean trials)] of the float64 fit on (x: train,
  y: held out) from the model's xavier-uniform start, measured after each epoch count in ``epochs`` (one fit,
  continued).  ``num_candidates`` given: BPR with DNS instead of WARP (share and trials are None)."""
  X, Y, b = bpr_util.xavier_tables(x.shape[0], x.shape[1], h, init_seed)
  steps = -(-x.nnz // batch_size)
  out, done = [], 0
  for ep in sorted(epochs):
    if num_candidates is None:
      X, Y, b, hist, stats = fit(x, X, Y, b, ep - done, batch_size, lr, reg, margin, max_draws, rank_weight, seed,
                                 first_step=done * steps)
    else:
      X, Y, b, hist = fit_dns(x, X, Y, b, ep - done, batch_size, lr, reg, num_candidates, seed, first_step=done * steps)
      stats = [(None, None)]
    done = ep
    r, n = recall_ndcg(X, Y, b, x, y)
    out.append((ep, r, n, hist[-1]) + tuple(stats[-1]))
  return out
