"""Numpy restatement of the BPR step (recoder_amd/bpr.py, the rk_als_bpr_* part of include/recoder_als.h):
the sampler bit for bit with numpy integers, grad / apply / fit in float64 (or, for the measurement of
what f32 costs, in float32), a literal per-triple step written the slow way, and the held-out AUC and
Recall / NDCG of a pair of tables."""
import os

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_DRAWS = 32
_U = np.uint64


# ------------------------------------------------------------------ sampler
def mix(z):
  """splitmix64's output function on uint64 arrays (arithmetic modulo 2^64)."""
  z = np.asarray(z, dtype=_U)
  with np.errstate(over="ignore"):
    z = z + _U(0x9E3779B97F4A7C15)
    z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def slot_keys(seed, step, T):
  seed_key = mix(np.array([int(seed) % 2 ** 64], dtype=_U))[0]
  packed = (_U(int(step)) << _U(32)) | np.arange(T, dtype=_U)
  return mix(seed_key ^ packed)


def draw(keys, d, rng):
  """Draw number d of every slot mapped to [0, rng): (high 32 bits * rng) >> 32."""
  with np.errstate(over="ignore"):
    r = mix(keys + _U(d))
  return (((r >> _U(32)) * _U(int(rng))) >> _U(32)).astype(np.int64)


class Sampler:
  """The kernel's draws over one CSR, restated with numpy integers."""

  def __init__(self, csr):
    csr = sp.csr_matrix(csr)
    self.n_users, self.n_items = csr.shape
    self.indptr, self.indices = csr.indptr.astype(np.int64), csr.indices.astype(np.int64)
    self.nnz = int(self.indptr[-1])
    assert 1 <= self.nnz < 2 ** 31 and csr.has_sorted_indices
    # every stored (user, item) as one ascending integer: membership is a binary search, as in the kernel
    self.held = np.repeat(np.arange(self.n_users, dtype=np.int64), np.diff(self.indptr)) * self.n_items + self.indices

  def sample(self, seed, step, T):
    keys = slot_keys(seed, step, T)
    e = draw(keys, 0, self.nnz)
    users = np.searchsorted(self.indptr, e, side="right") - 1         # the last u with indptr[u] <= e
    pos = self.indices[e]
    neg = np.full(T, -1, np.int64)
    open_ = np.ones(T, bool)
    for d in range(1, MAX_DRAWS + 1):
      if not open_.any():
        break
      c = draw(keys, d, self.n_items)
      q = users * self.n_items + c
      at = np.searchsorted(self.held, q)
      member = (at < len(self.held)) & (self.held[np.minimum(at, len(self.held) - 1)] == q)
      take = open_ & ~member
      neg[take] = c[take]
      open_ &= member
    return users.astype(np.int32), pos.astype(np.int32), neg.astype(np.int32)


def sample(csr, seed, step, T):
  """(users, pos, neg) int32 [T] of step ``step`` under ``seed``."""
  return Sampler(csr).sample(seed, step, T)


# --------------------------------------------------------------- grad / apply
def grad(users, pos, neg, X, Y, b, dtype=np.float64):
  """(x, g, loss, D, P) of the triples; invalid slots (neg < 0) give zeros everywhere."""
  X, Y, b = (np.asarray(a, dtype) for a in (X, Y, b))
  ok = neg >= 0
  u, i, j = users[ok], pos[ok], neg[ok]
  T, h = len(users), X.shape[1]
  D, P = np.zeros((T, h), dtype), np.zeros((T, h), dtype)
  D[ok], P[ok] = Y[i] - Y[j], X[u]
  x = np.zeros(T, dtype)
  x[ok] = (P[ok] * D[ok]).sum(1) + b[i] - b[j]
  e = np.exp(-np.abs(x))
  g = np.where(x >= 0, e / (1 + e), 1 / (1 + e)).astype(dtype)
  loss = (np.maximum(-x, 0) + np.log1p(e)).astype(dtype)
  g[~ok] = 0
  loss[~ok] = 0
  return x, g, loss, D, P


def apply(users, pos, neg, g, D, P, X, Y, b, lr, reg, dtype=np.float64):
  """New (X, Y, b) from the step's g and staging rows."""
  X, Y, b = (np.array(a, dtype) for a in (X, Y, b))
  ok = neg >= 0
  u, i, j = users[ok], pos[ok], neg[ok]
  gg = np.asarray(g, dtype)[ok]
  Dk, Pk = np.asarray(D, dtype)[ok], np.asarray(P, dtype)[ok]
  sX, sY, sb = np.zeros_like(X), np.zeros_like(Y), np.zeros_like(b)
  np.add.at(sX, u, gg[:, None] * Dk)
  np.add.at(sY, i, gg[:, None] * Pk)
  np.add.at(sY, j, -gg[:, None] * Pk)
  np.add.at(sb, i, gg)
  np.add.at(sb, j, -gg)
  cu = np.bincount(u, minlength=X.shape[0]).astype(dtype)
  ci = (np.bincount(i, minlength=Y.shape[0]) + np.bincount(j, minlength=Y.shape[0])).astype(dtype)
  lr, reg = dtype(lr), dtype(reg)
  return X + lr * (sX - reg * cu[:, None] * X), Y + lr * (sY - reg * ci[:, None] * Y), b + lr * (sb - reg * ci * b)


def step(users, pos, neg, X, Y, b, lr, reg, dtype=np.float64):
  """One step on given triples: (X, Y, b, summed loss, valid triples)."""
  _, g, loss, D, P = grad(users, pos, neg, X, Y, b, dtype)
  X, Y, b = apply(users, pos, neg, g, D, P, X, Y, b, lr, reg, dtype)
  return X, Y, b, float(loss.sum(dtype=np.float64)), int((neg >= 0).sum())


def step_literal(users, pos, neg, X, Y, b, lr, reg):
  """The same step written the slow way: every triple's gradient at the start-of-step tables, one at a
  time, into per-row sums and counts."""
  X0, Y0, b0 = (np.array(a, np.float64) for a in (X, Y, b))
  gX, gY, gb = np.zeros_like(X0), np.zeros_like(Y0), np.zeros_like(b0)
  cu, ci = np.zeros(len(X0)), np.zeros(len(Y0))
  for u, i, j in zip(users, pos, neg):
    if j < 0:
      continue
    x = X0[u] @ (Y0[i] - Y0[j]) + b0[i] - b0[j]
    g = 1.0 / (1.0 + np.exp(x))
    gX[u] += g * (Y0[i] - Y0[j])
    gY[i] += g * X0[u]
    gY[j] -= g * X0[u]
    gb[i] += g
    gb[j] -= g
    cu[u] += 1
    ci[i] += 1
    ci[j] += 1
  return (X0 + lr * (gX - reg * cu[:, None] * X0), Y0 + lr * (gY - reg * ci[:, None] * Y0),
          b0 + lr * (gb - reg * ci * b0))


def fit(csr, X, Y, b, num_epochs, batch_size, lr, reg, seed=0, dtype=np.float64, first_step=0):
  """(X, Y, b, history): recoder_amd.bpr.fit restated, on the triples the kernel's sampler draws."""
  csr = sp.csr_matrix(csr)
  sampler = Sampler(csr)
  X, Y, b = (np.array(a, dtype) for a in (X, Y, b))
  steps = -(-csr.nnz // batch_size)
  hist, s = [], int(first_step)
  for _ in range(num_epochs):
    total, count = 0.0, 0
    for _ in range(steps):
      users, pos, neg = sampler.sample(seed, s, batch_size)
      X, Y, b, l, c = step(users, pos, neg, X, Y, b, lr, reg, dtype)
      total, count, s = total + l, count + c, s + 1
    hist.append(total / count if count else float("nan"))
  return X, Y, b, hist


# ----------------------------------------------------------------- quality
def auc(X, Y, b, train, held_out):
  """Mean over the users with held-out items of the share of (held-out item, item in neither matrix) pairs
  the scores order correctly (ties count half), in float64."""
  X, Y, b = (np.asarray(a, np.float64) for a in (X, Y, b))
  train, held_out = sp.csr_matrix(train), sp.csr_matrix(held_out)
  out = []
  for u in range(held_out.shape[0]):
    t = held_out.indices[held_out.indptr[u]:held_out.indptr[u + 1]]
    if not len(t):
      continue
    s = Y @ X[u] + b
    rest = np.ones(Y.shape[0], bool)
    rest[t] = False
    rest[train.indices[train.indptr[u]:train.indptr[u + 1]]] = False
    if not rest.any():
      continue
    r = np.sort(s[rest])
    below = np.searchsorted(r, s[t], side="left")
    ties = np.searchsorted(r, s[t], side="right") - below
    out.append(float(np.mean((below + 0.5 * ties) / len(r))))
  return float(np.mean(out))


def edge_matrix():
  """37 users x 53 items: user 3 holds every item but one (rejection runs to many draws), user 5 every item
  (every slot that lands there is invalid), user 7 none."""
  rng = np.random.RandomState(11)
  m = (rng.rand(37, 53) < 0.15).astype(np.float32)
  m[3, :] = 1.0
  m[3, 17] = 0.0
  m[5, :] = 1.0
  m[7, :] = 0.0
  m = sp.csr_matrix(m)
  m.sort_indices()
  return m


def planted(n_users=200, n_items=120, rank=4, density=0.12, seed=0, hold=0.2):
  """(train, held_out): a user holds the items of its largest planted rank-``rank`` scores (plus a popularity
  term); a share ``hold`` of every user's items is held out."""
  rng = np.random.RandomState(seed)
  S = rng.randn(n_users, rank) @ rng.randn(rank, n_items) + 0.5 * rng.randn(n_items)[None, :]
  k = max(2, int(round(density * n_items)))
  tr, ho = sp.lil_matrix((n_users, n_items), dtype=np.float32), sp.lil_matrix((n_users, n_items), dtype=np.float32)
  for u in range(n_users):
    items = rng.permutation(np.argsort(-S[u])[:k])
    cut = max(1, int(round(hold * k)))
    ho[u, items[:cut]] = 1.0
    tr[u, items[cut:]] = 1.0
  tr, ho = tr.tocsr(), ho.tocsr()
  tr.sort_indices()
  ho.sort_indices()
  return tr, ho


def init_tables(n_users, n_items, h, seed, scale=0.1):
  rng = np.random.RandomState(seed)
  return ((scale * rng.randn(n_users, h)).astype(np.float32), (scale * rng.randn(n_items, h)).astype(np.float32),
          np.zeros(n_items, np.float32))


def xavier_tables(n_users, n_items, h, seed):
  """The start MatrixFactorization.init_model gives (xavier-uniform tables, zero bias), from numpy's generator."""
  rng = np.random.RandomState(seed)
  bu, bi = np.sqrt(6.0 / (n_users + h)), np.sqrt(6.0 / (n_items + h))
  return (rng.uniform(-bu, bu, (n_users, h)).astype(np.float32), rng.uniform(-bi, bi, (n_items, h)).astype(np.float32),
          np.zeros(n_items, np.float32))


def load_slice():
  from tests import userknn_util
  return userknn_util.load_slice()


def quality_f64(x, y, h, num_epochs, batch_size, lr, reg, seed=0, init_seed=0):
  """(Recall@20, NDCG@100, last epoch's loss) of the float64 fit on (x: train, y: held out), from
  the model's xavier-uniform start."""
  from tests import rp3_util
  X, Y, b = xavier_tables(x.shape[0], x.shape[1], h, init_seed)
  X, Y, b, hist = fit(x, X, Y, b, num_epochs, batch_size, lr, reg, seed)
  lists = []
  for b0 in range(0, x.shape[0], 1000):
    S = X[b0:b0 + 1000] @ Y.T + b[None, :]
    lists.append(rp3_util.top_k(S, x[b0:b0 + 1000], 100))
  r, n = rp3_util.metric_means(np.concatenate(lists), y)
  return r, n, hist[-1]
