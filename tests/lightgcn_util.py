"""Numpy restatement of LightGCN training (recoder_amd/lightgcn.py, the rk_als_lgcn_* part of
include/recoder_als.h) on the sampler, ``planted``, ``auc`` and ``load_slice`` of tests/bpr_util.py: in float64 (the
model, pinned by finite differences and by the dense normalised adjacency), and in float32 in the kernels'
operation order -- every fmaf(a, b, c) as the float64 a * b + c rounded to f32 (the product of two f32 is exact in
float64) -- for the measurement of what f32 costs.  The f32 form sums a long row as one chain, not in the kernel's
parts: it is used on matrices without such rows."""
import numpy as np
import scipy.sparse as sp

from tests import bpr_util

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
F32, F64 = np.float32, np.float64


def fma32(a, b, c):
  return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def scales(m):
  """(s_u, s_i): degree^-1/2 in float64 rounded once to f32, 0 for degree 0."""
  m = sp.csr_matrix(m)
  out = []
  for deg in (np.diff(m.indptr), np.bincount(m.indices, minlength=m.shape[1])):
    s = np.zeros(len(deg), F64)
    s[deg > 0] = deg[deg > 0].astype(F64) ** -0.5
    out.append(s.astype(F32))
  return out


def transpose(m):
  mt = sp.csr_matrix(m).T.tocsr()
  mt.sort_indices()
  return mt


def adjacency(m):
  """The dense (users + items) x (users + items) normalised adjacency, float64 (from the f32 scales)."""
  m = sp.csr_matrix(m)
  U, n = m.shape
  su, si = (s.astype(F64) for s in scales(m))
  B = su[:, None] * (m.toarray() != 0) * si[None, :]
  A = np.zeros((U + n, U + n))
  A[:U, U:], A[U:, :U] = B, B.T
  return A


def propagate(m, rs, cs, F, dtype=F64, acc=None, acc_scale=1.0):
  """(out, acc): out[r] = rs[r] sum_j cs[col_j] F[col_j]; acc = (acc + out) acc_scale when given."""
  m = sp.csr_matrix(m)
  if dtype == F64:
    B = sp.csr_matrix((np.asarray(cs, F64)[m.indices], m.indices, m.indptr), shape=m.shape)
    out = np.asarray(rs, F64)[:, None] * (B @ np.asarray(F, F64))
  else:
    F, rs, cs = np.asarray(F, F32), np.asarray(rs, F32), np.asarray(cs, F32)
    s = np.zeros((m.shape[0], F.shape[1]), F32)
    lens = np.diff(m.indptr)
    for j in range(int(lens.max()) if len(lens) else 0):      # entry j of every row that has one: ascending chains
      rows = np.nonzero(lens > j)[0]
      cols = m.indices[m.indptr[rows] + j]
      s[rows] = fma32(cs[cols][:, None], F[cols], s[rows])
    out = rs[:, None] * s
  if acc is not None:
    acc = ((np.asarray(acc, dtype) + out) * dtype(acc_scale)).astype(dtype)
  return out, acc


def forward(m, Eu, Ei, K, dtype=F64):
  """The final tables (P, Q): the mean over the layers 0..K."""
  m, mt = sp.csr_matrix(m), transpose(m)
  su, si = scales(m)
  Pk, Qk = np.asarray(Eu, dtype), np.asarray(Ei, dtype)
  P, Q = Pk.copy(), Qk.copy()
  for k in range(K):
    scale = (F32(1.0 / (K + 1)) if dtype == F32 else 1.0 / (K + 1)) if k == K - 1 else 1.0
    (Pk, P), (Qk, Q) = propagate(m, su, si, Qk, dtype, P, scale), propagate(mt, si, su, Pk, dtype, Q, scale)
  return P, Q


def scatter(users, pos, neg, g, D, Pt, n_users, n_items, dtype=F64):
  """(Gu, Gi, cu, ci): the gradient with respect to the final tables (divided by T) and the counts."""
  T, h = D.shape
  ok = neg >= 0
  u, i, j = users[ok], pos[ok], neg[ok]
  cu = np.bincount(u, minlength=n_users).astype(np.int32)
  ci = (np.bincount(i, minlength=n_items) + np.bincount(j, minlength=n_items)).astype(np.int32)
  Gu, Gi = np.zeros((n_users, h), dtype), np.zeros((n_items, h), dtype)
  if dtype == F64:
    gg = np.asarray(g, F64)[ok][:, None]
    np.add.at(Gu, u, -gg * D[ok])
    np.add.at(Gi, i, -gg * Pt[ok])
    np.add.at(Gi, j, gg * Pt[ok])
    return Gu / T, Gi / T, cu, ci
  g, D, Pt = np.asarray(g, F32), np.asarray(D, F32), np.asarray(Pt, F32)
  for t in np.nonzero(ok)[0]:                                  # ascending slots, the positive before the negative
    Gu[users[t]] = fma32(-g[t], D[t], Gu[users[t]])
    Gi[pos[t]] = fma32(-g[t], Pt[t], Gi[pos[t]])
    Gi[neg[t]] = fma32(g[t], Pt[t], Gi[neg[t]])
  s = F32(1.0 / T)
  return s * Gu, s * Gi, cu, ci


def adam(e, H, count, reg_scale, m, v, lr, t, dtype=F64):
  """(e, m, v) after Adam step t >= 1 with grad = H + reg_scale count e."""
  if dtype == F64:
    e, H, m, v = (np.asarray(a, F64) for a in (e, H, m, v))
    grad = H + reg_scale * count[:, None] * e
    m = BETA1 * m + (1 - BETA1) * grad
    v = BETA2 * v + (1 - BETA2) * grad * grad
    den = np.sqrt(v) / np.sqrt(1 - BETA2 ** t) + EPS
    return e - (lr / (1 - BETA1 ** t)) * m / den, m, v
  e, H, m, v = (np.asarray(a, F32) for a in (e, H, m, v))
  b1, b2, eps, lr, reg_scale = F32(BETA1), F32(BETA2), F32(EPS), F32(lr), F32(reg_scale)
  step = F32(F64(lr) / (1.0 - F64(b1) ** t))
  isb2 = F32(1.0 / np.sqrt(1.0 - F64(b2) ** t))
  grad = fma32((reg_scale * count.astype(F32))[:, None], e, H)
  m = fma32(b1, m, (F32(1) - b1) * grad)
  v = fma32(b2, v, ((F32(1) - b2) * grad) * grad)
  den = fma32(np.sqrt(v), isb2, eps)
  return fma32(-step, m / den, e), m, v


def new_state(Eu, Ei, dtype=F64):
  E = (np.array(Eu, dtype), np.array(Ei, dtype))
  return {"E0": E, "M": tuple(np.zeros_like(a) for a in E), "V": tuple(np.zeros_like(a) for a in E), "step": 0}


def loss(m, Eu, Ei, K, users, pos, neg, reg):
  """The step's float64 objective: mean softplus(-x) over the T slots (invalid ones add nothing) plus the paper's
  L2 term (reg / 2) (|e0_u|^2 + |e0_i|^2 + |e0_j|^2) / T over the valid triples."""
  Eu, Ei = np.asarray(Eu, F64), np.asarray(Ei, F64)
  P, Q = forward(m, Eu, Ei, K)
  ok = neg >= 0
  u, i, j = users[ok], pos[ok], neg[ok]
  x = (P[u] * (Q[i] - Q[j])).sum(1)
  l2 = (Eu[u] ** 2).sum() + (Ei[i] ** 2).sum() + (Ei[j] ** 2).sum()
  return (np.logaddexp(0.0, -x).sum() + 0.5 * reg * l2) / len(users)


def gradient(m, Eu, Ei, K, users, pos, neg, reg, dtype=F64):
  """(dL/dE0 users, dL/dE0 items, H users, H items, counts, summed softplus): steps 1-5 of one step."""
  T = len(users)
  P, Q = forward(m, Eu, Ei, K, dtype)
  _, g, ls, D, Pt = bpr_util.grad(users, pos, neg, P, Q, np.zeros(Q.shape[0], dtype), dtype)
  Gu, Gi, cu, ci = scatter(users, pos, neg, g, D, Pt, P.shape[0], Q.shape[0], dtype)
  Hu, Hi = forward(m, Gu, Gi, K, dtype)
  rs = reg / T
  return (Hu + rs * cu[:, None] * np.asarray(Eu, F64), Hi + rs * ci[:, None] * np.asarray(Ei, F64), Hu, Hi, cu, ci,
          float(ls.sum(dtype=F64)))


def adam_both(state, Hu, Hi, cu, ci, T, lr, reg, dtype=F64):
  """Adam on both sides of ``state`` in place, at reg / T in ``dtype``: the tail of every step of this family."""
  state["step"] += 1
  rs = F32(reg / T) if dtype == F32 else reg / T
  out = [adam(state["E0"][s], H, c, rs, state["M"][s], state["V"][s], lr, state["step"], dtype)
         for s, (H, c) in enumerate(((Hu, cu), (Hi, ci)))]
  state["E0"], state["M"], state["V"] = (tuple(o[k] for o in out) for k in range(3))


def step(m, state, K, users, pos, neg, lr, reg, dtype=F64):
  """One step on given triples, on ``state`` in place: (summed loss, valid triples)."""
  _, _, Hu, Hi, cu, ci, ls = gradient(m, *state["E0"], K, users, pos, neg, reg, dtype)
  adam_both(state, Hu, Hi, cu, ci, len(users), lr, reg, dtype)
  return ls, int((neg >= 0).sum())


def epochs(m, state, num_epochs, batch_size, seed, on_epoch, step_fn, zero, entry):
  """The history of ``num_epochs`` epochs on ``state`` in place, on the triples the kernel's sampler draws.
  ``step_fn(users, pos, neg, step_index)`` takes one step and returns what it adds to the epoch's sums (an array
  like ``zero``); ``entry(sums, steps)`` is an epoch's history entry; ``on_epoch(epoch, state)`` follows it."""
  m = sp.csr_matrix(m)
  sampler = bpr_util.Sampler(m)
  steps = -(-m.nnz // batch_size)
  hist = []
  for ep in range(num_epochs):
    sums = zero
    for _ in range(steps):
      s = state["step"]
      sums = sums + np.asarray(step_fn(*sampler.sample(seed, s, batch_size), s))
    hist.append(entry(sums, steps))
    if on_epoch is not None:
      on_epoch(ep + 1, state)
  return hist


def mean_loss(sums, steps=None):
  return float(sums[0] / sums[1]) if sums[1] else float("nan")


def fit(m, Eu, Ei, K, num_epochs, batch_size, lr, reg, seed=0, dtype=F64, state=None, on_epoch=None):
  """(P, Q, state, history): recoder_amd.lightgcn.fit restated, on the triples the kernel's sampler draws.
  ``state`` continues an earlier fit; ``on_epoch(epoch, state)`` is called after every epoch."""
  state = new_state(Eu, Ei, dtype) if state is None else state
  hist = epochs(m, state, num_epochs, batch_size, seed, on_epoch,
                lambda users, pos, neg, s: step(m, state, K, users, pos, neg, lr, reg, dtype), np.zeros(2), mean_loss)
  return forward(m, *state["E0"], K, dtype) + (state, hist)


def quality(P, Q, x, y):
  """(Recall@20, NDCG@100) of the tables on (x: train, y: held out)."""
  from tests import rp3_util
  lists = []
  for b0 in range(0, x.shape[0], 1000):
    lists.append(rp3_util.top_k(np.asarray(P[b0:b0 + 1000], F64) @ np.asarray(Q, F64).T, x[b0:b0 + 1000], 100))
  return rp3_util.metric_means(np.concatenate(lists), y)
