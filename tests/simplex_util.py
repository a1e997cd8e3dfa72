"""Numpy restatement of SimpleX training (recoder_amd/simplex.py, rk_als_sx_forward and rk_als_sx_backward of
include/recoder_als.h) on tests/ccl_util.py's loss, tests/lightgcn_util.py's Adam, the sampler of tests/bpr_util.py and
the per-slot draws of tests/ultragcn_util.py: in float64 (the model, pinned against torch autograd in
tests/test_simplex_host.py) and in float32 in the kernels' operation order -- the add chain of the pooling, the fmaf
chains of the two products, the chunked dW, every fmaf(a, b, c) as the float64 a * b + c rounded to f32 -- which the
kernels must reproduce bit for bit."""
import numpy as np
import scipy.sparse as sp

from tests import ccl_util as cu, lightgcn_util as lg
from tests.lightgcn_util import F32, F64, fma32
from tests.ultragcn_util import draws  # noqa: F401  (the negatives are UltraGCN's draws)

CHUNK = 256


def history_positions(r, L):
  """floor(j r / L), j < L, for r > L, else 0 .. r - 1: python integers, no width to overflow."""
  r, L = int(r), int(L)
  return np.array([j if r <= L else j * r // L for j in range(min(r, L))], dtype=np.int64)


def histories(m, users, L):
  """The item ids (int64 arrays) of H_u for the slots ``users``; an empty array for a user outside the matrix."""
  m = sp.csr_matrix(m)
  out = []
  for u in np.asarray(users).astype(np.int64):
    if not 0 <= u < m.shape[0]:
      out.append(np.zeros(0, np.int64))
      continue
    row = m.indices[m.indptr[u]:m.indptr[u + 1]].astype(np.int64)
    out.append(row[history_positions(len(row), L)])
  return out


def pool_matrix(m, users, L):
  """A [T, n_items] float64: A[t, k] = (multiplicity of k in H_{u_t}) / |H_{u_t}|, so that b = A Q."""
  hs = histories(m, users, L)
  rows = np.concatenate([np.full(len(x), t) for t, x in enumerate(hs)] + [np.zeros(0, np.int64)]).astype(np.int64)
  cols = np.concatenate(hs + [np.zeros(0, np.int64)])
  vals = np.concatenate([np.full(len(x), 1.0 / max(len(x), 1)) for x in hs] + [np.zeros(0)])
  return sp.csr_matrix((vals, (rows, cols)), shape=(len(hs), sp.csr_matrix(m).shape[1]))


def rows64(m, users, P, Q, W, gamma, L):
  """(B [T, h], X rows [T, h]) of the slots in float64; ``P`` None: the first term is 0."""
  Q, W = np.asarray(Q, F64), np.asarray(W, F64)
  users = np.asarray(users).astype(np.int64)
  B = np.asarray(pool_matrix(m, users, L) @ Q)
  X = (1.0 - gamma) * (B @ W.T)
  if P is not None:
    ok = (users >= 0) & (users < np.asarray(P).shape[0])
    X[ok] += gamma * np.asarray(P, F64)[users[ok]]
  return B, X


def tables64(m, P, Q, W, gamma, L):
  """The final tables (X of every user, Y = Q) in float64."""
  return rows64(m, np.arange(sp.csr_matrix(m).shape[0]), P, Q, W, gamma, L)[1], np.asarray(Q, F64)


# ------------------------------------------------------- the kernels' chains
def forward_f32(m, users, Q, P, W, gamma, L, E):
  """What rk_als_sx_forward leaves, bit for bit: (B [T, h], X rows [T, h], hkey int32 [T, E], hcoef f32 [T, E]).  The
  X row of a slot whose user lies outside the matrix is +0 (the compact form; the table form stores none)."""
  m = sp.csr_matrix(m)
  Q, W = np.asarray(Q, F32), np.asarray(W, F32)
  users = np.asarray(users).astype(np.int64)
  T, h, n_items = len(users), Q.shape[1], Q.shape[0]
  hs = histories(m, users, L)
  lens = np.array([len(x) for x in hs])
  acc = np.zeros((T, h), F32)
  for j in range(int(lens.max()) if T else 0):                 # entry j of every slot that has one: ascending chains
    rows = np.nonzero(lens > j)[0]
    acc[rows] = (acc[rows] + Q[[hs[t][j] for t in rows]]).astype(F32)
  with np.errstate(divide="ignore"):
    inv = np.where(lens > 0, F32(1) / lens.astype(F32), F32(0)).astype(F32)
  B = (acc * inv[:, None]).astype(F32)
  s = np.zeros((T, h), F32)
  for c in range(h):                                           # s_a = fmaf(W[a, c], b_c, s_a), c ascending
    s = fma32(W[None, :, c], B[:, c, None], s)
  g = F32(gamma)
  ok = (users >= 0) & (users < m.shape[0])
  p = np.zeros((T, h), F32)
  if P is not None:
    p[ok] = np.asarray(P, F32)[users[ok]]
  X = np.where(ok[:, None], fma32(g, p, ((F32(1) - g) * s).astype(F32)), F32(0)).astype(F32)
  hkey, hcoef = np.full((T, E), n_items, np.int32), np.zeros((T, E), F32)
  for t, x in enumerate(hs):
    n = min(len(x), E)
    hkey[t, :n], hcoef[t, :n] = x[:n], inv[t]
  return B, X, hkey, hcoef


def backward_f32(DU, valid, B, W, scale):
  """What rk_als_sx_backward leaves, bit for bit: (dB [T, h], dW [h, h])."""
  DU, B, W = np.asarray(DU, F32), np.asarray(B, F32), np.asarray(W, F32)
  T, h = DU.shape
  live = np.asarray(valid) > 0
  D = np.where(live[:, None], DU, F32(0)).astype(F32)
  scale = F32(scale)
  acc = np.zeros((T, h), F32)
  for a in range(h):                                           # dB_c = fmaf(W[a, c], DU_a, dB_c), a ascending
    acc = fma32(W[a][None, :], D[:, a, None], acc)
  dB = np.where(live[:, None], (scale * acc).astype(F32), F32(0)).astype(F32)
  total = None
  for lo in range(0, T, CHUNK):                                # the chunks' chains, then the chunks in ascending order
    part = np.zeros((h, h), F32)
    for t in range(lo, min(T, lo + CHUNK)):
      part = fma32(D[t][:, None], B[t][None, :], part)
    total = part if total is None else (total + part).astype(F32)
  return dB, (scale * total).astype(F32)


# --------------------------------------------------------------------- step
def new_state(P, Q, dtype=F64):
  E = (np.array(P, dtype), np.array(Q, dtype), np.eye(np.asarray(P).shape[1], dtype=dtype))
  return {"E0": E, "M": tuple(np.zeros_like(a) for a in E), "V": tuple(np.zeros_like(a) for a in E), "step": 0}


def gradient(m, P, Q, W, gamma, L, users, items, negs, margin, negative_weight, dtype=F64):
  """((dP, dQ, dW), (counts users, counts items), (positive, negatives) summed over the slots, valid slots, live
  negatives): the gradient of (1 / T) sum_valid L_t at X = gamma P + (1 - gamma) W b, Y = Q, before the L2 term.
  float32: every stage in the kernels' order (the users' rows summed in ascending slots)."""
  m = sp.csr_matrix(m)
  users = np.asarray(users).astype(np.int64)
  T, (n_users, h), n_items = len(users), np.asarray(P).shape, np.asarray(Q).shape[0]
  okv = (users >= 0) & (users < n_users)
  slot = np.where(okv, np.arange(T), -1)                       # the loss reads the slots' own rows: X = Xs, user = t
  if dtype == F64:
    P, Q, W = (np.asarray(a, F64) for a in (P, Q, W))
    A = pool_matrix(m, users, L)
    B, Xs = rows64(m, users, P, Q, W, gamma, L)
    r = cu.grad_rows(slot, items, negs, Xs, Q, margin, negative_weight)
    DU = r["DU"]
    dBt = (1.0 - gamma) * (DU @ W) / T
    dW = (1.0 - gamma) * (DU.T @ B) / T
    dQ = r["DI"] / T + np.asarray(A.T @ dBt)
    ci = r["count"]
  else:
    P, Q, W = (np.asarray(a, F32) for a in (P, Q, W))
    E = max(2, max(len(x) for x in histories(m, users, L)))
    B, Xs, hkey, hcoef = forward_f32(m, users, Q, P, W, gamma, L, E)
    r = cu.grad_rows_f32(slot, items, negs, Xs, Q, margin, negative_weight)
    DU = r["DU"]
    DI, ci = cu.scatter_rows(r["key"], r["coef"], r["self"], slot, Xs, Q, n_items, F32)
    dBt, dW = backward_f32(DU, r["valid"], B, W, (1.0 - gamma) / T)
    G2, _ = cu.scatter_rows(hkey, hcoef, np.zeros_like(hcoef), np.arange(T), dBt, Q, n_items, F32)
    dQ = ((F32(1.0 / T) * DI).astype(F32) + G2).astype(F32)
  ok = r["valid"] > 0
  u = users[ok]
  dP = np.zeros((n_users, h), dtype)
  np.add.at(dP, u, DU[ok])
  dP = (dP * F32(gamma / T)).astype(F32) if dtype == F32 else dP * gamma / T
  cu_ = np.bincount(u, minlength=n_users).astype(np.int32)
  return (dP, dQ, dW), (cu_, ci), r["loss"].sum(0, dtype=F64), int(ok.sum()), int(r["live"].sum())


def step(m, state, gamma, L, users, items, negs, lr, reg, margin, negative_weight, dtype=F64):
  """One step on given slots and draws, on ``state`` in place: ((positive, negatives) summed, valid slots, live)."""
  grads, counts, loss, cnt, live = gradient(m, *state["E0"], gamma, L, users, items, negs, margin, negative_weight,
                                            dtype)
  state["step"] += 1
  T = len(users)
  rs = F32(reg / T) if dtype == F32 else reg / T
  h = grads[2].shape[0]
  if gamma == 1:                                               # (the pooling branch is skipped: W is untouched)
    grads, counts = grads[:2], counts
  out = [lg.adam(state["E0"][s], g, c, rs, state["M"][s], state["V"][s], lr, state["step"], dtype)
         for s, (g, c) in enumerate(zip(grads, tuple(counts) + (np.zeros(h, np.int32),)))]
  for k, name in enumerate(("E0", "M", "V")):
    state[name] = tuple(o[k] for o in out) + tuple(state[name][len(out):])
  return loss, cnt, live


def fit(m, P, Q, gamma, L, num_epochs, batch_size, lr, reg, num_negatives, negative_weight, margin, seed=0, state=None,
        on_epoch=None):
  """(X, Y, state, history, stats): recoder_amd.simplex.fit restated (normalize=False) in float64, on the slots the
  kernel's sampler draws and the negatives of ``draws``."""
  m = sp.csr_matrix(m)
  state = new_state(P, Q) if state is None else state

  def one(users, pos, neg, s):
    negs = draws(seed, s, len(users), num_negatives, m.shape[1])
    loss, cnt, live = step(m, state, gamma, L, users, pos, negs, lr, reg, margin, negative_weight)
    return np.concatenate([loss, [cnt, live]])
  full = lg.epochs(m, state, num_epochs, batch_size, seed, on_epoch, one, np.zeros(4),
                   lambda sums, steps: tuple(sums[[0, 1, 3]] / sums[2]) if sums[2] else (float("nan"),) * 3)
  return tables64(m, *state["E0"], gamma, L) + (state, [e[:2] for e in full], [e[2] / num_negatives for e in full])


quality = lg.quality


def fit_and_score(train, held_out, start, gamma, L, **kw):
  """(Recall@20, NDCG@100, history, stats) of the float64 fit from the tables ``start``, ranked by the dot product."""
  X, Y, _, hist, stats = fit(train, start[0], start[1], gamma, L, **kw)
  return quality(X, Y, train, held_out) + (hist, stats)
