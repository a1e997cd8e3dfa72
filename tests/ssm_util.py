"""Numpy restatement of sampled-softmax training (recoder_amd/ssm.py, rk_als_ssm_grad of include/recoder_als.h) on
tests/lightgcn_util.py and the sampler of tests/bpr_util.py: the shared draws bit for bit with numpy integers, the
correction, the loss, its analytic gradient per slot and per column, ``step``, ``fit`` and ``quality`` -- in float64
(the model, pinned against torch autograd in tests/test_ssm_host.py), or in float32 (the propagation chains and Adam
in the kernels' operation order as lightgcn_util states them; the sums of the loss are numpy's), for the
measurement of what f32 costs."""
import numpy as np
import scipy.sparse as sp

from tests import bpr_util, lightgcn_util as lg
from tests.bpr_util import _U, mix
from tests.directau_util import normalise, valid_slots
from tests.lightgcn_util import F32, F64

TAG = 0xC0000000                                               # the domain of the shared draws in the key's low word


def shared_draws(seed, step, S, n_items):
  """The S shared negatives of step ``step`` under ``seed``: int32 [S], each in [0, n_items)."""
  seed_key = mix(np.array([int(seed) % 2 ** 64], dtype=_U))[0]
  packed = (_U(int(step)) << _U(32)) | _U(TAG) | np.arange(S, dtype=_U)
  return bpr_util.draw(mix(seed_key ^ packed), 0, n_items).astype(np.int32)


def candidates(items, seed, step, S, n_items):
  """The C = T + S columns' items: the slots' positives as they are, then the shared draws."""
  return np.concatenate([np.asarray(items, np.int32), shared_draws(seed, step, S, n_items)])


def correction(m, T, S, logq_weight):
  """corr [n_items] f32: logq_weight log((T d_j / nnz + S / n_items) / (T + S)) in float64, rounded once; 0 for an
  item that can hold no column."""
  m = sp.csr_matrix(m)
  d = np.bincount(m.indices, minlength=m.shape[1]).astype(F64)
  q = (T * d / max(float(m.nnz), 1.0) + S / float(m.shape[1])) / (T + S)
  return (float(logq_weight) * np.log(np.where(q > 0, q, 1.0))).astype(F32)


def inverse_temperature(temperature):
  """1 / temperature as rk_als_ssm_grad takes it: the float64 quotient rounded once to f32."""
  return float(F32(1.0 / float(temperature)))


def live_mask(users, items, cand, n_users, n_items):
  """(valid [T], cvalid [C], live [T, C]): entry (t, c) enters row t's sum."""
  T = len(users)
  ok = valid_slots(users, items, n_users, n_items)
  cvalid = np.concatenate([ok, np.ones(len(cand) - T, bool)])
  c = np.arange(len(cand))
  dup = (np.asarray(cand)[None, :] == np.asarray(items)[:, None]) & (c[None, :] != np.arange(T)[:, None])
  return ok, cvalid, ok[:, None] & cvalid[None, :] & ~dup


def grad_rows(users, items, cand, X, Y, temperature, cosine=True, corr=None, dtype=F64):
  """((loss, probability of the positive), m, valid [T], cvalid [C], DU [T, h], DC [C, h]): what rk_als_ssm_grad
  leaves for the columns ``cand``."""
  X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
  users, items, cand = (np.asarray(a).astype(np.int64) for a in (users, items, cand))
  T, C, h = len(users), len(cand), X.shape[1]
  ok, cvalid, live = live_mask(users, items, cand, X.shape[0], Y.shape[0])
  m = int(ok.sum())
  DU, DC = np.zeros((T, h), dtype), np.zeros((C, h), dtype)
  if m == 0:
    return (0.0, 0.0), 0, ok.astype(dtype), cvalid.astype(dtype), DU, DC
  A, B = np.zeros((T, h), dtype), np.zeros((C, h), dtype)
  A[ok], B[cvalid] = X[users[ok]], Y[cand[cvalid]]
  if cosine:
    (zu, iu), (zc, ic) = normalise(A, dtype), normalise(B, dtype)
  else:
    zu, zc, iu, ic = A, B, np.ones((T, 1), dtype), np.ones((C, 1), dtype)
  inv_tau = dtype(inverse_temperature(temperature))
  s = (zu @ zc.T) * inv_tau
  if corr is not None:
    cc = np.zeros(C, dtype)
    cc[cvalid] = np.asarray(corr, dtype)[cand[cvalid]]
    s = s - cc[None, :]
  s = np.where(live, s, -np.inf).astype(dtype)
  rows = np.nonzero(ok)[0]
  mx = s[rows].max(1, keepdims=True)
  e = np.exp(s[rows] - mx)
  tot = e.sum(1, dtype=dtype)[:, None]
  lse = mx[:, 0] + np.log(tot[:, 0])
  stt = s[rows, rows]
  W = np.zeros((T, C), dtype)
  W[rows] = e / tot
  W[rows, rows] -= 1
  W /= dtype(m)
  loss = float((lse - stt).astype(F64).sum() / m)
  prob = float(np.exp(stt - lse).astype(F64).sum() / m)
  dzu, dzc = (W @ zc) * inv_tau, (W.T @ zu) * inv_tau
  if cosine:
    DU = (dzu - zu * (zu * dzu).sum(1, dtype=dtype)[:, None]) * iu
    DC = (dzc - zc * (zc * dzc).sum(1, dtype=dtype)[:, None]) * ic
  else:
    DU, DC = dzu, dzc
  DU[~ok], DC[~cvalid] = 0, 0
  return (loss, prob), m, ok.astype(dtype), cvalid.astype(dtype), DU.astype(dtype), DC.astype(dtype)


def dense_loss(users, items, cand, X, Y, temperature, cosine=True, corr=None):
  """The softmax loss in float64 written row by row (no matrices)."""
  X, Y = np.asarray(X, F64), np.asarray(Y, F64)
  ok, cvalid, live = live_mask(users, items, cand, X.shape[0], Y.shape[0])
  unit = lambda v: v / np.linalg.norm(v) if cosine and np.linalg.norm(v) > 0 else v
  total = 0.0
  for t in np.nonzero(ok)[0]:
    a = unit(X[users[t]])
    s = {c: a @ unit(Y[cand[c]]) * inverse_temperature(temperature) - (corr[cand[c]] if corr is not None else 0.0)
         for c in np.nonzero(live[t])[0]}
    total += np.log(sum(np.exp(v) for v in s.values())) - s[t]
  return total / max(int(ok.sum()), 1)


# --------------------------------------------------------------------- step
def scatter(ids, valid, D, n_rows):
  """(G, count): the rows summed per key in ascending order, and the counts."""
  ok = np.asarray(valid) > 0
  k = np.asarray(ids)[ok].astype(np.int64)
  G = np.zeros((n_rows, D.shape[1]), D.dtype)
  np.add.at(G, k, D[ok])
  return G, np.bincount(k, minlength=n_rows).astype(np.int32)


def gradient(m, Eu, Ei, K, users, items, cand, reg, temperature, cosine=True, corr=None, dtype=F64):
  """(H users, H items, counts users, counts items, (loss, probability), valid slots): one step before Adam."""
  P, Q = lg.forward(m, Eu, Ei, K, dtype)
  losses, cnt, valid, cvalid, DU, DC = grad_rows(users, items, cand, P, Q, temperature, cosine, corr, dtype)
  Gu, cu = scatter(users, valid, DU, P.shape[0])
  Gi, ci = scatter(cand, cvalid, DC, Q.shape[0])
  Hu, Hi = lg.forward(m, Gu, Gi, K, dtype)
  return Hu, Hi, cu, ci, losses, cnt


def step(m, state, K, users, items, cand, lr, reg, temperature, cosine=True, corr=None, dtype=F64):
  """One step on given slots and columns, on ``state`` in place: ((loss, probability), valid slots)."""
  Hu, Hi, cu, ci, losses, cnt = gradient(m, *state["E0"], K, users, items, cand, reg, temperature, cosine, corr, dtype)
  lg.adam_both(state, Hu, Hi, cu, ci, len(users), lr, reg, dtype)
  return losses, cnt


def fit(m, Eu, Ei, K, num_epochs, batch_size, lr, reg, temperature, num_negatives, cosine=True, logq_weight=0.0, seed=0,
        dtype=F64, state=None, on_epoch=None):
  """(P, Q, state, history): recoder_amd.ssm.fit restated (normalize=False), on the slots the kernel's sampler draws
  and the shared draws of ``shared_draws``."""
  m = sp.csr_matrix(m)
  state = lg.new_state(Eu, Ei, dtype) if state is None else state
  corr = correction(m, batch_size, num_negatives, logq_weight) if logq_weight > 0 else None

  def one(users, pos, neg, s):
    cand = candidates(pos, seed, s, num_negatives, m.shape[1])
    return step(m, state, K, users, pos, cand, lr, reg, temperature, cosine, corr, dtype)[0]
  hist = lg.epochs(m, state, num_epochs, batch_size, seed, on_epoch, one, np.zeros(2),
                   lambda sums, steps: tuple(sums / steps))
  return lg.forward(m, *state["E0"], K, dtype) + (state, hist)


def unit_rows(V):
  return normalise(V)[0]


def recall_at(P, Q, train, held_out, k=20):
  """Mean over the users with held-out items of the share of them (at most k) among the top k unseen items."""
  train, held_out = sp.csr_matrix(train), sp.csr_matrix(held_out)
  S = np.asarray(P, F64) @ np.asarray(Q, F64).T
  S[train.nonzero()] = -np.inf
  top = np.argsort(-S, axis=1, kind="stable")[:, :k]
  out = []
  for u in range(S.shape[0]):
    t = held_out.indices[held_out.indptr[u]:held_out.indptr[u + 1]]
    if len(t):
      out.append(len(np.intersect1d(top[u], t)) / min(k, len(t)))
  return float(np.mean(out))


def popularity_recall(train, held_out, k=20):
  train = sp.csr_matrix(train)
  pop = np.bincount(train.indices, minlength=train.shape[1]).astype(F64)
  return recall_at(np.ones((train.shape[0], 1)), pop[:, None], train, held_out, k)


quality = lg.quality
