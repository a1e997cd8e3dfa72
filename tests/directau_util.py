"""Numpy restatement of DirectAU training (recoder_amd/directau.py, rk_als_dau_grad of include/recoder_als.h) on
tests/lightgcn_util.py and the sampler of tests/bpr_util.py: the loss, its analytic gradient per slot, ``step``,
``fit`` and ``quality`` -- in float64 (the model, pinned against torch autograd in tests/test_directau_host.py), or
in float32 (the propagation chains and Adam in the kernels' operation order as lightgcn_util states them; the sums
of the loss are numpy's), for the measurement of what f32 costs."""
import numpy as np

from tests import lightgcn_util as lg
from tests.lightgcn_util import F32, F64


def valid_slots(users, items, n_users, n_items):
  users, items = np.asarray(users).astype(np.int64), np.asarray(items).astype(np.int64)
  return (users >= 0) & (users < n_users) & (items >= 0) & (items < n_items)


def normalise(V, dtype=F64):
  """(z, 1 / |v|) per row; a row of norm 0 gives z = 0 and 1 / |v| = 0."""
  V = np.asarray(V, dtype)
  n = np.sqrt((V * V).sum(1, dtype=dtype))
  inv = np.where(n > 0, 1 / np.where(n > 0, n, 1), 0).astype(dtype)[:, None]
  return V * inv, inv


def weights(z):
  """E^ [m, m]: exp(-2 |z_p - z_q|^2) with a zero diagonal; the squared distance is |z_p|^2 + |z_q|^2 - 2 z_p . z_q
  from the rows as they are (a zero row lies at distance 1 from a unit row)."""
  n = (z * z).sum(1, dtype=z.dtype)
  E = np.exp(-2 * np.maximum(n[:, None] + n[None, :] - 2 * (z @ z.T), 0)).astype(z.dtype)
  np.fill_diagonal(E, 0)
  return E


def uniformity(z, gamma):
  """(unif(z), d ((gamma / 2) unif) / dz); 0 and zeros for fewer than two rows."""
  m = len(z)
  if m < 2:
    return 0.0, np.zeros_like(z)
  E = weights(z)
  r = E.sum(1, dtype=z.dtype)
  S = r.sum(dtype=z.dtype)                                     # (= 2 sum_{p < q} e_pq)
  c = z.dtype.type(4 * gamma) / S
  return float(np.log(F64(S) / (m * (m - 1.0)))), -c * (r[:, None] * z - E @ z)


def grad_rows(users, items, X, Y, gamma, dtype=F64):
  """((align, unif_users, unif_items), m, valid [T], DU [T, h], DI [T, h]): what rk_als_dau_grad leaves."""
  X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
  T, h = len(users), X.shape[1]
  ok = valid_slots(users, items, X.shape[0], Y.shape[0])
  m = int(ok.sum())
  DU, DI = np.zeros((T, h), dtype), np.zeros((T, h), dtype)
  if m == 0:
    return (0.0, 0.0, 0.0), 0, ok.astype(dtype), DU, DI
  (a, ia), (b, ib) = normalise(X[np.asarray(users)[ok]], dtype), normalise(Y[np.asarray(items)[ok]], dtype)
  d = a - b
  align = float((d * d).sum(dtype=F64) / m)
  (ua, dza), (ub, dzb) = uniformity(a, gamma), uniformity(b, gamma)
  dza, dzb = dza + (dtype(2) / dtype(m)) * d, dzb - (dtype(2) / dtype(m)) * d
  DU[ok] = (dza - a * (a * dza).sum(1, dtype=dtype)[:, None]) * ia
  DI[ok] = (dzb - b * (b * dzb).sum(1, dtype=dtype)[:, None]) * ib
  return (align, ua, ub), m, ok.astype(dtype), DU, DI


def dense_loss(users, items, X, Y, gamma):
  """align + (gamma / 2) (unif_users + unif_items) in float64 from the differences of the rows (no Gram matrix)."""
  X, Y = np.asarray(X, F64), np.asarray(Y, F64)
  ok = valid_slots(users, items, X.shape[0], Y.shape[0])
  m = int(ok.sum())
  if m == 0:
    return 0.0
  a, b = normalise(X[np.asarray(users)[ok]])[0], normalise(Y[np.asarray(items)[ok]])[0]
  total = ((a - b) ** 2).sum() / m
  if m >= 2:
    p, q = np.triu_indices(m, 1)
    for z in (a, b):
      total += 0.5 * gamma * np.log(np.exp(-2 * ((z[p] - z[q]) ** 2).sum(1)).mean())
  return float(total)


# --------------------------------------------------------------------- step
def scatter(users, items, valid, DU, DI, n_users, n_items):
  """(Gu, Gi, cu, ci): the rows summed per key in ascending slot order, and the counts."""
  ok = valid > 0
  u, i = np.asarray(users)[ok].astype(np.int64), np.asarray(items)[ok].astype(np.int64)
  Gu, Gi = np.zeros((n_users, DU.shape[1]), DU.dtype), np.zeros((n_items, DI.shape[1]), DI.dtype)
  np.add.at(Gu, u, DU[ok])
  np.add.at(Gi, i, DI[ok])
  return Gu, Gi, np.bincount(u, minlength=n_users).astype(np.int32), np.bincount(i, minlength=n_items).astype(np.int32)


def gradient(m, Eu, Ei, K, users, items, reg, gamma, dtype=F64):
  """(dL/dE0 users, dL/dE0 items, H users, H items, counts users, counts items, the three losses, valid slots):
  everything of one step before Adam."""
  T = len(users)
  P, Q = lg.forward(m, Eu, Ei, K, dtype)
  losses, cnt, valid, DU, DI = grad_rows(users, items, P, Q, gamma, dtype)
  Gu, Gi, cu, ci = scatter(users, items, valid, DU, DI, P.shape[0], Q.shape[0])
  Hu, Hi = lg.forward(m, Gu, Gi, K, dtype)
  rs = reg / T
  return (Hu + rs * cu[:, None] * np.asarray(Eu, F64), Hi + rs * ci[:, None] * np.asarray(Ei, F64), Hu, Hi, cu, ci,
          losses, cnt)


def step(m, state, K, users, items, lr, reg, gamma, dtype=F64):
  """One step on given slots, on ``state`` in place: ((align, unif_users, unif_items), valid slots)."""
  _, _, Hu, Hi, cu, ci, losses, cnt = gradient(m, *state["E0"], K, users, items, reg, gamma, dtype)
  lg.adam_both(state, Hu, Hi, cu, ci, len(users), lr, reg, dtype)
  return losses, cnt


def fit(m, Eu, Ei, K, num_epochs, batch_size, lr, reg, gamma, seed=0, dtype=F64, state=None, on_epoch=None):
  """(P, Q, state, history): recoder_amd.directau.fit restated, on the slots the kernel's sampler draws."""
  state = lg.new_state(Eu, Ei, dtype) if state is None else state
  hist = lg.epochs(m, state, num_epochs, batch_size, seed, on_epoch,
                   lambda users, pos, neg, s: step(m, state, K, users, pos, lr, reg, gamma, dtype)[0], np.zeros(3),
                   lambda sums, steps: tuple(sums / steps))
  return lg.forward(m, *state["E0"], K, dtype) + (state, hist)


quality = lg.quality
