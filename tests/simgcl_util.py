"""Numpy restatement of SimGCL training (recoder_amd/simgcl.py, the rk_als_gcl_* part of include/recoder_als.h) on
tests/lightgcn_util.py and the sampler of tests/bpr_util.py: the noise bit for bit with numpy integers, the views,
the contrast with its analytic gradient, ``step``, ``fit`` and ``quality`` -- in float64 (the model, pinned against
torch autograd in tests/test_simgcl_host.py), or in float32 in the kernels' operation order where that is cheap
to state (the propagation chains, the noise; the contrast's sums are numpy's), for the measurement of what f32
costs."""
import numpy as np
import scipy.sparse as sp

from tests import bpr_util, lightgcn_util as lg
from tests.bpr_util import _U, mix
from tests.lightgcn_util import F32, F64

TAG = 0x80000000          # bit 31 of the key's low word: a sampler slot is below 2^24


# -------------------------------------------------------------------- noise
def noise_key(seed, step, view, layer, side):
  """The uint64 key of one propagation's noise."""
  assert step >= 0 and 0 <= view <= 255 and 0 <= layer <= 255 and side in (0, 1)
  seed_key = mix(np.array([int(seed) % 2 ** 64], dtype=_U))[0]
  packed = _U((int(step) << 32) | TAG | (view << 16) | (layer << 8) | side)
  return mix(np.array([seed_key ^ packed], dtype=_U))[0]


def noise_m(key, rows, h):
  """m [len(rows), h] (uint64): the odd 24-bit integers with u = m 2^-24."""
  with np.errstate(over="ignore"):
    row_key = mix(_U(key) + np.asarray(rows, dtype=_U))
    r = mix(row_key[:, None] + np.arange(h, dtype=_U)[None, :])
  return ((r >> _U(41)) << _U(1)) | _U(1)


def perturb(x, eps, key, dtype=F64, rows=None):
  """x + eps sign(x) u / |u|_2 per row; ``rows``: the rows' indices in their table (None: 0, 1, ...).  float32: the
  kernel's operations -- the integer sum of m^2 rounded once, 2^-48, a square root, eps divided by it, one
  fmaf."""
  x = np.asarray(x, dtype)
  rows = np.arange(x.shape[0]) if rows is None else rows
  m = noise_m(key, rows, x.shape[1])
  ss = (m * m).sum(1)                                          # (below 2^57: exact)
  if dtype == F64:
    d = eps * (m.astype(F64) * 2.0 ** -24) / (np.sqrt(ss.astype(F64)) * 2.0 ** -24)[:, None]
    return x + np.sign(x) * d
  nscale = (F32(eps) / np.sqrt(ss.astype(F32) * F32(2.0 ** -48)))[:, None]
  u = m.astype(F32) * F32(2.0 ** -24)
  return np.where(x > 0, lg.fma32(nscale, u, x), np.where(x < 0, lg.fma32(-nscale, u, x), x)).astype(F32)


def propagate(m, rs, cs, F, eps, key, dtype=F64, acc=None, acc_scale=1.0):
  """``lg.propagate`` with the noise added to out before acc takes it."""
  out, _ = lg.propagate(m, rs, cs, F, dtype)
  out = perturb(out, eps, key, dtype)
  if acc is not None:
    acc = ((np.asarray(acc, dtype) + out) * dtype(acc_scale)).astype(dtype)
  return out, acc


def forward(m, Eu, Ei, K, dtype=F64, eps=None, seed=0, step=0, view=0):
  """(P, Q): the mean over the layers 1..K; ``eps`` None: the clean tables, else view ``view`` of step ``step``."""
  m, mt = sp.csr_matrix(m), lg.transpose(m)
  su, si = lg.scales(m)
  Pk, Qk = np.asarray(Eu, dtype), np.asarray(Ei, dtype)
  P, Q = np.zeros_like(Pk), np.zeros_like(Qk)
  for k in range(K):
    scale = (F32(1.0 / K) if dtype == F32 else 1.0 / K) if k == K - 1 else 1.0
    if eps is None:
      (Pk, P), (Qk, Q) = lg.propagate(m, su, si, Qk, dtype, P, scale), lg.propagate(mt, si, su, Pk, dtype, Q, scale)
    else:
      (Pk, P), (Qk, Q) = (propagate(m, su, si, Qk, eps, noise_key(seed, step, view, k + 1, 0), dtype, P, scale),
                          propagate(mt, si, su, Pk, eps, noise_key(seed, step, view, k + 1, 1), dtype, Q, scale))
  return P, Q


# ----------------------------------------------------------------- contrast
def active(keys, n_rows):
  """The sorted keys and the mask of the active slots: inside the table and unlike the key before."""
  keys = np.sort(np.asarray(keys).astype(np.int64))
  return keys, (keys >= 0) & (keys < n_rows) & np.concatenate([[True], keys[1:] != keys[:-1]])


def contrast(keys, V1, V2, tau, dtype=F64):
  """(NCE, m, dNCE / dV1, dNCE / dV2) over the distinct keys inside the tables; a row with |v| = 0 normalises to 0
  and takes the gradient 0."""
  V1, V2 = np.asarray(V1, dtype), np.asarray(V2, dtype)
  keys, act = active(keys, V1.shape[0])
  idx = keys[act]
  m = len(idx)
  G1, G2 = np.zeros_like(V1), np.zeros_like(V2)
  if m == 0:
    return 0.0, 0, G1, G2
  tau = dtype(tau)
  z, inv = [], []
  for v in (V1[idx], V2[idx]):
    n = np.sqrt((v * v).sum(1, dtype=dtype))
    i = np.where(n > 0, 1 / np.where(n > 0, n, 1), 0).astype(dtype)
    inv.append(i[:, None])
    z.append(v * i[:, None])
  S = (z[0] @ z[1].T) / tau
  mx = S.max(1)
  lse = mx + np.log(np.exp(S - mx[:, None]).sum(1, dtype=dtype))
  loss = float((lse - np.diag(S)).sum(dtype=F64) / m)
  P = np.exp(S - lse[:, None])
  c = dtype(1) / (tau * dtype(m))
  dz = ((P @ z[1] - z[1]) * c, (P.T @ z[0] - z[0]) * c)
  for G, zz, d, i in zip((G1, G2), z, dz, inv):
    G[idx] = (d - zz * (zz * d).sum(1, dtype=dtype)[:, None]) * i
  return loss, m, G1, G2


# --------------------------------------------------------------------- step
def gradient(m, Eu, Ei, K, users, pos, neg, reg, cl_weight, cl_eps, tau, seed=0, step_index=0, dtype=F64):
  """(dL/dE0 users, dL/dE0 items, H users, H items, counts users, counts items, summed softplus, NCE_users +
  NCE_items): everything of one step before Adam."""
  T = len(users)
  n_users, n_items = np.asarray(Eu).shape[0], np.asarray(Ei).shape[0]
  P, Q = forward(m, Eu, Ei, K, dtype)
  _, g, ls, D, Pt = bpr_util.grad(users, pos, neg, P, Q, np.zeros(n_items, dtype), dtype)
  Gu, Gi, cu, ci = lg.scatter(users, pos, neg, g, D, Pt, n_users, n_items, dtype)
  cl = 0.0
  if cl_weight > 0:
    views = [forward(m, Eu, Ei, K, dtype, cl_eps, seed, step_index, a) for a in (1, 2)]
    ok = neg >= 0
    w = dtype(cl_weight)
    lu, _, a1, a2 = contrast(np.where(ok, users, n_users), views[0][0], views[1][0], tau, dtype)
    li, _, b1, b2 = contrast(np.where(ok, pos, n_items), views[0][1], views[1][1], tau, dtype)
    Gu, Gi = (Gu + w * a1) + w * a2, (Gi + w * b1) + w * b2
    cl = lu + li
  Hu, Hi = forward(m, Gu, Gi, K, dtype)
  rs = reg / T
  return (Hu + rs * cu[:, None] * np.asarray(Eu, F64), Hi + rs * ci[:, None] * np.asarray(Ei, F64), Hu, Hi, cu, ci,
          float(ls.sum(dtype=F64)), cl)


def step(m, state, K, users, pos, neg, lr, reg, cl_weight, cl_eps, tau, seed=0, step_index=0, dtype=F64):
  """One step on given triples, on ``state`` in place: (summed softplus, valid triples, NCE_users + NCE_items)."""
  _, _, Hu, Hi, cu, ci, ls, cl = gradient(m, *state["E0"], K, users, pos, neg, reg, cl_weight, cl_eps, tau, seed,
                                          step_index, dtype)
  lg.adam_both(state, Hu, Hi, cu, ci, len(users), lr, reg, dtype)
  return ls, int((neg >= 0).sum()), cl


def fit(m, Eu, Ei, K, num_epochs, batch_size, lr, reg, cl_weight, cl_eps, tau, seed=0, dtype=F64, state=None,
        on_epoch=None):
  """(P, Q, state, history): recoder_amd.simgcl.fit restated, on the triples the kernel's sampler draws."""
  state = lg.new_state(Eu, Ei, dtype) if state is None else state
  hist = lg.epochs(m, state, num_epochs, batch_size, seed, on_epoch,
                   lambda users, pos, neg, s: step(m, state, K, users, pos, neg, lr, reg, cl_weight, cl_eps, tau, seed,
                                                   s, dtype),
                   np.zeros(3), lambda sums, steps: (lg.mean_loss(sums), float(sums[2] / steps)))
  return forward(m, *state["E0"], K, dtype) + (state, hist)


quality = lg.quality


# ------------------------------------------------------------------- bounds
U24 = 2.0 ** -24


def prop_bound(m, rs, cs, F):
  """tests/test_lightgcn.py's bound of one propagation: (L + 3) 2^-24 rs sum |cs F| per element."""
  mag, _ = lg.propagate(m, rs, cs, np.abs(F))
  return (np.diff(sp.csr_matrix(m).indptr)[:, None] + 3) * U24 * mag


def noisy_errors(got, m, rs, cs, F, eps, key):
  """(err / (2 x bound) per element, the mask of the elements whose sign is ambiguous) of a float32 noisy
  propagation ``got`` against float64.  The bound is the propagation's own B plus the noise chain's roundings -- h
  products under the norm, a division and a product on the noise d, then the sum's on |x| + |d| -- times 2^-24,
  and the whole doubled as the propagation's test does.  Where |x| <= 2 B the f32 row may carry either sign, or be
  exactly 0 and take no noise: such an element is compared against the nearest of x + d, x - d and x."""
  x, _ = lg.propagate(m, rs, cs, F)
  h = x.shape[1]
  d = np.abs(perturb(np.ones_like(x), eps, key) - 1.0)
  B = prop_bound(m, rs, cs, F)
  bound = 2 * (B + ((h + 2) * d + np.abs(x) + d) * U24)
  amb = (np.abs(x) <= 2 * B) & (B > 0)
  err = np.abs(got - (x + np.sign(x) * d))
  alt = np.minimum(np.minimum(np.abs(got - (x + d)), np.abs(got - (x - d))), np.abs(got - x))
  err = np.where(amb, np.minimum(err, alt), err)
  return err / np.maximum(bound, 1e-300), amb
