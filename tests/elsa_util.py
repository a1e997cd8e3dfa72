"""Restatements of ELSA (Vancura, Alves, Kasalicky & Kordik, RecSys 2022), written from the published formulation:

    A_j = W_j / max(|W_j|, 1e-12),   P = X_b A A^T - X_b,   loss = mse_loss(normalize(P), normalize(X_b)),
    scores = X A A^T - X,            Adam (0.9 / 0.999 / 1e-8, bias-corrected, no weight decay) on W

``dense``: that formulation in torch ops with the gradient by autograd, in float64 or float32, on the CPU.
``gram``: the same loss and gradient from the h x h Gram S = A^T A without the B x n block, in float64 numpy.
The rest restates, operation by operation, what include/recoder_ease.h says of the ELSA kernels' roundings.
It is the comparator of the ELSA tests and never the code under test."""
import math

import numpy as np
import scipy.sparse as sp
import torch

from tests import ease_util

BETA1, BETA2, EPS, TINY = 0.9, 0.999, 1e-8, 1e-12


# ------------------------------------------------------------ the formulation
def unit_rows(W):
  W = np.asarray(W)
  return W / np.maximum(np.sqrt((W.astype(np.float64) ** 2).sum(1)), TINY)[:, None].astype(W.dtype)


def dense(Xb, W, dtype=torch.float64):
  """(loss, dW) of the published dense formulation: torch ops in ``dtype``, the gradient by autograd."""
  X = torch.as_tensor(np.asarray(sp.csr_matrix(Xb).todense()), dtype=dtype)
  Wt = torch.tensor(np.asarray(W), dtype=dtype, requires_grad=True)
  A = torch.nn.functional.normalize(Wt, dim=-1)
  P = (X @ A) @ A.t() - X
  loss = torch.nn.functional.mse_loss(torch.nn.functional.normalize(P, dim=-1), torch.nn.functional.normalize(X, dim=-1))
  loss.backward()
  return float(loss.detach()), Wt.grad.numpy()


def gram(Xb, W):
  """(loss, dW, parts) from the Gram form, float64 numpy; ``parts``: Z, Q, t2, p2, E, F, dA, A, the row losses."""
  X = sp.csr_matrix(Xb).astype(np.float64)
  W = np.asarray(W, np.float64)
  B, n = X.shape
  nrm = np.maximum(np.sqrt((W ** 2).sum(1)), TINY)
  A = W / nrm[:, None]
  S = A.T @ A
  Z = np.asarray(X @ A)
  Q = Z @ S
  t2 = np.asarray(X.multiply(X).sum(1)).ravel()
  E, F, row_loss, p2, _, _ = rows64(Z, Q, t2, n)
  dA = np.asarray(X.T @ E) + A @ (Z.T @ F)
  dW = (dA - (dA * A).sum(1)[:, None] * A) / nrm[:, None]
  return float(row_loss.sum() / (B * n)), dW, dict(Z=Z, Q=Q, t2=t2, p2=p2, E=E, F=F, dA=dA, A=A, row_loss=row_loss)


def rows64(Z, Q, t2, n, z2=None, q=None):
  """(E, F, row_loss, p2, ce, b) of the per-row formulas in float64 from Z, Q [B, h] and t2 [B], E = ce Z + b Q and
  F = b Z; ``z2`` = |Z_u|^2 and ``q`` = <Z_u, Q_u> may be given (summed in another order)."""
  Z, Q, t2 = (np.asarray(a, np.float64) for a in (Z, Q, t2))
  B = Z.shape[0]
  z2 = (Z * Z).sum(1) if z2 is None else z2
  q = (Z * Q).sum(1) if q is None else q
  p2 = q - 2.0 * z2 + t2
  live = (t2 > 0) & (p2 > 0)
  sp2, st2 = np.sqrt(np.where(live, p2, 1.0)), np.sqrt(np.where(live, t2, 1.0))
  c = np.where(live, (z2 - t2) / (sp2 * st2), 0.0)
  a = np.where(live, -2.0 / (B * n * sp2 * st2), 0.0)
  b = np.where(live, 2.0 * c / (B * n * np.where(live, p2, 1.0)), 0.0)
  ce = 2.0 * (a - b)
  E = ce[:, None] * Z + b[:, None] * Q
  F = b[:, None] * Z
  E[~live], F[~live] = 0.0, 0.0
  row_loss = np.where(live, 2.0 - 2.0 * c, np.where(t2 > 0, 1.0, 0.0))
  return E, F, row_loss, p2, ce, b


def adam(W, dW, m, v, t, lr, dtype=np.float64):
  """One step of torch.optim.Adam's arithmetic in ``dtype``; returns (W, m, v)."""
  W, dW, m, v = (np.asarray(a, dtype) for a in (W, dW, m, v))
  one = dtype(1.0)
  m = dtype(BETA1) * m + (one - dtype(BETA1)) * dW
  v = dtype(BETA2) * v + (one - dtype(BETA2)) * dW * dW
  step = dtype(lr / (1.0 - BETA1 ** t))
  denom = np.sqrt(v) / dtype(math.sqrt(1.0 - BETA2 ** t)) + dtype(EPS)
  return (W - step * m / denom).astype(dtype), m.astype(dtype), v.astype(dtype)


def initial_factors(n, h, seed):
  r = math.sqrt(6.0 / (n + h))
  return np.random.RandomState(seed).uniform(-r, r, (n, h)).astype(np.float32)


def epoch_order(n_users, seed, epoch):
  return np.random.RandomState(seed + 1 + epoch).permutation(n_users)


def fit(X, h, num_epochs, batch_size, lr, seed, form="gram", read_at=()):
  """(W, history, reads): the training loop with the seeded start and user orders; ``form`` "gram" (float64),
  "dense64" or "dense32" (the published formulation by autograd; float32 with float32 Adam).  ``reads[e]`` is a copy
  of W after e epochs for e in ``read_at``."""
  X = sp.csr_matrix(X)
  U, n = X.shape
  dt = np.float32 if form == "dense32" else np.float64
  W = initial_factors(n, h, seed).astype(dt)
  m, v = np.zeros_like(W), np.zeros_like(W)
  t, history, reads = 0, [], {}
  for epoch in range(num_epochs):
    Xp = X[epoch_order(U, seed, epoch)]
    total, steps = 0.0, 0
    for lo in range(0, U, batch_size):
      Xb = Xp[lo:lo + batch_size]
      if form == "gram":
        loss, dW, _ = gram(Xb, W)
      else:
        loss, dW = dense(Xb, W, torch.float32 if form == "dense32" else torch.float64)
      t += 1
      W, m, v = adam(W, dW, m, v, t, lr, dt)
      total, steps = total + loss, steps + 1
    history.append(total / max(steps, 1))
    if epoch + 1 in read_at:
      reads[epoch + 1] = W.copy()
  return W, history, reads


def scores(X, W):
  """X A A^T - X in float64, dense."""
  X = sp.csr_matrix(X).astype(np.float64)
  A = unit_rows(np.asarray(W, np.float64))
  return np.asarray(X @ A) @ A.T - np.asarray(X.todense())


def quality(X, Y, W):
  """[Recall@20, NDCG@100] of the model W on the held-out Y with the items of X masked (tests/gfcf_util.py)."""
  from tests import gfcf_util
  return gfcf_util.quality(X, Y, S=scores(X, W))


# ---------------------------------------------- the header's orders, restated
def row_dot64(x, y):
  """The header's "row dot" of the rows of x and y [rows, h], float64: lane l of 64 chains k = l, l + 64, ..
  ascending from 0 (the products of two f32 are exact in float64, so fma = multiply and add), then the butterfly
  s += s[lane ^ d] for d = 32 .. 1."""
  x, y = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
  rows, h = x.shape
  s = np.zeros((rows, 64))
  for k0 in range(0, h, 64):
    w = min(64, h - k0)
    s[:, :w] = s[:, :w] + x[:, k0:k0 + w] * y[:, k0:k0 + w]
  lanes = np.arange(64)
  for d in (32, 16, 8, 4, 2, 1):
    s = s + s[:, lanes ^ d]
  return s[:, 0]


def normalize_f32(W):
  """(A, norms) as rk_ease_elsa_normalize forms them: the row dot rounded once, a f32 root, a f32 divide."""
  W = np.asarray(W, np.float32)
  nrm = np.sqrt(row_dot64(W, W).astype(np.float32))
  assert nrm.dtype == np.float32
  return W / np.maximum(nrm, np.float32(TINY))[:, None], nrm


def project_f32(dA, A, nrm):
  dA, A = np.asarray(dA, np.float32), np.asarray(A, np.float32)
  dot = row_dot64(dA, A).astype(np.float32)
  return ease_util.fmaf(-dot[:, None], A, dA) / np.maximum(np.asarray(nrm, np.float32), np.float32(TINY))[:, None]


def adam_f32(W, dA, A, nrm, m, v, t, lr):
  """(W, A, norms, m, v) after rk_ease_elsa_adam's step t, every operation one f32 rounding in the header's order."""
  f = np.float32
  g = project_f32(dA, A, nrm)
  omb1, omb2 = f(1.0) - f(BETA1), f(1.0) - f(BETA2)
  m = ease_util.fmaf(f(BETA1), np.asarray(m, f), omb1 * g)
  v = ease_util.fmaf(f(BETA2), np.asarray(v, f), (omb2 * g) * g)
  step, isb2 = f(lr / (1.0 - BETA1 ** t)), f(1.0 / math.sqrt(1.0 - BETA2 ** t))
  W = ease_util.fmaf(-step, m / ease_util.fmaf(np.sqrt(v), isb2, f(EPS)), np.asarray(W, f))
  A, nrm = normalize_f32(W)
  return W, A, nrm, m, v


def loss_sum(row_loss, bn):
  """rk_ease_elsa_rows' batch loss: 256 ascending partial sums, the pairwise tree, one divide."""
  r = np.asarray(row_loss, np.float64)
  s = np.zeros(256)
  for u0 in range(0, len(r), 256):
    w = min(256, len(r) - u0)
    s[:w] = s[:w] + r[u0:u0 + w]
  d = 128
  while d:
    s[:d] = s[:d] + s[d:2 * d]
    d >>= 1
  return s[0] / bn


def scatter_chain(Xb, E):
  """G0 = X_b^T E as the ascending ease_util.fmaf chain from +0 over the batch positions, f32."""
  Xb = sp.csr_matrix(Xb)
  E = np.asarray(E, np.float32)
  G = np.zeros((Xb.shape[1], E.shape[1]), np.float32)
  for u in range(Xb.shape[0]):
    js = Xb.indices[Xb.indptr[u]:Xb.indptr[u + 1]]
    xs = Xb.data[Xb.indptr[u]:Xb.indptr[u + 1]].astype(np.float32)
    G[js] = ease_util.fmaf(xs[:, None], E[u][None, :], G[js])
  return G


def sparse_matrix(n_users, n, seed, density=0.2, values=False):
  """A seeded user x item matrix with an empty user row (the second), an item nobody holds (the last) and, from 3
  items on, an item everybody else holds (the first)."""
  rng = np.random.RandomState(seed)
  M = (rng.rand(n_users, n) < density).astype(np.float32)
  if n >= 3:
    M[:, 0] = 1.0
    M[:, n - 1] = 0.0
  if values:
    M = M * rng.randint(1, 4, M.shape).astype(np.float32)
  if n_users >= 2:
    M[1] = 0.0
  X = sp.csr_matrix(M)
  X.sort_indices()
  return X
