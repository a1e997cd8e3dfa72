"""ELSA (Vancura, Alves, Kasalicky & Kordik, RecSys 2022, "Scalable Linear Shallow Autoencoder for Collaborative
Filtering") for ``LowRankShallowAutoencoder``, on the HIP kernels of librecoder_ease.so (include/recoder_ease.h) and
the Gram of librecoder_als.so.

The model is EASE's shape without the n x n matrix: ``scores = x (A A^T - I)`` with A [n, h] the rows of the
parameter W normalised to unit length, A_j = W_j / max(|W_j|, 1e-12).  It is trained by mini-batch Adam steps on the
cosine loss ``mse_loss(normalize(X_b A A^T - X_b), normalize(X_b))`` of the published code.  That code writes the
B x n prediction block P = Z A^T - X_b (Z = X_b A) and runs three B x n x h products over it; here every quantity
comes from the h x h Gram S = A^T A, sparse products over the batch's stored entries and one n x h x h product, exactly:

    Z = X_b A                                   rk_ease_scores   (the batch is ``indptr + lo`` of the permuted CSR)
    S = A^T A                                   rk_als_gram
    Q = Z S                                     rk_ease_gemm
    t2_u = |X_u|^2, z2_u = |Z_u|^2, q_u = <Z_u, Q_u>
    p2 = q - 2 z2 + t2 (= |P_u|^2),  dot = z2 - t2 (= <P_u, X_u>),  c = dot / (sqrt(p2) sqrt(t2))
    loss = 1 / (B n) sum_live (2 - 2 c)         a row is live if t2 > 0 and p2 > 0; a dead row with t2 > 0 adds 1
    a = -2 / (B n sqrt(p2) sqrt(t2)),  b = 2 c / (B n p2)
    E_u = 2 (a - b) Z_u + b Q_u,  F_u = b Z_u   rk_ease_elsa_rows (float64 row scalars)
    G0 = X_b^T E                                rk_ease_elsa_scatter (a position range of the item-major CSR)
    M = Z^T F                                   rk_ease_gemm
    dA = A M + G0                               rk_ease_gemm, accumulating in place
    dW_j = (dA_j - <dA_j, A_j> A_j) / max(|W_j|, 1e-12), Adam on W, the new A_j        rk_ease_elsa_adam

Adam is torch.optim.Adam's (betas 0.9 / 0.999, eps 1e-8, bias-corrected, no weight decay); every row moves every step.
The start is ``RandomState(seed).uniform(-r, r, (n, h))`` as float32 with r = sqrt(6 / (n + h)) and epoch e orders
the users by ``RandomState(seed + 1 + e).permutation(n_users)``, both drawn on the host: a fixed seed gives the same
bits.  The CSR pair of the permuted matrix is built on the device once per epoch, a batch is a contiguous range of
its positions, the last one ragged; the epoch's loss is read once, at its end.

``Recoder.train_elsa`` is the public entry point; the functions below are the layer under it (and what the tests and
tools/elsa_bench.py drive directly).
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _ease_lib, als
from ._lib import ptr
from .admm import _ld, gemm
from .device import DEVICE_HBM_BYTES, current_stream
from .ease import scores

MAX_H = 512
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
DEFAULT_EPOCHS = 5          # train_elsa's num_epochs=None (the grid's cell: nn.LowRankShallowAutoencoder's docstring)
_GRAM_CHUNKS = 64            # rk_als_gram splits the rows into at most this many chunks of h (h + 1) floats


def check_not_distributed():
  als.check_not_distributed("train_elsa runs on one GPU: a multi-GPU ELSA fit is not implemented")


def _check_int(name, value, lo, hi=2 ** 31):
  if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= value < hi:
    raise ValueError("%s must be an integer >= %d (got %r)" % (name, lo, value))
  return int(value)


def check_embedding_size(embedding_size):
  if isinstance(embedding_size, bool) or not isinstance(embedding_size, (int, np.integer)) or \
      not 1 <= embedding_size <= MAX_H:
    raise ValueError("embedding_size must be an integer in 1..%d (got %r)" % (MAX_H, embedding_size))
  return int(embedding_size)


def check_params(embedding_size, num_epochs, batch_size, lr, seed):
  """(embedding_size, num_epochs, batch_size, lr, seed), each checked: embedding_size in 1..512, integer epoch and
  batch counts >= 1, a finite lr > 0, an integer seed in [0, 2^32 - 1 - num_epochs] (numpy's RandomState range)."""
  embedding_size = check_embedding_size(embedding_size)
  num_epochs = _check_int("num_epochs", num_epochs, 1)
  batch_size = _check_int("batch_size", batch_size, 1)
  if isinstance(lr, bool) or not isinstance(lr, (int, float, np.integer, np.floating)) or \
      not (math.isfinite(float(lr)) and float(lr) > 0):
    raise ValueError("lr must be finite and > 0 (got %r)" % (lr,))
  if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed <= 2 ** 32 - 1 - num_epochs:
    raise ValueError("seed must be an integer in [0, 2^32 - 1 - num_epochs] (got %r)" % (seed,))
  return embedding_size, num_epochs, batch_size, float(lr), int(seed)


def check_config(model, num_epochs, batch_size, lr, seed):
  """The ELSA contract, checked before any GPU work; returns (embedding_size, num_epochs, batch_size, lr, seed)."""
  from .nn import LowRankShallowAutoencoder
  if not isinstance(model, LowRankShallowAutoencoder):
    raise ValueError("train_elsa fits a LowRankShallowAutoencoder, not %s" % type(model).__name__)
  return check_params(model.embedding_size, num_epochs, batch_size, lr, seed)


def required_bytes(n_users, n, h, batch_size, nnz, allocate_model=True):
  """Device bytes a fit allocates: W (unless the caller already holds it), the two Adam moments, A and dA [n, h] and
  the norms; the permuted CSR pair (two indptr, indices and values twice, the users' |X_u|^2) with the sort that builds
  it (keys, sorted keys and order, 8 bytes an entry each, and the gather's two int64 vectors); the five [B, h] buffers
  (Z, Z^T, Q, E, F) and the row losses; S, M and the Gram's workspace."""
  n_users, n, h, B, nnz = int(n_users), int(n), int(h), int(batch_size), int(nnz)
  B = min(B, max(n_users, 1))
  tables = ((5 if allocate_model else 4) * n * h + n) * 4
  csrs = (n_users + 1 + n + 1) * 8 + 2 * nnz * 8 + n_users * 4 + 5 * nnz * 8
  batch = 5 * B * h * 4 + B * 8
  small = 2 * h * h * 4 + _GRAM_CHUNKS * h * (h + 1) * 4
  return tables + csrs + batch + small


def check_memory(n_users, n, h, batch_size, nnz, free_bytes=None, allocate_model=True):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's whole HBM without
  touching a device, then (``free_bytes`` None: asked from the current device) against what is free."""
  n = int(n)
  if n < 1:
    raise ValueError("ELSA needs at least one item (got n = %d)" % n)
  if n >= 2 ** 31 - 4 or int(n_users) >= 2 ** 31 - 4:
    raise ValueError("ELSA over %d users and %d items is outside the kernels' index range" % (n_users, n))
  whole = required_bytes(n_users, n, h, batch_size, nnz, True)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError("ELSA over n = %d items with embedding_size %d needs %d bytes: more than one device's memory "
                     "(%d bytes); multi-device fits are not implemented" % (n, h, whole, DEVICE_HBM_BYTES))
  need = required_bytes(n_users, n, h, batch_size, nnz, allocate_model)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("ELSA over n = %d items with embedding_size %d needs %d bytes of device memory, %d are free"
                     % (n, h, need, free_bytes))
  return need


def initial_factors(n, h, seed):
  """The start of a fit: Xavier-uniform from the host generator, float32 [n, h]."""
  r = math.sqrt(6.0 / (n + h))
  return np.random.RandomState(seed).uniform(-r, r, (n, h)).astype(np.float32)


def epoch_order(n_users, seed, epoch):
  """The user order of epoch ``epoch`` (counted from 0): position p of the epoch holds user ``order[p]``."""
  return np.random.RandomState(seed + 1 + epoch).permutation(n_users)


def adam_scalars(lr, t):
  """(step, isb2) of Adam's step t >= 1, formed in float64: lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t)."""
  return lr / (1.0 - BETA1 ** t), 1.0 / math.sqrt(1.0 - BETA2 ** t)


# ------------------------------------------------------------------ kernels
def normalize(W, A=None, norms=None, At=None):
  """(A, norms): the rows of W [n, h] at unit length and their norms (rk_ease_elsa_normalize); ``At`` [h, n], when
  given, receives the transpose."""
  lib = _ease_lib.load()
  n, h = W.shape
  A = torch.empty(n, h, dtype=torch.float32, device=W.device) if A is None else A
  norms = torch.empty(n, dtype=torch.float32, device=W.device) if norms is None else norms
  assert A.shape == (n, h) and norms.shape == (n,) and norms.is_contiguous() and (At is None or At.shape == (h, n))
  _ease_lib.check(lib.rk_ease_elsa_normalize(ptr(W), _ld(W), n, h, ptr(A), _ld(A), ptr(norms), ptr(At),
                                             0 if At is None else _ld(At), current_stream()), "rk_ease_elsa_normalize")
  return A, norms


def rows(Z, Q, t2, n, E, F, row_loss, loss_acc=None):
  """E, F and the row losses of a batch from Z, Q [B, h] and t2 [B]; the batch's loss is added to ``loss_acc[0]``
  (float64) when given (rk_ease_elsa_rows)."""
  lib = _ease_lib.load()
  B, h = Z.shape
  assert Q.shape == E.shape == F.shape == (B, h) and t2.shape == (B,) and t2.dtype == torch.float32
  assert row_loss.shape == (B,) and row_loss.dtype == torch.float64 and (loss_acc is None or
                                                                         loss_acc.dtype == torch.float64)
  assert t2.is_contiguous() and row_loss.is_contiguous()
  _ease_lib.check(lib.rk_ease_elsa_rows(ptr(Z), _ld(Z), ptr(Q), _ld(Q), ptr(t2), B, h, int(n), ptr(E), _ld(E), ptr(F),
                                        _ld(F), ptr(row_loss), ptr(loss_acc), current_stream()), "rk_ease_elsa_rows")


def scatter(icsr, lo, hi, E, G):
  """G[j] = sum over the positions u in [lo, hi) of row j of the item-major CSR, ascending, of x_uj E[u - lo]
  (rk_ease_elsa_scatter); every row of G [n, h] is written."""
  lib = _ease_lib.load()
  n, h = G.shape
  assert icsr.shape[0] == n and 0 <= lo <= hi <= icsr.shape[1] and (lo == hi or E.shape == (hi - lo, h))
  _ease_lib.check(lib.rk_ease_elsa_scatter(ptr(icsr.indptr), ptr(icsr.indices), ptr(icsr.data), n, lo, hi,
                                           None if lo == hi else ptr(E), 0 if lo == hi else _ld(E), h, ptr(G), _ld(G),
                                           current_stream()), "rk_ease_elsa_scatter")
  return G


def project(dA, A, norms, dW=None):
  """dW = the gradient with respect to W of a gradient dA with respect to A (rk_ease_elsa_project)."""
  lib = _ease_lib.load()
  n, h = A.shape
  dW = torch.empty(n, h, dtype=torch.float32, device=A.device) if dW is None else dW
  assert dA.shape == dW.shape == (n, h) and norms.shape == (n,) and norms.is_contiguous()
  _ease_lib.check(lib.rk_ease_elsa_project(ptr(dA), _ld(dA), ptr(A), _ld(A), ptr(norms), n, h, ptr(dW), _ld(dW),
                                           current_stream()), "rk_ease_elsa_project")
  return dW


def adam(W, dA, A, norms, M, V, lr, t):
  """Adam's step t >= 1 on W from dA, in place, with A and the norms taken again (rk_ease_elsa_adam)."""
  lib = _ease_lib.load()
  n, h = W.shape
  assert dA.shape == A.shape == M.shape == V.shape == (n, h) and M.is_contiguous() and V.is_contiguous()
  assert norms.shape == (n,) and norms.is_contiguous()
  step, isb2 = adam_scalars(lr, t)
  _ease_lib.check(lib.rk_ease_elsa_adam(ptr(W), _ld(W), ptr(dA), _ld(dA), ptr(A), _ld(A), ptr(norms), ptr(M), ptr(V), n,
                                        h, BETA1, BETA2, EPS, step, isb2, current_stream()), "rk_ease_elsa_adam")


def csr_sub(csr, lo, hi, out, ld, n_rows):
  """out[u, j - lo] -= x_uj over the stored entries of the strip (rk_ease_csr_sub); ``out`` f32 with row stride ld."""
  lib = _ease_lib.load()
  _ease_lib.check(lib.rk_ease_csr_sub(ptr(csr.indptr), ptr(csr.indices), ptr(csr.data), n_rows, lo, hi, ptr(out), ld,
                                      current_stream()), "rk_ease_csr_sub")
  return out


# ------------------------------------------------------------- permuted CSRs
def row_squares(ucsr):
  """|X_u|^2 of every user row as f32 on the device, summed on the host in float64 and rounded once (a row of ones:
  its length).  One copy to the host, once per fit."""
  indptr = ucsr.indptr.cpu().numpy()
  if ucsr.data is None or ucsr.nnz == 0:
    t2 = np.diff(indptr).astype(np.float64) if ucsr.nnz else np.zeros(len(indptr) - 1)
  else:
    sq = np.concatenate([ucsr.data.cpu().numpy()[:ucsr.nnz].astype(np.float64) ** 2, [0.0]])
    t2 = np.add.reduceat(sq, np.minimum(indptr[:-1], ucsr.nnz))
    t2[np.diff(indptr) == 0] = 0.0
  return torch.from_numpy(t2.astype(np.float32)).to(ucsr.indptr.device)


def permuted_pair(ucsr, order):
  """(user-major, item-major) CSRs of X[order] on the device, from the user-major CSR of X and the int64 device tensor
  ``order``: row p of the first is user order[p]'s row, the columns of the second are positions p, ascending.  A
  gather for the first, one sort of (item, position) keys for the second; no host synchronisation."""
  U, n = ucsr.shape
  nnz, dev = ucsr.nnz, ucsr.indptr.device
  lens = (ucsr.indptr[1:] - ucsr.indptr[:-1])[order]
  indptr = torch.zeros(U + 1, dtype=torch.int64, device=dev)
  torch.cumsum(lens, 0, out=indptr[1:])
  t_indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
  if nnz == 0:
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    return (SimpleNamespace(indptr=indptr, indices=one, data=None, shape=(U, n), nnz=0),
            SimpleNamespace(indptr=t_indptr, indices=one, data=None, shape=(n, U), nnz=0))
  pos = torch.repeat_interleave(torch.arange(U, device=dev), lens, output_size=nnz)
  src = torch.arange(nnz, device=dev) - indptr[:-1][pos] + ucsr.indptr[:-1][order][pos]
  indices = ucsr.indices[:nnz][src]
  data = None if ucsr.data is None else ucsr.data[:nnz][src]
  keys, by_item = torch.sort(indices.to(torch.int64) * U + pos)
  # (row j of the item-major CSR starts at the first key >= j U: no count on the host, no synchronisation)
  t_indptr.copy_(torch.searchsorted(keys, torch.arange(n + 1, dtype=torch.int64, device=dev) * U))
  t_indices = (keys % U).to(torch.int32)
  t_data = None if data is None else data[by_item]
  return (SimpleNamespace(indptr=indptr, indices=indices.contiguous(), data=data, shape=(U, n), nnz=nnz),
          SimpleNamespace(indptr=t_indptr, indices=t_indices, data=t_data, shape=(n, U), nnz=nnz))


# --------------------------------------------------------------------- step
class State:
  """The buffers of a fit over W [n, h] (in place): A, the norms, dA, the Adam moments, the [B, h] buffers.
  ``gradient(pair, t2, lo, hi, loss_acc)`` leaves dA of the batch [lo, hi) of the pair's positions in ``self.dA``;
  ``step(...)`` follows it with Adam's step.  Nothing here synchronises."""

  def __init__(self, W, batch_size, moments=True):
    n, h = W.shape
    dev = W.device
    assert W.dtype == torch.float32 and W.is_contiguous()
    self.W, self.n, self.h, self.B = W, n, h, int(batch_size)
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    self.A, self.norms, self.dA = new(n, h), new(n), new(n, h)
    self.M, self.V = (torch.zeros(n, h, dtype=torch.float32, device=dev) for _ in range(2)) if moments else (None, None)
    self.Z, self.Q, self.E, self.F = (new(self.B, h) for _ in range(4))
    self.Mm = new(h, h)
    self.row_loss = torch.empty(self.B, dtype=torch.float64, device=dev)
    lib = als._als_lib.load()
    self.gws = torch.empty(max(lib.rk_als_gram_workspace_bytes(n, h), 4), dtype=torch.uint8, device=dev)
    self.t = 0
    normalize(W, self.A, self.norms)

  def gradient(self, pair, t2, lo, hi, loss_acc=None):
    pu, pt = pair
    b, h = hi - lo, self.h
    assert 0 < b <= self.B
    Z, Q, E, F = (x[:b] for x in (self.Z, self.Q, self.E, self.F))
    batch = SimpleNamespace(indptr=pu.indptr[lo:], indices=pu.indices, data=pu.data, shape=(b, self.n))
    scores(batch, self.A, 0, h, out=Z, ld=h, n_rows=b)                       # Z = X_b A
    S, _ = als.gram(self.A, 0.0, None, self.gws)                            # S = A^T A
    gemm(Z, S, Q)                                                            # Q = Z S
    rows(Z, Q, t2[lo:hi], self.n, E, F, self.row_loss[:b], loss_acc)
    scatter(pt, lo, hi, E, self.dA)                                          # G0 = X_b^T E
    gemm(Z.t().contiguous(), F, self.Mm)                                     # M = Z^T F
    gemm(self.A, self.Mm, self.dA, 1.0, 1.0, E=self.dA)                      # dA = A M + G0
    return self.dA

  def step(self, pair, t2, lo, hi, lr, loss_acc=None):
    self.gradient(pair, t2, lo, hi, loss_acc)
    self.t += 1
    adam(self.W, self.dA, self.A, self.norms, self.M, self.V, lr, self.t)


def gradient(csr_pair, W, lo, hi):
  """(loss, dW) of the batch of the user rows [lo, hi) of the (user-major, item-major) CSR pair at the parameter W
  [n, h] (f32, on the device), through the kernels and without a step: the batch's loss as a float and the gradient
  with respect to W as a new tensor."""
  ucsr, icsr = csr_pair
  assert 0 <= lo < hi <= ucsr.shape[0] and W.shape[0] == ucsr.shape[1]
  W = W.contiguous()
  st = State(W, hi - lo, moments=False)
  acc = torch.zeros(1, dtype=torch.float64, device=W.device)
  st.gradient(csr_pair, row_squares(ucsr), lo, hi, acc)
  return float(acc.cpu().item()), project(st.dA, st.A, st.norms)


# ---------------------------------------------------------------------- fit
def fit(csr_pair, embedding_size, num_epochs, batch_size, lr, seed, out=None):
  """(W, history) for the (user-major, item-major) CSR pair of ``als.csr_pair`` (only the first is read):
  ``num_epochs`` epochs of ceil(n_users / batch_size) Adam steps from the seeded start; W [n, h] lands in ``out`` when
  given.  ``history`` is the mean batch loss of each epoch; one host synchronisation per epoch, at its end."""
  ucsr = csr_pair[0]
  h, num_epochs, batch_size, lr, seed = check_params(embedding_size, num_epochs, batch_size, lr, seed)
  check_not_distributed()
  U, n = ucsr.shape
  check_memory(U, n, h, batch_size, ucsr.nnz, allocate_model=out is None)
  dev = ucsr.indptr.device
  W = torch.empty(n, h, dtype=torch.float32, device=dev) if out is None else out
  assert W.shape == (n, h) and W.dtype == torch.float32 and W.is_contiguous()
  W.copy_(torch.from_numpy(initial_factors(n, h, seed)))
  st = State(W, min(batch_size, max(U, 1)))
  t2 = row_squares(ucsr)
  history = []
  for epoch in range(num_epochs):
    order = torch.from_numpy(epoch_order(U, seed, epoch).astype(np.int64)).to(dev)
    pair = permuted_pair(ucsr, order)
    pt2 = t2[order]
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    steps = 0
    for lo in range(0, U, batch_size):
      st.step(pair, pt2, lo, min(U, lo + batch_size), lr, acc)
      steps += 1
    history.append(float(acc.cpu().item()) / max(steps, 1))         # (the synchronisation)
  return W, history
