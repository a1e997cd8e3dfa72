"""WARP (Weston, Bengio & Usunier 2011, "WSABIE"; the loss of LightFM) and dynamic negative sampling
(Zhang, Chen, Wang & Yu 2013) for ``MatrixFactorization``, on rk_als_rank_sample and rk_als_warp_grad of
librecoder_als.so (include/recoder_als.h) and the rest of the BPR step (recoder_amd/bpr.py).

Both look at the model while they sample.  A slot's stored entry (u, i) is BPR's draw; its further draws that
the user does not hold are its candidates, scored s(u, c) = p_u . q_c + b_c in draw order.

WARP takes the first candidate j that violates the margin, (s(u, j) - s(u, i)) + margin > 0, after N scored
candidates; the slot's loss is w(N) ((s(u, j) - s(u, i)) + margin) with the rank weight w(N) of
``weight_table``: log(max(1, (n_items - 1) // N)) (LightFM's) or the harmonic number of (n_items - 1) // N
(WSABIE's).  The hinge's gradient has BPR's form with g = w(N), so one step is sample, grad,
``bpr.sorted_keys`` and ``bpr.apply`` twice.  A slot without a violator within ``max_draws`` draws is invalid:
as the model learns there are more of them, which ``fit`` reports per epoch beside the mean N.

DNS takes the highest-scored of the first ``num_candidates`` candidates; ``bpr.step`` draws with it when
``Recoder.train_bpr`` is given ``num_candidates`` > 1, and everything behind the sampler stays BPR's.

``Recoder.train_warp`` is the public entry point; the functions below are the layer under it (and what the
tests and tools/warp_bench.py drive directly).
"""
import numpy as np
import torch

from . import _als_lib, als, bpr
from ._lib import ptr
from .bpr import _count, _f32, _i32, _number, _round256
from .device import DEVICE_HBM_BYTES, current_stream

MAX_H = bpr.MAX_H
MAX_BATCH = bpr.MAX_BATCH
MAX_DRAWS = _als_lib.RANK_MAX_DRAWS      # RK_ALS_RANK_MAX_DRAWS
WARP, DNS = _als_lib.RANK_WARP, _als_lib.RANK_DNS
RANK_WEIGHTS = ("log", "harmonic")


def check_not_distributed():
  als.check_not_distributed("train_warp runs on one GPU: multi-GPU WARP is not implemented")


def check_config(model, num_epochs, batch_size, lr, reg, margin, max_draws, rank_weight, seed):
  """The WARP contract, checked before any GPU work; returns (num_epochs, batch_size, lr, reg, margin,
  max_draws, rank_weight, seed).  What BPR refuses is refused in its words, with this method's name."""
  try:
    num_epochs, batch_size, lr, reg, seed = bpr.check_config(model, num_epochs, batch_size, lr, reg, seed)
  except ValueError as e:
    raise ValueError(str(e).replace("train_bpr", "train_warp")) from None
  if rank_weight not in RANK_WEIGHTS:
    raise ValueError("rank_weight must be 'log' or 'harmonic' (got %r)" % (rank_weight,))
  return (num_epochs, batch_size, lr, reg, _number("margin", margin, False),
          _count("max_draws", max_draws, 1, MAX_DRAWS), rank_weight, seed)


def check_data(nnz, n_items, num_epochs, batch_size):
  return bpr.check_data(nnz, n_items, num_epochs, batch_size, method="train_warp")


def weight_table(n_items, rank_weight):
  """w(N) for N = 0..MAX_DRAWS as float32 (w(0) = 0: an invalid slot), computed in float64 and rounded once.
  With r = (n_items - 1) // N, the rank N scored candidates estimate: 'log' is log(max(1, r)), 'harmonic' is
  sum_{k = 1..r} 1 / k (0 for r = 0)."""
  if rank_weight not in RANK_WEIGHTS:
    raise ValueError("rank_weight must be 'log' or 'harmonic' (got %r)" % (rank_weight,))
  r = np.zeros(MAX_DRAWS + 1, np.int64)
  r[1:] = (int(n_items) - 1) // np.arange(1, MAX_DRAWS + 1)
  if rank_weight == "log":
    w = np.log(np.maximum(1, r).astype(np.float64))
  else:
    w = np.concatenate([[0.0], np.cumsum(1.0 / np.arange(1, max(1, int(r.max())) + 1, dtype=np.float64))])[r]
  w[0] = 0.0
  return w.astype(np.float32)


def workspace_bytes(T, h):
  """BPR's workspace and three more arrays of T entries: trials (int32), s_pos, s_neg (f32)."""
  base = bpr.workspace_bytes(T, h)
  return base if base < 0 else base + 3 * _round256(4 * int(T))


def required_bytes(n_users, n_items, h, nnz, T, allocate_model=True, snapshot=False):
  """``bpr.required_bytes`` with this workspace, the weight table and the epoch's three device counters."""
  return (bpr.required_bytes(n_users, n_items, h, nnz, T, allocate_model, snapshot) - bpr.workspace_bytes(T, h)
          + workspace_bytes(T, h) + 4 * (MAX_DRAWS + 1) + 3 * 8)


def check_memory(n_users, n_items, h, nnz, T, free_bytes=None, allocate_model=True, snapshot=False):
  """``bpr.check_memory`` for the bytes of a WARP fit."""
  n_users, n_items, h, nnz, T = int(n_users), int(n_items), int(h), int(nnz), int(T)
  if workspace_bytes(T, h) < 0:
    raise ValueError("WARP needs 1 <= batch_size <= %d and 1 <= h <= %d (got %d, %d)" % (MAX_BATCH, MAX_H, T, h))
  whole = required_bytes(n_users, n_items, h, nnz, T, True, snapshot)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError("WARP over %d users x %d items at h = %d with %d entries and batches of %d needs %d bytes: "
                     "more than one device's memory (%d bytes); multi-device fits are not implemented"
                     % (n_users, n_items, h, nnz, T, whole, DEVICE_HBM_BYTES))
  need = required_bytes(n_users, n_items, h, nnz, T, allocate_model, snapshot)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("WARP over %d users x %d items at h = %d with %d entries and batches of %d needs %d bytes "
                     "of device memory, %d are free" % (n_users, n_items, h, nnz, T, need, free_bytes))
  return need


# ------------------------------------------------------------------ kernels
class Workspace(bpr.Workspace):
  """BPR's buffers, then trials (int32 [T]), s_pos and s_neg (f32 [T]) in an allocation of their own."""

  def __init__(self, T, h, device):
    super().__init__(T, h, device)
    assert workspace_bytes(T, h) == self.raw.numel() + 3 * _round256(4 * T)
    self.extra = torch.empty(3 * _round256(4 * T), dtype=torch.uint8, device=device)
    step = _round256(4 * T)
    self.trials = self.extra[:4 * T].view(torch.int32)
    self.s_pos, self.s_neg = (self.extra[k * step:k * step + 4 * T].view(torch.float32) for k in (1, 2))


def sample(csr, seed, step, X, Y, bias, mode, max_draws, num_candidates, margin, users, pos, neg, trials,
           s_pos=None, s_neg=None, scores=None):
  """users / pos / neg / trials (int32 [T], filled in place) of step ``step`` under ``seed`` at the tables as
  they stand (rk_als_rank_sample); ``s_pos``, ``s_neg`` [T] and ``scores`` [T, max_draws], when given, receive
  the scores."""
  T, h = users.shape[0], X.shape[1]
  for t in (users, pos, neg, trials):
    _i32(t, T)
  for t in (s_pos, s_neg):
    if t is not None:
      _f32(t, (T,))
  if scores is not None:
    _f32(scores, (T, max_draws))
  _f32(bias, (Y.shape[0],))
  assert X.dtype == Y.dtype == torch.float32 and Y.shape[1] == h and X.stride(1) == 1 and Y.stride(1) == 1
  assert X.shape[0] == csr.shape[0] and Y.shape[0] == csr.shape[1], (X.shape, Y.shape, csr.shape)
  if csr.nnz >= 2 ** 31:
    raise ValueError("the rank sampler needs nnz below 2^31 (got %d)" % csr.nnz)
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_rank_sample(ptr(csr.indptr), ptr(csr.indices), csr.shape[0], csr.shape[1], csr.nnz,
                                        int(seed), int(step), T, ptr(X), X.stride(0), ptr(Y), Y.stride(0),
                                        ptr(bias), h, int(mode), int(max_draws), int(num_candidates),
                                        float(margin), ptr(users), ptr(pos), ptr(neg), ptr(trials), ptr(s_pos),
                                        ptr(s_neg), ptr(scores), current_stream()), "rk_als_rank_sample")


def grad(users, pos, neg, trials, X, Y, bias, margin, weight, g, loss, D, P):
  """g = weight[trials], the hinge loss [T] and the staging rows D = q_i - q_j, P = p_u [T, h] of the triples
  (rk_als_warp_grad); ``weight`` is ``weight_table`` on the device."""
  T, h = users.shape[0], X.shape[1]
  for t in (users, pos, neg, trials):
    _i32(t, T)
  _f32(g, (T,)), _f32(loss, (T,)), _f32(D, (T, h)), _f32(P, (T, h)), _f32(bias, (Y.shape[0],))
  _f32(weight, (MAX_DRAWS + 1,))
  assert X.dtype == Y.dtype == torch.float32 and Y.shape[1] == h and X.stride(1) == 1 and Y.stride(1) == 1
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_warp_grad(ptr(users), ptr(pos), ptr(neg), ptr(trials), T, X.shape[0], Y.shape[0],
                                      ptr(X), X.stride(0), ptr(Y), Y.stride(0), ptr(bias), h, float(margin),
                                      ptr(weight), ptr(g), ptr(loss), ptr(D), ptr(P), current_stream()),
                 "rk_als_warp_grad")


def step(X, Y, bias, ucsr, ws, weight, seed, step_index, lr, reg, margin, max_draws):
  """One WARP step on the tables in place; the triples, trials, g and loss of the step stay in ``ws``."""
  sample(ucsr, seed, step_index, X, Y, bias, WARP, max_draws, 1, margin, ws.users, ws.pos, ws.neg, ws.trials,
         ws.s_pos, ws.s_neg)
  grad(ws.users, ws.pos, ws.neg, ws.trials, X, Y, bias, margin, weight, ws.g, ws.loss, ws.D, ws.P)
  (uk, uo), (ik, io) = bpr.sorted_keys(ws.users, ws.pos, ws.neg, X.shape[0], Y.shape[0])
  bpr.apply(uk, uo, 1, ws.g, ws.D, lr, reg, X)
  bpr.apply(ik, io, 2, ws.g, ws.P, lr, reg, Y, bias)


# ---------------------------------------------------------------------- fit
def fit(X, Y, bias, ucsr, num_epochs, batch_size, lr, reg, margin=1.0, max_draws=32, rank_weight="log", seed=0,
        first_step=0, monitor=None):
  """num_epochs epochs of ceil(nnz / batch_size) WARP steps on the tables X [users, h], Y [items, h] and bias
  [items] (in place, f32, row-major); step s of the fit draws as step ``first_step + s``.  Returns (history,
  stats): the mean loss per valid slot of each epoch (nan for an epoch without one), and per epoch (the share
  of slots that found a violator, the mean trials of those that did).  One host synchronisation per epoch, to
  read that epoch's sums.  ``monitor``: as in ``bpr.fit``; the history and the stats keep every epoch that ran."""
  steps = check_data(ucsr.nnz, ucsr.shape[1], num_epochs, batch_size)
  check_memory(X.shape[0], Y.shape[0], X.shape[1], ucsr.nnz, batch_size, allocate_model=False,
               snapshot=monitor is not None and monitor.restore_best)
  ws = Workspace(int(batch_size), X.shape[1], X.device)
  weight = torch.as_tensor(weight_table(Y.shape[0], rank_weight), device=X.device)
  hist, stats = [], []
  s = int(first_step)
  for e in range(num_epochs):
    total = torch.zeros((), dtype=torch.float64, device=X.device)
    count = torch.zeros((), dtype=torch.int64, device=X.device)
    drawn = torch.zeros((), dtype=torch.int64, device=X.device)
    for _ in range(steps):
      step(X, Y, bias, ucsr, ws, weight, seed, s, lr, reg, margin, max_draws)
      total += ws.loss.sum(dtype=torch.float64)
      count += (ws.neg >= 0).sum()
      drawn += ws.trials.sum(dtype=torch.int64)
      s += 1
    total, count, drawn = torch.stack([total, count.double(), drawn.double()]).cpu().tolist()   # (the synchronisation)
    hist.append(total / count if count else float("nan"))
    stats.append((count / (steps * int(batch_size)), drawn / count if count else float("nan")))
    if monitor is not None and monitor.due(e) and monitor.epoch_end(e, (X, Y, bias)):
      break
  if monitor is not None:
    monitor.finish((X, Y, bias), len(hist))
  return hist, stats
