"""Sampled-softmax training (Wu et al. 2022, "On the Effectiveness of Sampled Softmax Loss for Item Recommendation";
the in-batch softmax of two-tower retrieval with the log-Q correction of Yi et al. 2019; the mixed in-batch and
uniform negatives of Yang et al. 2020) for ``MatrixFactorization``, on rk_als_ssm_grad of librecoder_als.so
(include/recoder_als.h) and the sampler, graph, scatter and Adam of recoder_amd/bpr.py and recoder_amd/lightgcn.py.

The model is a ``MatrixFactorization`` with ``activation_type="none"``; the trainable parameters are the base
tables E0 = (P^0, Q^0) and the final tables (X, Y) are LightGCN's: the mean over the layers 0..K of E0 propagated
over the normalised graph of the stored entries (K = 0: the base tables themselves).  A step draws T slots
(u_t, i_t) with BPR's sampler -- the negative of the draw is ignored -- and S items uniformly from the catalogue,
shared by the batch, and descends

    (1 / m) sum_t (log sum_c exp(s_tc) - s_tt) + the L2 term of LightGCN,
    s_tc = sim(X[u_t], Y[j_c]) / temperature - corr[j_c],

over the C = T + S candidate columns: column c < T is slot c's positive (the in-batch negatives of every other
row), the columns after them are the shared draws.  A column that holds row t's own positive once more is left out
of row t's sum; other items the user holds are not.  corr[j] = logq_weight log((T d_j / nnz + S / n_items) / C)
is the logarithm of the share of the columns item j is expected to hold, d_j its users.  rk_als_ssm_grad leaves
one gradient row per slot and per column, rk_als_lgcn_scatter sums them per table row, one ``lightgcn.forward``
propagates them back and Adam steps both base tables.  2 K propagations forward and 2 K back a step.

``Recoder.train_ssm`` is the public entry point; the functions below are the layer under it (and what the tests
and tools/ssm_bench.py drive directly).
"""
import math

import numpy as np
import torch

from . import _als_lib, als, bpr, lightgcn
from ._lib import ptr
from .bpr import _count, _f32, _i32, _number, _round256
from .device import current_stream
from .lightgcn import _table, new_state, scatter  # noqa: F401  (new_state: this module's too)

MAX_H = als.MAX_H                             # rk_als_max_h()
MAX_LAYERS = lightgcn.MAX_LAYERS
MAX_BATCH = _als_lib.SSM_MAX_BATCH            # RK_ALS_SSM_MAX_BATCH: the workspace holds one T x (T + S) tile
MAX_NEGATIVES = _als_lib.SSM_MAX_NEGATIVES    # RK_ALS_SSM_MAX_NEGATIVES
SIMILARITIES = ("cosine", "dot")


def check_not_distributed():
  """ValueError under more than one rank."""
  try:
    als.check_not_distributed("train_ssm runs on one GPU: multi-GPU sampled-softmax training is not implemented")
  except NotImplementedError as e:
    raise ValueError(str(e)) from None


def check_config(model, num_layers, num_epochs, batch_size, lr, reg, temperature, num_negatives, similarity,
                 logq_weight, normalize, seed):
  """The contract of ``train_ssm``, checked before any GPU work; returns (num_layers, num_epochs, batch_size, lr,
  reg, temperature, num_negatives, similarity, logq_weight, normalize, seed).  ``num_layers`` may be 0."""
  c = lightgcn.check_config(model, num_layers, num_epochs, batch_size, lr, reg, seed, METHOD)
  if similarity not in SIMILARITIES:
    raise ValueError("similarity must be one of %s (got %r)" % (", ".join(map(repr, SIMILARITIES)), similarity))
  tau = _number("temperature", temperature, True)
  if not math.isfinite(1.0 / tau):
    raise ValueError("temperature must be finite and > 0 (got %r)" % (temperature,))
  return c[:5] + (tau, _count("num_negatives", num_negatives, 0, MAX_NEGATIVES), similarity,
                  _number("logq_weight", logq_weight, False), bool(normalize), c[5])


def check_resume(state, num_layers, shapes=None):
  """ValueError unless ``state`` (an ``ssm_state``) can continue a fit with ``num_layers`` layers on base tables of
  ``shapes``."""
  lightgcn.check_resume(state, num_layers, shapes, method="train_ssm")


def check_data(nnz, n_items, num_epochs, batch_size):
  return bpr.check_data(nnz, n_items, num_epochs, batch_size, method="train_ssm")


def grad_workspace_bytes(T, S, h):
  """rk_als_ssm_workspace_bytes(T, S, h), restated on the host: with C = T + S two [T, h] and two [C, h] images, the
  T x C tile, four vectors of T and three of C, each rounded up to 64 floats."""
  T, S, h = int(T), int(S), int(h)
  if not (1 <= T <= MAX_BATCH and 0 <= S <= MAX_NEGATIVES and 1 <= h <= MAX_H):
    return -2
  C = T + S
  return 2 * _round256(4 * T * h) + 2 * _round256(4 * C * h) + _round256(4 * T * C) + 4 * _round256(4 * T) + \
      3 * _round256(4 * C)


def extra_bytes(n_users, n_items, h, T, num_negatives=0):
  """The workspace of rk_als_ssm_grad, the candidates' gradient image, ids and validity, the correction vector, the
  two losses and the count, and the keys of the two sorts this step makes itself (T users and C candidates: an
  int32 key in, a key and an int64 position out, as much again for its scratch)."""
  C = T + int(num_negatives)
  return grad_workspace_bytes(T, num_negatives, h) + C * h * 4 + 2 * C * 4 + n_items * 4 + 12 + \
      2 * (T + C) * (4 + 4 + 8)


def required_bytes(n_users, n_items, h, nnz, T, num_negatives=0, allocate_model=True, allocate_state=True,
                   allocate_csrs=True):
  """Device bytes of a fit: what LightGCN's fit holds (``lightgcn.required_bytes``: its BPR workspace is where
  the draws, the validity vector and the users' [T, h] gradient image live) and ``extra_bytes``."""
  return lightgcn.method_required_bytes(METHOD, n_users, n_items, h, nnz, T, allocate_model, allocate_state,
                                        allocate_csrs, num_negatives=num_negatives)


def check_memory(n_users, n_items, h, nnz, T, num_negatives=0, free_bytes=None, allocate_model=True,
                 allocate_state=True, allocate_csrs=True):
  """``lightgcn.method_check_memory`` of the sampled softmax."""
  return lightgcn.method_check_memory(METHOD, n_users, n_items, h, nnz, T, free_bytes, allocate_model, allocate_state,
                                      allocate_csrs, num_negatives=num_negatives)


def correction(item_degrees, T, S, logq_weight):
  """corr [n_items] f32 = logq_weight log((T d_j / nnz + S / n_items) / (T + S)) in float64, rounded once: the
  logarithm of the share of a step's columns that item j is expected to hold.  An item that can hold no column
  (no user and S = 0) gets 0: no logit ever reads it."""
  d = np.asarray(item_degrees, dtype=np.float64)
  q = (T * d / max(float(d.sum()), 1.0) + S / float(len(d))) / (T + S)
  return (float(logq_weight) * np.log(np.where(q > 0, q, 1.0))).astype(np.float32)


# ------------------------------------------------------------------ kernels
def grad(users, items, num_negatives, seed, step_index, X, Y, temperature, similarity, corr, raw, cand, DU, DC, valid,
         cvalid, loss, count):
  """DU [T, h] / DC [C, h] = the gradient rows of the slots (``users``, ``items``) and of the C = T +
  ``num_negatives`` candidate columns at the tables X / Y, ``cand`` [C] = the columns' items (the shared draws of
  (``seed``, ``step_index``) after the slots' positives), ``valid`` [T] / ``cvalid`` [C] = 1.0 / 0.0, ``loss`` [2]
  = (the softmax loss, the mean probability of the positive) and ``count`` [1] = the valid slots
  (rk_als_ssm_grad); ``corr`` is None or an f32 [n_items] vector, ``raw`` a uint8 workspace of
  ``grad_workspace_bytes`` at least."""
  T, S = users.shape[0], int(num_negatives)
  C = T + S
  _i32(users, T), _i32(items, T), _table(X), _table(Y, X.shape[1])
  h = X.shape[1]
  _i32(cand, C), _f32(DU, (T, h)), _f32(DC, (C, h)), _f32(valid, (T,)), _f32(cvalid, (C,)), _f32(loss, (2,))
  _i32(count, 1)
  if corr is not None:
    _f32(corr, (Y.shape[0],))
  assert raw.dtype == torch.uint8 and raw.is_contiguous() and similarity in SIMILARITIES
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_ssm_grad(ptr(users), ptr(items), T, S, int(seed), int(step_index), X.shape[0], Y.shape[0],
                                     ptr(X), X.stride(0), ptr(Y), Y.stride(0), h, 1.0 / float(temperature),
                                     1 if similarity == "cosine" else 0, ptr(corr), ptr(raw), raw.numel(), ptr(cand),
                                     ptr(DU), ptr(DC), ptr(valid), ptr(cvalid), ptr(loss), ptr(count),
                                     current_stream()), "rk_als_ssm_grad")


# --------------------------------------------------------------------- step
class Workspace(lightgcn.Workspace):
  """LightGCN's workspace (the draws in ``bpr.users`` / ``bpr.pos``, the validity vector in ``bpr.g``, the users'
  gradient image DU in ``bpr.D``), the workspace of rk_als_ssm_grad, the candidates' side and the results."""

  def __init__(self, n_users, n_items, T, h, device, num_negatives=0):
    super().__init__(n_users, n_items, T, h, device)
    S = int(num_negatives)
    need = _als_lib.load().rk_als_ssm_workspace_bytes(T, S, h)
    assert need == grad_workspace_bytes(T, S, h) and need > 0, (need, T, S, h)
    self.num_negatives = S
    self.raw = torch.empty(need, dtype=torch.uint8, device=device)
    self.cand = torch.zeros(T + S, dtype=torch.int32, device=device)
    self.cvalid = torch.zeros(T + S, dtype=torch.float32, device=device)
    self.DC = torch.zeros((T + S, h), dtype=torch.float32, device=device)
    self.loss = torch.zeros(2, dtype=torch.float32, device=device)
    self.valid_count = torch.zeros(1, dtype=torch.int32, device=device)
    self.corr = {}                                       # logq_weight -> the device vector, made at the first step


def sorted_keys(ids, valid, n_rows):
  """(keys, order) of the slots or columns, stably sorted by row on the device; an invalid one carries the key
  past the table."""
  return torch.sort(bpr.masked_keys(ids, valid > 0, n_rows), stable=True)


def _corr(graph, ws, logq_weight):
  if not logq_weight > 0:
    return None
  if logq_weight not in ws.corr:
    degrees = np.diff(graph.icsr.indptr.cpu().numpy())
    ws.corr[logq_weight] = torch.from_numpy(correction(degrees, ws.bpr.T, ws.num_negatives, logq_weight)).to(
        graph.si.device)
  return ws.corr[logq_weight]


def gradient(X, Y, graph, state, ws, seed, step_index, hyper):
  """rk_als_ssm_grad at the draws (the negative is ignored) and the sum of its rows per table row: the users over
  the T slots, the items over the C candidate columns; the two losses of the step stay in ``ws.loss``, its valid
  slots in ``ws.valid_count`` and the columns' items in ``ws.cand``."""
  temperature, num_negatives, similarity, logq_weight = hyper
  assert num_negatives == ws.num_negatives
  b = ws.bpr
  grad(b.users, b.pos, num_negatives, seed, step_index, X, Y, temperature, similarity, _corr(graph, ws, logq_weight),
       ws.raw, ws.cand, b.D, ws.DC, b.g, ws.cvalid, ws.loss, ws.valid_count)
  for t in ws.G + ws.count:
    t.zero_()
  for side, (ids, g, V) in enumerate(((b.users, b.g, b.D), (ws.cand, ws.cvalid, ws.DC))):
    keys, order = sorted_keys(ids, g, ws.G[side].shape[0])
    # (scatter's weight of a roles = 1 entry is -g: the scale -1 undoes it, exactly)
    scatter(keys, order, 1, g, V, -1.0, ws.G[side], ws.count[side])


def _sums_add(sums, ws):
  sums[0] += ws.loss


METHOD = lightgcn.Method(
    "SSM", "train_ssm", MAX_BATCH, 0, skip_layer0=False, gradient=gradient, sums=(((2,), torch.float64),),
    sums_add=_sums_add, entry=lambda v, steps: tuple(x / steps for x in v), workspace=Workspace,
    extra_bytes=extra_bytes,
    opts=lambda temperature, num_negatives, similarity, logq_weight: {"num_negatives": num_negatives})


def step(X, Y, graph, state, ws, seed, step_index, lr, reg, temperature, num_negatives, similarity="cosine",
         logq_weight=0.0):
  """One sampled-softmax step (``lightgcn.method_step``); the draws of the step stay in ``ws.bpr``, the columns'
  items in ``ws.cand``, its two losses in ``ws.loss`` and its valid slots in ``ws.valid_count``."""
  lightgcn.method_step(METHOD, X, Y, graph, state, ws, seed, step_index, lr, reg,
                       (temperature, num_negatives, similarity, logq_weight))


# ---------------------------------------------------------------------- fit
def normalize_rows(table):
  """``table`` row-normalised in place (a row of norm 0 stays 0): after it a dot product ranks by the cosine."""
  n = torch.linalg.vector_norm(table, dim=1, keepdim=True)
  table.div_(torch.where(n > 0, n, torch.ones_like(n)))


def fit(X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg, temperature, num_negatives,
        similarity="cosine", logq_weight=0.0, normalize=False, seed=0, state=None, first_step=None, monitor=None):
  """``lightgcn.method_fit`` of the sampled softmax; with ``normalize`` the model's tables X, Y are left
  row-normalised (the state's base tables are not touched), and a ``monitor`` scores them row-normalised too: what
  a fit ending at that epoch would leave.  Returns (state, one (loss, probability of the
  positive) pair of per-step means per epoch)."""
  state, hist = lightgcn.method_fit(METHOD, X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg,
                                    (temperature, num_negatives, similarity, logq_weight), seed, state, first_step,
                                    monitor, normalize_rows if normalize else None)
  if normalize:
    normalize_rows(X), normalize_rows(Y)
  return state, hist
