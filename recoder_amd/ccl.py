"""SimpleX's cosine contrastive loss (CCL; Mao, Zhu, Wang, Dai, Dong, Xiao & He, CIKM 2021, "SimpleX: A Simple and
Strong Baseline for Collaborative Filtering") for ``MatrixFactorization``, on rk_als_ccl_grad and rk_als_ccl_scatter
of librecoder_als.so (include/recoder_als.h), the sampler of recoder_amd/bpr.py and the scatter, Adam and driver of
recoder_amd/lightgcn.py.

The model is a ``MatrixFactorization`` with ``activation_type="none"``; the trainable parameters are the base tables
E0 = (P^0, Q^0) and the final tables (X, Y) are LightGCN's: the mean over the layers 0..K of E0 propagated over the
normalised graph of the stored entries (K = 0: the base tables themselves).  A step draws T slots (u_t, i_t) with
BPR's sampler -- the negative of the draw is ignored -- and R items j_t1 .. j_tR per slot uniformly from the
catalogue (UltraGCN's draws: a counter hash of (seed, step, t R + r); nothing rejected), and descends the mean over
the valid slots of

    L_t = (1 - c_ui) + (negative_weight / R) sum_r max(0, c_uj_r - margin),    c_ux = cos(X[u], Y[x]),

plus the driver's L2 term on the base rows a slot touches as user or as positive.  A row of norm 0 normalises to the
zero vector and gets no gradient.  The hinge kills most negatives: rk_als_ccl_grad leaves the E = 1 + R candidates of
every slot with two coefficients and a key, the item where the entry carries a gradient and a sentinel past the table
where it does not, so that the sort puts the dead entries last and rk_als_ccl_scatter walks the live ones only;
rk_als_lgcn_scatter sums the users' rows; one ``lightgcn.forward`` propagates both back and Adam steps the base
tables.  This module is SimpleX's loss alone: the pooling of a user's history into the user's vector is
recoder_amd/simplex.py (``Recoder.train_simplex``), which runs this loss at pooled user rows; the embedding dropout
and the attention poolings are not built.

``Recoder.train_ccl`` is the public entry point; the functions below are the layer under it (and what the tests and
tools/ccl_bench.py drive directly).
"""
import numbers

import torch

from . import _als_lib, als, bpr, lightgcn
from ._lib import ptr
from .bpr import _carve, _count, _f32, _i32, _number, _round256
from .device import current_stream
from .lightgcn import _table, new_state  # noqa: F401  (new_state: this module's too)
from .ssm import normalize_rows
from .ultragcn import check_entries

MAX_H = als.MAX_H                                   # rk_als_max_h()
MAX_LAYERS = lightgcn.MAX_LAYERS
MAX_BATCH = _als_lib.CCL_MAX_BATCH                  # RK_ALS_CCL_MAX_BATCH
MAX_NEGATIVES = _als_lib.CCL_MAX_NEGATIVES          # RK_ALS_CCL_MAX_NEGATIVES
MAX_ENTRIES = _als_lib.CCL_MAX_ENTRIES              # RK_ALS_CCL_MAX_ENTRIES: T (1 + R) at most
LONG_KEY = _als_lib.UGCN_LONG_KEY                   # RK_ALS_UGCN_LONG_KEY: the scatter's walk is UltraGCN's


def check_not_distributed():
  """ValueError under more than one rank."""
  try:
    als.check_not_distributed("train_ccl runs on one GPU: multi-GPU CCL training is not implemented")
  except NotImplementedError as e:
    raise ValueError(str(e)) from None


def check_config(model, num_layers, num_epochs, batch_size, lr, reg, num_negatives, negative_weight, margin, normalize,
                 seed):
  """The contract of ``train_ccl``, checked before any GPU work; returns (num_layers, num_epochs, batch_size, lr, reg,
  num_negatives, negative_weight, margin, normalize, seed).  ``num_layers`` may be 0."""
  c = lightgcn.check_config(model, num_layers, num_epochs, batch_size, lr, reg, seed, METHOD)
  R = _count("num_negatives", num_negatives, 1, MAX_NEGATIVES)
  if c[2] * (1 + R) > MAX_ENTRIES:
    raise ValueError("batch_size * (1 + num_negatives) must be at most %d (got %d * %d)" % (MAX_ENTRIES, c[2], 1 + R))
  if isinstance(margin, bool) or not isinstance(margin, numbers.Real) or not -1.0 <= margin < 1.0:
    raise ValueError("margin must be a number in [-1, 1) (got %r)" % (margin,))
  return c[:5] + (R, _number("negative_weight", negative_weight, False), float(margin), bool(normalize), c[5])


def check_resume(state, num_layers, shapes=None):
  """ValueError unless ``state`` (a ``ccl_state``) can continue a fit with ``num_layers`` layers on base tables of
  ``shapes``."""
  lightgcn.check_resume(state, num_layers, shapes, method="train_ccl")


def check_data(nnz, n_items, num_epochs, batch_size):
  return bpr.check_data(nnz, n_items, num_epochs, batch_size, method="train_ccl")


def workspace_bytes(T, R, h):
  """rk_als_ccl_workspace_bytes(T, R, h), restated on the host: cand, key, coef and self [T, E], loss [T, 2] and live
  [T], each rounded up to 256 bytes."""
  T, R, h = int(T), int(R), int(h)
  if not (1 <= T <= MAX_BATCH and 1 <= R <= MAX_NEGATIVES and 1 <= h <= MAX_H):
    return -2
  n = T * (1 + R)
  if n > MAX_ENTRIES:
    return -2
  return 4 * _round256(4 * n) + _round256(8 * T) + _round256(4 * T)


def extra_bytes(n_users, n_items, h, T, num_negatives=1):
  """On top of ``lightgcn.required_bytes``: the step's buffers and the keys of the sort of the T E entries (an int32
  key in, a key and an int64 position out, as much again for its scratch) and of the T users."""
  E = 1 + int(num_negatives)
  return workspace_bytes(T, num_negatives, h) + 2 * (T * E + T) * (4 + 4 + 8)


def required_bytes(n_users, n_items, h, nnz, T, num_negatives=1, allocate_model=True, allocate_state=True,
                   allocate_csrs=True):
  """Device bytes of a fit: what the driver holds (``lightgcn.required_bytes``) and ``extra_bytes``."""
  return lightgcn.method_required_bytes(METHOD, n_users, n_items, h, nnz, T, allocate_model, allocate_state,
                                        allocate_csrs, num_negatives=num_negatives)


def check_memory(n_users, n_items, h, nnz, T, num_negatives=1, free_bytes=None, allocate_model=True,
                 allocate_state=True, allocate_csrs=True):
  """``lightgcn.method_check_memory`` of CCL."""
  return lightgcn.method_check_memory(METHOD, n_users, n_items, h, nnz, T, free_bytes, allocate_model, allocate_state,
                                      allocate_csrs, num_negatives=num_negatives)


# ------------------------------------------------------------------ kernels
def _entries(t, T, E, dtype):
  assert t.dtype == dtype and tuple(t.shape) == (T, E) and t.is_contiguous(), (t.dtype, t.shape, t.stride())


def grad(users, items, num_negatives, seed, step_index, X, Y, margin, negative_weight, cand, key, coef, self_, DU, valid,
         loss, live):
  """``cand`` / ``key`` / ``coef`` / ``self_`` [T, E] = the E = 1 + ``num_negatives`` candidates of the slots
  (``users``, ``items``), the item of an entry that carries a gradient (else the sentinel, the items' row count) and
  its two coefficients, ``DU`` [T, h] the users' gradient rows, ``valid`` [T] = 1.0 / 0.0, ``loss`` [T, 2] the two
  terms of L_t and ``live`` [T] the slots' live negatives (rk_als_ccl_grad)."""
  T, R = users.shape[0], int(num_negatives)
  if workspace_bytes(T, R, X.shape[1]) < 0:
    raise ValueError("rk_als_ccl_grad needs 1 <= T <= %d, 1 <= R <= %d, T (1 + R) <= %d and 1 <= h <= %d (got T = %d, "
                     "R = %d, h = %d)" % (MAX_BATCH, MAX_NEGATIVES, MAX_ENTRIES, MAX_H, T, R, X.shape[1]))
  E = 1 + R
  _i32(users, T), _i32(items, T), _table(X), _table(Y, X.shape[1])
  h = X.shape[1]
  _entries(cand, T, E, torch.int32), _entries(key, T, E, torch.int32)
  _f32(coef, (T, E)), _f32(self_, (T, E)), _f32(DU, (T, h)), _f32(valid, (T,)), _f32(loss, (T, 2)), _i32(live, T)
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_ccl_grad(ptr(users), ptr(items), T, R, int(seed), int(step_index), X.shape[0], Y.shape[0],
                                     ptr(X), X.stride(0), ptr(Y), Y.stride(0), h, float(margin),
                                     float(negative_weight), ptr(cand), ptr(key), ptr(coef), ptr(self_), ptr(DU),
                                     ptr(valid), ptr(loss), ptr(live), current_stream()), "rk_als_ccl_grad")


def scatter(keys, order, E, users, coef, self_, X, Y, scale, G, count):
  """G[key] = scale (sum coef[e] X[users[e / E]] - (sum self_[e]) Y[key]) and count[key] = the key's positives, for
  the rows among the sorted keys (rk_als_ccl_scatter); the caller zeroes G and count."""
  n, E = check_entries("rk_als_ccl_scatter", keys, order, E, users, (coef, self_), X, G, count, MAX_BATCH, MAX_ENTRIES,
                       1 + MAX_NEGATIVES)
  _table(Y, X.shape[1])
  assert Y.shape[0] >= G.shape[0], (Y.shape, G.shape)
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_ccl_scatter(ptr(keys), ptr(order), n, E, ptr(users), ptr(coef), ptr(self_), ptr(X),
                                        X.stride(0), X.shape[0], ptr(Y), Y.stride(0), X.shape[1], float(scale),
                                        G.shape[0], ptr(G), G.stride(0), ptr(count), current_stream()),
                 "rk_als_ccl_scatter")


# --------------------------------------------------------------------- step
class Workspace(lightgcn.Workspace):
  """The driver's workspace (the draws in ``bpr.users`` / ``bpr.pos``, the validity vector in ``bpr.g``, the users'
  gradient image DU in ``bpr.D``) and one allocation of rk_als_ccl_workspace_bytes cut into ``cand``, ``key``,
  ``coef``, ``self_``, ``loss`` and ``live``."""

  def __init__(self, n_users, n_items, T, h, device, num_negatives=1):
    super().__init__(n_users, n_items, T, h, device)
    R = int(num_negatives)
    need = _als_lib.load().rk_als_ccl_workspace_bytes(T, R, h)
    assert need == workspace_bytes(T, R, h) and need > 0, (need, T, R, h)
    self.num_negatives = R
    E = 1 + R
    self.raw = torch.empty(need, dtype=torch.uint8, device=device)
    self.cand, self.key, self.coef, self.self_, self.loss, self.live = _carve(
        self.raw, *[(torch.int32, (T, E))] * 2, *[(torch.float32, (T, E))] * 2, (torch.float32, (T, 2)),
        (torch.int32, (T,)))


def gradient(X, Y, graph, state, ws, seed, step_index, hyper):
  """rk_als_ccl_grad at the draws (the negative is ignored), then the users' rows summed per user by
  rk_als_lgcn_scatter and the live entries' per item by rk_als_ccl_scatter; the slots' two terms stay in ``ws.loss``
  and their live negatives in ``ws.live``."""
  num_negatives, negative_weight, margin = hyper
  assert num_negatives == ws.num_negatives
  b = ws.bpr
  grad(b.users, b.pos, num_negatives, seed, step_index, X, Y, margin, negative_weight, ws.cand, ws.key, ws.coef,
       ws.self_, b.D, b.g, ws.loss, ws.live)
  for t in ws.G + ws.count:
    t.zero_()
  keys, order = torch.sort(bpr.masked_keys(b.users, b.g > 0, X.shape[0]), stable=True)
  # (scatter's weight of a roles = 1 entry is -g: the negative scale undoes it, exactly)
  lightgcn.scatter(keys, order, 1, b.g, b.D, -1.0 / b.T, ws.G[0], ws.count[0])
  keys, order = torch.sort(ws.key.view(-1), stable=True)
  scatter(keys, order, ws.key.shape[1], b.users, ws.coef, ws.self_, X, Y, 1.0 / b.T, ws.G[1], ws.count[1])


def _sums_add(sums, ws):
  sums[0] += ws.loss.sum(0, dtype=torch.float64)
  sums[1] += ws.bpr.g.sum(dtype=torch.float64)
  sums[2] += ws.live.sum(dtype=torch.int64)


def _entry(v, steps):
  """(positive term, negative term, live negatives) means per valid slot; ``fit`` turns the last into a share."""
  return tuple(x / v[2] for x in (v[0], v[1], v[3])) if v[2] else (float("nan"),) * 3


METHOD = lightgcn.Method(
    "CCL", "train_ccl", MAX_BATCH, 0, skip_layer0=False, gradient=gradient,
    sums=(((2,), torch.float64), ((), torch.float64), ((), torch.int64)), sums_add=_sums_add, entry=_entry,
    workspace=Workspace, extra_bytes=extra_bytes,
    opts=lambda num_negatives, negative_weight, margin: {"num_negatives": num_negatives})


def step(X, Y, graph, state, ws, seed, step_index, lr, reg, num_negatives, negative_weight, margin):
  """One CCL step (``lightgcn.method_step``); the draws of the step stay in ``ws.bpr``, its candidates in ``ws.cand``
  / ``ws.key`` / ``ws.coef`` / ``ws.self_``, the slots' terms in ``ws.loss`` and their live negatives in ``ws.live``."""
  lightgcn.method_step(METHOD, X, Y, graph, state, ws, seed, step_index, lr, reg,
                       (num_negatives, negative_weight, margin))


# ---------------------------------------------------------------------- fit
def fit(X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg, num_negatives, negative_weight, margin,
        normalize=False, seed=0, state=None, first_step=None, monitor=None):
  """``lightgcn.method_fit`` of CCL; with ``normalize`` the model's tables X, Y are left row-normalised (the state's
  base tables are not touched), and a ``monitor`` scores them row-normalised too: what a fit ending at that epoch
  would leave.  Returns (state, one (positive term, negative term) pair of means per valid slot per epoch); the mean
  share of live negatives of each epoch of this call is kept in ``state["live_share"]``."""
  state, hist = lightgcn.method_fit(METHOD, X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg,
                                    (num_negatives, negative_weight, margin), seed, state, first_step, monitor,
                                    normalize_rows if normalize else None)
  if normalize:
    normalize_rows(X), normalize_rows(Y)
  state["live_share"] = [e[2] / num_negatives for e in hist]
  return state, [e[:2] for e in hist]
