"""DirectAU (Wang, Yu, Wang, Zhang & Ma 2022) for ``MatrixFactorization``, on rk_als_dau_grad of librecoder_als.so
(include/recoder_als.h) and the sampler, graph, scatter and Adam of recoder_amd/bpr.py and recoder_amd/lightgcn.py.

The model is a ``MatrixFactorization`` with ``activation_type="none"``; the trainable parameters are the base
tables E0 = (P^0, Q^0) and the final tables (X, Y) are LightGCN's: the mean over the layers 0..K of E0 propagated
over the normalised graph of the stored entries (K = 0: the base tables themselves, the paper's DirectAU-MF).  A
step draws T slots (u_t, i_t) with BPR's sampler -- the negative of the draw is ignored -- and descends

    (1 / m) sum_t |a_t - b_t|^2 + (gamma / 2) (unif(a) + unif(b)) + the L2 term of LightGCN,
    unif(z) = log(2 / (m (m - 1)) sum_{p < q} exp(-2 |z_p - z_q|^2)),

a_t = X[u_t] / |X[u_t]| and b_t = Y[i_t] / |Y[i_t]| over the m slots whose ids lie in the tables; a repeated user
or item is a slot of its own, as in the paper's code.  No negatives are drawn.  rk_als_dau_grad leaves the
gradient rows per slot, rk_als_lgcn_scatter sums them per row, one ``lightgcn.forward`` propagates them back and
Adam steps both base tables.  2 K propagations forward and 2 K back a step.

``Recoder.train_directau`` is the public entry point; the functions below are the layer under it (and what the
tests and tools/directau_bench.py drive directly).
"""
import torch

from . import _als_lib, als, bpr, lightgcn, simgcl
from ._lib import ptr
from .bpr import _f32, _i32, _number
from .device import current_stream
from .lightgcn import _table, new_state, scatter  # noqa: F401  (new_state: this module's too)

MAX_H = als.MAX_H                         # rk_als_max_h()
MAX_LAYERS = lightgcn.MAX_LAYERS
MAX_BATCH = _als_lib.GCL_MAX_BATCH        # RK_ALS_GCL_MAX_BATCH: the workspace holds one T x T tile


def check_not_distributed():
  """ValueError under more than one rank."""
  try:
    als.check_not_distributed("train_directau runs on one GPU: multi-GPU DirectAU is not implemented")
  except NotImplementedError as e:
    raise ValueError(str(e)) from None


def check_config(model, num_layers, num_epochs, batch_size, lr, reg, gamma, seed):
  """The DirectAU contract, checked before any GPU work; returns (num_layers, num_epochs, batch_size, lr, reg,
  gamma, seed).  ``num_layers`` may be 0."""
  c = lightgcn.check_config(model, num_layers, num_epochs, batch_size, lr, reg, seed, METHOD)
  return c[:5] + (_number("gamma", gamma, False), c[5])


def check_resume(state, num_layers, shapes=None):
  """ValueError unless ``state`` (a ``directau_state``) can continue a fit with ``num_layers`` layers on base
  tables of ``shapes``."""
  lightgcn.check_resume(state, num_layers, shapes, method="train_directau")


def check_data(nnz, n_items, num_epochs, batch_size):
  return bpr.check_data(nnz, n_items, num_epochs, batch_size, method="train_directau")


def grad_workspace_bytes(T, h):
  """rk_als_dau_workspace_bytes(T, h), restated on the host: the contrast's layout (four [T, h] images, the T x T
  tile, five vectors of T) and 64 floats for the two coefficients."""
  base = simgcl.contrast_workspace_bytes(T, h)
  return base if base < 0 else base + 256


def extra_bytes(n_users, n_items, h, T):
  """The workspace of rk_als_dau_grad, the three losses and the count, and the keys of the two sorts of T entries
  this step makes itself (an int32 key in, a key and an int64 position out, as much again for its scratch)."""
  return grad_workspace_bytes(T, h) + 16 + 2 * 2 * T * (4 + 4 + 8)


def required_bytes(n_users, n_items, h, nnz, T, allocate_model=True, allocate_state=True, allocate_csrs=True):
  """Device bytes of a fit: what LightGCN's fit holds (``lightgcn.required_bytes``: its BPR workspace is where
  the draws, the validity vector and both [T, h] gradient images live) and ``extra_bytes``."""
  return lightgcn.method_required_bytes(METHOD, n_users, n_items, h, nnz, T, allocate_model, allocate_state,
                                        allocate_csrs)


def check_memory(n_users, n_items, h, nnz, T, free_bytes=None, allocate_model=True, allocate_state=True,
                 allocate_csrs=True):
  """``lightgcn.method_check_memory`` of DirectAU."""
  return lightgcn.method_check_memory(METHOD, n_users, n_items, h, nnz, T, free_bytes, allocate_model, allocate_state,
                                      allocate_csrs)


# ------------------------------------------------------------------ kernels
def grad(users, items, X, Y, gamma, raw, DU, DI, valid, loss, count):
  """DU / DI [T, h] = the gradient rows of the slots (``users``, ``items``) at the tables X / Y, ``valid`` [T]
  = 1.0 / 0.0, ``loss`` [3] = (alignment, uniformity of the users' rows, of the items' rows) and ``count`` [1] = the
  valid slots (rk_als_dau_grad); ``raw`` is a uint8 workspace of ``grad_workspace_bytes`` at least."""
  T = users.shape[0]
  _i32(users, T), _i32(items, T), _table(X), _table(Y, X.shape[1])
  h = X.shape[1]
  _f32(DU, (T, h)), _f32(DI, (T, h)), _f32(valid, (T,)), _f32(loss, (3,)), _i32(count, 1)
  assert raw.dtype == torch.uint8 and raw.is_contiguous()
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_dau_grad(ptr(users), ptr(items), T, X.shape[0], Y.shape[0], ptr(X), X.stride(0), ptr(Y),
                                     Y.stride(0), h, float(gamma), ptr(raw), raw.numel(), ptr(DU), ptr(DI),
                                     ptr(valid), ptr(loss), ptr(count), current_stream()), "rk_als_dau_grad")


# --------------------------------------------------------------------- step
class Workspace(lightgcn.Workspace):
  """LightGCN's workspace (the draws in ``bpr.users`` / ``bpr.pos``, the validity vector in ``bpr.g``, the
  gradient images DU / DI in ``bpr.D`` / ``bpr.P``), the workspace of rk_als_dau_grad and its results."""

  def __init__(self, n_users, n_items, T, h, device):
    super().__init__(n_users, n_items, T, h, device)
    need = _als_lib.load().rk_als_dau_workspace_bytes(T, h)
    assert need == grad_workspace_bytes(T, h) and need > 0, (need, T, h)
    self.raw = torch.empty(need, dtype=torch.uint8, device=device)
    self.loss = torch.zeros(3, dtype=torch.float32, device=device)
    self.valid_count = torch.zeros(1, dtype=torch.int32, device=device)


def sorted_keys(ids, valid, n_rows):
  """(keys, order) of one side's T slots, stably sorted by row on the device; an invalid slot carries the key
  past the table."""
  return torch.sort(bpr.masked_keys(ids, valid > 0, n_rows), stable=True)


def gradient(X, Y, graph, state, ws, seed, step_index, hyper):
  """rk_als_dau_grad at the draws (the negative is ignored) and the sum of its rows per table row; the three losses
  of the step stay in ``ws.loss`` and its valid slots in ``ws.valid_count``."""
  b = ws.bpr
  grad(b.users, b.pos, X, Y, hyper[0], ws.raw, b.D, b.P, b.g, ws.loss, ws.valid_count)
  for t in ws.G + ws.count:
    t.zero_()
  for side, (ids, V) in enumerate(((b.users, b.D), (b.pos, b.P))):
    keys, order = sorted_keys(ids, b.g, ws.G[side].shape[0])
    # (scatter's weight of a roles = 1 entry is -g_t: the scale -1 undoes it, exactly)
    scatter(keys, order, 1, b.g, V, -1.0, ws.G[side], ws.count[side])


def _sums_add(sums, ws):
  sums[0] += ws.loss


METHOD = lightgcn.Method(
    "DirectAU", "train_directau", MAX_BATCH, 0, skip_layer0=False, gradient=gradient, sums=(((3,), torch.float64),),
    sums_add=_sums_add, entry=lambda v, steps: tuple(x / steps for x in v), workspace=Workspace, extra_bytes=extra_bytes)


def step(X, Y, graph, state, ws, seed, step_index, lr, reg, gamma):
  """One DirectAU step (``lightgcn.method_step``); the draws of the step stay in ``ws.bpr``, its three losses in
  ``ws.loss`` and its valid slots in ``ws.valid_count``."""
  lightgcn.method_step(METHOD, X, Y, graph, state, ws, seed, step_index, lr, reg, (gamma,))


# ---------------------------------------------------------------------- fit
def fit(X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg, gamma, seed=0, state=None,
        first_step=None, monitor=None):
  """``lightgcn.method_fit`` of DirectAU.  Returns (state, one (alignment, uniformity of the users, uniformity of the
  items) triple of per-step means per epoch)."""
  return lightgcn.method_fit(METHOD, X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg, (gamma,),
                             seed, state, first_step, monitor)
