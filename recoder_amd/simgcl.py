"""SimGCL (Yu, Yin, Xia, Chen, Cui & Nguyen 2022) for ``MatrixFactorization``, on the rk_als_gcl_* kernels of
librecoder_als.so (include/recoder_als.h) and the graph, scatter and Adam of recoder_amd/lightgcn.py.

The model is a ``MatrixFactorization`` with ``activation_type="none"``; the trainable parameters are the base
tables E0 = (P^0, Q^0) and A is LightGCN's normalised operator over the stored entries.  The clean tables are

    W = (1 / K) sum_{k = 1..K} A^k E0                                (the mean skips layer 0),

view a of a step is W_a = (1 / K) sum_{k = 1..K} L_a^k with L_a^0 = E0 and L_a^k = A L_a^{k-1} + D_a^k, where
D[r] = eps sign(x[r]) u[r] / |u[r]|_2 for x the propagated row and u a counter hash in (0, 1)^h of (seed, step,
view, layer, side, row, column).  A step draws T triples with BPR's sampler and descends

    mean_t softplus(-x_t) at W + cl_weight (NCE_users + NCE_items) + the L2 term of LightGCN,

NCE = (1 / m) sum_r (log sum_s exp(z1_r . z2_s / tau) - z1_r . z2_r / tau) over the m distinct users (positive
items) of the valid triples, z = v / |v| the rows of W_1 and W_2.  The sign is a constant, so all three
tables have the derivative (1 / K) sum_{k >= 1} A^k with respect to E0: the three gradients are summed, propagated
once without noise, and Adam steps both base tables.  8 K propagations a step; cl_weight = 0 runs 4 K.

``Recoder.train_simgcl`` is the public entry point; the functions below are the layer under it (and what the
tests and tools/simgcl_bench.py drive directly).
"""
import torch

from . import _als_lib, als, bpr, lightgcn
from ._lib import ptr
from .bpr import _f32, _i32, _number, _round256
from .device import current_stream
from .lightgcn import _table, new_state  # noqa: F401  (new_state: this module's too)

MAX_H = als.MAX_H                         # rk_als_max_h()
MAX_LAYERS = lightgcn.MAX_LAYERS
MAX_BATCH = _als_lib.GCL_MAX_BATCH        # RK_ALS_GCL_MAX_BATCH: the contrast holds the T x T scores


def check_not_distributed():
  als.check_not_distributed("train_simgcl runs on one GPU: multi-GPU SimGCL is not implemented")


def check_config(model, num_layers, num_epochs, batch_size, lr, reg, cl_weight, cl_eps, cl_temperature, seed):
  """The SimGCL contract, checked before any GPU work; returns (num_layers, num_epochs, batch_size, lr, reg,
  cl_weight, cl_eps, cl_temperature, seed)."""
  c = lightgcn.check_config(model, num_layers, num_epochs, batch_size, lr, reg, seed, METHOD)
  return c[:5] + (_number("cl_weight", cl_weight, False), _number("cl_eps", cl_eps, False),
                  _number("cl_temperature", cl_temperature, True), c[5])


def check_resume(state, num_layers, shapes=None):
  """ValueError unless ``state`` (a ``simgcl_state``) can continue a fit with ``num_layers`` layers on base tables
  of ``shapes``."""
  lightgcn.check_resume(state, num_layers, shapes, method="train_simgcl")


def check_data(nnz, n_items, num_epochs, batch_size):
  return bpr.check_data(nnz, n_items, num_epochs, batch_size, method="train_simgcl")


def contrast_workspace_bytes(T, h):
  """rk_als_gcl_contrast_workspace_bytes(T, h), restated on the host: four [T, h] images, the T x T scores and
  five vectors of T, each rounded up to 64 floats."""
  T, h = int(T), int(h)
  if not (1 <= T <= MAX_BATCH and 1 <= h <= MAX_H):
    return -2
  return 4 * _round256(4 * T * h) + _round256(4 * T * T) + 5 * _round256(4 * T)


def extra_bytes(n_users, n_items, h, T, contrast=True):
  """With ``contrast`` (cl_weight > 0): both views (2 (users + items) h floats), the contrast's workspace and the
  third sort (the positive items: T entries, an int32 key in, a key and an int64 position out, as much again for
  its scratch)."""
  return 2 * (n_users + n_items) * h * 4 + contrast_workspace_bytes(T, h) + 2 * T * (4 + 4 + 8) if contrast else 0


def required_bytes(n_users, n_items, h, nnz, T, contrast=True, allocate_model=True, allocate_state=True,
                   allocate_csrs=True):
  """Device bytes of a fit: what LightGCN's fit holds (``lightgcn.required_bytes``) and ``extra_bytes``."""
  return lightgcn.method_required_bytes(METHOD, n_users, n_items, h, nnz, T, allocate_model, allocate_state,
                                        allocate_csrs, contrast=contrast)


def check_memory(n_users, n_items, h, nnz, T, contrast=True, free_bytes=None, allocate_model=True,
                 allocate_state=True, allocate_csrs=True):
  """``lightgcn.method_check_memory`` of SimGCL."""
  return lightgcn.method_check_memory(METHOD, n_users, n_items, h, nnz, T, free_bytes, allocate_model, allocate_state,
                                      allocate_csrs, contrast=contrast)


# ------------------------------------------------------------------ kernels
def propagate(csr, row_scale, col_scale, F, out=None, acc=None, acc_scale=1.0, eps=0.0, seed=0, step=0, view=0,
              layer=0, side=0, row_lo=0, row_hi=None):
  """``lightgcn.propagate`` with the noise of (seed, step, view, layer, side) and length ``eps`` added to every
  row of ``out`` (and so to what ``acc`` accumulates) in the epilogue (rk_als_gcl_propagate)."""
  lightgcn.propagate(csr, row_scale, col_scale, F, out, acc, acc_scale, row_lo, row_hi,
                     (eps, seed, step, view, layer, side))


def contrast(keys, V1, V2, tau, weight, G1, G2, raw, loss, count):
  """loss[0] = the NCE between the rows of V1 and V2 over the distinct keys inside the table among the sorted
  ``keys``, count[0] = how many there are, and G1 / G2 += weight times its gradient with respect to V1 / V2
  (rk_als_gcl_contrast); ``raw`` is a uint8 workspace of ``contrast_workspace_bytes`` at least."""
  T = keys.shape[0]
  _i32(keys, T), _table(V1), _table(V2, V1.shape[1]), _table(G1, V1.shape[1]), _table(G2, V1.shape[1])
  n_rows, h = V1.shape
  assert V2.shape[0] == G1.shape[0] == G2.shape[0] == n_rows
  assert raw.dtype == torch.uint8 and raw.is_contiguous()
  _f32(loss, (1,))
  _i32(count, 1)
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_gcl_contrast(ptr(keys), T, n_rows, ptr(V1), V1.stride(0), ptr(V2), V2.stride(0), h,
                                         float(tau), float(weight), ptr(G1), G1.stride(0), ptr(G2), G2.stride(0),
                                         ptr(raw), raw.numel(), ptr(loss), ptr(count), current_stream()),
                 "rk_als_gcl_contrast")


# --------------------------------------------------------------------- step
class Workspace(lightgcn.Workspace):
  """LightGCN's workspace and, with ``contrast``, both views, the contrast's workspace and its two results
  (users, items)."""

  def __init__(self, n_users, n_items, T, h, device, contrast=True):
    super().__init__(n_users, n_items, T, h, device)
    self.cl_loss = torch.zeros(2, dtype=torch.float32, device=device)
    self.cl_count = torch.zeros(2, dtype=torch.int32, device=device)
    if contrast:
      f = lambda rows: torch.empty((rows, h), dtype=torch.float32, device=device)
      self.views = ((f(n_users), f(n_items)), (f(n_users), f(n_items)))
      need = _als_lib.load().rk_als_gcl_contrast_workspace_bytes(T, h)
      assert need == contrast_workspace_bytes(T, h) and need > 0, (need, T, h)
      self.raw = torch.empty(need, dtype=torch.uint8, device=device)


def forward(graph, base, num_layers, layers, out, eps=None, seed=0, step=0, view=0):
  """out = the mean over the layers 1..K of ``base`` propagated over ``graph`` (``lightgcn.forward``): the clean
  tables (``eps`` None), or view ``view`` of step ``step`` with noise of length ``eps`` after every layer."""
  lightgcn.forward(graph, base, num_layers, layers, out, True, None if eps is None else (eps, seed, step, view))


def gradient(X, Y, graph, state, ws, seed, step_index, hyper):
  """LightGCN's gradient of the triples and, with cl_weight > 0, that of both contrasts on top of it: 4 K noisy
  propagations and two rk_als_gcl_contrast calls; the two NCE terms (users, items) stay in ``ws.cl_loss``."""
  cl_weight, cl_eps, cl_temperature = hyper
  uk = lightgcn.bpr_gradient(X, Y, ws)
  if cl_weight > 0:
    b = ws.bpr
    for a in (0, 1):
      forward(graph, state["E0"], state["num_layers"], ws.layers, ws.views[a], cl_eps, seed, step_index, a + 1)
    pk = torch.sort(bpr.masked_keys(b.pos, b.neg >= 0, Y.shape[0]))[0]
    for side, keys in enumerate((uk, pk)):
      contrast(keys, ws.views[0][side], ws.views[1][side], cl_temperature, cl_weight, ws.G[side], ws.G[side],
               ws.raw, ws.cl_loss[side:side + 1], ws.cl_count[side:side + 1])


def _sums_add(sums, ws):
  lightgcn.bpr_sums_add(sums, ws)
  sums[2] += ws.cl_loss.sum(dtype=torch.float64)


METHOD = lightgcn.Method(
    "SimGCL", "train_simgcl", MAX_BATCH, 1, skip_layer0=True, gradient=gradient,
    sums=lightgcn.BPR_SUMS + (((), torch.float64),), sums_add=_sums_add,
    entry=lambda v, steps: (v[0] / v[1] if v[1] else float("nan"), v[2] / steps),
    workspace=Workspace, extra_bytes=extra_bytes,
    opts=lambda cl_weight, cl_eps, cl_temperature: {"contrast": cl_weight > 0})


def step(X, Y, graph, state, ws, seed, step_index, lr, reg, cl_weight, cl_eps, cl_temperature):
  """One SimGCL step (``lightgcn.method_step``): X / Y receive the clean tables; the triples, g and loss of the
  step stay in ``ws.bpr``, the two NCE terms (users, items) in ``ws.cl_loss``."""
  lightgcn.method_step(METHOD, X, Y, graph, state, ws, seed, step_index, lr, reg, (cl_weight, cl_eps, cl_temperature))


# ---------------------------------------------------------------------- fit
def fit(X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg, cl_weight, cl_eps, cl_temperature,
        seed=0, state=None, first_step=None, monitor=None):
  """``lightgcn.method_fit`` of SimGCL.  Returns (state, one (mean BPR loss per valid triple, mean NCE_users +
  NCE_items per step) pair per epoch)."""
  return lightgcn.method_fit(METHOD, X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg,
                             (cl_weight, cl_eps, cl_temperature), seed, state, first_step, monitor)
