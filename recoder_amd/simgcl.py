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
from .bpr import _f32, _i32, _number
from .device import DEVICE_HBM_BYTES, current_stream
from .lightgcn import _table, adam, new_state, scatter

MAX_H = als.MAX_H                         # rk_als_max_h()
MAX_LAYERS = lightgcn.MAX_LAYERS
MAX_BATCH = _als_lib.GCL_MAX_BATCH        # RK_ALS_GCL_MAX_BATCH: the contrast holds the T x T scores


def check_not_distributed():
  als.check_not_distributed("train_simgcl runs on one GPU: multi-GPU SimGCL is not implemented")


def check_config(model, num_layers, num_epochs, batch_size, lr, reg, cl_weight, cl_eps, cl_temperature, seed):
  """The SimGCL contract, checked before any GPU work; returns (num_layers, num_epochs, batch_size, lr, reg,
  cl_weight, cl_eps, cl_temperature, seed)."""
  c = lightgcn.check_config(model, num_layers, num_epochs, batch_size, lr, reg, seed, method="train_simgcl",
                            max_batch=MAX_BATCH)
  return c[:5] + (_number("cl_weight", cl_weight, False), _number("cl_eps", cl_eps, False),
                  _number("cl_temperature", cl_temperature, True), c[5])


def check_resume(state, num_layers, shapes=None):
  """ValueError unless ``state`` (a ``simgcl_state``) can continue a fit with ``num_layers`` layers on base tables
  of ``shapes``."""
  lightgcn.check_resume(state, num_layers, shapes, method="train_simgcl")


def check_data(nnz, n_items, num_epochs, batch_size):
  return bpr.check_data(nnz, n_items, num_epochs, batch_size, method="train_simgcl")


def _round256(x):
  return -(-int(x) // 256) * 256


def contrast_workspace_bytes(T, h):
  """rk_als_gcl_contrast_workspace_bytes(T, h), restated on the host: four [T, h] images, the T x T scores and
  five vectors of T, each rounded up to 64 floats."""
  T, h = int(T), int(h)
  if not (1 <= T <= MAX_BATCH and 1 <= h <= MAX_H):
    return -2
  return 4 * _round256(4 * T * h) + _round256(4 * T * T) + 5 * _round256(4 * T)


def required_bytes(n_users, n_items, h, nnz, T, contrast=True, allocate_model=True, allocate_state=True,
                   allocate_csrs=True):
  """Device bytes of a fit: what LightGCN's fit holds (``lightgcn.required_bytes``) and, with ``contrast``
  (cl_weight > 0), both views (2 (users + items) h floats), the contrast's workspace and the third sort (the
  positive items: T entries, an int32 key in, a key and an int64 position out, as much again for its scratch)."""
  base = lightgcn.required_bytes(n_users, n_items, h, nnz, T, allocate_model, allocate_state, allocate_csrs)
  if not contrast:
    return base
  return base + 2 * (int(n_users) + int(n_items)) * int(h) * 4 + contrast_workspace_bytes(T, h) + \
      2 * int(T) * (4 + 4 + 8)


def check_memory(n_users, n_items, h, nnz, T, contrast=True, free_bytes=None, allocate_model=True,
                 allocate_state=True, allocate_csrs=True):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's whole HBM
  without touching a device, then (``free_bytes`` None: asked from the current device) against what is free."""
  n_users, n_items, h, nnz, T = int(n_users), int(n_items), int(h), int(nnz), int(T)
  if contrast_workspace_bytes(T, h) < 0:
    raise ValueError("SimGCL needs 1 <= batch_size <= %d and 1 <= h <= %d (got %d, %d)" % (MAX_BATCH, MAX_H, T, h))
  whole = required_bytes(n_users, n_items, h, nnz, T, contrast)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError("SimGCL over %d users x %d items at h = %d with %d entries and batches of %d needs %d bytes: "
                     "more than one device's memory (%d bytes); multi-device fits are not implemented"
                     % (n_users, n_items, h, nnz, T, whole, DEVICE_HBM_BYTES))
  need = required_bytes(n_users, n_items, h, nnz, T, contrast, allocate_model, allocate_state, allocate_csrs)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("SimGCL over %d users x %d items at h = %d with %d entries and batches of %d needs %d bytes "
                     "of device memory, %d are free" % (n_users, n_items, h, nnz, T, need, free_bytes))
  return need


# ------------------------------------------------------------------ kernels
def propagate(csr, row_scale, col_scale, F, out=None, acc=None, acc_scale=1.0, eps=0.0, seed=0, step=0, view=0,
              layer=0, side=0, row_lo=0, row_hi=None):
  """``lightgcn.propagate`` with the noise of (seed, step, view, layer, side) and length ``eps`` added to every
  row of ``out`` (and so to what ``acc`` accumulates) in the epilogue (rk_als_gcl_propagate)."""
  rows, cols = csr.shape
  row_hi = rows if row_hi is None else row_hi
  _table(F)
  h = F.shape[1]
  assert F.shape[0] == cols and 0 <= row_lo <= row_hi <= rows and (out is not None or acc is not None)
  _f32(row_scale, (rows,)), _f32(col_scale, (cols,))
  for t in (out, acc):
    if t is not None:
      _table(t, h)
      assert t.shape[0] == rows and t.data_ptr() != F.data_ptr()
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_gcl_propagate(
      ptr(csr.indptr), ptr(csr.indices), ptr(row_scale), ptr(col_scale), row_lo, row_hi, ptr(F), F.stride(0), h,
      ptr(out), out.stride(0) if out is not None else 0, ptr(acc), acc.stride(0) if acc is not None else 0,
      float(acc_scale), float(eps), int(seed), int(step), int(view), int(layer), int(side), current_stream()),
      "rk_als_gcl_propagate")


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
  """out = the mean over the layers 1..K of ``base`` propagated over ``graph``: the clean tables (``eps`` None,
  rk_als_lgcn_propagate), or view ``view`` of step ``step`` with noise of length ``eps`` after every layer.  2 K
  propagations; the mean is formed in their epilogues."""
  out[0].zero_()
  out[1].zero_()
  cur = base
  for k in range(num_layers):
    last = k == num_layers - 1
    nxt = (None, None) if last else layers[k % 2]
    scale = 1.0 / num_layers if last else 1.0
    for side, (csr, rs, cs) in enumerate(((graph.ucsr, graph.su, graph.si), (graph.icsr, graph.si, graph.su))):
      if eps is None:
        lightgcn.propagate(csr, rs, cs, cur[1 - side], nxt[side], out[side], scale)
      else:
        propagate(csr, rs, cs, cur[1 - side], nxt[side], out[side], scale, eps, seed, step, view, k + 1, side)
    cur = nxt


def step(X, Y, graph, state, ws, seed, step_index, lr, reg, cl_weight, cl_eps, cl_temperature):
  """One SimGCL step: the state's base tables and moments move, X / Y receive the clean tables of the base tables
  as they were at the START of the step; the triples, g and loss of the step stay in ``ws.bpr``, the two NCE
  terms (users, items) in ``ws.cl_loss``."""
  K, b = state["num_layers"], ws.bpr
  T = b.T
  E0 = state["E0"]
  forward(graph, E0, K, ws.layers, (X, Y))
  bpr.sample(graph.ucsr, seed, step_index, b.users, b.pos, b.neg)
  bpr.grad(b.users, b.pos, b.neg, X, Y, ws.zero_bias, b.g, b.loss, b.D, b.P)
  (uk, uo), (ik, io) = bpr.sorted_keys(b.users, b.pos, b.neg, X.shape[0], Y.shape[0])
  for t in ws.G + ws.count:
    t.zero_()
  scatter(uk, uo, 1, b.g, b.D, 1.0 / T, ws.G[0], ws.count[0])
  scatter(ik, io, 2, b.g, b.P, 1.0 / T, ws.G[1], ws.count[1])
  if cl_weight > 0:
    for a in (0, 1):
      forward(graph, E0, K, ws.layers, ws.views[a], cl_eps, seed, step_index, a + 1)
    pk = torch.sort(torch.where(b.neg >= 0, b.pos, torch.full_like(b.pos, Y.shape[0])))[0]
    for side, keys in enumerate((uk, pk)):
      contrast(keys, ws.views[0][side], ws.views[1][side], cl_temperature, cl_weight, ws.G[side], ws.G[side],
               ws.raw, ws.cl_loss[side:side + 1], ws.cl_count[side:side + 1])
  forward(graph, ws.G, K, ws.layers, ws.H)
  state["step"] += 1
  for side in (0, 1):
    adam(E0[side], ws.H[side], ws.count[side], reg / T, state["M"][side], state["V"][side], lr, state["step"])


# ---------------------------------------------------------------------- fit
def fit(X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg, cl_weight, cl_eps, cl_temperature,
        seed=0, state=None, first_step=None):
  """num_epochs epochs of ceil(nnz / batch_size) steps, in the manner of ``lightgcn.fit`` (``state``,
  ``first_step``, the tables, the bias and the one host synchronisation per epoch as there).  Returns (state,
  one (mean BPR loss per valid triple, mean NCE_users + NCE_items per step) pair per epoch)."""
  steps = check_data(ucsr.nnz, ucsr.shape[1], num_epochs, batch_size)
  if state is not None:
    check_resume(state, num_layers, (X.shape, Y.shape))
  on = cl_weight > 0
  check_memory(X.shape[0], Y.shape[0], X.shape[1], ucsr.nnz, batch_size, on, allocate_model=False,
               allocate_state=state is None, allocate_csrs=False)
  if state is None:
    state = new_state(X, Y, num_layers)
  graph = lightgcn.Graph(ucsr, icsr)
  ws = Workspace(X.shape[0], Y.shape[0], int(batch_size), X.shape[1], X.device, on)
  bias.zero_()
  hist = []
  s = state["step"] if first_step is None else int(first_step)
  for _ in range(num_epochs):
    total = torch.zeros((), dtype=torch.float64, device=X.device)
    cl = torch.zeros((), dtype=torch.float64, device=X.device)
    count = torch.zeros((), dtype=torch.int64, device=X.device)
    for _ in range(steps):
      step(X, Y, graph, state, ws, seed, s, lr, reg, cl_weight, cl_eps, cl_temperature)
      total += ws.bpr.loss.sum(dtype=torch.float64)
      cl += ws.cl_loss.sum(dtype=torch.float64)
      count += (ws.bpr.neg >= 0).sum()
      s += 1
    total, cl, count = torch.stack([total, cl, count.double()]).cpu().tolist()      # (the synchronisation)
    hist.append((total / count if count else float("nan"), cl / steps))
  forward(graph, state["E0"], state["num_layers"], ws.layers, (X, Y))
  return state, hist
