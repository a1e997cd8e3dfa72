"""LightGCN (He, Deng, Wang, Li, Zhang & Wang 2020) for ``MatrixFactorization``, on the rk_als_lgcn_* kernels of
librecoder_als.so (include/recoder_als.h) and the BPR sampler and triple gradient of recoder_amd/bpr.py.

The model is a ``MatrixFactorization`` with ``activation_type="none"``.  The trainable parameters are the base
tables E0 = (P^0 [users, h], Q^0 [items, h]); the stored entries of the interaction matrix are the edges of a
bipartite graph (their values play no part).  With r_u the items of user u, d_i the users of item i and
s = degree^-1/2 (0 for degree 0),

    P^{k+1}[u] = s_u sum_{i in u} s_i Q^k[i],    Q^{k+1}[i] = s_i sum_{u in i} s_u P^k[u],
    P = (1 / (K + 1)) sum_{k <= K} P^k,          Q likewise,

and a user scores p_u . q_i: what the fit leaves in the model's tables is (P, Q) with a zero bias, an ordinary
``MatrixFactorization`` state.  One step draws T triples with BPR's sampler, takes g_t = sigma(-x_t) at the
final tables, forms the gradient Gf with respect to them (divided by T), propagates it back -- the operator is
symmetric, so the backward pass is the forward pass applied to Gf -- adds the L2 term (reg / T) c_row E0[row]
and takes one Adam step on both base tables.

``Recoder.train_lightgcn`` is the public entry point; the functions below are the layer under it (and what
the tests and tools/lightgcn_bench.py drive directly).

SimGCL (recoder_amd/simgcl.py) and DirectAU (recoder_amd/directau.py) train the same base tables over the same
graph with the same sampler, backward propagation and Adam: the one memory check, step and fit of all three are
``method_check_memory``, ``method_step`` and ``method_fit`` below, and a ``Method`` says what differs.
"""
import collections

import numpy as np
import torch

from . import _als_lib, als, bpr
from ._lib import ptr
from .bpr import _count, _f32, _i32, _number
from .device import DEVICE_HBM_BYTES, current_stream
from .nn import MatrixFactorization

MAX_H = als.MAX_H                         # rk_als_max_h()
MAX_LAYERS = 8
LONG_ROW = _als_lib.LGCN_LONG_ROW         # RK_ALS_LGCN_LONG_ROW
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8      # (torch.optim.Adam's)


def check_not_distributed():
  als.check_not_distributed("train_lightgcn runs on one GPU: multi-GPU LightGCN is not implemented")


def check_config(model, num_layers, num_epochs, batch_size, lr, reg, seed, method=None):
  """The LightGCN contract, checked before any GPU work; returns (num_layers, num_epochs, batch_size, lr, reg,
  seed).  ``method`` (a ``Method``; None: LightGCN) names the caller in the messages and bounds its batches and
  layers: recoder_amd/simgcl.py and recoder_amd/directau.py train the same model under the same contract."""
  method = method or METHOD
  name = method.method
  if not isinstance(model, MatrixFactorization):
    raise ValueError("%s trains a MatrixFactorization, not %s" % (name, type(model).__name__))
  if model.activation_type != "none":
    raise ValueError("%s needs activation_type='none' (got %r)" % (name, model.activation_type))
  if model.dropout_prob and model.dropout_prob > 0:
    raise ValueError("%s needs dropout_prob == 0 (got %r)" % (name, model.dropout_prob))
  h = model.embedding_size
  if not isinstance(h, (int, np.integer)) or not 1 <= h <= MAX_H:
    raise ValueError("%s supports embedding sizes 1..%d (got %r)" % (name, MAX_H, h))
  if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not -2 ** 63 <= seed < 2 ** 63:
    raise ValueError("seed must be an integer that fits 64 bits (got %r)" % (seed,))
  return (_count("num_layers", num_layers, method.min_layers, MAX_LAYERS), _count("num_epochs", num_epochs, 0),
          _count("batch_size", batch_size, 1, method.max_batch), _number("lr", lr, True), _number("reg", reg, False),
          int(seed))


def check_resume(state, num_layers, shapes=None, method="train_lightgcn"):
  """ValueError unless ``state`` (a ``lightgcn_state``) can continue a fit with ``num_layers`` layers on base
  tables of ``shapes`` = ((users, h), (items, h)) (None: not known yet)."""
  if state is None:
    raise ValueError("resume=True needs the state of an earlier %s on this Recoder (there is none)" % method)
  if state["num_layers"] != num_layers:
    raise ValueError("resume=True continues a fit with num_layers = %d (got %d)" % (state["num_layers"], num_layers))
  if shapes is not None:
    have = tuple(tuple(t.shape) for t in state["E0"])
    if have != tuple(tuple(s) for s in shapes):
      raise ValueError("resume=True: the state's base tables %s do not match the model's %s" % (have, tuple(shapes)))


def check_data(nnz, n_items, num_epochs, batch_size):
  """What the sampler needs of the matrix (bpr.check_data under this method's name); returns the steps of one epoch."""
  return bpr.check_data(nnz, n_items, num_epochs, batch_size, method=METHOD.method)


def required_bytes(n_users, n_items, h, nnz, T, allocate_model=True, allocate_state=True, allocate_csrs=True,
                   snapshot=False):
  """Device bytes of a fit: the model's tables and bias, the state (the base tables E0 and both Adam moments)
  and both CSRs (int64 indptr, int32 indices), each unless the caller already holds it; the gradient G and
  its propagated form H; two layer buffers; the counts and the two scale vectors; BPR's workspace and the
  buffers of its two sorts.  ``snapshot``: and the copy of the state that validation with ``restore_best`` keeps
  (recoder_amd/validation.py)."""
  n_users, n_items, h, nnz, T = int(n_users), int(n_items), int(h), int(nnz), int(T)
  rows = n_users + n_items
  model = rows * h * 4 + n_items * 4 if allocate_model else 0
  state = (3 * rows * h * 4 if allocate_state else 0) + (3 * rows * h * 4 if snapshot else 0)
  csrs = (n_users + 1) * 8 + (n_items + 1) * 8 + 2 * max(1, nnz) * 4 if allocate_csrs else 0
  return model + state + csrs + (2 + 2) * rows * h * 4 + 2 * rows * 4 + bpr.workspace_bytes(T, h) + \
      2 * 3 * T * (4 + 4 + 8)


def method_required_bytes(method, n_users, n_items, h, nnz, T, allocate_model=True, allocate_state=True,
                          allocate_csrs=True, snapshot=False, **opts):
  """``required_bytes`` and what ``method`` holds on top of it under its options ``opts``."""
  return required_bytes(n_users, n_items, h, nnz, T, allocate_model, allocate_state, allocate_csrs, snapshot) + \
      method.extra_bytes(int(n_users), int(n_items), int(h), int(T), **opts)


def method_check_memory(method, n_users, n_items, h, nnz, T, free_bytes=None, allocate_model=True,
                        allocate_state=True, allocate_csrs=True, snapshot=False, **opts):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's whole HBM
  without touching a device, then (``free_bytes`` None: asked from the current device) against what is free."""
  n_users, n_items, h, nnz, T = int(n_users), int(n_items), int(h), int(nnz), int(T)
  if not (1 <= T <= method.max_batch and 1 <= h <= MAX_H):               # (where the workspaces' bytes are negative)
    raise ValueError("%s needs 1 <= batch_size <= %d and 1 <= h <= %d (got %d, %d)"
                     % (method.name, method.max_batch, MAX_H, T, h))
  whole = method_required_bytes(method, n_users, n_items, h, nnz, T, snapshot=snapshot, **opts)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError("%s over %d users x %d items at h = %d with %d entries and batches of %d needs %d bytes: "
                     "more than one device's memory (%d bytes); multi-device fits are not implemented"
                     % (method.name, n_users, n_items, h, nnz, T, whole, DEVICE_HBM_BYTES))
  need = method_required_bytes(method, n_users, n_items, h, nnz, T, allocate_model, allocate_state, allocate_csrs,
                               snapshot, **opts)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("%s over %d users x %d items at h = %d with %d entries and batches of %d needs %d bytes "
                     "of device memory, %d are free" % (method.name, n_users, n_items, h, nnz, T, need, free_bytes))
  return need


def check_memory(n_users, n_items, h, nnz, T, free_bytes=None, allocate_model=True, allocate_state=True,
                 allocate_csrs=True):
  """``method_check_memory`` of LightGCN."""
  return method_check_memory(METHOD, n_users, n_items, h, nnz, T, free_bytes, allocate_model, allocate_state,
                             allocate_csrs)


def degree_scales(degrees):
  """degree^-1/2 in float64, rounded once to f32; 0 where the degree is 0."""
  d = np.asarray(degrees, dtype=np.float64)
  return np.where(d > 0, 1.0 / np.sqrt(np.maximum(d, 1.0)), 0.0).astype(np.float32)


class Graph:
  """Both device CSRs of ``als.csr_pair`` with the two scale vectors s_u [users] and s_i [items]."""

  def __init__(self, ucsr, icsr):
    self.ucsr, self.icsr = ucsr, icsr
    self.su, self.si = (torch.from_numpy(degree_scales(np.diff(c.indptr.cpu().numpy()))).to(c.indptr.device)
                        for c in (ucsr, icsr))


# ------------------------------------------------------------------ kernels
def _table(t, h=None):
  assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and (h is None or t.shape[1] == h), \
      (t.dtype, t.shape, t.stride())


def propagate(csr, row_scale, col_scale, F, out=None, acc=None, acc_scale=1.0, row_lo=0, row_hi=None, noise=None):
  """out[r] = row_scale[r] sum_j col_scale[col_j] F[col_j] and acc[r] = (acc[r] + out[r]) acc_scale for the rows
  [row_lo, row_hi) of ``csr`` (rk_als_lgcn_propagate); either of ``out`` / ``acc`` may be None.  ``noise`` = (eps,
  seed, step, view, layer, side): SimGCL's noise of that key and length eps is added to every row of ``out`` (and
  so to what ``acc`` accumulates) in the epilogue (rk_als_gcl_propagate)."""
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
  args = (ptr(csr.indptr), ptr(csr.indices), ptr(row_scale), ptr(col_scale), row_lo, row_hi, ptr(F), F.stride(0), h,
          ptr(out), out.stride(0) if out is not None else 0, ptr(acc), acc.stride(0) if acc is not None else 0,
          float(acc_scale))
  if noise is None:
    _als_lib.check(lib.rk_als_lgcn_propagate(*args, current_stream()), "rk_als_lgcn_propagate")
  else:
    eps, seed, step, view, layer, side = noise
    _als_lib.check(lib.rk_als_gcl_propagate(*args, float(eps), int(seed), int(step), int(view), int(layer), int(side),
                                            current_stream()), "rk_als_gcl_propagate")


def scatter(keys, order, roles, g, V, scale, G, count):
  """G[row] = scale sum +-g_t V_t and count[row] for the rows among the sorted keys (rk_als_lgcn_scatter); the
  caller zeroes G and count."""
  n, (T, h) = keys.shape[0], V.shape
  _i32(keys, n)
  assert order.dtype == torch.int64 and order.shape == (n,) and order.is_contiguous() and n == roles * T
  _f32(g, (T,)), _f32(V, (T, h)), _table(G, h), _i32(count, G.shape[0])
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_lgcn_scatter(ptr(keys), ptr(order), n, roles, ptr(g), ptr(V), h, float(scale),
                                         G.shape[0], ptr(G), G.stride(0), ptr(count), current_stream()),
                 "rk_als_lgcn_scatter")


def adam(E0, H, count, reg_scale, M, V, lr, t, beta1=BETA1, beta2=BETA2, eps=EPS):
  """Adam step ``t`` (from 1) on E0 in place with grad = H + reg_scale count E0 (rk_als_lgcn_adam)."""
  _table(E0), _table(H, E0.shape[1])
  rows, h = E0.shape
  assert H.shape[0] == rows
  _f32(M, (rows, h)), _f32(V, (rows, h)), _i32(count, rows)
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_lgcn_adam(ptr(E0), E0.stride(0), ptr(H), H.stride(0), ptr(count), float(reg_scale),
                                      ptr(M), ptr(V), rows, h, float(lr), float(beta1), float(beta2), float(eps),
                                      int(t), current_stream()), "rk_als_lgcn_adam")


# --------------------------------------------------------------------- step
class Workspace:
  """What a fit holds beside the state: G, H, two layer buffers (each users + items rows), the counts, BPR's
  workspace and a zero bias."""

  def __init__(self, n_users, n_items, T, h, device):
    f = lambda rows: torch.empty((rows, h), dtype=torch.float32, device=device)
    self.G, self.H = (f(n_users), f(n_items)), (f(n_users), f(n_items))
    self.layers = ((f(n_users), f(n_items)), (f(n_users), f(n_items)))
    self.count = (torch.zeros(n_users, dtype=torch.int32, device=device),
                  torch.zeros(n_items, dtype=torch.int32, device=device))
    self.bpr = bpr.Workspace(T, h, device)
    self.zero_bias = torch.zeros(n_items, dtype=torch.float32, device=device)


def new_state(X, Y, num_layers):
  """The state of a fresh fit: the base tables are the tables as they stand; zero moments; no step taken."""
  E0 = (X.detach().clone().contiguous(), Y.detach().clone().contiguous())
  return {"E0": E0, "M": tuple(torch.zeros_like(e) for e in E0), "V": tuple(torch.zeros_like(e) for e in E0),
          "step": 0, "num_layers": int(num_layers)}


def forward(graph, base, num_layers, layers, out, skip_layer0=False, noise=None):
  """out = the mean over the layers 0..K (``skip_layer0``: 1..K) of ``base`` = (users' table, items' table)
  propagated over ``graph``; ``layers`` are two pairs of buffers.  ``noise`` = (eps, seed, step, view): SimGCL's
  view ``view`` of step ``step``, noise of length ``eps`` after every layer.  2 K propagations; the mean is formed
  in their epilogues."""
  for o, b in zip(out, base):
    if skip_layer0:
      o.zero_()
    else:
      o.copy_(b)
  cur = base
  for k in range(num_layers):
    last = k == num_layers - 1
    nxt = (None, None) if last else layers[k % 2]
    scale = 1.0 / (num_layers + (0 if skip_layer0 else 1)) if last else 1.0
    for side, (csr, rs, cs) in enumerate(((graph.ucsr, graph.su, graph.si), (graph.icsr, graph.si, graph.su))):
      propagate(csr, rs, cs, cur[1 - side], nxt[side], out[side], scale,
                noise=None if noise is None else noise + (k + 1, side))
    cur = nxt


def bpr_gradient(X, Y, ws):
  """``ws.G`` / ``ws.count`` = the gradient of the mean softplus(-x_t) over the triples in ``ws.bpr`` with respect
  to the tables X / Y, and the rows' counts; g and the loss of the triples stay in ``ws.bpr``.  Returns the sorted
  user keys."""
  b = ws.bpr
  bpr.grad(b.users, b.pos, b.neg, X, Y, ws.zero_bias, b.g, b.loss, b.D, b.P)
  (uk, uo), (ik, io) = bpr.sorted_keys(b.users, b.pos, b.neg, X.shape[0], Y.shape[0])
  for t in ws.G + ws.count:
    t.zero_()
  scatter(uk, uo, 1, b.g, b.D, 1.0 / b.T, ws.G[0], ws.count[0])
  scatter(ik, io, 2, b.g, b.P, 1.0 / b.T, ws.G[1], ws.count[1])
  return uk


def bpr_sums_add(sums, ws):
  sums[0] += ws.bpr.loss.sum(dtype=torch.float64)
  sums[1] += (ws.bpr.neg >= 0).sum()


# What a method of this family says of itself; the loop below is shared:
#   name, method, max_batch, min_layers   "LightGCN", "train_lightgcn" (so the messages call it), the bounds of its
#                   batches and layers
#   skip_layer0     the layer mean leaves layer 0 out
#   gradient(X, Y, graph, state, ws, seed, step_index, hyper)   from the final tables X / Y and the draws in ``ws.bpr``
#                   to the summed gradient in ``ws.G`` and the row counts in ``ws.count``; ``hyper`` is what follows
#                   lr and reg among the hyperparameters
#   sums, sums_add(sums, ws), entry(values, steps)   the (shape, dtype) of an epoch's running sums on the device, what
#                   a step adds to them, and the history entry from their values on the host
#   workspace(n_users, n_items, T, h, device, **opts), extra_bytes(n_users, n_items, h, T, **opts)   its ``Workspace``
#                   and that workspace's device bytes on top of ``required_bytes``, under ``opts(*hyper)``
# A method whose final tables are not the layer mean of two base tables (recoder_amd/simplex.py: a third parameter, user
# rows pooled from the batch's histories) also says, every field None for the methods above:
#   step_forward(X, Y, graph, state, ws, hyper)   in place of the step's ``forward``, run AFTER the draw: the final rows
#                   the step's gradient reads
#   full_forward(X, Y, graph, state, ws, hyper)   in place of the ``forward`` at a validated epoch and at the fit's end
#   backward(graph, state, ws, hyper)   in place of the gradient's ``forward``: returns the Adam jobs, one (parameter,
#                   gradient, count, first moment, second moment) per parameter
#   new_state(X, Y, num_layers, hyper), check_resume(state, num_layers, shapes, hyper)   its state and the resume check
Method = collections.namedtuple(
    "Method", "name method max_batch min_layers skip_layer0 gradient sums sums_add entry workspace extra_bytes opts "
    "step_forward full_forward backward new_state check_resume",
    defaults=(Workspace, lambda n_users, n_items, h, T: 0, lambda *hyper: {}, None, None, None, None, None))

BPR_SUMS = (((), torch.float64), ((), torch.int64))     # the summed loss and the valid triples
METHOD = Method("LightGCN", "train_lightgcn", bpr.MAX_BATCH, 1, skip_layer0=False,
                gradient=lambda X, Y, graph, state, ws, seed, step_index, hyper: bpr_gradient(X, Y, ws),
                sums=BPR_SUMS, sums_add=bpr_sums_add, entry=lambda v, steps: v[0] / v[1] if v[1] else float("nan"))


def method_step(method, X, Y, graph, state, ws, seed, step_index, lr, reg, hyper=()):
  """One step of ``method``: the state's base tables and moments move, X / Y receive the final tables of the base
  tables as they were at the START of the step; the draws of the step stay in ``ws.bpr``."""
  K, b = state["num_layers"], ws.bpr
  if method.step_forward is None:
    forward(graph, state["E0"], K, ws.layers, (X, Y), method.skip_layer0)
    bpr.sample(graph.ucsr, seed, step_index, b.users, b.pos, b.neg)
  else:
    bpr.sample(graph.ucsr, seed, step_index, b.users, b.pos, b.neg)
    method.step_forward(X, Y, graph, state, ws, hyper)
  method.gradient(X, Y, graph, state, ws, seed, step_index, hyper)
  if method.backward is None:
    forward(graph, ws.G, K, ws.layers, ws.H, method.skip_layer0)
    jobs = [(state["E0"][side], ws.H[side], ws.count[side], state["M"][side], state["V"][side]) for side in (0, 1)]
  else:
    jobs = method.backward(graph, state, ws, hyper)
  state["step"] += 1
  for E0, H, count, M, V in jobs:
    adam(E0, H, count, reg / b.T, M, V, lr, state["step"])


def step(X, Y, graph, state, ws, seed, step_index, lr, reg):
  """One LightGCN step (``method_step``); the triples, g and loss of the step stay in ``ws.bpr``."""
  method_step(METHOD, X, Y, graph, state, ws, seed, step_index, lr, reg)


# ---------------------------------------------------------------------- fit
def state_tensors(state):
  """The device tensors of a state (``new_state``), in a fixed order: what a snapshot copies."""
  return list(state["E0"]) + list(state["M"]) + list(state["V"])


def method_fit(method, X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg, hyper=(), seed=0,
               state=None, first_step=None, monitor=None, monitor_prepare=None):
  """num_epochs epochs of ceil(nnz / batch_size) steps of ``method``.  ``state`` None: a fresh state (``new_state``:
  the base tables are X, Y as they stand), made once every check has passed; else an earlier fit's, continued.
  Step s of the fit draws as step ``first_step + s`` (None: the state's step count, so that a continued fit draws
  what one longer fit would have).  The model's tables X [users, h], Y [items, h] (f32, row-major, may be strided)
  end as the final tables of the last base tables, ``bias`` as 0.  Returns (state, the history: ``method.entry`` of
  each epoch's sums).  One host synchronisation per epoch.
  ``monitor`` (a ``validation.Monitor``): after every epoch that is due the final tables of the base tables as they
  stand are written into X, Y -- what a fit ending there leaves; the next step's own forward pass overwrites them
  with the same bits -- and the monitor scores them (``monitor_prepare``: a function applied in place to X and Y for
  the scoring alone, the sampled softmax's normalisation); it may stop the fit, and at the end puts the best
  epoch's state back, so that the tables, the state and its step count are those of a fit of that many epochs.  The
  history keeps every epoch that ran."""
  steps = bpr.check_data(ucsr.nnz, ucsr.shape[1], num_epochs, batch_size, method=method.method)
  if state is not None:
    if method.check_resume is None:
      check_resume(state, num_layers, (X.shape, Y.shape), method=method.method)
    else:
      method.check_resume(state, num_layers, (X.shape, Y.shape), hyper)
  opts = method.opts(*hyper)
  method_check_memory(method, X.shape[0], Y.shape[0], X.shape[1], ucsr.nnz, batch_size, allocate_model=False,
                      allocate_state=state is None, allocate_csrs=False,
                      snapshot=monitor is not None and monitor.restore_best, **opts)
  if state is None:
    state = new_state(X, Y, num_layers) if method.new_state is None else method.new_state(X, Y, num_layers, hyper)
  graph = Graph(ucsr, icsr)

  def final_tables():
    if method.full_forward is None:
      forward(graph, state["E0"], state["num_layers"], ws.layers, (X, Y), method.skip_layer0)
    else:
      method.full_forward(X, Y, graph, state, ws, hyper)
  ws = method.workspace(X.shape[0], Y.shape[0], int(batch_size), X.shape[1], X.device, **opts)
  bias.zero_()
  hist = []
  s = state["step"] if first_step is None else int(first_step)
  for e in range(num_epochs):
    sums = [torch.zeros(shape, dtype=dtype, device=X.device) for shape, dtype in method.sums]
    for _ in range(steps):
      method_step(method, X, Y, graph, state, ws, seed, s, lr, reg, hyper)
      method.sums_add(sums, ws)
      s += 1
    values = torch.cat([t.double().reshape(-1) for t in sums]).cpu().tolist()      # (the synchronisation)
    hist.append(method.entry(values, steps))
    if monitor is not None and monitor.due(e):
      final_tables()
      if monitor.epoch_end(e, state_tensors(state), state["step"],
                           prepare=None if monitor_prepare is None else ((X, Y), monitor_prepare)):
        break
  if monitor is not None and monitor.finish(state_tensors(state), len(hist)):
    state["step"] = monitor.best_step
  final_tables()
  return state, hist


def fit(X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg, seed=0, state=None, first_step=None,
        monitor=None):
  """``method_fit`` of LightGCN.  Returns (state, the mean loss per valid triple of each epoch: floats, nan for an
  epoch without one)."""
  return method_fit(METHOD, X, Y, bias, ucsr, icsr, num_layers, num_epochs, batch_size, lr, reg, (), seed, state,
                    first_step, monitor)
