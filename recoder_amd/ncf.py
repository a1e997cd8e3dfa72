"""NeuMF, the fusion of GMF and an MLP of Neural Collaborative Filtering (He, Liao, Zhang, Nie, Hu & Chua, WWW 2017),
for ``nn.NeuralMatrixFactorization`` on the rk_als_ncf_* kernels of librecoder_als.so (include/recoder_als.h).

    s(u, i) = w[:dg] . (Pg[u] o Qg[i]) + w[dg:] . phi_L + b0,   phi_0 = [Pm[u] ; Qm[i]],   phi_l = relu(W_l phi_{l-1} + c_l)

A step takes T slots (u, i), ``train_bpr``'s stored-entry draw for the same (seed, step, slot), and for each slot R
private negatives from the candidate round UltraGCN and CCL share: uniform over the items, pure integer functions of
(seed, step, slot, r), nothing rejected -- an item the user holds can come up as a negative, as in those two.  The
E = T (1 + R) entries carry the labels 1 and 0 and the loss is the mean over them of the binary cross-entropy on the
logit s.  rk_als_ncf_step leaves one gradient row per entry and side and a slab of dense partial gradients per tile of
32 entries; the rows are summed per table row by the key sort and rk_als_lgcn_scatter and applied by rk_als_lgcn_adam
(the L2 term reg / E on a row times the entries that touch it) -- once per side, because the fit keeps [Pg | Pm] and
[Qg | Qm] as one matrix each -- and rk_als_ncf_dense_adam adds the slabs in tile order and steps every dense parameter,
with the decay ``reg`` on W_l and w and none on the biases.

Not built: GMF-only and MLP-only models and the paper's pre-training from them, activations other than relu, dropout,
multi-GPU training, the Adam moments in checkpoints, HIP-graph capture of the step, bf16 and the fold-in of unseen users.

``Recoder.train_ncf`` is the public entry point; the functions below are the layer under it (and what the tests drive
directly).
"""
import numpy as np
import torch

from . import _als_lib, als, bpr, ccl, lightgcn
from ._lib import ptr
from .bpr import _carve, _count, _number, _round256
from .device import DEVICE_HBM_BYTES, current_stream

TILE = _als_lib.NCF_TILE                            # RK_ALS_NCF_TILE
MAX_WIDTH = _als_lib.NCF_MAX_WIDTH                  # RK_ALS_NCF_MAX_WIDTH
MAX_LAYERS = _als_lib.NCF_MAX_LAYERS                # RK_ALS_NCF_MAX_LAYERS
MAX_BATCH = ccl.MAX_BATCH                           # RK_ALS_CCL_MAX_BATCH
MAX_NEGATIVES = ccl.MAX_NEGATIVES                   # RK_ALS_CCL_MAX_NEGATIVES
MAX_ENTRIES = ccl.MAX_ENTRIES                       # RK_ALS_CCL_MAX_ENTRIES
LDS_LIMIT = 160 * 1024                              # bytes of LDS a workgroup may hold
BETA1, BETA2, EPS = lightgcn.BETA1, lightgcn.BETA2, lightgcn.EPS


def check_not_distributed():
  """ValueError under more than one rank."""
  try:
    als.check_not_distributed("train_ncf runs on one GPU: multi-GPU NeuMF training is not implemented")
  except NotImplementedError as e:
    raise ValueError(str(e)) from None


# -------------------------------------------------------------------- sizes
def _width(name, v):
  if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 4 <= v <= MAX_WIDTH or v % 4:
    raise ValueError("%s must be a multiple of 4 in 4..%d (got %r)" % (name, MAX_WIDTH, v))
  return int(v)


def dims(sizes):
  """(dg, dm, L, d1, d2, d3) of ``sizes`` = (dg, dm, layers), the kernels' size arguments (0 past L)."""
  dg, dm, layers = sizes
  return (dg, dm, len(layers)) + tuple(layers) + (0,) * (MAX_LAYERS - len(layers))


def layout(sizes):
  """Where the dense parameters lie in theta = [W_1, c_1, ..., W_L, c_L, w, b0]: ([(W_l offset, c_l offset, d_l,
  d_{l-1})], w offset, b0 offset, the count) -- rk_als_ncf_dense_count restated."""
  dg, dm, layers = sizes
  off, prev, rows = 0, 2 * dm, []
  for d in layers:
    rows.append((off, off + d * prev, d, prev))
    off, prev = off + d * prev + d, d
  return rows, off, off + dg + prev, off + dg + prev + 1


def lds_bytes(sizes, scores=False):
  """rk_als_ncf_lds_bytes restated: the LDS of the step kernel (``scores``: of the scores kernel)."""
  dg, dm, layers = sizes
  widths = [2 * dm] + list(layers)
  L = len(layers)
  if scores:
    f = dg + layers[-1] + 1 + TILE * (layers[0] + 1) + TILE * (dg + 1) + 2 * TILE * (max(layers) + 1) + layers[0] + dg
    f += sum(widths[l] * (widths[l - 1] + 1) + widths[l] for l in range(2, L + 1))
  else:
    f = dg + layers[-1] + 1 + 4 * TILE
    f += sum(widths[l] * (widths[l - 1] + 1) + widths[l] + TILE * (widths[l] + 1) for l in range(1, L + 1))
  return 4 * f


def check_sizes(embedding_size, mlp_embedding_size, mlp_layers):
  """ValueError unless the three sizes are what the kernels take; returns (dg, dm, layers)."""
  dg = _width("embedding_size", embedding_size)
  dm = _width("mlp_embedding_size", mlp_embedding_size)
  if isinstance(mlp_layers, (str, bytes)) or not hasattr(mlp_layers, "__len__") or \
      not 1 <= len(mlp_layers) <= MAX_LAYERS:
    raise ValueError("mlp_layers must hold 1..%d layer widths (got %r)" % (MAX_LAYERS, mlp_layers))
  layers = tuple(_width("every width of mlp_layers", d) for d in mlp_layers)
  sizes = (dg, dm, layers)
  need = max(lds_bytes(sizes), lds_bytes(sizes, True))
  if need > LDS_LIMIT:
    raise ValueError("mlp_layers %r at mlp_embedding_size %d need %d bytes of LDS, a workgroup has %d: the layers' "
                     "weights must fit it together" % (layers, dm, need, LDS_LIMIT))
  return sizes


def check_config(model, num_epochs, batch_size, lr, reg, num_negatives, seed):
  """The contract of ``train_ncf``, checked before any GPU work; returns (sizes, num_epochs, batch_size, lr, reg,
  num_negatives, seed)."""
  from .nn import NeuralMatrixFactorization
  if not isinstance(model, NeuralMatrixFactorization):
    raise ValueError("train_ncf trains a NeuralMatrixFactorization, not %s" % type(model).__name__)
  sizes = check_sizes(model.embedding_size, model.mlp_embedding_size, model.mlp_layers)
  if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not -2 ** 63 <= seed < 2 ** 63:
    raise ValueError("seed must be an integer that fits 64 bits (got %r)" % (seed,))
  T = _count("batch_size", batch_size, 1, MAX_BATCH)
  R = _count("num_negatives", num_negatives, 1, MAX_NEGATIVES)
  if T * (1 + R) > MAX_ENTRIES:
    raise ValueError("batch_size * (1 + num_negatives) must be at most %d (got %d * %d)" % (MAX_ENTRIES, T, 1 + R))
  return (sizes, _count("num_epochs", num_epochs, 0), T, _number("lr", lr, True), _number("reg", reg, False), R,
          int(seed))


def check_data(nnz, n_items, num_epochs, batch_size):
  return bpr.check_data(nnz, n_items, num_epochs, batch_size, method="train_ncf")


def check_resume(state, sizes, shapes=None):
  """ValueError unless ``state`` (an ``ncf_state``) can continue a fit of a model of ``sizes`` with ``shapes`` =
  (users, items)."""
  if state is None:
    raise ValueError("resume=True needs the state of an earlier train_ncf on this Recoder (there is none)")
  if state["sizes"] != sizes:
    raise ValueError("resume=True continues a fit of sizes %r (got %r)" % (state["sizes"], sizes))
  if shapes is not None and (state["U"].shape[0], state["I"].shape[0]) != tuple(shapes):
    raise ValueError("resume=True: the state's tables %r do not match the model's %r"
                     % ((state["U"].shape[0], state["I"].shape[0]), tuple(shapes)))


def workspace_bytes(T, R, sizes):
  """rk_als_ncf_workspace_bytes restated: ukey, ikey [E], GU, GI [E, dg + dm], the slabs [ceil(E / 32), n + 1] and
  the loss slot, each rounded up to 256 bytes."""
  T, R = int(T), int(R)
  if not (1 <= T <= MAX_BATCH and 1 <= R <= MAX_NEGATIVES) or T * (1 + R) > MAX_ENTRIES:
    return -2
  E, n = T * (1 + R), layout(sizes)[3]
  return 2 * _round256(4 * E) + 2 * _round256(4 * E * (sizes[0] + sizes[1])) + \
      _round256(4 * -(-E // TILE) * (n + 1)) + _round256(4)


def required_bytes(n_users, n_items, nnz, T, R, sizes, allocate_model=True, snapshot=False):
  """Device bytes of a fit: the model (unless the caller holds it), the fit's copies of the tables and of theta with
  two moments each (and a snapshot of them with ``snapshot``), the user CSR, the slots, the workspace, the summed
  gradient rows and counts of both sides, and the keys of both sorts with what torch.sort holds meanwhile."""
  h, n, E = sizes[0] + sizes[1], layout(sizes)[3], int(T) * (1 + int(R))
  tables = (int(n_users) + int(n_items)) * h * 4
  state = 3 * (tables + 4 * n) * (1 + int(bool(snapshot)))
  model = (tables + 4 * n) * int(bool(allocate_model))
  csr = (int(n_users) + 1) * 8 + max(1, int(nnz)) * 4
  return model + state + csr + 3 * 4 * int(T) + workspace_bytes(T, R, sizes) + tables + \
      4 * (int(n_users) + int(n_items)) + 4 * E + 2 * 2 * E * (4 + 4 + 8)


def check_memory(n_users, n_items, nnz, T, R, sizes, free_bytes=None, allocate_model=True, snapshot=False):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's whole HBM without
  touching a device, then (``free_bytes`` None: asked from the current device) against what is free."""
  whole = required_bytes(n_users, n_items, nnz, T, R, sizes, True, snapshot)
  what = "NeuMF over %d users x %d items at sizes %r with batches of %d x %d" % (n_users, n_items, sizes, T, 1 + R)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError("%s needs %d bytes: more than one device's memory (%d bytes)" % (what, whole, DEVICE_HBM_BYTES))
  need = required_bytes(n_users, n_items, nnz, T, R, sizes, allocate_model, snapshot)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("%s needs %d bytes of device memory, %d are free" % (what, need, free_bytes))
  return need


# ------------------------------------------------------------------ packing
def pack(model):
  """(U = [Pg | Pm], I = [Qg | Qm], theta) as new tensors from the model's parameters."""
  U = torch.cat([model.Pg.data, model.Pm.data], dim=1).contiguous()
  I = torch.cat([model.Qg.data, model.Qm.data], dim=1).contiguous()
  parts = []
  for W, c in zip(model.mlp_weights, model.mlp_biases):
    parts += [W.data.reshape(-1), c.data.reshape(-1)]
  theta = torch.cat(parts + [model.w.data.reshape(-1), model.b0.data.reshape(-1)]).contiguous()
  return U, I, theta


def unpack(model, U, I, theta):
  """The model's parameters written in place from the fit's matrices."""
  dg = model.embedding_size
  model.Pg.data.copy_(U[:, :dg]), model.Pm.data.copy_(U[:, dg:])
  model.Qg.data.copy_(I[:, :dg]), model.Qm.data.copy_(I[:, dg:])
  rows, w_off, b0_off, n = layout(model.sizes())
  for (wo, co, d, prev), W, c in zip(rows, model.mlp_weights, model.mlp_biases):
    W.data.copy_(theta[wo:co].view(d, prev)), c.data.copy_(theta[co:co + d])
  model.w.data.copy_(theta[w_off:b0_off]), model.b0.data.copy_(theta[b0_off:n].view(model.b0.shape))
  model._weights_written()


# ------------------------------------------------------------------ kernels
def _check_tables(sizes, Pg, Qg, Pm, Qm, theta):
  dg, dm, _ = sizes
  for t, d in ((Pg, dg), (Qg, dg), (Pm, dm), (Qm, dm)):
    assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == d and t.stride(1) == 1, (t.shape, d)
  assert Pg.shape[0] == Pm.shape[0] and Qg.shape[0] == Qm.shape[0]
  assert theta.dtype == torch.float32 and theta.is_contiguous() and theta.shape == (layout(sizes)[3],), theta.shape


def step_kernel(users, pos, R, seed, step_index, Pg, Qg, Pm, Qm, theta, sizes, ukey, ikey, GU, GI, slabs):
  """rk_als_ncf_step over the T slots (users, pos) and their R negatives."""
  T = users.shape[0]
  E, h, n = T * (1 + R), sizes[0] + sizes[1], layout(sizes)[3]
  if workspace_bytes(T, R, sizes) < 0:
    raise ValueError("rk_als_ncf_step needs 1 <= T <= %d, 1 <= R <= %d and T (1 + R) <= %d (got T = %d, R = %d)"
                     % (MAX_BATCH, MAX_NEGATIVES, MAX_ENTRIES, T, R))
  _check_tables(sizes, Pg, Qg, Pm, Qm, theta)
  bpr._i32(users, T), bpr._i32(pos, T), bpr._i32(ukey, E), bpr._i32(ikey, E)
  bpr._f32(GU, (E, h)), bpr._f32(GI, (E, h)), bpr._f32(slabs, (-(-E // TILE), n + 1))
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_ncf_step(ptr(users), ptr(pos), T, R, int(seed), int(step_index), Pg.shape[0], Qg.shape[0],
                                     ptr(Pg), Pg.stride(0), ptr(Qg), Qg.stride(0), ptr(Pm), Pm.stride(0), ptr(Qm),
                                     Qm.stride(0), ptr(theta), *dims(sizes), ptr(ukey), ptr(ikey), ptr(GU), ptr(GI),
                                     ptr(slabs), current_stream()), "rk_als_ncf_step")


def dense_adam(theta, M, V, slabs, entries, sizes, lr, reg, t, loss, beta1=BETA1, beta2=BETA2, eps=EPS):
  """rk_als_ncf_dense_adam: Adam step ``t`` (from 1) on theta from the slabs of ``entries`` entries; loss[0] = the
  slabs' loss sum."""
  n = layout(sizes)[3]
  tiles = -(-int(entries) // TILE)
  for x in (theta, M, V):
    bpr._f32(x, (n,))
  bpr._f32(slabs, (tiles, n + 1)), bpr._f32(loss, (1,))
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_ncf_dense_adam(ptr(theta), ptr(M), ptr(V), ptr(slabs), tiles, int(entries), *dims(sizes),
                                           float(lr), float(reg), float(beta1), float(beta2), float(eps), int(t),
                                           ptr(loss), current_stream()), "rk_als_ncf_dense_adam")


def item_part(Qm, theta, sizes, out=None):
  """A [items, d1] = Qm W_1[:, dm:]^T (rk_als_ncf_item_part)."""
  dm, d1 = sizes[1], sizes[2][0]
  assert Qm.dtype == torch.float32 and Qm.shape[1] == dm and Qm.stride(1) == 1
  out = torch.empty((Qm.shape[0], d1), dtype=torch.float32, device=Qm.device) if out is None else out
  bpr._f32(out, (Qm.shape[0], d1))
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_ncf_item_part(ptr(Qm), Qm.stride(0), Qm.shape[0], ptr(theta), dm, d1, ptr(out),
                                          current_stream()), "rk_als_ncf_item_part")
  return out


def scores(users, lo, hi, Pg, Qg, Pm, A, theta, sizes, out, ld):
  """out[b, c] = s(users[b], lo + c) for the B ids ``users`` (int32, device) and c < hi - lo, ``out`` f32 with row
  stride ``ld`` (rk_als_ncf_scores)."""
  B, n_items = users.shape[0], Qg.shape[0]
  if not (1 <= B and 0 <= lo < hi <= n_items and ld >= hi - lo):
    raise ValueError("rk_als_ncf_scores needs B >= 1, 0 <= lo < hi <= n_items and ld >= hi - lo (got B = %d, lo = %d, "
                     "hi = %d, ld = %d)" % (B, lo, hi, ld))
  bpr._i32(users, B)
  assert out.dtype == torch.float32 and out.numel() >= (B - 1) * ld + hi - lo
  bpr._f32(A, (n_items, sizes[2][0]))
  UH = torch.empty((B, sizes[2][0]), dtype=torch.float32, device=out.device)
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_ncf_scores(ptr(users), B, Pg.shape[0], int(lo), int(hi), n_items, ptr(Pg), Pg.stride(0),
                                       ptr(Qg), Qg.stride(0), ptr(Pm), Pm.stride(0), ptr(A), ptr(theta), *dims(sizes),
                                       ptr(UH), ptr(out), int(ld), current_stream()), "rk_als_ncf_scores")
  return out


# --------------------------------------------------------------------- step
class Workspace:
  """The slots, one allocation of rk_als_ncf_workspace_bytes cut into its buffers, the summed gradient rows and
  counts of both sides and the ones the row scatter weighs every entry with."""

  def __init__(self, n_users, n_items, T, R, sizes, device):
    need = _als_lib.load().rk_als_ncf_workspace_bytes(T, R, *dims(sizes))
    assert need == workspace_bytes(T, R, sizes) and need > 0, (need, T, R, sizes)
    E, h, n = T * (1 + R), sizes[0] + sizes[1], layout(sizes)[3]
    self.T, self.R, self.E = T, R, E
    self.users, self.pos, self.neg = (torch.empty(T, dtype=torch.int32, device=device) for _ in range(3))
    # (neg: rk_als_bpr_sample writes its own rejected negative there; NeuMF's negatives are the step kernel's draws
    #  and this buffer is never read)
    self.raw = torch.empty(need, dtype=torch.uint8, device=device)
    self.ukey, self.ikey, self.GU, self.GI, self.slabs, self.loss = _carve(
        self.raw, *[(torch.int32, (E,))] * 2, *[(torch.float32, (E, h))] * 2,
        (torch.float32, (-(-E // TILE), n + 1)), (torch.float32, (1,)))
    self.G = (torch.zeros((n_users, h), dtype=torch.float32, device=device),
              torch.zeros((n_items, h), dtype=torch.float32, device=device))
    self.count = (torch.zeros(n_users, dtype=torch.int32, device=device),
                  torch.zeros(n_items, dtype=torch.int32, device=device))
    self.ones = torch.ones(E, dtype=torch.float32, device=device)


def new_state(model):
  """The state of a fresh fit: the model's parameters as they stand, zero moments."""
  U, I, theta = pack(model)
  E0 = (U, I, theta)
  return {"U": U, "I": I, "theta": theta, "M": tuple(torch.zeros_like(e) for e in E0),
          "V": tuple(torch.zeros_like(e) for e in E0), "step": 0, "sizes": model.sizes()}


def state_tensors(state):
  return [state["U"], state["I"], state["theta"]] + list(state["M"]) + list(state["V"])


def step(ucsr, state, ws, seed, step_index, lr, reg):
  """One NeuMF step on the state in place; ``ws.loss[0]`` is the step's loss sum over its entries."""
  sizes, dg = state["sizes"], state["sizes"][0]
  U, I, theta = state["U"], state["I"], state["theta"]
  bpr.sample(ucsr, seed, step_index, ws.users, ws.pos, ws.neg)
  step_kernel(ws.users, ws.pos, ws.R, seed, step_index, U[:, :dg], I[:, :dg], U[:, dg:], I[:, dg:], theta, sizes,
              ws.ukey, ws.ikey, ws.GU, ws.GI, ws.slabs)
  state["step"] += 1
  t = state["step"]
  for side, (key, rows, table) in enumerate(((ws.ukey, ws.GU, U), (ws.ikey, ws.GI, I))):
    ws.G[side].zero_(), ws.count[side].zero_()
    keys, order = torch.sort(key, stable=True)
    lightgcn.scatter(keys, order, 1, ws.ones, rows, -1.0 / ws.E, ws.G[side], ws.count[side])
    lightgcn.adam(table, ws.G[side], ws.count[side], reg / ws.E, state["M"][side], state["V"][side], lr, t)
  dense_adam(theta, state["M"][2], state["V"][2], ws.slabs, ws.E, sizes, lr, reg, t, ws.loss)


# ---------------------------------------------------------------------- fit
def fit(model, ucsr, num_epochs, batch_size, lr, reg, num_negatives, seed=0, state=None, monitor=None):
  """num_epochs epochs of ceil(nnz / batch_size) steps on ``model`` (a placed NeuralMatrixFactorization).  ``state``
  None: a fresh state from the model's parameters; else an earlier fit's, continued: step s draws as the state's step
  count, so that a continued fit draws what one longer fit would have.  The model's parameters are written at the end
  (and before every scoring of a ``monitor``, which may stop the fit and puts the best epoch's state back).  Returns
  (state, the mean loss per entry of each epoch).  One host synchronisation per epoch."""
  sizes = model.sizes()
  n_users, n_items = model.Pg.shape[0], model.Qg.shape[0]
  steps = check_data(ucsr.nnz, ucsr.shape[1], num_epochs, batch_size)
  if state is not None:
    check_resume(state, sizes, (n_users, n_items))
  check_memory(n_users, n_items, ucsr.nnz, batch_size, num_negatives, sizes, allocate_model=False,
               snapshot=monitor is not None and monitor.restore_best)
  if state is None:
    state = new_state(model)
  ws = Workspace(n_users, n_items, int(batch_size), int(num_negatives), sizes, model.Pg.device)
  hist = []
  for e in range(num_epochs):
    total = torch.zeros((), dtype=torch.float64, device=model.Pg.device)
    for _ in range(steps):
      step(ucsr, state, ws, seed, state["step"], lr, reg)
      total += ws.loss[0].double()
    hist.append(float(total.cpu()) / (steps * ws.E))                 # (the synchronisation)
    if monitor is not None and monitor.due(e):
      unpack(model, state["U"], state["I"], state["theta"])
      if monitor.epoch_end(e, state_tensors(state), state["step"]):
        break
  if monitor is not None and monitor.finish(state_tensors(state), len(hist)):
    state["step"] = monitor.best_step
  unpack(model, state["U"], state["I"], state["theta"])
  return state, hist
