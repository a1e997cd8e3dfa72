"""UserKNN (user-based cosine neighbourhoods; the baseline of Dacrema et al. 2019) for
``UserNeighbourhoodModel``, on the rk_rp3_user_* kernels of librecoder_rp3.so (include/recoder_rp3.h).

The model is the training matrix X itself (U users x n items).  With H_v the items of training user v and
H_q the stored non-zero items of a query row q (the query's values play no part):

    c[q, v]   = |H_q and H_v|
    sim[q, v] = c[q, v] / (sqrt(|H_q|) * sqrt(|H_v|) + shrink)
    q keeps its ``neighbours`` largest sim > 0 by (sim descending, v ascending)
    scores[q, j] = sum over the kept v, ascending, of sim[q, v] * X[v, j]     (the stored training values)

All the work happens at serving time: neighbours are found from whatever history the caller passes,
also for users the fit has never seen, and a new interaction takes effect by replacing the CSR.  A
training user identical to the query is NOT excluded (the scores interface carries no user ids): it takes
one of the slots and contributes only items that the masked top-k removes.

``Recoder.train_userknn`` is the public entry point; the functions below are the layer under it (and what
the tests and tools/userknn_bench.py drive directly).
"""
import numpy as np
import torch

from . import _neighbours, _rp3_lib, als
from ._lib import ptr
from .device import current_stream
from .rp3 import LDS_ITEMS as LDS_USERS      # rk_rp3_lds_items(): the users whose counts live in LDS
from .rp3 import MAX_NEIGHBOURS              # rk_rp3_max_neighbours()

_GROUPS = 512              # (resident workgroups of rk_rp3_user_neighbours)
SERVING_ROWS = 512         # (query rows of a batch that the memory check counts)


def check_not_distributed():
  als.check_not_distributed("train_userknn runs on one GPU: a multi-GPU UserKNN is not implemented")


def check_config(model, neighbours, shrink):
  """The UserKNN contract, checked before any GPU work; returns (neighbours, shrink)."""
  from .nn import UserNeighbourhoodModel
  if not isinstance(model, UserNeighbourhoodModel):
    raise ValueError("train_userknn fits a UserNeighbourhoodModel, not %s" % type(model).__name__)
  return check_params(neighbours, shrink)


def check_params(neighbours, shrink):
  shrink = _neighbours.check_number("shrink", shrink)
  return _neighbours.check_neighbours(neighbours, MAX_NEIGHBOURS), shrink


def norms(lengths):
  """sqrt of the row lengths in float64, rounded once to f32 (no sqrt runs on the device)."""
  return np.sqrt(np.asarray(lengths, np.float64)).astype(np.float32)


def workspace_bytes(n_users):
  """rk_rp3_user_workspace_bytes(n_users), restated on the host (the memory check needs no library)."""
  U = int(n_users)
  if U < 1:
    return -2
  if U <= LDS_USERS:
    return 256
  return 256 + _GROUPS * 2 * (-(-U // 64) * 64) * 4


def required_bytes(n_users, n_items, N, nnz, rows=SERVING_ROWS):
  """Device bytes of the model and of serving ``rows`` query rows: both CSRs of X (int64 indptr, int32
  indices), its f32 values, the norms, the [rows, N] neighbour lists with their counts and norms, and the
  workspace."""
  U, n, N, nnz, rows = int(n_users), int(n_items), int(N), int(nnz), int(rows)
  model = (U + 1 + n + 1) * 8 + 3 * max(1, nnz) * 4 + U * 4
  return model + rows * (N * 8 + 8) + max(256, workspace_bytes(U))


def check_memory(n_users, n_items, N, nnz, free_bytes=None):
  """ValueError naming the sizes and the bytes needed when the model cannot be held and served: against one
  device's whole HBM without touching a device, then (``free_bytes`` None: asked from the current
  device) against what is free."""
  U, n, N, nnz = int(n_users), int(n_items), int(N), int(nnz)
  if U < 1 or n < 1:
    raise ValueError("UserKNN needs at least one user and one item (got %d users x %d items)" % (U, n))
  what = "UserKNN over %(users)d users x %(n)d items with %(K)d neighbours and %(nnz)d entries needs %(need)d bytes"
  return _neighbours.check_memory(
      lambda allocate: required_bytes(U, n, N, nnz), dict(users=U, n=n, K=N, nnz=nnz),
      what + ": more than one device's memory (%(hbm)d bytes); multi-device serving is not implemented",
      what + " of device memory, %(free)d are free", free_bytes)


# ------------------------------------------------------------------ kernels
def query_norms(csr, n_rows=None):
  """qn f32 [rows] on the csr's device: sqrt(stored entries of every row), made on the host."""
  deg = getattr(csr, "degrees", None)
  if deg is None:
    deg = np.diff(csr.indptr.cpu().numpy())
  deg = np.asarray(deg)[:csr.shape[0] if n_rows is None else n_rows]
  return torch.from_numpy(norms(deg)).to(csr.indptr.device)


def neighbours(csr, icsr, un, N, shrink, qn=None, out=None, row_lo=0, row_hi=None, ws=None):
  """(ids int32 [Q, N], sim f32 [Q, N], count int32 [Q]) of the rows [row_lo, row_hi) of the query ``csr``
  against the item-major CSR ``icsr`` of X (rk_rp3_user_neighbours); ``un`` f32 [U] the training users'
  norms, ``qn`` the queries' (None: made from the csr).  ``csr``: anything with int64 ``indptr`` and int32
  ``indices`` on the device.  ``out``: the three tensors to fill.  Returns them and the workspace."""
  lib = _rp3_lib.load()
  n, U = icsr.shape
  Q = csr.shape[0]
  row_hi = Q if row_hi is None else row_hi
  dev = un.device
  assert un.shape == (U,) and un.dtype == torch.float32 and 0 <= row_lo <= row_hi <= Q
  qn = query_norms(csr) if qn is None else qn
  assert qn.shape == (Q,) and qn.dtype == torch.float32
  ids, sim, count = _neighbours.lists(Q, N, dev, out)
  ws = _neighbours.workspace(ws, lib.rk_rp3_user_workspace_bytes(U), dev)
  _rp3_lib.check(lib.rk_rp3_user_neighbours(ptr(csr.indptr), ptr(csr.indices), ptr(icsr.indptr), ptr(icsr.indices),
                                            U, n, ptr(un), ptr(qn), float(shrink), N, row_lo, row_hi, ptr(ids),
                                            ptr(sim), ptr(count), ptr(ws), ws.numel(), current_stream()),
                 "rk_rp3_user_neighbours")
  return ids, sim, count, ws


def scores(nbr, ucsr, lo=0, hi=None, out=None, ld=None, n_rows=None):
  """out[q, c] = sum over the kept neighbours v of row q, ascending, of sim * X[v, lo + c]
  (rk_rp3_user_scores).  ``nbr``: (ids, sim, count) of ``neighbours``; ``ucsr``: the user-major CSR of X
  with fp32 ``data`` (or None: every value 1.0) on the device."""
  lib = _rp3_lib.load()
  ids, sim, count = nbr[:3]
  Q, N = ids.shape
  U, n = ucsr.shape
  hi = n if hi is None else hi
  n_rows = Q if n_rows is None else n_rows
  assert ids.dtype == torch.int32 and sim.dtype == torch.float32 and count.dtype == torch.int32
  assert ids.is_contiguous() and sim.is_contiguous() and sim.shape == (Q, N) and count.shape == (Q,)
  assert 0 <= lo < hi <= n and 0 <= n_rows <= Q
  if out is None:
    ld = hi - lo if ld is None else ld
    out = torch.empty(n_rows, ld, dtype=torch.float32, device=ids.device)
  ld = out.stride(0) if ld is None else ld
  _rp3_lib.check(lib.rk_rp3_user_scores(ptr(ids), ptr(sim), ptr(count), n_rows, N, ptr(ucsr.indptr),
                                        ptr(ucsr.indices), ptr(ucsr.data), U, n, lo, hi, ptr(out), ld,
                                        current_stream()), "rk_rp3_user_scores")
  return out


# ---------------------------------------------------------------------- fit
def fit(csr_pair, neighbours, shrink, model=None):
  """The "fit" of a model that is its training matrix: checks, the training users' norms, and (``model``:
  a UserNeighbourhoodModel on the device) the copy of both CSRs into its tensors.  Returns (un, info);
  ``info`` holds n_users, n, nnz, neighbours, shrink and fit_ms (HIP events around the device copies)."""
  ucsr, icsr = csr_pair
  N, shrink = check_params(neighbours, shrink)
  check_not_distributed()
  U, n = ucsr.shape
  check_memory(U, n, N, ucsr.nnz)
  dev = ucsr.indptr.device
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
  ev[0].record()
  un = torch.from_numpy(norms(np.diff(ucsr.indptr.cpu().numpy()))).to(dev)
  if model is not None:
    model.store(ucsr, icsr, un)
  ev[1].record()
  ev[1].synchronize()
  info = dict(n_users=int(U), n=int(n), nnz=int(ucsr.nnz), neighbours=N, shrink=shrink,
              fit_ms=ev[0].elapsed_time(ev[1]))
  return un, info
