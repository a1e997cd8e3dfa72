"""What the neighbour-list models share (recoder_amd.rp3, itemknn and slim store an item-item matrix as
[n, K] ids, weights and counts; userknn makes such lists per query row): the checks of their numbers, the
two stages of their memory check, the lists and the workspace of a fit, its event-timed run, and the wrapper
of the scores kernels that take the same arguments."""
import math

import numpy as np
import torch

from ._lib import ptr
from .device import DEVICE_HBM_BYTES, current_stream


def check_neighbours(neighbours, max_neighbours):
  if isinstance(neighbours, bool) or not isinstance(neighbours, (int, np.integer)) or \
      not 1 <= neighbours <= max_neighbours:
    raise ValueError("neighbours must be an integer in [1, %d] (got %r)" % (max_neighbours, neighbours))
  return int(neighbours)


def check_number(name, v, lo=0.0, hi=math.inf):
  """float(v) of a finite number in [lo, hi] (a bool is no number)."""
  if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
      not (math.isfinite(float(v)) and lo <= float(v) <= hi):
    raise ValueError("%s must be finite and %s (got %r)" % (name, ">= 0" if hi == math.inf else
                                                            "in [%g, %g]" % (lo, hi), v))
  return float(v)


def check_memory(required_bytes, sizes, too_large, too_full, free_bytes=None, allocate_model=True, index_range=None):
  """The two stages of a model's memory check; returns the bytes needed.  ``required_bytes(allocate_model)``:
  the model's device bytes; ``sizes``: what its messages name (n and K among them), to which the templates
  add need and hbm / free.  The whole fit against one device's HBM without touching a device, n * K against
  the kernels' index range (where ``index_range`` is a message), then what this call allocates against
  ``free_bytes`` (None: asked from the current device)."""
  whole = required_bytes(True)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError(too_large % dict(sizes, need=whole, hbm=DEVICE_HBM_BYTES))
  if index_range is not None and sizes["n"] * sizes["K"] >= 2 ** 40:
    raise ValueError(index_range % sizes)
  need = required_bytes(allocate_model)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError(too_full % dict(sizes, need=need, free=free_bytes))
  return need


def lists(rows, K, device, out=None):
  """(ids int32 [rows, K], values f32 [rows, K], count int32 [rows]): ``out`` checked, or new tensors."""
  if out is None:
    out = (torch.empty(rows, K, dtype=torch.int32, device=device),
           torch.empty(rows, K, dtype=torch.float32, device=device), torch.empty(rows, dtype=torch.int32, device=device))
  ids, w, count = out
  assert ids.shape == (rows, K) and ids.dtype == torch.int32 and ids.is_contiguous()
  assert w.shape == (rows, K) and w.dtype == torch.float32 and w.is_contiguous()
  assert count.shape == (rows,) and count.dtype == torch.int32
  return out


def workspace(ws, need, device):
  """``ws`` when it holds ``need`` bytes, else a new uint8 workspace."""
  return ws if ws is not None and ws.numel() >= need else torch.empty(need, dtype=torch.uint8, device=device)


def timed_fit(launch, count):
  """(kept, fit_ms) of ``launch()``: the total of ``count`` after it, read in the one host synchronisation,
  and the ms between HIP events around it."""
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
  ev[0].record()
  launch()
  ev[1].record()
  kept = int(count.sum(dtype=torch.int64).item())      # (the synchronisation)
  ev[1].synchronize()
  return kept, ev[0].elapsed_time(ev[1])


def scores(binding, symbol, csr, ids, w, count, lo=0, hi=None, out=None, ld=None, n_rows=None):
  """out[u, c] = sum_i x_ui W[i, lo + c] by ``symbol`` (rk_rp3_scores / rk_slim_scores) of the library that
  ``binding`` (_rp3_lib / _slim_lib) loads; rp3.scores and slim.scores say what W is."""
  lib = binding.load()
  n, K = ids.shape
  hi = n if hi is None else hi
  n_rows = csr.shape[0] if n_rows is None else n_rows
  assert ids.dtype == torch.int32 and w.dtype == torch.float32 and count.dtype == torch.int32
  assert ids.is_contiguous() and w.is_contiguous() and w.shape == (n, K) and count.shape == (n,)
  assert 0 <= lo < hi <= n and csr.shape[1] <= n
  if out is None:
    ld = hi - lo if ld is None else ld
    out = torch.empty(n_rows, ld, dtype=torch.float32, device=ids.device)
  ld = out.stride(0) if ld is None else ld
  binding.check(getattr(lib, symbol)(ptr(csr.indptr), ptr(csr.indices), ptr(csr.data), n_rows, n, ptr(ids),
                                     ptr(w), ptr(count), K, lo, hi, ptr(out), ld, current_stream()), symbol)
  return out
