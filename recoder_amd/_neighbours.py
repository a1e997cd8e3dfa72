"""What the two neighbour-list models share (recoder_amd.rp3 and recoder_amd.slim store an item-item
matrix as [n, K] ids, weights and counts): the check of ``neighbours`` and the wrapper of their scores
kernels, which take the same arguments."""
import numpy as np
import torch

from ._lib import ptr
from .device import current_stream


def check_neighbours(neighbours, max_neighbours):
  if isinstance(neighbours, bool) or not isinstance(neighbours, (int, np.integer)) or \
      not 1 <= neighbours <= max_neighbours:
    raise ValueError("neighbours must be an integer in [1, %d] (got %r)" % (max_neighbours, neighbours))
  return int(neighbours)


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
