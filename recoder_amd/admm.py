"""ADMM-SLIM (Steck, Dimakis, Riabov & Jebara, WSDM 2020, "ADMM SLIM: Sparse Recommendations for Many Users") for
``AdmmSlimModel``, on the HIP kernels of librecoder_ease.so (include/recoder_ease.h).

For the user x item matrix X (values as stored), G = X^T X and n items it minimises SLIM's objective over the whole
n x n matrix at once,

    1/2 |X - X B|_F^2 + l2_reg/2 |B|_F^2 + l1_reg |C|_1     subject to  B = C, diag(B) = 0  (and C >= 0 with nonneg),

by the alternating direction method of multipliers with penalty ``rho``.  With kappa = l2_reg + rho,
theta = l1_reg / rho, U the scaled dual and P = (G + kappa I)^-1 (EASE's Gram and inverse at reg = kappa):

    C = U = M = 0
    repeat num_iterations times:
        T      = rho (P M) - kappa P                    rk_ease_gemm      (P G = I - kappa P: G is not kept)
        gamma  = (diag(T) + 1) / diag(P)
        B      = T - P diag(gamma),  diag(B) = 0        rk_ease_admm_update, with all that follows
        V      = B + U
        C_new  = max(V - theta, 0) (nonneg)  or  sign(V) max(|V| - theta, 0)
        U      = V - C_new
        M      = C_new - U
    item_weights = C                                    (the sparse iterate, as in the paper's code)

With ``l1_reg`` = 0 and no sign constraint the fixed point is EASE's B at reg = l2_reg; ``rho`` has to be of the order
of l2_reg for that to be reached in a few dozen iterations.  One iteration is one dense n^3 product and one
element-wise pass; the fit holds P, C, U, M and the inverse's workspace, whose n x n image becomes T once the inverse
is done.

``Recoder.train_admm_slim`` is the public entry point; the functions below are the layer under it (and what the tests
and tools/admm_bench.py drive directly).
"""
import math

import numpy as np
import torch

from . import _ease_lib, _neighbours, als, ease
from ._lib import ptr
from .device import DEVICE_HBM_BYTES, current_stream


def check_not_distributed():
  als.check_not_distributed("train_admm_slim runs on one GPU: a multi-GPU ADMM-SLIM fit is not implemented")


def check_params(l1_reg, l2_reg, rho, num_iterations, nonneg):
  """(l1_reg, l2_reg, rho, num_iterations, nonneg), each checked: l1_reg, l2_reg >= 0, rho > 0, all finite, an
  integer iteration count >= 1, a bool."""
  l1_reg = _neighbours.check_number("l1_reg", l1_reg)
  l2_reg = _neighbours.check_number("l2_reg", l2_reg)
  if isinstance(rho, bool) or not isinstance(rho, (int, float, np.integer, np.floating)) or \
      not (math.isfinite(float(rho)) and float(rho) > 0):
    raise ValueError("rho must be finite and > 0 (got %r)" % (rho,))
  if isinstance(num_iterations, bool) or not isinstance(num_iterations, (int, np.integer)) or \
      not 1 <= num_iterations < 2 ** 31:
    raise ValueError("num_iterations must be an integer >= 1 (got %r)" % (num_iterations,))
  if not isinstance(nonneg, (bool, np.bool_)):
    raise ValueError("nonneg must be True or False (got %r)" % (nonneg,))
  return l1_reg, l2_reg, float(rho), int(num_iterations), bool(nonneg)


def check_config(model, l1_reg, l2_reg, rho, num_iterations, nonneg):
  """The ADMM-SLIM contract, checked before any GPU work; returns (l1_reg, l2_reg, rho, num_iterations, nonneg)."""
  from .nn import AdmmSlimModel
  if not isinstance(model, AdmmSlimModel):
    raise ValueError("train_admm_slim fits an AdmmSlimModel, not %s" % type(model).__name__)
  return check_params(l1_reg, l2_reg, rho, num_iterations, nonneg)


def check_values(host):
  """ValueError when a stored value is negative (or NaN); asked for with ``nonneg`` only, as SLIM does."""
  data = np.asarray(host.data)
  if data.size and not bool(np.all(data >= 0)):
    raise ValueError("ADMM-SLIM with nonneg needs interaction values >= 0: %d of the %d stored values are negative "
                     "or NaN" % (int((~(data >= 0)).sum()), data.size))


def _image_offset(n):
  """Byte offset of the n x n image (the carries) inside the workspace of rk_ease_spd_inverse: it comes last."""
  return ease.inverse_workspace_bytes(n) - int(n) * int(n) * 4


def required_bytes(n, num_iterations=1, allocate_matrix=True):
  """Device bytes a fit over n items allocates: C (the n x n fp32 model matrix, unless the caller already holds
  it), P, U and M, the inverse's workspace (its n x n image is T after the inverse: four n x n buffers beside
  it, not five), gamma and the three row statistics, the status word and the per-iteration sums."""
  n = int(n)
  return ((4 if allocate_matrix else 3) * n * n * 4 + ease.inverse_workspace_bytes(n) + 4 * n * 4 + 4
          + int(num_iterations) * 3 * 8)


def check_memory(n, num_iterations=1, free_bytes=None, allocate_matrix=True):
  """ValueError naming n and the bytes needed when the fit cannot fit: against one device's whole HBM without
  touching a device, then (``free_bytes`` None: asked from the current device) against what is free."""
  n = int(n)
  if n < 1:
    raise ValueError("ADMM-SLIM needs at least one item (got n = %d)" % n)
  whole = required_bytes(n, num_iterations, True)
  if whole > DEVICE_HBM_BYTES:
    raise ValueError("ADMM-SLIM over n = %d items needs %d bytes for its five n x n fp32 matrices: more than one "
                     "device's memory (%d bytes); multi-device fits are not implemented"
                     % (n, whole, DEVICE_HBM_BYTES))
  if n >= 2 ** 31 // 256:
    raise ValueError("ADMM-SLIM over n = %d items is outside the kernels' index range" % n)
  need = required_bytes(n, num_iterations, allocate_matrix)
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("ADMM-SLIM over n = %d items needs %d bytes of device memory, %d are free"
                     % (n, need, free_bytes))
  return need


# ------------------------------------------------------------------ kernels
def _ld(t):
  """Leading dimension of a 2-D tensor whose rows are contiguous (a one-row tensor's stride says nothing)."""
  assert t.dim() == 2 and t.dtype == torch.float32 and (t.stride(1) == 1 or t.shape[1] == 1)
  return max(t.shape[1], t.stride(0)) if t.shape[0] > 1 else t.shape[1]


def gemm(A, B, out, alpha=1.0, beta=0.0, E=None, row_lo=0, row_hi=None):
  """out[i, j] = alpha (A @ B)[i, j] + beta E[i, j] for i in [row_lo, row_hi) (rk_ease_gemm); ``E`` None (beta is
  ignored), ``out`` itself, or a tensor that does not overlap it.  Returns ``out``."""
  lib = _ease_lib.load()
  m, k = A.shape
  n = B.shape[1]
  row_hi = m if row_hi is None else row_hi
  assert B.shape[0] == k and out.shape == (m, n) and (E is None or E.shape == (m, n))
  _ease_lib.check(lib.rk_ease_gemm(ptr(A), _ld(A), ptr(B), _ld(B), None if E is None else ptr(E),
                                   0 if E is None else _ld(E), ptr(out), _ld(out), m, n, k, float(alpha), float(beta),
                                   row_lo, row_hi, current_stream()), "rk_ease_gemm")
  return out


def admm_update(T, P, C, U, M, theta, nonneg, gamma, row_primal, row_dual, row_nnz, row_lo=0, row_hi=None):
  """The element-wise pass of one iteration over the rows [row_lo, row_hi), in place (rk_ease_admm_update)."""
  lib = _ease_lib.load()
  n = T.shape[0]
  row_hi = n if row_hi is None else row_hi
  assert all(t.shape == (n, n) for t in (T, P, C, U, M))
  assert all(v.shape == (n,) and v.is_contiguous() for v in (gamma, row_primal, row_dual, row_nnz))
  assert gamma.dtype == row_primal.dtype == row_dual.dtype == torch.float32 and row_nnz.dtype == torch.int32
  _ease_lib.check(lib.rk_ease_admm_update(ptr(T), _ld(T), ptr(P), _ld(P), ptr(C), _ld(C), ptr(U), _ld(U), ptr(M),
                                          _ld(M), n, float(theta), int(bool(nonneg)), ptr(gamma), ptr(row_primal),
                                          ptr(row_dual), ptr(row_nnz), row_lo, row_hi, current_stream()),
                  "rk_ease_admm_update")


# ---------------------------------------------------------------------- fit
class State:
  """The buffers of a fit after the Gram and the inverse: P, T (inside the inverse's workspace), C, U, M and the
  vectors of the update.  ``iterate()`` runs one iteration and returns the device tensor
  (sum (B - C_new)^2, sum (C_new - C)^2, nnz of C_new) in float64, without synchronising."""

  def __init__(self, csr_pair, l2_reg, rho, out=None):
    ucsr, icsr = csr_pair
    n = ucsr.shape[1]
    dev = ucsr.indptr.device
    self.n, self.kappa, self.rho = n, float(l2_reg) + float(rho), float(rho)
    self.status = torch.zeros(1, dtype=torch.int32, device=dev)
    self.C = torch.empty(n, n, dtype=torch.float32, device=dev) if out is None else out
    assert self.C.shape == (n, n) and self.C.dtype == torch.float32 and self.C.is_contiguous()
    self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    self.ev[0].record()
    self.P = ease.gram(ucsr, icsr, self.kappa)
    self.ev[1].record()
    self.ws = ease.spd_inverse_async(self.P, self.status)
    self.ev[2].record()
    off = _image_offset(n)
    self.T = self.ws[off:off + n * n * 4].view(torch.float32).view(n, n)
    self.U = torch.empty(n, n, dtype=torch.float32, device=dev)
    self.M = torch.empty(n, n, dtype=torch.float32, device=dev)
    self.gamma, self.row_primal, self.row_dual = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
    self.row_nnz = torch.empty(n, dtype=torch.int32, device=dev)
    self.restart()

  def restart(self):
    for t in (self.C, self.U, self.M):
      t.zero_()

  def iterate(self, theta, nonneg):
    gemm(self.P, self.M, self.T, alpha=self.rho, beta=-self.kappa, E=self.P)
    admm_update(self.T, self.P, self.C, self.U, self.M, theta, nonneg, self.gamma, self.row_primal, self.row_dual,
                self.row_nnz)
    return torch.stack((self.row_primal.sum(dtype=torch.float64), self.row_dual.sum(dtype=torch.float64),
                        self.row_nnz.sum(dtype=torch.float64)))


def residuals(sums, rho):
  """(primal, dual) from the [iterations, 3] host array of ``State.iterate``'s sums: the Frobenius norms |B - C| and
  rho |C - C_previous| per iteration."""
  sums = np.asarray(sums, np.float64)
  return [float(v) for v in np.sqrt(sums[:, 0])], [float(rho) * float(v) for v in np.sqrt(sums[:, 1])]


def fit(csr_pair, l1_reg, l2_reg, rho, num_iterations, nonneg, out=None):
  """(C, info) for the (user-major, item-major) CSR pair of ``als.csr_pair``: the Gram at reg = l2_reg + rho, its
  inverse and ``num_iterations`` iterations; C lands in ``out`` when given.  One host synchronisation, at the
  end; ``info`` holds n, nnz, the hyperparameters, ``iterations``, ``primal_residual`` and ``dual_residual`` (per
  iteration: |B - C|_F and rho |C - C_previous|_F), ``density`` (the share of non-zeros of C) and gram_ms,
  inverse_ms and admm_ms from HIP events."""
  ucsr, icsr = csr_pair
  l1_reg, l2_reg, rho, num_iterations, nonneg = check_params(l1_reg, l2_reg, rho, num_iterations, nonneg)
  check_not_distributed()
  n = ucsr.shape[1]
  check_memory(n, num_iterations, allocate_matrix=out is None)
  st = State(csr_pair, l2_reg, rho, out)
  theta = l1_reg / rho
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  sums = torch.stack([st.iterate(theta, nonneg) for _ in range(num_iterations)])
  end.record()
  ease.raise_on_status(st.status)            # (the synchronisation)
  end.synchronize()
  sums = sums.cpu().numpy()
  primal, dual = residuals(sums, rho)
  info = dict(n=int(n), nnz=int(ucsr.nnz), l1_reg=l1_reg, l2_reg=l2_reg, rho=rho, nonneg=nonneg,
              iterations=num_iterations, primal_residual=primal, dual_residual=dual,
              density=float(sums[-1, 2]) / (float(n) * float(n)), gram_ms=st.ev[0].elapsed_time(st.ev[1]),
              inverse_ms=st.ev[1].elapsed_time(st.ev[2]), admm_ms=start.elapsed_time(end))
  return st.C, info
