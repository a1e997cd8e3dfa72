"""PureSVD (Cremonesi, Koren & Turrin 2010) for ``MatrixFactorization``: a randomized truncated SVD
(Halko, Martinsson & Tropp 2011, algorithms 4.4 + 5.1) of the user x item matrix A, on the HIP kernels
of librecoder_svd.so (include/recoder_svd.h) and the Gram of librecoder_als.so.

With h = the embedding size, l = h + oversample and q power iterations:

    Omega [items, l] standard normal;  Q = orth(A Omega);  Z = orth(A^T Q)
    q times:  Q = orth(A Z);  Z = orth(A^T Q)
    W = A Z;  T = W^T W = S diag(lambda) S^T (float64, on the host);  sigma_k = sqrt(lambda_k)
    V = Z S[:, :h] (items),  U = W S[:, :h] = A V (users)

orth(Y) is Cholesky-QR done twice: G = Y^T Y, R = chol(G), Y <- Y R^-1.  The model's score
``U[u] . V[i]`` is then row u of ``A V V^T``: PureSVD.  The bias is 0.

``Recoder.train_svd`` is the public entry point; the functions below are the layer under it (and what
the tests and tools/svd_bench.py drive directly).
"""
import time

import numpy as np
import torch

from . import _svd_lib, als
from ._lib import ptr
from .device import DEVICE_HBM_BYTES, current_stream
from .nn import MatrixFactorization

MAX_L = 512                      # rk_svd_max_l()
LONG_ROW = _svd_lib.LONG_ROW     # rows this long take the sparse product's 16-wave path
_CHOL_LDS_L = 128                # (up to here rk_svd_chol_inverse needs no workspace)


def _is_int(v):
  return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


# ------------------------------------------------------------------ config
def check_config(model, oversample, num_power_iterations, seed):
  """The PureSVD contract, checked before any GPU work; returns (h, l)."""
  if not isinstance(model, MatrixFactorization):
    raise ValueError("train_svd fits a MatrixFactorization, not %s" % type(model).__name__)
  if model.activation_type != "none":
    raise ValueError("train_svd needs activation_type='none' (got %r)" % (model.activation_type,))
  if model.dropout_prob and model.dropout_prob > 0:
    raise ValueError("train_svd needs dropout_prob == 0 (got %r)" % (model.dropout_prob,))
  h = model.embedding_size
  if not _is_int(h) or h < 1:
    raise ValueError("train_svd needs an embedding size >= 1 (got %r)" % (h,))
  if not _is_int(oversample) or oversample < 0:
    raise ValueError("oversample must be an integer >= 0 (got %r)" % (oversample,))
  if h + oversample > MAX_L:
    raise ValueError("embedding size + oversample must be at most %d (got %d + %d)" % (MAX_L, h, oversample))
  if not _is_int(num_power_iterations) or num_power_iterations < 0:
    raise ValueError("num_power_iterations must be an integer >= 0 (got %r)" % (num_power_iterations,))
  if not _is_int(seed):
    raise ValueError("seed must be an integer (got %r)" % (seed,))
  return int(h), int(h + oversample)


def check_not_distributed():
  als.check_not_distributed("train_svd runs on one GPU: a multi-GPU PureSVD fit is not implemented")


def check_rank(l, n_users, n_items):
  if l > min(n_users, n_items):
    raise ValueError("embedding size + oversample = %d exceeds min(users, items) = %d: the sketch cannot have "
                     "more columns than the matrix has rows or columns" % (l, min(n_users, n_items)))


def required_bytes(n_users, n_items, l, nnz, with_data=True):
  """Device bytes a fit allocates: two [users, l] and two [items, l] fp32 buffers, the CSR and its
  transpose (int64 indptr, int32 indices, fp32 values unless all are 1), the Cholesky workspace."""
  n_users, n_items, l, nnz = int(n_users), int(n_items), int(l), int(nnz)
  csr = 2 * nnz * (8 if with_data else 4) + (n_users + n_items + 2) * 8
  return 2 * (n_users + n_items) * l * 4 + csr + (l * l * 8 if l > _CHOL_LDS_L else 0)


def check_memory(n_users, n_items, l, nnz, free_bytes=None):
  """ValueError naming the sizes and the bytes needed when the fit cannot fit: against one device's
  whole HBM without touching a device, then (``free_bytes`` None: asked from the current device)
  against what is free."""
  need = required_bytes(n_users, n_items, l, nnz)
  if need > DEVICE_HBM_BYTES:
    raise ValueError("PureSVD over %d users x %d items at l = %d needs %d bytes: more than one device's memory "
                     "(%d bytes); multi-device fits are not implemented"
                     % (n_users, n_items, l, need, DEVICE_HBM_BYTES))
  if free_bytes is None:
    free_bytes = torch.cuda.mem_get_info()[0]
  if need > free_bytes:
    raise ValueError("PureSVD over %d users x %d items at l = %d needs %d bytes of device memory, %d are free"
                     % (n_users, n_items, l, need, free_bytes))
  return need


# ------------------------------------------------------------------ kernels
def gaussian(rows, l, seed, out=None):
  """[rows, l] standard normals keyed on (seed, row, column) (rk_svd_gaussian)."""
  lib = _svd_lib.load()
  if out is None:
    out = torch.empty(rows, l, dtype=torch.float32, device="cuda")
  assert out.shape == (rows, l) and out.dtype == torch.float32 and (out.stride(1) == 1 or l == 1)
  ld = out.stride(0) if rows > 1 else l
  _svd_lib.check(lib.rk_svd_gaussian(ptr(out), rows, l, ld, int(seed) & (2 ** 64 - 1), current_stream()),
                 "rk_svd_gaussian")
  return out


def spmm(csr, F, out=None, row_lo=0, row_hi=None):
  """out[r] = sum_j a_rj F[col_j] over the stored entries of CSR row r in [row_lo, row_hi)
  (rk_svd_spmm).  ``csr``: an ``als.AlsCSR``; rows outside the range are left alone."""
  lib = _svd_lib.load()
  row_hi = csr.shape[0] if row_hi is None else row_hi
  l = F.shape[1]
  if out is None:
    out = torch.empty(csr.shape[0], l, dtype=torch.float32, device=F.device)
  assert 0 <= row_lo <= row_hi <= min(csr.shape[0], out.shape[0]) and F.shape[0] >= csr.shape[1]
  assert F.dtype == out.dtype == torch.float32 and out.shape[1] == l
  assert (F.stride(1) == 1 and out.stride(1) == 1) or l == 1
  ldf = F.stride(0) if F.shape[0] > 1 else l
  ldy = out.stride(0) if out.shape[0] > 1 else l
  _svd_lib.check(lib.rk_svd_spmm(ptr(csr.indptr), ptr(csr.indices), ptr(csr.data), row_lo, row_hi, ptr(F),
                                 ldf, l, ptr(out), ldy, current_stream()), "rk_svd_spmm")
  return out


def chol_workspace(l, device):
  need = _svd_lib.load().rk_svd_chol_inverse_workspace_bytes(l)
  return torch.empty(max(need, 16), dtype=torch.uint8, device=device)


def chol_inverse(G, status, ws=None):
  """R^-1 [l, l] (upper triangular, f32) for G = R^T R (rk_svd_chol_inverse); a breakdown is left in
  ``status`` (int32 [1] on the device, never cleared here) for the caller to read."""
  lib = _svd_lib.load()
  l = G.shape[0]
  assert G.shape == (l, l) and G.dtype == torch.float32 and G.is_contiguous()
  need = lib.rk_svd_chol_inverse_workspace_bytes(l)
  if ws is None or ws.numel() < need:
    ws = chol_workspace(l, G.device)
  Rinv = torch.empty(l, l, dtype=torch.float32, device=G.device)
  _svd_lib.check(lib.rk_svd_chol_inverse(ptr(G), l, ptr(Rinv), ptr(ws), ws.numel(), ptr(status),
                                         current_stream()), "rk_svd_chol_inverse")
  return Rinv


def rotate(Y, M, out=None):
  """out = Y M for a tall Y [rows, l] and a small M [l, l2], out of place (rk_svd_rotate)."""
  lib = _svd_lib.load()
  rows, l = Y.shape
  l2 = M.shape[1]
  if out is None:
    out = torch.empty(rows, l2, dtype=torch.float32, device=Y.device)
  assert M.shape[0] == l and out.shape == (rows, l2) and Y.dtype == M.dtype == out.dtype == torch.float32
  assert (Y.stride(1) == 1 or l == 1) and (M.stride(1) == 1 or l2 == 1) and (out.stride(1) == 1 or l2 == 1)
  assert out.data_ptr() != Y.data_ptr()
  ldy = Y.stride(0) if rows > 1 else l
  ldm = M.stride(0) if l > 1 else l2
  ldo = out.stride(0) if rows > 1 else l2
  _svd_lib.check(lib.rk_svd_rotate(ptr(Y), rows, l, ldy, ptr(M), l2, ldm, ptr(out), ldo, current_stream()),
                 "rk_svd_rotate")
  return out


def raise_on_status(status, l):
  s = int(status.cpu().item())
  if s:
    raise RuntimeError("the matrix's numerical rank is below embedding size + oversample = %d (pivot %d of a "
                       "Cholesky factorisation of the sketch's Gram broke down): lower them" % (l, s - 1))


def orthonormalize(Y, tmp=None, status=None, ws=None, gws=None):
  """Y <- an orthonormal basis of its columns, by Cholesky-QR done twice (through ``tmp``, back into Y).
  ``status`` None: read back here, RuntimeError on a breakdown; otherwise left for the caller."""
  own = status is None
  if own:
    status = torch.zeros(1, dtype=torch.int32, device=Y.device)
  if tmp is None:
    tmp = torch.empty_like(Y)
  a, b = Y, tmp
  for _ in range(2):
    G, _v = als.gram(a, 0.0, None, gws)
    rotate(a, chol_inverse(G, status, ws), out=b)
    a, b = b, a
  if own:
    raise_on_status(status, Y.shape[1])
  return Y


# ---------------------------------------------------------------------- fit
class _Phases:
  """HIP events at the phase boundaries; the milliseconds per label after the synchronisation."""

  def __init__(self):
    self.events, self.labels = [self._mark()], []

  @staticmethod
  def _mark():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e

  def done(self, label):
    self.events.append(self._mark())
    self.labels.append(label)

  def totals(self):
    self.events[-1].synchronize()
    out = {}
    for a, b, label in zip(self.events[:-1], self.events[1:], self.labels):
      out[label] = out.get(label, 0.0) + a.elapsed_time(b)
    out.pop("_host", None)
    return out


def eig_host(T, h):
  """(sigma [h] descending, S [l, h]) from T = W^T W: float64 eigh, the top h pairs, the sign of every
  column fixed so that its largest-magnitude entry is positive."""
  T = np.asarray(T, np.float64)
  lam, S = np.linalg.eigh((T + T.T) / 2)
  order = np.argsort(-lam, kind="stable")[:h]
  lam, S = lam[order], S[:, order]
  big = np.abs(S).argmax(axis=0)
  S = S * np.where(S[big, np.arange(S.shape[1])] < 0, -1.0, 1.0)[None, :]
  return np.sqrt(np.maximum(lam, 0.0)), S


def fit(U, V, ucsr, icsr, oversample, num_power_iterations, seed, omega=None, residual=True):
  """The randomized SVD of the CSR pair of ``als.csr_pair`` into the tables U [users, h], V [items, h]
  (in place, f32, row-major).  ``omega`` ([items, l]) replaces the seeded Gaussian.  One host
  synchronisation (the l x l eigendecomposition, where the status word is read too), one more for the
  Ritz residual when it is asked for.  Returns ``info``."""
  n_users, h = U.shape
  n_items = V.shape[0]
  l = h + int(oversample)
  assert V.shape[1] == h and ucsr.shape == (n_users, n_items) and icsr.shape == (n_items, n_users)
  assert 1 <= h <= l <= MAX_L
  check_rank(l, n_users, n_items)
  dev = U.device
  lib = als._als_lib.load()
  gws = torch.empty(max(lib.rk_als_gram_workspace_bytes(n_users, l), lib.rk_als_gram_workspace_bytes(n_items, l), 4),
                    dtype=torch.uint8, device=dev)
  ws = chol_workspace(l, dev)
  status = torch.zeros(1, dtype=torch.int32, device=dev)
  Qa, Qb = (torch.empty(n_users, l, dtype=torch.float32, device=dev) for _ in range(2))
  Za, Zb = (torch.empty(n_items, l, dtype=torch.float32, device=dev) for _ in range(2))
  if omega is None:
    gaussian(n_items, l, seed, out=Za)
  else:
    Za.copy_(torch.as_tensor(np.asarray(omega, np.float32) if not torch.is_tensor(omega) else omega).reshape(n_items, l))
  ph = _Phases()

  def product(csr, F, out, tmp):
    spmm(csr, F, out=out)
    ph.done("spmm_ms")
    orthonormalize(out, tmp, status, ws, gws)
    ph.done("orth_ms")

  product(ucsr, Za, Qa, Qb)
  product(icsr, Qa, Za, Zb)
  for _ in range(int(num_power_iterations)):
    product(ucsr, Za, Qa, Qb)
    product(icsr, Qa, Za, Zb)
  W = spmm(ucsr, Za, out=Qa)
  ph.done("spmm_ms")
  T, _v = als.gram(W, 0.0, None, gws)
  ph.done("orth_ms")
  T_host = T.cpu().numpy()               # (the synchronisation)
  raise_on_status(status, l)
  if not np.all(np.isfinite(T_host)):
    raise RuntimeError("the sketch of the matrix is not finite (non-finite values in the interaction matrix?)")
  t0 = time.perf_counter()
  sigma, S = eig_host(T_host, h)
  eig_ms = (time.perf_counter() - t0) * 1e3
  ph.done("_host")                       # (the device sat idle: not a kernel's time)
  Sd = torch.from_numpy(np.ascontiguousarray(S, dtype=np.float32)).to(dev)
  rotate(Za, Sd, out=V)
  rotate(W, Sd, out=U)
  ph.done("orth_ms")
  info = dict(h=int(h), l=int(l), nnz=int(ucsr.nnz), singular_values=[float(s) for s in sigma])
  if residual:
    # max_k |A^T u_k - sigma_k^2 v_k| / sigma_1^2: how far the pairs are from singular pairs of A
    AtU = spmm(icsr, U.contiguous() if U.stride(1) != 1 else U)
    ph.done("spmm_ms")
    sig2 = torch.from_numpy(sigma ** 2).to(dev)
    r = (AtU.double() - V.double() * sig2[None, :]).norm(dim=0).max() / max(float(sigma[0]) ** 2, 1e-300)
    info["ritz_residual"] = float(r.item())
  else:
    info["ritz_residual"] = None
  info.update(dict(spmm_ms=0.0, orth_ms=0.0))
  info.update(ph.totals())
  info["eig_ms"] = eig_ms
  return info
