#!/usr/bin/env python
"""PureSVD (recoder_amd/svd.py, librecoder_svd.so) on the MI355X: milliseconds per kernel and per fit,
the sparse product's gathered bytes per second against its bound, the same fit restated in torch ops
on the same GPU, and (--quality) the ranking metrics on the ML-20M slice over the rank.

    python tools/svd_bench.py [--quality] [--quick] [--out profiles/svd_bench.jsonl]

Data: the slice (tests/golden/real_ml20m_slice.npz, 10 000 x 7 915) and C2 = synthetic.ml20m_like
(116 677 x 20 108, 6.32 M nnz), at (h, l) = (4, 20), (64, 80), (200, 216), 6 power iterations.

Bounds: the sparse product gathers nnz * l * 4 bytes (from a table that fits L2 / Infinity Cache at these
sizes, so HBM's rate is a floor for it, not a ceiling) and writes rows * l * 4; the rotation moves
rows * (l + l2) * 4 bytes and does 2 * rows * l * l2 flop.

Rank matters: on the very sparse slice PureSVD is at its best at h = 4 (Recall@20 0.125 against
popularity's 0.108) and falls below popularity from about h = 16 on; --quality prints the curve.  Needs
the GPU: there is no CPU path."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_util import emit  # noqa: E402

SHAPES = [(4, 20), (64, 80), (200, 216)]
Q = 6
HBM_BPS = 8.0e12            # MI355X HBM3E
F32_MFMA_FLOPS = 157.3e12


def load_slice():
  z = np.load(os.path.join(ROOT, "tests", "golden", "real_ml20m_slice.npz"))
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


def timed(fn, reps):
  fn()                                     # warm-up (code objects)
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(reps):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / reps


def kernels(svd, als, uc, ic, l, reps):
  """Milliseconds of each kernel at width l, on buffers of the fit's shapes."""
  dev = uc.indptr.device
  n_users, n_items = uc.shape
  Z = svd.gaussian(n_items, l, 0)
  Qm = svd.spmm(uc, Z)
  Q2 = torch.empty_like(Qm)
  Z2 = torch.empty_like(Z)
  status = torch.zeros(1, dtype=torch.int32, device=dev)
  G, _ = als.gram(Qm, 0.0)
  Rinv = svd.chol_inverse(G, status)
  ms = dict(
      gaussian=timed(lambda: svd.gaussian(n_items, l, 0, out=Z2), reps),
      spmm_users=timed(lambda: svd.spmm(uc, Z, out=Q2), reps),
      spmm_items=timed(lambda: svd.spmm(ic, Qm, out=Z2), reps),
      gram_users=timed(lambda: als.gram(Qm, 0.0), reps),
      gram_items=timed(lambda: als.gram(Z, 0.0), reps),
      chol_inverse=timed(lambda: svd.chol_inverse(G, status), reps),
      rotate_users=timed(lambda: svd.rotate(Qm, Rinv, out=Q2), reps),
      rotate_items=timed(lambda: svd.rotate(Z, Rinv, out=Z2), reps))
  return ms


def torch_fit(At, AtT, h, l, q, omega):
  """The same algorithm in torch ops on the GPU: torch.sparse.mm, torch.mm, Cholesky on the host."""
  def orth(Y):
    for _ in range(2):
      G = (Y.T @ Y).double().cpu()
      R = torch.linalg.cholesky(G).T
      Rinv = torch.linalg.inv(R).float().to(Y.device)
      Y = Y @ Rinv
    return Y
  Z = omega
  Qm = orth(torch.sparse.mm(At, Z))
  Z = orth(torch.sparse.mm(AtT, Qm))
  for _ in range(q):
    Qm = orth(torch.sparse.mm(At, Z))
    Z = orth(torch.sparse.mm(AtT, Qm))
  W = torch.sparse.mm(At, Z)
  T = (W.T @ W).double().cpu().numpy()
  lam, S = np.linalg.eigh(T)
  S = torch.from_numpy(np.ascontiguousarray(S[:, ::-1][:, :h], dtype=np.float32)).to(Z.device)
  return W @ S, Z @ S, np.sqrt(np.maximum(lam[::-1][:h], 0))


def torch_csr(m, dev):
  m = sp.csr_matrix(m).astype(np.float32)
  return torch.sparse_csr_tensor(torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int64)),
                                 torch.from_numpy(m.data), size=m.shape).to(dev)


def metric_means(lists, y):
  from recoder_amd import metrics as M
  out = {}
  for k, kind in ((20, "recall"), (50, "recall"), (100, "ndcg")):
    vals = []
    for u in range(y.shape[0]):
      t = y.indices[y.indptr[u]:y.indptr[u + 1]]
      if len(t):
        vals.append(M.recall(lists[u], t, k) if kind == "recall" else M.ndcg(lists[u], t, k))
    out["%s@%d" % (kind, k)] = round(float(np.mean(vals)), 4)
  return out


def top_k(S, seen, k):
  S = np.array(S, np.float64)
  for u in range(S.shape[0]):
    S[u, seen.indices[seen.indptr[u]:seen.indptr[u + 1]]] = -np.inf
  return np.argsort(-S, axis=1, kind="stable")[:, :k]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--quality", action="store_true", help="Recall@20/50 and NDCG@100 on the slice over h")
  ap.add_argument("--quick", action="store_true", help="the slice only")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--reps", type=int, default=10)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_bench.jsonl"))
  args = ap.parse_args()
  from recoder_amd import als, svd, synthetic
  dev = torch.device("cuda")
  x, y = load_slice()
  sets = [("slice", lambda: x)] + ([] if args.quick else [("c2", synthetic.ml20m_like)])
  for name, gen in sets:
    m = sp.csr_matrix(gen()).astype(np.float32)
    uc, ic = als.csr_pair(m, m.shape[0], m.shape[1], dev)
    if not args.no_torch:
      At, AtT = torch_csr(m, dev), torch_csr(m.T.tocsr(), dev)
    for h, l in SHAPES:
      rec = {"bench": "svd", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h, "l": l,
             "power_iterations": Q}
      ms = kernels(svd, als, uc, ic, l, args.reps)
      rec["kernel_ms"] = {k: round(v, 4) for k, v in ms.items()}
      for side, rows in (("users", m.shape[0]), ("items", m.shape[1])):
        t = ms["spmm_" + side] * 1e-3
        gathered, written = float(m.nnz) * l * 4, float(rows) * l * 4
        rec["spmm_%s_gathered_GBps" % side] = round(gathered / t / 1e9, 1)
        rec["spmm_%s_share_of_hbm_bound" % side] = round((gathered + written) / HBM_BPS / t, 3)
        tr = ms["rotate_" + side] * 1e-3
        bound = max(float(rows) * 2 * l * 4 / HBM_BPS, 2.0 * rows * l * l / F32_MFMA_FLOPS)
        rec["rotate_%s_share_of_bound" % side] = round(bound / tr, 3)
      U = torch.empty(m.shape[0], h, device=dev)
      V = torch.empty(m.shape[1], h, device=dev)
      svd.fit(U, V, uc, ic, l - h, Q, 0)                    # warm-up
      torch.cuda.synchronize()
      fits = []
      for _ in range(3):
        t0 = time.perf_counter()
        info = svd.fit(U, V, uc, ic, l - h, Q, 0, residual=False)
        torch.cuda.synchronize()
        fits.append((time.perf_counter() - t0) * 1e3)
      info_r = svd.fit(U, V, uc, ic, l - h, Q, 0)
      rec["fit_ms"] = round(min(fits), 3)
      rec["fit_ms_all"] = [round(v, 3) for v in fits]
      rec["fit_split_ms"] = {k: round(info[k], 3) for k in ("spmm_ms", "orth_ms", "eig_ms")}
      rec["ritz_residual"] = info_r["ritz_residual"]
      rec["sigma_1"], rec["sigma_h"] = info["singular_values"][0], info["singular_values"][-1]
      if not args.no_torch:
        omega = svd.gaussian(m.shape[1], l, 0)
        torch_fit(At, AtT, h, l, Q, omega)                  # warm-up
        torch.cuda.synchronize()
        tf = []
        for _ in range(3):
          t0 = time.perf_counter()
          Ut, Vt, st = torch_fit(At, AtT, h, l, Q, omega)
          torch.cuda.synchronize()
          tf.append((time.perf_counter() - t0) * 1e3)
        rec["torch_fit_ms"] = round(min(tf), 3)
        rec["torch_fit_ms_all"] = [round(v, 3) for v in tf]
        rec["torch_over_hip"] = round(min(tf) / min(fits), 3)
        rec["sigma_rel_diff_vs_torch"] = float(np.abs(st - np.asarray(info["singular_values"])).max() / st[0])
      emit(rec, args.out)
  if args.quality:
    uc, ic = als.csr_pair(x, x.shape[0], x.shape[1], dev)
    pop = np.broadcast_to(np.asarray(x.sum(axis=0)).ravel().astype(np.float64), x.shape)
    emit({"bench": "svd_quality", "data": "slice", "model": "popularity", **metric_means(top_k(pop, x, 100), y)}, args.out)
    for h in (2, 4, 8, 16, 64):
      U = torch.empty(x.shape[0], h, device=dev)
      V = torch.empty(x.shape[1], h, device=dev)
      info = svd.fit(U, V, uc, ic, 16, Q, 0)
      S = U.double().cpu().numpy() @ V.double().cpu().numpy().T
      emit({"bench": "svd_quality", "data": "slice", "model": "puresvd", "h": h, "l": h + 16, "power_iterations": Q,
            "ritz_residual": info["ritz_residual"], **metric_means(top_k(S, x, 100), y)}, args.out)


if __name__ == "__main__":
  main()
