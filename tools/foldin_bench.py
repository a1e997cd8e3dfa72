"""Fold-in of unseen users (recoder_amd/foldin.py, rk_als_foldin): quality on the CPU, time on the GPU.

  python tools/foldin_bench.py --cpu-grid     float64, no GPU -> profiles/foldin_quality.jsonl
      tests/golden/real_ml20m_slice.npz: the first 8 000 users are the fit, the last 2 000 are folded in from their
      training part and scored on their held-out part, over a grid of (alpha, reg); beside it popularity and the same
      figures for 2 000 users inside the fit, scored from their own rows.  States: ALS (tests/als_util.py: half_step
      at 3 CG steps, h = 32, 3 iterations, confidence 10, reg 100) and PureSVD (tests/svd_util.py: rsvd, h = 32).
      BPR and LightGCN restatements are not run: their host fits take longer than this tool should.
  python tools/foldin_bench.py --quality      GPU -> profiles/foldin_bench.jsonl
      ms per batch of 500 histories and users / s, the minimum of 5 timed loops with the largest beside it, on the
      slice and on the C2-shaped matrix (synthetic.ml20m_like) at h = 64 and 128: rk_als_foldin; rk_als_solve from
      a zero start at 3 and at h CG steps; the same solve in torch ops (A by einsum over the padded histories,
      torch.linalg.cholesky, cholesky_solve).  G is given to all of them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIT_USERS, FOLD_USERS = 8000, 2000
ALPHAS = (0.0, 1.0, 3.0, 10.0, 30.0, 100.0)
REGS = (0.1, 1.0, 10.0, 100.0, 1000.0)


def ndcg_at(lists, y, k=100):
  y = sp.csr_matrix(y)
  w = 1.0 / np.log2(2.0 + np.arange(k))
  out = []
  for u in range(y.shape[0]):
    t = y.indices[y.indptr[u]:y.indptr[u + 1]]
    if len(t):
      hit = np.isin(lists[u][:k], t)
      out.append(float((hit * w[:len(hit)]).sum() / w[:min(k, len(t))].sum()))
  return float(np.mean(out))


def fold_in64(x, Y, b, alpha, reg):
  """The float64 fold-in of every row of x: the exact solve of the user-side normal equations."""
  x = sp.csr_matrix(x)
  h = Y.shape[1]
  G = Y.T @ Y + reg * np.eye(h)
  v = Y.T @ b
  X = np.zeros((x.shape[0], h))
  for u in range(x.shape[0]):
    lo, hi = x.indptr[u], x.indptr[u + 1]
    cols, r = x.indices[lo:hi], x.data[lo:hi].astype(np.float64)
    a = np.where(r > 0, alpha, 0.0)
    y = Y[cols]
    A = G + (y * a[:, None]).T @ y
    X[u] = np.linalg.solve(A, y.T @ ((1 + a) * r - a * b[cols]) - v)
  return X


def cpu_grid(out):
  from tests import als_util, svd_util
  x, y = svd_util.load_slice()
  n_items = x.shape[1]
  xf, xo, yo = x[:FIT_USERS], x[FIT_USERS:FIT_USERS + FOLD_USERS], y[FIT_USERS:FIT_USERS + FOLD_USERS]
  xi, yi = x[:FOLD_USERS], y[:FOLD_USERS]
  h = 32

  def score(S, seen, tgt):
    lists = svd_util.top_k(S, seen, 100)
    return svd_util.recall_at(lists, tgt, 20), ndcg_at(lists, tgt, 100)
  pop = np.asarray(xf.sum(axis=0)).ravel().astype(np.float64)
  base = score(np.broadcast_to(pop, xo.shape), xo, yo)
  rows = [{"bench": "foldin_quality", "state": "popularity", "recall20": base[0], "ndcg100": base[1]}]
  # ALS
  t0 = time.perf_counter()
  rng = np.random.RandomState(0)
  X, Y, b = 0.01 * rng.randn(FIT_USERS, h), 0.01 * rng.randn(n_items, h), np.zeros(n_items)
  csc = xf.T.tocsr()
  for _ in range(3):
    X = als_util.half_step(xf, Y, X, b, 10.0, 100.0, 3, "user")
    Y = als_util.half_step(csc, X, Y, b, 10.0, 100.0, 3, "item")
  inside = score(X[:FOLD_USERS] @ Y.T, xi, yi)
  rows.append({"bench": "foldin_quality", "state": "als", "h": h, "fit": "als_util.half_step x 3, alpha 10, reg 100",
               "fit_s": round(time.perf_counter() - t0, 1), "inside_recall20": inside[0], "inside_ndcg100": inside[1]})
  best = None
  for alpha in ALPHAS:
    for reg in REGS:
      r20, n100 = score(fold_in64(xo, Y, b, alpha, reg) @ Y.T, xo, yo)
      rows.append({"bench": "foldin_quality", "state": "als", "alpha": alpha, "reg": reg, "recall20": r20,
                   "ndcg100": n100})
      if best is None or r20 > best[0]:
        best = (r20, alpha, reg)
  rows.append({"bench": "foldin_quality", "state": "als", "best_alpha": best[1], "best_reg": best[2],
               "best_recall20": best[0],
               "on_grid_edge": best[1] in (ALPHAS[0], ALPHAS[-1]) or best[2] in (REGS[0], REGS[-1])})
  # PureSVD
  _, V, Us = svd_util.rsvd(xf, h, 16, 6, svd_util.omega(n_items, h + 16, 0))
  inside = score(Us[:FOLD_USERS] @ V.T, xi, yi)
  rows.append({"bench": "foldin_quality", "state": "svd", "h": h, "inside_recall20": inside[0],
               "inside_ndcg100": inside[1]})
  for alpha, reg in ((0.0, 0.0), (0.0, 10.0), (10.0, 10.0), (10.0, 100.0)):
    r20, n100 = score(fold_in64(xo, V, np.zeros(n_items), alpha, reg) @ V.T, xo, yo)
    rows.append({"bench": "foldin_quality", "state": "svd", "alpha": alpha, "reg": reg, "recall20": r20,
                 "ndcg100": n100})
  with open(out, "w") as f:
    for r in rows:
      f.write(json.dumps(r) + "\n")
      print(json.dumps(r), flush=True)


# ---------------------------------------------------------------------------------------------------------- GPU
def timed(fn, loops=5, reps=10):
  """(min, max) ms per call over ``loops`` timed loops of ``reps`` calls, after a warm-up loop."""
  import torch
  for _ in range(2):
    fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  ms = []
  for _ in range(loops):
    e0.record()
    for _ in range(reps):
      fn()
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1) / reps)
  return min(ms), max(ms)


def torch_fold(indptr, indices, Y, G, v, b, alpha, width):
  """The same solve in torch ops on binary histories padded to ``width`` entries."""
  import torch
  B = indptr.shape[0] - 1
  lens = (indptr[1:] - indptr[:-1])
  pos = torch.arange(width, device=Y.device)[None, :]
  live = pos < lens[:, None]
  idx = (indptr[:-1, None] + pos).clamp(max=indices.shape[0] - 1)
  cols = indices[idx].long()
  y = Y[cols] * live[:, :, None]
  A = G[None] + alpha * torch.einsum("bek,bel->bkl", y, y)
  coef = ((1 + alpha) - alpha * b[cols]) * live
  rhs = torch.einsum("be,bek->bk", coef, y) - v[None]
  L = torch.linalg.cholesky(A)
  return torch.cholesky_solve(rhs[:, :, None], L)[:, :, 0]


def quality(out):
  import torch
  from recoder_amd import als, foldin, synthetic
  from tests import svd_util
  dev = torch.device("cuda")
  x, _ = svd_util.load_slice()
  sets = [("slice", x[FIT_USERS:]), ("c2", synthetic.ml20m_like()[:2000])]
  rows = []
  for name, m in sets:
    m = sp.csr_matrix(m)
    m.data[:] = 1.0
    n_items = m.shape[1]
    for h in (64, 128):
      g = torch.Generator(device="cpu").manual_seed(h)
      Y = (0.1 * torch.randn(n_items, h, generator=g)).to(dev)
      b = torch.zeros(n_items, device=dev)
      G, v = als.gram(Y, 10.0, b)
      batches = [als.AlsCSR(m[lo:lo + 500], dev) for lo in range(0, m.shape[0], 500)]
      widths = [int(np.diff(m[lo:lo + 500].indptr).max()) for lo in range(0, m.shape[0], 500)]
      X = torch.zeros(500, h, device=dev)
      st = torch.zeros(500, dtype=torch.int32, device=dev)
      nb = len(batches)

      def run_fold():
        for c in batches:
          foldin.solve(c, Y, G, v, b, 10.0, X=X, status=st)

      def run_cg(steps):
        def go():
          for c in batches:
            X.zero_()
            als.solve(c, Y, G, v, X, 10.0, steps, col_bias=b)
        return go

      def run_torch():
        for c, w in zip(batches, widths):
          torch_fold(c.indptr, c.indices, Y, G, v, b, 10.0, w)
      rec = {"bench": "foldin", "data": name, "users": m.shape[0], "items": n_items, "nnz": int(m.nnz), "h": h,
             "batch": 500}
      for key, fn in (("foldin", run_fold), ("cg3", run_cg(3)), ("cg_h", run_cg(h)), ("torch", run_torch)):
        lo, hi = timed(fn)
        rec[key + "_ms_per_batch"] = round(lo / nb, 4)
        rec[key + "_ms_per_batch_max"] = round(hi / nb, 4)
        rec[key + "_users_per_s"] = round(500 * nb / (lo * 1e-3))
      rows.append(rec)
      print(json.dumps(rec), flush=True)
  with open(out, "w") as f:
    for r in rows:
      f.write(json.dumps(r) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    cpu_grid(args.out or os.path.join(ROOT, "profiles", "foldin_quality.jsonl"))
  if args.quality:
    quality(args.out or os.path.join(ROOT, "profiles", "foldin_bench.jsonl"))


if __name__ == "__main__":
  main()
