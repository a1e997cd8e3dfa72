#!/usr/bin/env python
"""SLIM fit and serving times (recoder_amd/slim.py, include/recoder_slim.h), one JSON line per run:

    python tools/slim_bench.py [--data slice|c2] [--quality] [--no-torch] [--no-rp3] [--out FILE]

  hip     ms of the Gram (rk_ease_gram) and of rk_slim_fit (HIP events, second of two fits), the coordinate
          updates of the fit (sum over the columns of sweeps x candidates) and updates per second; users/s
          of rk_slim_scores + rk_topk_masked at B = 500, k = 100, beside rk_rp3_scores + rk_topk_masked on
          the same users (an RP3beta model of the same K fitted in the same run)
  torch   coordinate descent restated in torch ops on the same GPU, in a guarded step: every column at
          once, coordinate k of all of them as one rank-1 update of the dense n x n residual Q = G - G W
          (no screening: torch has no per-column candidate lists); ms of one such sweep, beside the HIP fit's
          ms divided by the mean sweeps of its columns
  quality (--quality, on the ML-20M slice) Recall@20 and NDCG@100 over a small (l1_reg, l2_reg, K) grid,
          beside popularity

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz; a dense Gram: nearly every pair is a candidate at a small l1_reg).
No number from this tool exists yet: it has not been run on an MI355X, and it fixes no target.
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_util import emit, load  # noqa: E402

L1, L2, NEIGHBOURS, MAX_SWEEPS, TOL, B, K = 1.0, 1000.0, 200, 50, 1e-5, 500, 100
GRID = [(1.0, 1000.0, 200), (1.0, 1000.0, 100), (1.0, 1000.0, 1024), (2.0, 1000.0, 200), (0.5, 1000.0, 200),
        (1.0, 500.0, 200), (1.0, 2000.0, 200), (5.0, 100.0, 200)]


def guarded(fn):
  try:
    return fn()
  except Exception as e:          # (an op this torch build lacks, or no room for the dense matrices: reported, not fatal)
    print("torch restatement step not available: %s: %s" % (type(e).__name__, e), file=sys.stderr)
    return None


def serve_time(rec, inp, reps=10):
  rec.recommend_array(inp, K)
  t0 = time.perf_counter()
  for _ in range(reps):
    rec.recommend_array(inp, K)              # (ends with its own device-to-host copy)
  return (time.perf_counter() - t0) / reps


def hip_side(x, out, with_rp3):
  from recoder_amd import als, ease, slim
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import RandomWalkItemModel, SparseLinearModel
  rec = Recoder(model=SparseLinearModel(L1, L2, NEIGHBOURS))
  ds = RecommendationDataset(x)
  rec.train_slim(ds, max_sweeps=MAX_SWEEPS, tol=TOL)      # warm: allocations, first touches, module load
  info = rec.train_slim(ds, max_sweeps=MAX_SWEEPS, tol=TOL)
  # the coordinate updates: the kernel's own sweeps per column times the column's candidates
  n = x.shape[1]
  pair = als.csr_pair(x, x.shape[0], n, "cuda")
  G = ease.gram(pair[0], pair[1], 0.0)
  diag = torch.diagonal(G)
  inv = torch.from_numpy(slim.inv_denom(diag.cpu().numpy(), L2)).cuda()
  ids = torch.empty(n, NEIGHBOURS, dtype=torch.int32, device="cuda")
  w = torch.empty(n, NEIGHBOURS, dtype=torch.float32, device="cuda")
  count, sweeps, support = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
  slim.fit_columns(G, inv, L1, ids, w, count, sweeps, support, MAX_SWEEPS, TOL)
  cands = torch.zeros(n, dtype=torch.int64, device="cuda")
  for lo in range(0, n, 4096):
    cands[lo:lo + 4096] = (G[lo:lo + 4096] > L1).sum(1)
  cands -= (diag > L1).to(torch.int64)
  updates = float((cands * sweeps.to(torch.int64)).sum().item())
  live = cands > 0
  mean_sweeps = float(sweeps[live].to(torch.float64).mean().item()) if bool(live.any()) else 0.0
  out.update(n=info["n"], nnz=info["nnz"], l1_reg=L1, l2_reg=L2, neighbours=NEIGHBOURS, max_sweeps=MAX_SWEEPS, tol=TOL,
             kept=info["kept"], cut_columns=info["cut_columns"], unconverged_columns=info["unconverged_columns"],
             max_sweeps_run=info["max_sweeps_run"], mean_sweeps=mean_sweeps, max_candidates=int(cands.max().item()),
             workspace_columns=int((cands > slim.LDS_CANDIDATES).sum().item()), gram_ms=info["gram_ms"],
             fit_ms=info["fit_ms"], updates=updates, updates_per_s=updates / (info["fit_ms"] * 1e-3),
             fit_ms_per_mean_sweep=info["fit_ms"] / mean_sweeps if mean_sweeps else None)
  del G, ids, w
  users = np.arange(min(B, x.shape[0]))
  inp = UsersInteractions(users, x[users])
  dt = serve_time(rec, inp)
  out.update(serve_batch=len(users), serve_k=K, serve_ms=dt * 1e3, serve_users_per_s=len(users) / dt)
  if with_rp3:
    rp3 = Recoder(model=RandomWalkItemModel(0.6, 0.3, NEIGHBOURS))
    rp3.train_rp3beta(ds)
    dr = serve_time(rp3, inp)
    out.update(rp3_serve_ms=dr * 1e3, rp3_serve_users_per_s=len(users) / dr, serve_speedup_vs_rp3=dr / dt)
    del rp3
  torch.cuda.empty_cache()
  return rec


def torch_sweep(x, sweeps=1):
  """ms of one sweep of the column-parallel coordinate descent in torch ops (dense, unscreened)."""
  from recoder_amd import slim
  dev = "cuda"
  X = torch.as_tensor(np.asarray(sp.csr_matrix(x).astype(np.float32).todense()), device=dev)
  G = X.T @ X
  del X
  n = G.shape[0]
  inv = torch.from_numpy(slim.inv_denom(torch.diagonal(G).cpu().numpy(), L2)).to(dev)
  W = torch.zeros(n, n, device=dev)
  Q = G.clone()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  a.record()
  for _ in range(sweeps):
    for k in range(n):
      t = torch.addcmul(Q[k], W[k], G[k, k])
      new = torch.clamp(t - L1, min=0) * inv[k]
      new[k] = 0
      d = new - W[k]
      Q.addr_(G[:, k], d, alpha=-1)
      W[k] = new
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / sweeps


def torch_side(x, out):
  res = guarded(lambda: (torch_sweep(x), torch_sweep(x))[1]) if x.shape[1] <= 2 ** 15 else None
  out["torch_sweep_ms"] = res
  if res is not None and out.get("fit_ms_per_mean_sweep"):
    out["sweep_speedup_vs_torch"] = res / out["fit_ms_per_mean_sweep"]


def quality(x, y, out):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import SparseLinearModel
  ds, ev = RecommendationDataset(x), RecommendationDataset(x, y)
  metrics = [Recall(k=20, normalize=True), NDCG(k=100)]
  grid = []
  for l1, l2, nb in GRID:
    rec = Recoder(model=SparseLinearModel(l1, l2, nb))
    info = rec.train_slim(ds, max_sweeps=MAX_SWEEPS, tol=TOL)
    res = rec.evaluate(ev, num_recommendations=100, metrics=metrics, batch_size=B)
    row = dict(l1_reg=l1, l2_reg=l2, neighbours=nb, kept=info["kept"], cut_columns=info["cut_columns"],
               unconverged_columns=info["unconverged_columns"], fit_ms=info["fit_ms"])
    row.update({str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()})
    print("SLIM %s" % row)
    grid.append(row)
  out["grid"] = grid
  # popularity: every user gets the most held items they have not seen (host: it is a baseline, not a kernel)
  from recoder_amd import metrics as M
  d = np.bincount(x.indices, minlength=x.shape[1])
  order = np.argsort(-d, kind="stable")
  vals = []
  for u in range(x.shape[0]):
    t = y.indices[y.indptr[u]:y.indptr[u + 1]]
    if len(t):
      seen = x.indices[x.indptr[u]:x.indptr[u + 1]]
      vals.append(M.recall(order[~np.isin(order, seen)][:20], t, 20))
  out["popularity_recall@20"] = float(np.mean(vals))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--data", choices=["c2", "slice"], action="append")
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--no-rp3", action="store_true")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slim_bench.jsonl"))
  args = ap.parse_args()
  for name in (args.data or ["slice"]):
    x, y = load(name)
    out = dict(bench="slim", data=name, users=int(x.shape[0]), device=torch.cuda.get_device_name(0))
    rec = hip_side(x, out, not args.no_rp3)
    if not args.no_torch:
      torch_side(x, out)
    if args.quality and y is not None:
      quality(x, y, out)
    emit(out, args.out)
    del rec
    torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
