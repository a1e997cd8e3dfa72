#!/usr/bin/env python
"""SLIM fit and serving times (recoder_amd/slim.py, include/recoder_slim.h), one JSON line per run:

    python tools/slim_bench.py [--data slice|c2] [--quality] [--no-torch] [--no-rp3] [--out FILE]
    python tools/slim_bench.py --cpu-grid [--jobs N]        (no GPU) fsSLIM's quality grid on the slice by the float64
          restatement of tests/fsslim_util.py, into profiles/fsslim_quality.jsonl and tests/golden/fsslim_slice.json
    python tools/slim_bench.py --candidates [--data slice|c2|large]   fsSLIM's fit times at M = 100 and 200 beside the
          dense-Gram fit, into profiles/fsslim_bench.jsonl; large = synthetic.uniform(100 000, 1 000 000, 100), which
          the dense path refuses

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


# ------------------------------------------------------------ fsSLIM: the CPU cells
FS_GOLDEN = os.path.join(ROOT, "tests", "golden", "fsslim_slice.json")
FS_DENSE = dict(recall20=0.1301, ndcg100=0.1142)       # unrestricted SLIM at the same (l1, l2, K) on the slice
# (M, shrink, precision): cosine candidates; the f32 cell is the one the GPU test is held against
FS_CELLS = [(50, 0.0, "f64"), (100, 0.0, "f64"), (200, 0.0, "f64"), (400, 0.0, "f64"), (100, 300.0, "f64"),
            (100, 0.0, "f32")]


def fs_cell(cell):
  """One cell of the fsSLIM grid on the slice by the restatement of tests/fsslim_util.py at SLIM's defaults: the
  model cut to K, Recall@20 / NDCG@100 and the density.  float64: weights and scores in float64; f32: the kernels'
  chains (``cd_f32`` and the ascending f32 chain of rk_slim_scores)."""
  from tests import fsslim_util as fu, gfcf_util as gu, itemknn_util
  M, shrink, prec = cell
  x, y = load("slice")
  x64 = sp.csr_matrix(x).astype(np.float64)
  G = (x64.T @ x64).tocsr()
  n = x.shape[1]
  t0 = time.perf_counter()
  cand, cnt = fu.select(x, M, "cosine", shrink)
  passed = fu.screened(G, cand, cnt, L1)
  if prec == "f64":
    W, run = fu.cd_f64(G, cand, cnt, L1, L2, MAX_SWEEPS, TOL, K=NEIGHBOURS)
    kept = int(W.nnz)
    S = np.asarray((x64 @ W).todense())
  else:
    d = G.diagonal() + L2
    inv = np.where(d > 0, 1.0 / np.where(d > 0, d, 1.0), 0.0).astype(np.float32)
    ids, w, count, run, _ = fu.cd_f32(G, inv, cand, cnt, L1, NEIGHBOURS, MAX_SWEEPS, TOL)
    kept = int(count.sum())
    S = itemknn_util.scores_binary_f32(x, ids, w, count)
  r20, n100 = gu.quality(x, y, S=S)
  return [dict(bench="fsslim_quality", data="slice", precision=prec, candidates=M, candidate_similarity="cosine",
               candidate_shrink=shrink, l1_reg=L1, l2_reg=L2, neighbours=NEIGHBOURS, max_sweeps=MAX_SWEEPS, tol=TOL,
               recall20=r20, ndcg100=n100, density=kept / (n * n), kept=kept,
               mean_candidates=float(passed.mean()), max_sweeps_run=int(run.max()),
               dense_recall20=FS_DENSE["recall20"], dense_ndcg100=FS_DENSE["ndcg100"],
               seconds=round(time.perf_counter() - t0, 1))]


def fs_cpu_grid(out, jobs):
  import json
  import multiprocessing as mp
  with mp.get_context("spawn").Pool(min(jobs, len(FS_CELLS))) as pool:
    recs = [r for rs in pool.map(fs_cell, FS_CELLS) for r in rs]
  for r in recs:
    emit(r, out)
  at = {(r["candidates"], r["candidate_shrink"], r["precision"]): r for r in recs}
  f32, f64 = at[100, 0.0, "f32"], at[100, 0.0, "f64"]
  keys = ("candidates", "candidate_similarity", "candidate_shrink", "l1_reg", "l2_reg", "neighbours", "max_sweeps",
          "tol")
  golden = dict(params={k: f32[k] for k in keys},
                f32=dict(recall20=f32["recall20"], ndcg100=f32["ndcg100"], density=f32["density"],
                         mean_candidates=f32["mean_candidates"]),
                f64=dict(recall20=f64["recall20"], ndcg100=f64["ndcg100"], density=f64["density"]),
                recall20_f32_minus_f64=f32["recall20"] - f64["recall20"])
  with open(FS_GOLDEN, "w") as f:
    json.dump(golden, f, indent=1, sort_keys=True)
    f.write("\n")


# -------------------------------------------------------------- fsSLIM: the times
FS_LARGE = (100_000, 1_000_000, 100)     # synthetic.uniform(users, items, degree): a catalogue the dense path refuses


def fs_times(names, out, loops=5):
  """Per data set and M in (100, 200): the smallest of ``loops`` timed ``train_slim`` calls after a warm one (wall
  ms of the whole call, the ItemKNN candidate ms and the Gram-build + sweep ms of that call) with the largest
  beside it, and the dense-Gram ``train_slim`` on the slice."""
  from recoder_amd import slim, synthetic
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import SparseLinearModel

  def timed(ds, **kw):
    rec = Recoder(model=SparseLinearModel(L1, L2, NEIGHBOURS))
    rec.train_slim(ds, max_sweeps=MAX_SWEEPS, tol=TOL, **kw)
    rows = []
    for _ in range(loops):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      info = rec.train_slim(ds, max_sweeps=MAX_SWEEPS, tol=TOL, **kw)
      rows.append((time.perf_counter() - t0) * 1e3)
    best = int(np.argmin(rows))
    return dict(call_ms=rows[best], call_ms_max=max(rows), fit_ms=info["fit_ms"], gram_ms=info["gram_ms"],
                candidate_ms=info.get("candidate_ms"), mean_candidates=info.get("mean_candidates"), kept=info["kept"])

  for name in names:
    x = sp.csr_matrix(synthetic.uniform(*FS_LARGE)) if name == "large" else load(name)[0]
    ds = RecommendationDataset(x)
    base = dict(bench="fsslim", data=name, users=int(x.shape[0]), n=int(x.shape[1]), nnz=int(x.nnz), loops=loops,
                device=torch.cuda.get_device_name(0))
    # (the dense fit beside it where it ends in reasonable time: on c2 nearly every pair of the 20 108 items is a
    # candidate at l1 = 1, sweeps x candidates^2 per column; the large catalogue's Gram is refused outright)
    if name == "slice":
      emit(dict(base, candidates=None, **timed(ds)), out)
    for M in ((100,) if name == "large" else (100, 200)):
      emit(dict(base, candidates=M, **timed(ds, candidates=M)), out)
    torch.cuda.empty_cache()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--data", choices=["c2", "slice", "large"], action="append")
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--no-rp3", action="store_true")
  ap.add_argument("--cpu-grid", action="store_true", help="fsSLIM's float64 grid on the slice (no GPU)")
  ap.add_argument("--candidates", action="store_true", help="fsSLIM's fit times beside the dense-Gram fit")
  ap.add_argument("--jobs", type=int, default=6)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    return fs_cpu_grid(args.out or os.path.join(ROOT, "profiles", "fsslim_quality.jsonl"), args.jobs)
  if args.candidates:
    return fs_times(args.data or ["slice", "c2", "large"],
                    args.out or os.path.join(ROOT, "profiles", "fsslim_bench.jsonl"))
  args.out = args.out or os.path.join(ROOT, "profiles", "slim_bench.jsonl")
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
