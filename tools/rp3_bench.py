#!/usr/bin/env python
"""RP3beta fit and serving times (recoder_amd/rp3.py, include/recoder_rp3.h), one JSON line per run:

    python tools/rp3_bench.py [--data c2|slice] [--quality] [--no-torch] [--no-ease] [--out FILE]

  hip     ms of rk_rp3_fit (HIP events, second of two fits) and co-occurrence adds per second, with
          adds = sum over the users of r_v^2 (what the accumulation performs); users/s of
          rk_rp3_scores + rk_topk_masked at B = 500, k = 100, beside rk_ease_scores + rk_topk_masked on
          the same users (an EASE model fitted at reg = 500 in the same run)
  torch   the fit restated in torch ops on the same GPU, in a guarded step (an op this torch build does
          not have is reported as null, not as a failure): row-blocked torch.sparse.mm of the item-major
          matrix with the dense, user-weighted matrix, the two scalings, the diagonal at 0 and torch.topk
  quality (--quality, on the ML-20M slice) Recall@20 and NDCG@100 over a small (alpha, beta, K) grid,
          beside popularity

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz: above rk_rp3_lds_items(), so the workspace path).
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
from bench_util import emit, guarded, load  # noqa: E402

ALPHA, BETA, NEIGHBOURS, B, K, EASE_REG = 0.6, 0.3, 100, 500, 100, 500.0
GRID = [(0.6, 0.3, 100), (0.6, 0.2, 100), (0.6, 0.3, 20), (0.6, 0.3, 200), (0.4, 0.3, 100), (0.8, 0.3, 100),
        (0.6, 0.0, 100), (1.0, 0.6, 100)]


def serve_time(rec, inp, reps=10):
  rec.recommend_array(inp, K)
  t0 = time.perf_counter()
  for _ in range(reps):
    rec.recommend_array(inp, K)              # (ends with its own device-to-host copy)
  return (time.perf_counter() - t0) / reps


def hip_side(x, out, with_ease):
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import RandomWalkItemModel, ShallowAutoencoder
  rec = Recoder(model=RandomWalkItemModel(ALPHA, BETA, NEIGHBOURS))
  ds = RecommendationDataset(x)
  rec.train_rp3beta(ds)                    # warm: allocations, first touches, module load
  info = rec.train_rp3beta(ds)
  adds = float((np.diff(x.indptr).astype(np.float64) ** 2).sum())
  out.update(n=info["n"], nnz=info["nnz"], alpha=ALPHA, beta=BETA, neighbours=NEIGHBOURS, kept=info["kept"],
             fit_ms=info["fit_ms"], adds=adds, adds_per_s=adds / (info["fit_ms"] * 1e-3))
  users = np.arange(min(B, x.shape[0]))
  inp = UsersInteractions(users, x[users])
  dt = serve_time(rec, inp)
  out.update(serve_batch=len(users), serve_k=K, serve_ms=dt * 1e3, serve_users_per_s=len(users) / dt)
  if with_ease:
    ease = Recoder(model=ShallowAutoencoder(EASE_REG))
    ease.train_ease(ds)
    de = serve_time(ease, inp)
    out.update(ease_serve_ms=de * 1e3, ease_serve_users_per_s=len(users) / de, serve_speedup_vs_ease=de / dt)
    del ease
    torch.cuda.empty_cache()
  return rec


def torch_fit(x, block=2048):
  """The fit in torch ops; returns (ids, w) of the top NEIGHBOURS per row (torch.topk's order among ties)."""
  from recoder_amd import rp3
  dev = "cuda"
  uw, rs, cs = (torch.from_numpy(a).to(dev) for a in rp3.weights(x, ALPHA, BETA))
  n = x.shape[1]
  xw = torch.as_tensor(np.asarray(sp.csr_matrix(x).astype(bool).astype(np.float32).todense()), device=dev)
  xw *= uw[:, None]
  xt = sp.csr_matrix(x).astype(bool).astype(np.float32).T.tocsr()
  ids = torch.empty(n, NEIGHBOURS, dtype=torch.int64, device=dev)
  w = torch.empty(n, NEIGHBOURS, dtype=torch.float32, device=dev)
  blocks = []
  for lo in range(0, n, block):
    c = xt[lo:lo + block].tocoo()
    blocks.append((lo, torch.sparse_coo_tensor(np.vstack([c.row, c.col]), c.data, c.shape).to(dev).coalesce()))
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  a.record()
  for lo, blk in blocks:
    hi = lo + blk.shape[0]
    W = torch.sparse.mm(blk, xw)
    W *= rs[lo:hi, None]
    W *= cs[None, :]
    W[torch.arange(hi - lo, device=dev), torch.arange(lo, hi, device=dev)] = 0
    w[lo:hi], ids[lo:hi] = torch.topk(W, min(NEIGHBOURS, n), dim=1)
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b)


def torch_side(x, out):
  res = guarded(lambda: (torch_fit(x), torch_fit(x))[1]) if x.shape[0] * x.shape[1] * 4 <= 2 ** 34 else None
  out["torch_fit_ms"] = res
  if res is not None:
    out["fit_speedup_vs_torch"] = res / out["fit_ms"]


def quality(x, y, out):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import RandomWalkItemModel
  ds, ev = RecommendationDataset(x), RecommendationDataset(x, y)
  metrics = [Recall(k=20, normalize=True), NDCG(k=100)]
  grid = []
  for alpha, beta, nb in GRID:
    rec = Recoder(model=RandomWalkItemModel(alpha, beta, nb))
    rec.train_rp3beta(ds)
    res = rec.evaluate(ev, num_recommendations=100, metrics=metrics, batch_size=B)
    row = dict(alpha=alpha, beta=beta, neighbours=nb)
    row.update({str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()})
    print("RP3beta %s" % row)
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
  ap.add_argument("--no-ease", action="store_true")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rp3_bench.jsonl"))
  args = ap.parse_args()
  for name in (args.data or ["slice", "c2"]):
    x, y = load(name)
    out = dict(bench="rp3", data=name, users=int(x.shape[0]), device=torch.cuda.get_device_name(0))
    rec = hip_side(x, out, not args.no_ease)
    if not args.no_torch:
      torch_side(x, out)
    if args.quality and y is not None:
      quality(x, y, out)
    emit(out, args.out)
    del rec
    torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
