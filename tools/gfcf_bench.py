#!/usr/bin/env python
"""GF-CF quality grid, fit and serving times (recoder_amd/gfcf.py, rk_ease_lowrank_add), one JSON line per record:

    python tools/gfcf_bench.py --cpu-grid [--out FILE]                     (no GPU)
    python tools/gfcf_bench.py [--data c2|slice] [--quality] [--no-torch] [--out FILE]

  --cpu-grid  the float64 restatement (tests/gfcf_util.py) on the ML-20M slice: Recall@20 / NDCG@100 over
          rank in {16, 64, 128, 256} x alpha in {0.1, 0.3, 1, 3, 10} with the exact eigenvectors of the
          normalised Gram and with the float64 randomized SVD (tests/svd_util.py, oversample 16, seed 0) at
          q in {2, 6} power iterations; the linear filter alone; then, at the (rank, alpha) whose exact
          Recall@20 is best, the randomized SVD at q = 6 over seeds 0..4 and the spread (max - min) of its
          Recall@20: the margin of tests/test_gfcf.py is twice that.  Into profiles/gfcf_quality.jsonl.
  hip     ms of the Gram, the randomized SVD and rk_ease_lowrank_add (HIP events, second of two fits); the
          kernel alone (mean of 10 after a warm call): TF/s on its 2 n^2 k flop, the share of the 157 TF
          f32-matrix peak, GB/s on its 8 n^2 bytes; users/s of rk_ease_scores + rk_topk_masked at B = 500,
          k = 100 (the path EASE serves through)
  torch   the same update in torch ops on the same GPU: A.addmm_ on scaled copies of V
  quality (--quality, on the slice) Recall@20, Recall@50 and NDCG@100 at the defaults, through the kernels

Data: c2 = synthetic.ml20m_like(seed=0) (116 677 x 20 108, 6.32 M nnz); slice =
tests/golden/real_ml20m_slice.npz (10 000 x 7 915).  Into profiles/gfcf_bench.jsonl.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_util import emit, event_ms, guarded, load  # noqa: E402

B, K = 500, 100
F32_MATRIX_PEAK_TF = 157.0
RANKS, ALPHAS, QS, SEEDS, OVERSAMPLE = (16, 64, 128, 256), (0.1, 0.3, 1.0, 3.0, 10.0), (2, 6), range(5), 16


# ------------------------------------------------------------------ the CPU grid
def cpu_grid(out):
  import scipy.sparse as sp
  from tests import gfcf_util as gu
  x, y = load("slice")
  x64 = sp.csr_matrix(x).astype(np.float64)
  _, di, dh = gu.scales_f64(x)
  G = gu.gram_f64(x)
  XG = np.asarray(x64 @ G)
  src = "float64 restatement (tests/gfcf_util.py), CPU"

  def point(V, rank, alpha, **tags):
    P, Q = np.asarray(x64 @ (di[:, None] * V)), V.T * dh[None, :]
    r20, n100 = gu.quality(x, y, S=XG + alpha * (P @ Q))
    emit(dict(bench="gfcf_quality", rank=rank, alpha=alpha, recall20=round(r20, 4), ndcg100=round(n100, 4),
              source=src, **tags), out)
    return r20

  r20, n100 = gu.quality(x, y, S=XG.copy())
  emit(dict(bench="gfcf_quality", basis="none (linear filter alone)", rank=0, alpha=0.0, recall20=round(r20, 4),
            ndcg100=round(n100, 4), source=src), out)
  t0 = time.perf_counter()
  sigma, E = gu.top_eigenvectors(G, max(RANKS))
  emit(dict(bench="gfcf_spectrum", eigh_s=round(time.perf_counter() - t0, 1),
            sigma=[round(float(s), 6) for s in sigma[[0, 1, 2, 3, 4, 5, 7, 15, 16, 63, 64, 127, 128, 255]]],
            sigma_at=[1, 2, 3, 4, 5, 6, 8, 16, 17, 64, 65, 128, 129, 256], source=src), out)
  best = (-1.0, None, None)
  for rank in RANKS:
    for alpha in ALPHAS:
      best = max(best, (point(E[:, :rank], rank, alpha, basis="exact"), rank, alpha))
  for q in QS:
    for rank in RANKS:
      V = gu.rsvd_basis(x, rank, OVERSAMPLE, q, 0)
      for alpha in ALPHAS:
        point(V, rank, alpha, basis="rsvd", q=q, oversample=OVERSAMPLE, seed=0)
  _, rank, alpha = best
  vals = [point(gu.rsvd_basis(x, rank, OVERSAMPLE, 6, s), rank, alpha, basis="rsvd", q=6, oversample=OVERSAMPLE,
                seed=s, spread_run=True) for s in SEEDS]
  emit(dict(bench="gfcf_quality_spread", rank=rank, alpha=alpha, q=6, oversample=OVERSAMPLE, seeds=list(SEEDS),
            recall20=[round(v, 6) for v in vals], spread=round(max(vals) - min(vals), 6),
            exact_recall20=round(best[0], 6), source=src), out)


# ------------------------------------------------------------------ the GPU runs
def hip_side(x, rec_out):
  import torch
  from recoder_amd import gfcf
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import GraphFilterModel
  rec = Recoder(model=GraphFilterModel())
  ds = RecommendationDataset(x)
  rec.train_gfcf(ds)                       # warm: allocations, first touches, module load
  info = rec.train_gfcf(ds)
  n, k = info["n"], info["rank"]
  rec_out.update(n=n, nnz=info["nnz"], rank=k, alpha=info["alpha"], l=info["l"], gram_ms=info["gram_ms"],
                 svd_ms=info["svd_ms"], filter_ms=info["filter_ms"], ritz_residual=info["ritz_residual"],
                 sigma_1=info["singular_values"][0], sigma_k=info["singular_values"][-1])
  # the kernel alone, on a scratch matrix of the model's size (the values do not change its time)
  V = rec.gfcf_info["V"]
  A = torch.zeros(n, n, device=V.device)
  a = torch.rand(n, device=V.device)
  ms = event_ms(lambda: gfcf.lowrank_add(A, V, a, a, 0.5), 10)
  tf = 2.0 * n * n * k / (ms * 1e-3) / 1e12
  rec_out.update(kernel_ms=ms, kernel_flop="2n^2k", kernel_tf=tf, kernel_share_of_f32_peak=tf / F32_MATRIX_PEAK_TF,
                 kernel_gb_per_s=8.0 * n * n / (ms * 1e-3) / 1e9)
  for kk in (16, 64):
    Vk = V[:, :kk].contiguous()
    ms = event_ms(lambda: gfcf.lowrank_add(A, Vk, a, a, 0.5), 10)
    rec_out["kernel_ms_k%d" % kk] = ms
    rec_out["kernel_gb_per_s_k%d" % kk] = 8.0 * n * n / (ms * 1e-3) / 1e9
  del A
  users = np.arange(min(B, x.shape[0]))
  inp = UsersInteractions(users, x[users])
  rec.recommend_array(inp, K)
  t0 = time.perf_counter()
  reps = 10
  for _ in range(reps):
    rec.recommend_array(inp, K)              # (ends with its own device-to-host copy)
  dt = (time.perf_counter() - t0) / reps
  rec_out.update(serve_batch=len(users), serve_k=K, serve_ms=dt * 1e3, serve_users_per_s=len(users) / dt)
  return rec


def torch_side(rec, rec_out):
  import torch
  V = rec.gfcf_info["V"]
  n = V.shape[0]

  def update():
    A = torch.zeros(n, n, device=V.device)
    a = torch.rand(n, device=V.device)
    return event_ms(lambda: A.addmm_(V * a[:, None], (V * a[:, None]).t(), alpha=0.5), 10)
  ms = guarded(update)
  rec_out["torch_addmm_ms"] = ms
  if ms is not None:
    rec_out["kernel_speedup_vs_torch"] = ms / rec_out["kernel_ms"]


def quality(rec, x, y, rec_out):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), Recall(k=50, normalize=True), NDCG(k=100)],
                     batch_size=B)
  for k, v in res.items():
    rec_out[str(k)] = float(np.nanmean(np.asarray(v, np.float64)))
    print("GF-CF rank=%d alpha=%g %s: %.4f" % (rec_out["rank"], rec_out["alpha"], k, rec_out[str(k)]))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--data", choices=["c2", "slice"], action="append")
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    return cpu_grid(args.out or os.path.join(ROOT, "profiles", "gfcf_quality.jsonl"))
  import torch
  out_file = args.out or os.path.join(ROOT, "profiles", "gfcf_bench.jsonl")
  for name in (args.data or ["slice", "c2"]):
    x, y = load(name)
    out = dict(bench="gfcf", data=name, users=int(x.shape[0]), device=torch.cuda.get_device_name(0))
    rec = hip_side(x, out)
    if not args.no_torch:
      torch_side(rec, out)
    if args.quality and y is not None:
      quality(rec, x, y, out)
    emit(out, out_file)
    del rec
    torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
