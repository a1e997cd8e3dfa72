#!/usr/bin/env python
"""EASE fit and serving times (recoder_amd/ease.py, include/recoder_ease.h), one JSON line per run:

    python tools/ease_bench.py [--data c2|slice] [--quality] [--no-torch] [--out FILE]

  hip     ms of rk_ease_gram, rk_ease_spd_inverse and rk_ease_finalize (HIP events, second of two
          fits); the inverse's achieved TF against the 2 n^3 flop it performs and against the 157 TF
          f32-matrix peak; users/s and GB/s (d . n . 4 bytes gathered per user) of rk_ease_scores +
          rk_topk_masked at B = 500, k = 100
  torch   the same steps restated in torch ops on the same GPU, each in a guarded step of its own
          (one that this torch build does not have is reported as null, not as a failure):
          torch.sparse.mm for the Gram, torch.linalg.inv, a dense matmul + topk for the scores
  quality (--quality, on the ML-20M slice) Recall@20, Recall@50 and NDCG@100 at reg = 500, next to
          what tools/vae_bench.py --quality prints

Data: c2 = synthetic.ml20m_like(seed=0) (116 677 x 20 108, 6.32 M nnz); slice =
tests/golden/real_ml20m_slice.npz (10 000 x 7 915).  reg = 500.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_util import emit, load  # noqa: E402

REG, B, K = 500.0, 500, 100
F32_MATRIX_PEAK_TF = 157.0


def timed(fn, reps=1):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  a.record()
  for _ in range(reps):
    r = fn()
  b.record()
  torch.cuda.synchronize()
  return r, a.elapsed_time(b) / reps


def guarded(fn):
  try:
    return fn()
  except Exception as e:          # (an op this torch build lacks: reported, not fatal)
    print("torch restatement step not available: %s: %s" % (type(e).__name__, e), file=sys.stderr)
    return None


def hip_side(x, rec_out):
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ShallowAutoencoder
  rec = Recoder(model=ShallowAutoencoder(REG))
  ds = RecommendationDataset(x)
  rec.train_ease(ds)                       # warm: allocations, first touches, module load
  info = rec.train_ease(ds)
  n = info["n"]
  flop = 2.0 * n ** 3
  tf = flop / (info["inverse_ms"] * 1e-3) / 1e12
  rec_out.update(n=n, nnz=info["nnz"], reg=REG, gram_ms=info["gram_ms"], inverse_ms=info["inverse_ms"],
                 finalize_ms=info["finalize_ms"], inverse_flop="2n^3", inverse_tf=tf,
                 inverse_share_of_f32_peak=tf / F32_MATRIX_PEAK_TF)
  users = np.arange(min(B, x.shape[0]))
  inp = UsersInteractions(users, x[users])
  rec.recommend_array(inp, K)
  t0 = time.perf_counter()
  reps = 10
  for _ in range(reps):
    rec.recommend_array(inp, K)              # (ends with its own device-to-host copy)
  dt = (time.perf_counter() - t0) / reps
  gathered = float(x[users].nnz) * n * 4
  rec_out.update(serve_batch=len(users), serve_k=K, serve_ms=dt * 1e3, serve_users_per_s=len(users) / dt,
                 serve_gather_gb_per_s=gathered / dt / 1e9)
  return rec


def torch_side(x, rec, rec_out):
  dev = "cuda"
  n = x.shape[1]
  coo = x.tocoo()
  xt = guarded(lambda: torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]), coo.data.astype(np.float32),
                                               x.shape).to(dev).coalesce())

  def gram():
    xd = xt.to_dense() if x.shape[0] * n * 4 <= 2 ** 33 else None
    g = torch.sparse.mm(xt.t(), xd) if xd is not None else torch.sparse.mm(xt.t(), xt).to_dense()
    g.diagonal().add_(REG)
    return g
  res = guarded(lambda: timed(gram)) if xt is not None else None
  rec_out["torch_gram_ms"] = None if res is None else res[1]
  A = res[0] if res is not None else None
  if A is None:
    A = guarded(lambda: torch.as_tensor(np.asarray((x.T @ x).todense(), np.float32) + REG * np.eye(n, dtype=np.float32),
                                        device=dev))
  res = guarded(lambda: (torch.linalg.inv(A), timed(lambda: torch.linalg.inv(A)))[1]) if A is not None else None
  rec_out["torch_inverse_ms"] = None if res is None else res[1]
  if res is not None:
    rec_out["inverse_speedup_vs_torch"] = res[1] / rec_out["inverse_ms"]
  W = rec.model.item_weights.data
  users = np.arange(min(B, x.shape[0]))
  dense = torch.as_tensor(np.asarray(x[users].todense(), np.float32), device=dev)

  def serve():
    s = dense @ W
    s[dense > 0] = -float("inf")
    return torch.topk(s, K, dim=1)[1].cpu()
  res = guarded(lambda: (serve(), timed(serve, 10))[1])
  rec_out["torch_serve_ms"] = None if res is None else res[1]
  if res is not None:
    rec_out["serve_speedup_vs_torch"] = res[1] / rec_out["serve_ms"]


def quality(rec, x, y, rec_out):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), Recall(k=50, normalize=True), NDCG(k=100)],
                     batch_size=B)
  for k, v in res.items():
    rec_out[str(k)] = float(np.nanmean(np.asarray(v, np.float64)))
    print("EASE reg=%g %s: %.4f" % (REG, k, rec_out[str(k)]))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--data", choices=["c2", "slice"], action="append")
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ease_bench.jsonl"))
  args = ap.parse_args()
  for name in (args.data or ["slice", "c2"]):
    x, y = load(name)
    out = dict(bench="ease", data=name, users=int(x.shape[0]), device=torch.cuda.get_device_name(0))
    rec = hip_side(x, out)
    if not args.no_torch:
      torch_side(x, rec, out)
    if args.quality and y is not None:
      quality(rec, x, y, out)
    emit(out, args.out)
    del rec
    torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
