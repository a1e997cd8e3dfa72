#!/usr/bin/env python
"""WARP and dynamic negative sampling (recoder_amd/warp.py, rk_als_rank_sample / rk_als_warp_grad of
include/recoder_als.h): quality on the host, speed on an MI355X, one JSON line per record.

    python tools/warp_bench.py --cpu-grid [--jobs N] [--out FILE]
    python tools/warp_bench.py [--data slice|c2] [--h H] [--batch T] [--steps N] [--no-quality] [--out FILE]

  --cpu-grid  the float64 restatement (tests/warp_util.py) on the ML-20M slice at h = 64, batch 1024, no GPU:
              WARP over lr x reg x max_draws in {8, 32, 128} x both rank weights, measured after 5 and 10 epochs of
              one fit, and BPR with num_candidates in {1, 2, 4, 8, 16} at train_bpr's defaults, measured after 10,
              20 and 40 epochs.  Writes profiles/warp_quality.jsonl; train_warp's defaults are its best Recall@20
  otherwise   on the GPU: ms per step of a WARP step, a DNS step (num_candidates 4) and a train_bpr step; the
              split of a WARP step by kernel; rk_als_rank_sample in both modes beside the same work in torch ops
              (the gather of all max_draws candidate rows, a batched product, the selection); and, on the slice,
              Recoder.train_warp at its defaults: Recall@20 / NDCG@100, the share of valid slots and the mean
              trials per epoch.  Writes profiles/warp_bench.jsonl

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915, 118 k nnz); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_util import cpu_grid, emit, load, loop_ms  # noqa: E402

H, BATCH = 64, 1024
WARP_GRID = [(lr, reg, md, w) for lr in (0.005, 0.01, 0.02, 0.05) for reg in (0.01, 0.05) for md in (8, 32, 128)
             for w in ("log", "harmonic")]
WARP_EPOCHS = (5, 10)
DNS_GRID = (1, 2, 4, 8, 16)
BPR_LR, BPR_REG, BPR_EPOCHS = 0.1, 0.01, (10, 20, 40)       # (train_bpr's defaults)
SOURCE = "float64 restatement (tests/warp_util.py), host"


def grid_job(w):
  """One fit of the grid: its records, one per epoch count measured."""
  from tests import warp_util
  x, y = load("slice")
  if w[0] == "dns":
    rows = warp_util.quality_f64(x, y, H, BPR_EPOCHS, BATCH, BPR_LR, BPR_REG, num_candidates=w[1])
    return [{"bench": "dns_quality", "h": H, "lr": BPR_LR, "reg": BPR_REG, "batch_size": BATCH, "num_candidates": w[1],
             "num_epochs": ep, "recall20": round(r, 4), "ndcg100": round(n, 4), "loss": round(l, 4), "source": SOURCE}
            for ep, r, n, l, _, _ in rows]
  _, lr, reg, md, weight = w
  rows = warp_util.quality_f64(x, y, H, WARP_EPOCHS, BATCH, lr, reg, 1.0, md, weight)
  return [{"bench": "warp_quality", "h": H, "lr": lr, "reg": reg, "batch_size": BATCH, "margin": 1.0, "max_draws": md,
           "rank_weight": weight, "num_epochs": ep, "recall20": round(r, 4), "ndcg100": round(n, 4),
           "loss": round(l, 4), "valid_share": round(v, 4), "mean_trials": round(t, 3), "source": SOURCE}
          for ep, r, n, l, v, t in rows]


# ---------------------------------------------------------------------- GPU
def torch_rank_sample(X, Y, b, users, pos, C, cand, mode, num_candidates, margin):
  """rk_als_rank_sample's scoring and selection in torch ops on given draws: every candidate row of every slot
  is gathered and multiplied (nothing stops early), then the first violator / the hardest of M is picked."""
  import torch
  S = torch.bmm(Y[C], X[users][:, :, None])[:, :, 0] + b[C]
  rank = torch.cumsum(cand, 1)
  if mode == 0:
    s_pos = (X[users] * Y[pos]).sum(1) + b[pos]
    hit = cand & ((S - s_pos[:, None]) + margin > 0)
    at = torch.argmax(hit.to(torch.int8), 1)
    has = hit.any(1)
  else:
    taken = cand & (rank <= num_candidates)
    at = torch.argmax(torch.where(taken, S, torch.full_like(S, -float("inf"))), 1)
    has = taken.any(1)
  rows = torch.arange(len(users), device=X.device)
  return torch.where(has, C[rows, at], torch.full_like(at, -1)), torch.where(has, rank[rows, at], torch.zeros_like(at))


def speed(m, name, h, T, steps, out):
  import torch
  from bench_util import xavier_tables
  from recoder_amd import bpr, warp
  from tests import warp_util
  dev = torch.device("cuda")
  csr = bpr.user_csr(m, m.shape[0], m.shape[1], dev)
  rec = {"bench": "warp", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h,
         "batch_size": T, "steps": steps, "margin": 1.0, "max_draws": 32}
  lr, reg = 0.02, 0.01
  weight = torch.as_tensor(warp.weight_table(m.shape[1], "log"), device=dev)
  ws = warp.Workspace(T, h, dev)

  def tables():
    X, Y = xavier_tables(m.shape[0], m.shape[1], h, dev)
    return X, Y, torch.zeros(m.shape[1], device=dev)
  X, Y, b = tables()
  rec["warp_ms_per_step"] = loop_ms(lambda s: warp.step(X, Y, b, csr, ws, weight, 0, s, lr, reg, 1.0, 32), steps)[0]
  X, Y, b = tables()
  rec["dns4_ms_per_step"] = loop_ms(lambda s: bpr.step(X, Y, b, csr, ws, 0, s, 0.1, reg, 4), steps)[0]
  X, Y, b = tables()
  rec["bpr_ms_per_step"] = loop_ms(lambda s: bpr.step(X, Y, b, csr, ws, 0, s, 0.1, reg), steps)[0]
  # the kernels alone, at tables a short WARP fit leaves (trials then spread over several draws)
  X, Y, b = tables()
  for s in range(200):
    warp.step(X, Y, b, csr, ws, weight, 0, s, lr, reg, 1.0, 32)
  rec["mean_trials_at_timing"] = round(float(ws.trials.sum()) / max(1, int((ws.neg >= 0).sum())), 3)
  rec["valid_share_at_timing"] = round(float((ws.neg >= 0).float().mean()), 4)
  for mode, M, key in ((warp.WARP, 1, "warp"), (warp.DNS, 4, "dns4"), (warp.DNS, 16, "dns16")):
    rec["rank_sample_%s_ms" % key] = loop_ms(
        lambda s: warp.sample(csr, 0, s, X, Y, b, mode, 32, M, 1.0, ws.users, ws.pos, ws.neg, ws.trials, ws.s_pos,
                              ws.s_neg), steps)[0]
  rec["bpr_sample_ms"] = loop_ms(lambda s: bpr.sample(csr, 0, s, ws.users, ws.pos, ws.neg), steps)[0]
  rec["warp_grad_ms"] = loop_ms(lambda s: warp.grad(ws.users, ws.pos, ws.neg, ws.trials, X, Y, b, 1.0, weight, ws.g,
                                                    ws.loss, ws.D, ws.P), steps)[0]
  rec["bpr_grad_ms"] = loop_ms(lambda s: bpr.grad(ws.users, ws.pos, ws.neg, X, Y, b, ws.g, ws.loss, ws.D, ws.P),
                               steps)[0]
  # the torch-ops comparator: the draws (integer work) are given to it, only scoring and selection are timed
  sm = warp_util.Sampler(m)
  users, pos, C, cand = (torch.as_tensor(a, device=dev) for a in sm.draws(0, 0, T, 32))
  for mode, M, key in ((0, 1, "warp"), (1, 4, "dns4")):
    rec["torch_rank_sample_%s_ms" % key] = loop_ms(
        lambda s: torch_rank_sample(X, Y, b, users, pos, C, cand, mode, M, 1.0), steps)[0]
    rec["rank_sample_%s_vs_torch" % key] = round(rec["torch_rank_sample_%s_ms" % key] / rec["rank_sample_%s_ms" % key], 2)
  rec["note"] = "torch comparator excludes the hashing and the membership search, which the kernel's time includes"
  emit(rec, out)


def quality(out):
  import torch
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  x, y = load("slice")
  torch.manual_seed(0)
  rec = Recoder(model=MatrixFactorization(H), optimizer_type="adam")
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  hist = rec.train_warp(RecommendationDataset(x))
  e1.record()
  torch.cuda.synchronize()
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  r20, n100 = (float(np.nanmean(np.asarray(v, dtype=np.float64))) for v in res.values())
  emit({"bench": "warp_default_quality", "h": H, "num_epochs": len(hist), "recall20": round(r20, 4),
        "ndcg100": round(n100, 4), "loss": round(hist[-1], 4), "fit_ms": round(e0.elapsed_time(e1), 1),
        "valid_share": [round(v, 4) for v, _ in rec.warp_stats], "mean_trials": [round(t, 3) for _, t in rec.warp_stats],
        "source": "Recoder.train_warp at its defaults, MI355X"}, out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--jobs", type=int, default=8)
  ap.add_argument("--data", default="slice", choices=["c2", "slice"])
  ap.add_argument("--h", type=int, default=64)
  ap.add_argument("--batch", type=int, default=1024)
  ap.add_argument("--steps", type=int, default=50)
  ap.add_argument("--no-quality", action="store_true")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    work = [("dns", M) for M in DNS_GRID] + [("warp",) + g for g in WARP_GRID]
    cpu_grid(grid_job, work, args.jobs, args.out or os.path.join(ROOT, "profiles", "warp_quality.jsonl"))
    return
  out = args.out or os.path.join(ROOT, "profiles", "warp_bench.jsonl")
  m, _ = load(args.data)
  speed(m, args.data, args.h, args.batch, args.steps, out)
  if not args.no_quality:
    quality(out)


if __name__ == "__main__":
  main()
