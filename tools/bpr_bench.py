#!/usr/bin/env python
"""BPR step throughput and quality (recoder_amd/bpr.py, the rk_als_bpr_* part of include/recoder_als.h), one
JSON line per run:

    python tools/bpr_bench.py [--data c2|slice] [--h H] [--batch T] [--steps N] [--quality] [--no-torch] [--out FILE]

  hip     ms per step of bpr.step (HIP events over N steps after a warm-up) and triples/s; the per-kernel
          split of N instrumented steps: sample, grad, sort (torch.sort of the keys: plumbing), apply
          (users, items); the bytes grad and apply move over their times
  torch   the same step restated in torch ops on the GPU, on the same triples (gather, sigmoid,
          index_add_ for the sums -- atomics, so not bitwise repeatable -- and bincount for the counts):
          ms per step and the speed-up of the HIP path
  quality (--quality, on the ML-20M slice) Recall@20 / NDCG@100 of Recoder.train_bpr over a small
          (lr, reg, h) grid

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915, 118 k nnz); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz).  Writes profiles/bpr_bench.jsonl unless --out says otherwise.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_util import emit, load  # noqa: E402

LR, REG, EPOCHS, BATCH = 0.1, 0.01, 40, 1024          # (train_bpr's defaults)
GRID = [(0.1, 0.01, 64), (0.05, 0.01, 64), (0.2, 0.01, 64), (0.1, 0.002, 64), (0.1, 0.05, 64), (0.1, 0.01, 16),
        (0.1, 0.01, 128)]


def init_tables(n_users, n_items, h, dev):
  torch.manual_seed(0)
  X, Y = torch.empty(n_users, h), torch.empty(n_items, h)
  torch.nn.init.xavier_uniform_(X)
  torch.nn.init.xavier_uniform_(Y)
  return X.to(dev), Y.to(dev), torch.zeros(n_items, device=dev)


class Ev:
  def __init__(self):
    self.t = {}

  def time(self, name, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    self.t.setdefault(name, []).append((a, b))
    return r

  def ms(self):
    torch.cuda.synchronize()
    return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.t.items()}


def instrumented_steps(bpr, X, Y, b, csr, ws, steps, first):
  ev = Ev()
  for s in range(first, first + steps):
    ev.time("sample", lambda: bpr.sample(csr, 0, s, ws.users, ws.pos, ws.neg))
    ev.time("grad", lambda: bpr.grad(ws.users, ws.pos, ws.neg, X, Y, b, ws.g, ws.loss, ws.D, ws.P))
    (uk, uo), (ik, io) = ev.time("sort", lambda: bpr.sorted_keys(ws.users, ws.pos, ws.neg, X.shape[0], Y.shape[0]))
    ev.time("apply_users", lambda: bpr.apply(uk, uo, 1, ws.g, ws.D, LR, REG, X))
    ev.time("apply_items", lambda: bpr.apply(ik, io, 2, ws.g, ws.P, LR, REG, Y, b))
  return {k: v / steps for k, v in ev.ms().items()}


def torch_step(X, Y, b, users, pos, neg):
  """The step in torch ops, on given triples (int64 ids; neg < 0: invalid)."""
  ok = neg >= 0
  u, i, j = users[ok], pos[ok], neg[ok]
  P, D = X[u], Y[i] - Y[j]
  g = torch.sigmoid(-((P * D).sum(1) + b[i] - b[j]))
  sX = torch.zeros_like(X).index_add_(0, u, g[:, None] * D)
  gP = g[:, None] * P
  sY = torch.zeros_like(Y).index_add_(0, i, gP).index_add_(0, j, -gP)
  sb = torch.zeros_like(b).index_add_(0, i, g).index_add_(0, j, -g)
  cu = torch.bincount(u, minlength=X.shape[0]).float()
  ci = (torch.bincount(i, minlength=Y.shape[0]) + torch.bincount(j, minlength=Y.shape[0])).float()
  X += LR * (sX - REG * cu[:, None] * X)
  Y += LR * (sY - REG * ci[:, None] * Y)
  b += LR * (sb - REG * ci * b)


def throughput(m, name, h, T, steps, with_torch, out):
  from recoder_amd import bpr
  dev = torch.device("cuda")
  csr = bpr.user_csr(m, m.shape[0], m.shape[1], dev)
  rec = {"bench": "bpr", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h,
         "batch_size": T, "steps": steps, "lr": LR, "reg": REG}
  X, Y, b = init_tables(m.shape[0], m.shape[1], h, dev)
  ws = bpr.Workspace(T, h, dev)
  for s in range(3):                                      # warm-up (code objects, the sort's scratch)
    bpr.step(X, Y, b, csr, ws, 0, s, LR, REG)
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for s in range(3, 3 + steps):
    bpr.step(X, Y, b, csr, ws, 0, s, LR, REG)
  e1.record()
  torch.cuda.synchronize()
  rec["hip_ms_per_step"] = round(e0.elapsed_time(e1) / steps, 4)
  rec["triples_per_s"] = round(T / (rec["hip_ms_per_step"] * 1e-3))
  split = instrumented_steps(bpr, X, Y, b, csr, ws, steps, 3 + steps)
  rec["split_ms"] = {k: round(v, 4) for k, v in split.items()}
  # grad reads three rows and writes two per triple; an apply reads a staging row per entry and reads and writes a row
  rows = T * h * 4
  rec["grad_GBps"] = round(5 * rows / (split["grad"] * 1e-3) / 1e9, 1)
  rec["apply_users_GBps"] = round(3 * rows / (split["apply_users"] * 1e-3) / 1e9, 1)
  rec["apply_items_GBps"] = round(6 * rows / (split["apply_items"] * 1e-3) / 1e9, 1)
  if with_torch:
    X, Y, b = init_tables(m.shape[0], m.shape[1], h, dev)
    triples = []
    for s in range(steps + 1):
      bpr.sample(csr, 0, s, ws.users, ws.pos, ws.neg)
      triples.append((ws.users.long(), ws.pos.long(), ws.neg.long()))
    torch_step(X, Y, b, *triples[0])                      # warm-up
    torch.cuda.synchronize()
    e0.record()
    for tr in triples[1:]:
      torch_step(X, Y, b, *tr)
    e1.record()
    torch.cuda.synchronize()
    rec["torch_ms_per_step"] = round(e0.elapsed_time(e1) / steps, 4)
    rec["speedup_vs_torch"] = round(rec["torch_ms_per_step"] / rec["hip_ms_per_step"], 2)
  emit(rec, out)


def quality(out):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  x, y = load("slice")
  for lr, reg, h in GRID:
    torch.manual_seed(0)
    rec = Recoder(model=MatrixFactorization(h), optimizer_type="adam")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    hist = rec.train_bpr(RecommendationDataset(x), num_epochs=EPOCHS, batch_size=BATCH, lr=lr, reg=reg, seed=0)
    e1.record()
    torch.cuda.synchronize()
    res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                       metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
    r20, n100 = (float(np.nanmean(np.asarray(v, dtype=np.float64))) for v in res.values())
    emit({"bench": "bpr_quality", "lr": lr, "reg": reg, "h": h, "batch_size": BATCH, "num_epochs": EPOCHS,
          "recall20": round(r20, 4), "ndcg100": round(n100, 4), "loss": round(hist[-1], 4),
          "fit_ms": round(e0.elapsed_time(e1), 1), "source": "Recoder.train_bpr, MI355X"}, out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--data", default="c2", choices=["c2", "slice"])
  ap.add_argument("--h", type=int, default=64)
  ap.add_argument("--batch", type=int, default=4096)
  ap.add_argument("--steps", type=int, default=50)
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--no-torch", action="store_true")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpr_bench.jsonl"))
  args = ap.parse_args()
  m, _ = load(args.data)
  throughput(m, args.data, args.h, args.batch, args.steps, not args.no_torch, args.out)
  if args.quality:
    quality(args.out)


if __name__ == "__main__":
  main()
