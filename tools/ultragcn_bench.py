#!/usr/bin/env python
"""UltraGCN step throughput and quality (recoder_amd/ultragcn.py, rk_als_ugcn_grad and rk_als_ugcn_scatter of
include/recoder_als.h), one JSON line per measurement:

    python tools/ultragcn_bench.py [--h H] [--batch T] [--steps N] [--reps R] [--quality] [--out FILE]
    python tools/ultragcn_bench.py --cpu-grid [--jobs J] [--lrs LR,..] [--checkpoints E,..] [--out FILE]
    python tools/ultragcn_bench.py --test-reference [--out FILE]

  step       ms per ultragcn.step on the ML-20M slice and on the C2-shaped matrix at (R, K) = (64, 10) and (512, 10)
             (HIP events over N steps after a warm-up; the minimum of R repetitions, the largest beside it) and the
             split of N instrumented steps: the sampler, rk_als_ugcn_grad, the two sorts with the zeroing, the users'
             rk_als_lgcn_scatter, rk_als_ugcn_scatter, Adam; beside it a bpr.step, a lightgcn.step at 3 layers, the
             item side done by staging the T E user rows and calling rk_als_lgcn_scatter, and the same step in torch
             ops (embedding, bmm, logsigmoid, autograd, index_add_ through autograd, torch.optim.Adam)
  quality    (--quality, on the ML-20M slice) Recall@20 / NDCG@100 of Recoder.train_ultragcn at its defaults
  cpu-grid   (--cpu-grid, no GPU) the float64 restatement of tests/ultragcn_util.py on the ML-20M slice over GRID at
             h = 64 and batch 1024, evaluated at the epochs of CHECKPOINTS; then the best cell under five seeds (the
             sampler's and the start's), whose spread is the margin of tests/test_ultragcn.py; appends to
             profiles/ultragcn_quality.jsonl.  --lrs and --checkpoints restrict the grid (what the records then cover
             is in their fields)

  test-reference  (--test-reference, no GPU) the float64 restatement of the two-epoch fit that tests/test_ultragcn.py
             runs through the kernels; appends to profiles/ultragcn_quality.jsonl

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915, 118 k nnz); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz).  Writes profiles/ultragcn_bench.jsonl unless --out says otherwise.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_util import cpu_grid, emit, guarded, load, loop_ms, xavier_tables  # noqa: E402

H, BATCH, REG, NEIGHBOURS = 64, 1024, 1e-3, 10
LRS, NEGATIVES, ITEM_WEIGHTS = (0.001, 0.003, 0.01), (32, 128, 512), (0.0, 1e-3, 1e-2, 0.1)
PAPER_W, PLAIN_W = (1e-7, 1.0, 1e-7, 1.0), (1.0, 0.0, 1.0, 0.0)
CHECKPOINTS = (5, 10, 20)
SEEDS = (0, 1, 2, 3, 4)


def grid(lrs=LRS):
  """(lr, R, negative_weight, item_weight, w) cells: every lr x R x (weight R, weight R / 4) at item_weight 1e-3 and
  the paper's w; the other item weights and the plain log-loss w at R = 128, weight 128, under every lr."""
  cells = [(lr, R, nw, 1e-3, PAPER_W) for lr in lrs for R in NEGATIVES for nw in (float(R), R / 4.0)]
  cells += [(lr, 128, 128.0, iw, PAPER_W) for lr in lrs for iw in ITEM_WEIGHTS if iw != 1e-3]
  cells += [(lr, 128, 128.0, 1e-3, PLAIN_W) for lr in lrs]
  return cells


# ----------------------------------------------------------------- cpu grid
def _grid_point(args):
  (lr, R, nw, iw, w), checkpoints, seed, lists = args
  from tests import bpr_util, ultragcn_util as uu
  x, y = bpr_util.load_slice()
  Eu, Ei, _ = bpr_util.xavier_tables(x.shape[0], x.shape[1], H, seed)
  cons = uu.Constraints(x, 0, 0.0)
  if iw > 0:
    cons.nbr_ids, cons.nbr_w = lists
  rows = []

  def on_epoch(ep, state):
    if ep in checkpoints:
      rows.append((ep,) + tuple(float(v) for v in uu.quality(*state["E0"], x, y)))
  _, _, _, hist = uu.fit(x, Eu, Ei, max(checkpoints), BATCH, lr, REG, R, nw, NEIGHBOURS, iw, w, seed=seed,
                         on_epoch=on_epoch, cons=cons)
  return [{"bench": "ultragcn_quality", "lr": lr, "num_negatives": R, "negative_weight": nw, "neighbours": NEIGHBOURS,
           "item_weight": iw, "w": list(w), "reg": REG, "h": H, "batch_size": BATCH, "seed": seed, "num_epochs": ep,
           "recall20": round(r, 4), "ndcg100": round(n, 4), "loss": [round(float(v), 5) for v in hist[ep - 1]],
           "source": "float64 restatement (tests/ultragcn_util.py), CPU"} for ep, r, n in rows]


def run_cpu_grid(jobs, lrs, checkpoints, out):
  import json
  from tests import bpr_util, ultragcn_util as uu
  lists = uu.item_graph(bpr_util.load_slice()[0], NEIGHBOURS)
  start = sum(1 for _ in open(out)) if os.path.exists(out) else 0
  cpu_grid(_grid_point, [(g, checkpoints, 0, lists) for g in grid(lrs)], jobs, out)
  recs = [json.loads(l) for l in open(out)][start:]
  best = max(recs, key=lambda r: r["recall20"])
  cell = (best["lr"], best["num_negatives"], best["negative_weight"], best["item_weight"], tuple(best["w"]))
  first = sum(1 for _ in open(out))
  cpu_grid(_grid_point, [(cell, (best["num_epochs"],), s, lists) for s in SEEDS], jobs, out)
  seeds = [json.loads(l) for l in open(out)][first:]
  r = [v["recall20"] for v in seeds]
  emit({"bench": "ultragcn_seed_spread", "cell": best, "seeds": list(SEEDS), "recall20": r,
        "recall20_spread": round(max(r) - min(r), 4), "ndcg100": [v["ndcg100"] for v in seeds],
        "source": "float64 restatement (tests/ultragcn_util.py), CPU"}, out)


TEST_CELL, TEST_EPOCHS = (0.01, 64, 64.0, 1e-3, PAPER_W), 2      # the fit of tests/test_ultragcn.py on the slice


def run_test_reference(out):
  """The float64 restatement of the end-to-end fit of tests/test_ultragcn.py: the figure its constant copies."""
  from tests import bpr_util, ultragcn_util as uu
  lists = uu.item_graph(bpr_util.load_slice()[0], NEIGHBOURS)
  for rec in _grid_point((TEST_CELL, (TEST_EPOCHS,), 0, lists)):
    emit(dict(rec, bench="ultragcn_test_reference"), out)


# ------------------------------------------------------------------ timing
def torch_step(m, graph, h, T, R, K, lists, bu, bi, lr, reg, nw, iw, w):
  """The same step in torch ops on the same slots: private uniform negatives from torch's generator."""
  import torch
  import torch.nn.functional as Fn
  from recoder_amd import bpr
  dev = graph.su.device
  E = [torch.nn.Parameter(t) for t in xavier_tables(m.shape[0], m.shape[1], h, dev)]
  opt = torch.optim.Adam(E, lr=lr)
  users, pos, neg = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(3))
  gen = torch.Generator(device=dev)
  ids, wts = lists
  safe = ids.clamp(min=0).long()

  def one(s):
    bpr.sample(graph.ucsr, 0, s, users, pos, neg)
    u, i = users.long(), pos.long()
    j = torch.randint(0, m.shape[1], (T, R), device=dev, generator=gen)
    cand = torch.cat([i[:, None], j, safe[i]], 1)
    p = Fn.embedding(u, E[0])
    s_ = torch.bmm(Fn.embedding(cand, E[1]), p[:, :, None])[:, :, 0]
    beta = bu[u][:, None] * bi[cand[:, :1 + R]]
    loss = ((w[0] + w[1] * beta[:, 0]) * -Fn.logsigmoid(s_[:, 0])).sum()
    loss = loss + (nw / R) * ((w[2] + w[3] * beta[:, 1:]) * -Fn.logsigmoid(-s_[:, 1:1 + R])).sum()
    loss = loss + iw * (wts[i] * (ids[i] >= 0) * -Fn.logsigmoid(s_[:, 1 + R:])).sum()
    loss = loss / T + 0.5 * reg * (p.pow(2).sum() + E[1][i].pow(2).sum()) / T
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
  return one


def step_lines(m, name, h, T, R, K, steps, reps, out):
  import torch
  from recoder_amd import als, bpr, lightgcn, ultragcn
  dev = torch.device("cuda")
  graph = lightgcn.Graph(*als.csr_pair(m, m.shape[0], m.shape[1], dev))
  lr, reg, nw, iw, w = 0.001, REG, float(R), 1e-3, PAPER_W
  E = 1 + R + K
  rec = {"bench": "ultragcn_step", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h,
         "batch_size": T, "num_negatives": R, "neighbours": K, "steps": steps, "repetitions": reps}
  X, Y = xavier_tables(m.shape[0], m.shape[1], h, dev)
  state = ultragcn.new_state(X, Y, 0)
  ws = ultragcn.Workspace(m.shape[0], m.shape[1], T, h, dev, num_negatives=R, neighbours=K)
  hyper = (R, nw, K, iw, w)
  rec["hip_ms_per_step"], rec["hip_ms_per_step_max"] = loop_ms(
      lambda s: ultragcn.step(X, Y, graph, state, ws, 0, s, lr, reg, *hyper), steps, reps)
  rec["slots_per_s"] = round(T / (rec["hip_ms_per_step"] * 1e-3))
  rec["gathered_bytes_per_step"] = 2 * T * E * h * 4
  b = ws.bpr
  bstate_X, bstate_Y = X.clone(), Y.clone()
  bws = bpr.Workspace(T, h, dev)
  zero_bias = torch.zeros(m.shape[1], device=dev)
  rec["bpr_ms_per_step"], rec["bpr_ms_per_step_max"] = loop_ms(
      lambda s: bpr.step(bstate_X, bstate_Y, zero_bias, graph.ucsr, bws, 0, s, 0.05, reg), steps, reps)
  lstate, lws = lightgcn.new_state(X, Y, 3), lightgcn.Workspace(m.shape[0], m.shape[1], T, h, dev)
  LX, LY = X.clone(), Y.clone()
  rec["lightgcn3_ms_per_step"], rec["lightgcn3_ms_per_step_max"] = loop_ms(
      lambda s: lightgcn.step(LX, LY, graph, lstate, lws, 0, s, 0.01, reg), steps, reps)
  rec["over_bpr_step"] = round(rec["hip_ms_per_step"] / rec["bpr_ms_per_step"], 3)
  rec["over_lightgcn3_step"] = round(rec["hip_ms_per_step"] / rec["lightgcn3_ms_per_step"], 3)
  parts = {}

  def timed(key, fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    parts.setdefault(key, []).append((a, z))
  sorted_ = {}

  def sorts():
    for t in ws.G + ws.count:
      t.zero_()
    sorted_["u"] = torch.sort(bpr.masked_keys(b.users, b.g > 0, X.shape[0]), stable=True)
    sorted_["i"] = torch.sort(ws.cand.view(-1), stable=True)

  def adam_both():
    state["step"] += 1
    for side in (0, 1):
      lightgcn.adam(state["E0"][side], ws.G[side], ws.count[side], reg / T, state["M"][side], state["V"][side], lr,
                    state["step"])
  stage = torch.empty((T * E, h), device=dev)
  ones = torch.ones(T * E, device=dev)

  def staged():
    torch.mul(X[b.users.long().clamp(0, X.shape[0] - 1)].repeat_interleave(E, 0), ws.coef.view(-1, 1), out=stage)
    lightgcn.scatter(sorted_["i"][0], sorted_["i"][1], 1, ones, stage, -1.0 / T, ws.G[1], ws.count[1])
  for s in range(10000, 10000 + steps):
    timed("sample", lambda: bpr.sample(graph.ucsr, 0, s, b.users, b.pos, b.neg))
    timed("ugcn_grad", lambda: ultragcn.grad(b.users, b.pos, R, K, 0, s, X, Y, ws.bu, ws.bi, ws.nbr_ids, ws.nbr_w, w,
                                             nw, iw, ws.cand, ws.coef, b.D, b.g, ws.loss))
    timed("sorts_zero", sorts)
    timed("lgcn_scatter_users", lambda: lightgcn.scatter(*sorted_["u"], 1, b.g, b.D, -1.0 / T, ws.G[0], ws.count[0]))
    timed("staged_rows_lgcn_scatter", staged)
    timed("ugcn_scatter", lambda: ultragcn.scatter(*sorted_["i"], E, b.users, ws.coef, X, 1.0 / T, ws.G[1],
                                                   ws.count[1]))
    timed("adam", adam_both)
  torch.cuda.synchronize()
  rec["split_ms"] = {k: round(sum(a.elapsed_time(z) for a, z in v) / steps, 4) for k, v in parts.items()}
  rec["scatter_faster_than_staging"] = rec["split_ms"]["ugcn_scatter"] < rec["split_ms"]["staged_rows_lgcn_scatter"]
  lists = (ws.nbr_ids, ws.nbr_w) if K else (torch.zeros((m.shape[1], 0), dtype=torch.int32, device=dev),
                                              torch.zeros((m.shape[1], 0), device=dev))
  t = guarded(lambda: loop_ms(torch_step(m, graph, h, T, R, K, lists, ws.bu, ws.bi, lr, reg, nw, iw, w), steps, reps))
  if isinstance(t, tuple):
    rec["torch_ops_step_ms"], rec["torch_ops_step_ms_max"] = t
    rec["step_faster_than_torch_ops"] = rec["hip_ms_per_step"] < rec["torch_ops_step_ms"]
  else:
    rec["torch_ops_step_ms"] = t
  emit(rec, out)


def quality(out):
  import inspect
  import torch
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  x, y = load("slice")
  d = {k: p.default for k, p in inspect.signature(Recoder.train_ultragcn).parameters.items()
       if p.default is not inspect.Parameter.empty}
  torch.manual_seed(0)
  rec = Recoder(model=MatrixFactorization(H), optimizer_type="adam")
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  hist = rec.train_ultragcn(RecommendationDataset(x))
  e1.record()
  torch.cuda.synchronize()
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  r20, n100 = (float(np.nanmean(np.asarray(v, dtype=np.float64))) for v in res.values())
  emit(dict({k: d[k] for k in ("num_epochs", "batch_size", "lr", "reg", "num_negatives", "negative_weight",
                               "neighbours", "item_weight")},
            bench="ultragcn_quality", w=list(d["w"]), h=H, recall20=round(r20, 4), ndcg100=round(n100, 4),
            loss=[round(v, 5) for v in hist[-1]], fit_ms=round(e0.elapsed_time(e1), 1),
            source="Recoder.train_ultragcn, MI355X"), out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--h", type=int, default=H)
  ap.add_argument("--batch", type=int, default=BATCH)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--test-reference", action="store_true")
  ap.add_argument("--jobs", type=int, default=16)
  ap.add_argument("--lrs", default=",".join(str(v) for v in LRS))
  ap.add_argument("--checkpoints", default=",".join(str(v) for v in CHECKPOINTS))
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.test_reference:
    return run_test_reference(args.out or os.path.join(ROOT, "profiles", "ultragcn_quality.jsonl"))
  if args.cpu_grid:
    return run_cpu_grid(args.jobs, tuple(float(v) for v in args.lrs.split(",")),
                        tuple(int(v) for v in args.checkpoints.split(",")),
                        args.out or os.path.join(ROOT, "profiles", "ultragcn_quality.jsonl"))
  import torch
  if not torch.cuda.is_available():
    sys.exit("ultragcn_bench.py measures on the GPU (only --cpu-grid runs without one)")
  out = args.out or os.path.join(ROOT, "profiles", "ultragcn_bench.jsonl")
  for name in ("slice", "c2"):
    m, _ = load(name)
    for R in (64, 512):
      step_lines(m, name, args.h, args.batch, R, NEIGHBOURS, args.steps, args.reps, out)
  if args.quality:
    quality(out)


if __name__ == "__main__":
  main()
