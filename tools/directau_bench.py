#!/usr/bin/env python
"""DirectAU step throughput and quality (recoder_amd/directau.py, rk_als_dau_grad of include/recoder_als.h), one JSON
line per measurement:

    python tools/directau_bench.py [--h H] [--layers K] [--batch T] [--steps N] [--reps R] [--quality] [--out FILE]
    python tools/directau_bench.py --cpu-grid [--jobs J] [--out FILE]

  step       ms per directau.step on the ML-20M slice and on the C2-shaped matrix (HIP events over N steps after a
             warm-up; the minimum of R repetitions, the largest beside it) and the split of N instrumented steps:
             the forward propagation, the sampler, rk_als_dau_grad, the sorts / zeroing / scatters, the backward
             propagation, Adam; beside it rk_als_dau_grad alone and one pair of rk_als_gcl_contrast calls at the
             same T and h, a lightgcn.step at the same shape, and the same step in torch ops (torch.sparse.mm,
             F.normalize, torch.pdist, autograd, torch.optim.Adam)
  quality    (--quality, on the ML-20M slice) Recall@20 / NDCG@100 of Recoder.train_directau at its defaults
  cpu-grid   (--cpu-grid, no GPU) the float64 restatement of tests/directau_util.py on the ML-20M slice over GRID at
             h = 64, evaluated at the epochs of CHECKPOINTS, after the f32-beside-float64 gaps on the planted matrix
             that the margin of tests/test_directau.py is derived from; appends to profiles/directau_quality.jsonl

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915, 118 k nnz); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz).  Writes profiles/directau_bench.jsonl unless --out says otherwise.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_util import cpu_grid, emit, guarded, load, loop_ms, xavier_tables  # noqa: E402

H, BATCH, REG = 64, 1024, 1e-3
# (num_layers, gamma, lr): the paper's range of gamma, DirectAU-MF and a 2-layer encoder, three learning rates
GRID = [(K, g, lr) for K in (0, 2) for g in (0.2, 0.5, 1.0, 2.0, 5.0, 10.0) for lr in (0.003, 0.01, 0.03)]
CHECKPOINTS = (5, 10, 20)


# ----------------------------------------------------------------- cpu grid
def _grid_point(args):
  K, gamma, lr = args
  from tests import bpr_util, directau_util as du, lightgcn_util as lg
  x, y = bpr_util.load_slice()
  Eu, Ei, _ = bpr_util.xavier_tables(x.shape[0], x.shape[1], H, 0)
  rows = []

  def on_epoch(ep, state):
    if ep in CHECKPOINTS:
      P, Q = lg.forward(x, *state["E0"], K)
      r, n = du.quality(P, Q, x, y)
      rows.append((ep, float(r), float(n)))
  _, _, _, hist = du.fit(x, Eu, Ei, K, max(CHECKPOINTS), BATCH, lr, REG, gamma, seed=0, on_epoch=on_epoch)
  return [{"bench": "directau_quality", "num_layers": K, "gamma": gamma, "lr": lr, "reg": REG, "h": H,
           "batch_size": BATCH, "num_epochs": ep, "recall20": round(r, 4), "ndcg100": round(n, 4),
           "align": round(hist[ep - 1][0], 4), "unif_users": round(hist[ep - 1][1], 4),
           "unif_items": round(hist[ep - 1][2], 4),
           "source": "float64 restatement (tests/directau_util.py), CPU"} for ep, r, n in rows]


def _auc_gap(seed):
  """What tests/test_directau.py's held-out margin is derived from: its fit in f32 beside float64."""
  from tests import bpr_util, directau_util as du
  f32 = lambda v: float(np.float32(v))
  tr, ho = bpr_util.planted()
  start = bpr_util.init_tables(200, 120, 16, seed)[:2]
  zero = np.zeros(120)
  fits = [du.fit(tr, *start, 2, 5, 256, f32(0.05), f32(1e-3), 1.0, seed=seed, dtype=d)[:2] for d in (np.float64, np.float32)]
  a64, a32 = (bpr_util.auc(P, Q, zero, tr, ho) for P, Q in fits)
  return [{"bench": "directau_auc_gap", "data": "bpr_util.planted()", "seed": seed, "h": 16, "num_layers": 2,
           "batch_size": 256, "num_epochs": 5, "lr": 0.05, "reg": 1e-3, "gamma": 1.0,
           "auc_start": round(bpr_util.auc(*start, zero, tr, ho), 6), "auc_float64": round(a64, 6),
           "auc_float32": round(a32, 6), "auc_gap": abs(a64 - a32),
           "max_table_difference": [float(np.abs(a - b).max()) for a, b in zip(fits[0], fits[1])],
           "source": "float64 and f32 restatement (tests/directau_util.py), CPU"}]


def _job(job):
  return _auc_gap(job[1]) if job[0] == "gap" else _grid_point(job)


# ------------------------------------------------------------------ timing
def torch_step(m, graph, h, K, T, lr, reg, gamma):
  """The same step in torch ops on the same draws, as the paper's code writes the loss."""
  import torch
  import torch.nn.functional as Fn
  from recoder_amd import bpr
  dev = graph.su.device
  coo = m.tocoo()
  vals = graph.su.cpu().numpy()[coo.row].astype(np.float64) * graph.si.cpu().numpy()[coo.col]
  idx = torch.as_tensor(np.stack([coo.row, coo.col]), device=dev, dtype=torch.int64)
  A = torch.sparse_coo_tensor(idx, torch.as_tensor(vals, dtype=torch.float32, device=dev), m.shape).coalesce()
  At = A.t().coalesce()
  E = [torch.nn.Parameter(t) for t in xavier_tables(m.shape[0], m.shape[1], h, dev)]
  opt = torch.optim.Adam(E, lr=lr)
  users, pos, neg = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(3))
  unif = lambda z: torch.pdist(z, p=2).pow(2).mul(-2).exp().mean().log()

  def one(s):
    bpr.sample(graph.ucsr, 0, s, users, pos, neg)
    u, i = users.long(), pos.long()
    Pk, Qk = E
    P, Q = Pk, Qk
    for _ in range(K):
      Pk, Qk = torch.sparse.mm(A, Qk), torch.sparse.mm(At, Pk)
      P, Q = P + Pk, Q + Qk
    a, b = Fn.normalize(P[u] / (K + 1), dim=-1), Fn.normalize(Q[i] / (K + 1), dim=-1)
    loss = (a - b).norm(p=2, dim=1).pow(2).mean() + gamma * (unif(a) + unif(b)) / 2
    loss = loss + 0.5 * reg * (E[0][u].pow(2).sum() + E[1][i].pow(2).sum()) / T
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
  return one


def step_lines(m, name, h, K, T, steps, reps, out):
  import torch
  from recoder_amd import als, bpr, directau, lightgcn, simgcl
  dev = torch.device("cuda")
  graph = lightgcn.Graph(*als.csr_pair(m, m.shape[0], m.shape[1], dev))
  lr, reg, gamma = 0.01, REG, 1.0
  rec = {"bench": "directau_step", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h,
         "num_layers": K, "batch_size": T, "steps": steps, "repetitions": reps, "gamma": gamma}
  X, Y = xavier_tables(m.shape[0], m.shape[1], h, dev)
  state = directau.new_state(X, Y, K)
  ws = directau.Workspace(m.shape[0], m.shape[1], T, h, dev)
  run = lambda s: directau.step(X, Y, graph, state, ws, 0, s, lr, reg, gamma)
  rec["hip_ms_per_step"], rec["hip_ms_per_step_max"] = loop_ms(run, steps, reps)
  rec["slots_per_s"] = round(T / (rec["hip_ms_per_step"] * 1e-3))
  lstate, lws = lightgcn.new_state(X, Y, K), lightgcn.Workspace(m.shape[0], m.shape[1], T, h, dev)
  if K >= 1:
    rec["lightgcn_ms_per_step"], rec["lightgcn_ms_per_step_max"] = loop_ms(
        lambda s: lightgcn.step(X, Y, graph, lstate, lws, 0, s, lr, reg), steps, reps)
    rec["over_lightgcn_step"] = round(rec["hip_ms_per_step"] / rec["lightgcn_ms_per_step"], 3)
  # the loss-and-gradient call beside one pair of contrasts (users, items) at the same T and h
  b = ws.bpr
  bpr.sample(graph.ucsr, 0, 0, b.users, b.pos, b.neg)
  rec["dau_grad_ms"], rec["dau_grad_ms_max"] = loop_ms(
      lambda s: directau.grad(b.users, b.pos, X, Y, gamma, ws.raw, b.D, b.P, b.g, ws.loss, ws.valid_count), steps, reps)
  craw = torch.empty(simgcl.contrast_workspace_bytes(T, h), dtype=torch.uint8, device=dev)
  closs, ccount = torch.zeros(2, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
  keys = (torch.sort(b.users)[0], torch.sort(b.pos)[0])
  X2, Y2 = X + 0.01, Y + 0.01

  def pair(s):
    for side, (V1, V2) in enumerate(((X, X2), (Y, Y2))):
      simgcl.contrast(keys[side], V1, V2, 0.2, 0.5, ws.G[side], ws.G[side], craw, closs[side:side + 1],
                      ccount[side:side + 1])
  rec["contrast_pair_ms"], rec["contrast_pair_ms_max"] = loop_ms(pair, steps, reps)
  rec["distinct_users_items_of_the_pair"] = ccount.cpu().tolist()
  rec["dau_grad_faster_than_contrast_pair"] = rec["dau_grad_ms"] < rec["contrast_pair_ms"]
  # the split: the step's calls one by one between events
  parts = {}

  def timed(key, fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    parts.setdefault(key, []).append((a, z))

  def sums():
    for t in ws.G + ws.count:
      t.zero_()
    for side, (ids, V) in enumerate(((b.users, b.D), (b.pos, b.P))):
      k, o = directau.sorted_keys(ids, b.g, ws.G[side].shape[0])
      lightgcn.scatter(k, o, 1, b.g, V, -1.0, ws.G[side], ws.count[side])

  def adam_both():
    state["step"] += 1
    for side in (0, 1):
      lightgcn.adam(state["E0"][side], ws.H[side], ws.count[side], reg / T, state["M"][side], state["V"][side], lr,
                    state["step"])
  for s in range(10000, 10000 + steps):
    timed("propagate_forward", lambda: lightgcn.forward(graph, state["E0"], K, ws.layers, (X, Y)))
    timed("sample", lambda: bpr.sample(graph.ucsr, 0, s, b.users, b.pos, b.neg))
    timed("dau_grad", lambda: directau.grad(b.users, b.pos, X, Y, gamma, ws.raw, b.D, b.P, b.g, ws.loss, ws.valid_count))
    timed("sorts_zero_scatters", sums)
    timed("propagate_backward", lambda: lightgcn.forward(graph, ws.G, K, ws.layers, ws.H))
    timed("adam", adam_both)
  torch.cuda.synchronize()
  rec["split_ms"] = {k: round(sum(a.elapsed_time(z) for a, z in v) / steps, 4) for k, v in parts.items()}
  rec["dau_grad_share_of_step"] = round(rec["split_ms"]["dau_grad"] / sum(rec["split_ms"].values()), 4)
  rec["losses_last_step"] = [round(v, 4) for v in ws.loss.cpu().tolist()]

  def torch_ms():
    return loop_ms(torch_step(m, graph, h, K, T, lr, reg, gamma), steps, reps)
  t = guarded(torch_ms)
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
  d = {k: p.default for k, p in inspect.signature(Recoder.train_directau).parameters.items()
       if p.default is not inspect.Parameter.empty}
  torch.manual_seed(0)
  rec = Recoder(model=MatrixFactorization(H), optimizer_type="adam")
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  hist = rec.train_directau(RecommendationDataset(x))
  e1.record()
  torch.cuda.synchronize()
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  r20, n100 = (float(np.nanmean(np.asarray(v, dtype=np.float64))) for v in res.values())
  emit({"bench": "directau_quality", "num_layers": d["num_layers"], "gamma": d["gamma"], "lr": d["lr"],
        "reg": d["reg"], "h": H, "batch_size": d["batch_size"], "num_epochs": d["num_epochs"],
        "recall20": round(r20, 4), "ndcg100": round(n100, 4), "align": round(hist[-1][0], 4),
        "unif_users": round(hist[-1][1], 4), "unif_items": round(hist[-1][2], 4),
        "fit_ms": round(e0.elapsed_time(e1), 1), "source": "Recoder.train_directau, MI355X"}, out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--h", type=int, default=H)
  ap.add_argument("--layers", type=int, default=2)
  ap.add_argument("--batch", type=int, default=2048)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--jobs", type=int, default=16)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    return cpu_grid(_job, [("gap", s) for s in (0, 1, 2)] + GRID, args.jobs,
                    args.out or os.path.join(ROOT, "profiles", "directau_quality.jsonl"))
  import torch
  if not torch.cuda.is_available():
    sys.exit("directau_bench.py measures on the GPU (only --cpu-grid runs without one)")
  out = args.out or os.path.join(ROOT, "profiles", "directau_bench.jsonl")
  for name in ("slice", "c2"):
    m, _ = load(name)
    step_lines(m, name, args.h, args.layers, args.batch, args.steps, args.reps, out)
  if args.quality:
    quality(out)


if __name__ == "__main__":
  main()
