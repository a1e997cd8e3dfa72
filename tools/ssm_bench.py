#!/usr/bin/env python
"""Sampled-softmax step throughput and quality (recoder_amd/ssm.py, rk_als_ssm_grad of include/recoder_als.h), one
JSON line per measurement:

    python tools/ssm_bench.py [--h H] [--layers K] [--batch T] [--steps N] [--reps R] [--quality] [--out FILE]
    python tools/ssm_bench.py --cpu-grid [--jobs J] [--lrs LR,..] [--checkpoints E,..] [--out FILE]

  step       ms per ssm.step on the ML-20M slice and on the C2-shaped matrix at S = 0 and S = T (HIP events over N
             steps after a warm-up; the minimum of R repetitions, the largest beside it) and the split of N
             instrumented steps: the forward propagation, the sampler, rk_als_ssm_grad, the sorts / zeroing /
             scatters, the backward propagation, Adam; beside it (S = 0) rk_als_ssm_grad alone, rk_als_dau_grad and
             one pair of rk_als_gcl_contrast calls at the same T and h, a lightgcn.step at the same shape, and the
             same step in torch ops (torch.sparse.mm, F.normalize, mm, cross_entropy, autograd, torch.optim.Adam)
  quality    (--quality, on the ML-20M slice) Recall@20 / NDCG@100 of Recoder.train_ssm at its defaults
  cpu-grid   (--cpu-grid, no GPU) the float64 restatement of tests/ssm_util.py on the ML-20M slice over GRID at
             h = 64 and batch 1024, evaluated at the epochs of CHECKPOINTS, every cosine cell ranked by the dot
             product and by the cosine; then the best cell once more with either similarity; appends to
             profiles/ssm_quality.jsonl.  --lrs and --checkpoints restrict the grid (what the records then cover
             is in their fields)

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915, 118 k nnz); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz).  Writes profiles/ssm_bench.jsonl unless --out says otherwise.
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
LAYERS, TEMPERATURES, NEGATIVES, LOGQ, LRS = (0, 2), (0.05, 0.1, 0.2), (0, 1024), (0.0, 1.0), (0.003, 0.01)
CHECKPOINTS = (5, 10, 20)


def grid(lrs=LRS):
  return [(K, tau, S, w, lr, "cosine") for K in LAYERS for tau in TEMPERATURES for S in NEGATIVES for w in LOGQ
          for lr in lrs]


# ----------------------------------------------------------------- cpu grid
def _grid_point(args):
  (K, tau, S, w, lr, similarity), checkpoints = args
  from tests import bpr_util, lightgcn_util as lg, ssm_util as su
  x, y = bpr_util.load_slice()
  Eu, Ei, _ = bpr_util.xavier_tables(x.shape[0], x.shape[1], H, 0)
  rows = []

  def on_epoch(ep, state):
    if ep in checkpoints:
      P, Q = lg.forward(x, *state["E0"], K)
      rows.append((ep,) + tuple(float(v) for v in su.quality(P, Q, x, y)) +
                  tuple(float(v) for v in su.quality(su.unit_rows(P), su.unit_rows(Q), x, y)))
  _, _, _, hist = su.fit(x, Eu, Ei, K, max(checkpoints), BATCH, lr, REG, tau, S, similarity == "cosine", w, seed=0,
                         on_epoch=on_epoch)
  return [{"bench": "ssm_quality", "num_layers": K, "temperature": tau, "num_negatives": S, "logq_weight": w, "lr": lr,
           "similarity": similarity, "reg": REG, "h": H, "batch_size": BATCH, "num_epochs": ep,
           "recall20": round(r, 4), "ndcg100": round(n, 4), "recall20_by_cosine": round(rc, 4),
           "ndcg100_by_cosine": round(nc, 4), "loss": round(hist[ep - 1][0], 4),
           "positive_probability": round(hist[ep - 1][1], 6),
           "source": "float64 restatement (tests/ssm_util.py), CPU"} for ep, r, n, rc, nc in rows]


def run_cpu_grid(jobs, lrs, checkpoints, out):
  import json
  start = sum(1 for _ in open(out)) if os.path.exists(out) else 0
  cpu_grid(_grid_point, [(g, checkpoints) for g in grid(lrs)], jobs, out)
  recs = [json.loads(l) for l in open(out)][start:]
  best = max(recs, key=lambda r: max(r["recall20"], r["recall20_by_cosine"]))
  cell = tuple(best[k] for k in ("num_layers", "temperature", "num_negatives", "logq_weight", "lr"))
  cpu_grid(_grid_point, [(cell + (s,), checkpoints) for s in ("cosine", "dot")], jobs, out)


# ------------------------------------------------------------------ timing
def torch_step(m, graph, h, K, T, S, lr, reg, tau):
  """The same step in torch ops on the same draws: the in-batch and shared columns, the duplicates of a row's own
  positive masked, cross_entropy against the diagonal."""
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
  gen = torch.Generator(device=dev)
  target = torch.arange(T, device=dev)

  def one(s):
    bpr.sample(graph.ucsr, 0, s, users, pos, neg)
    u, i = users.long(), pos.long()
    cand = torch.cat([i, torch.randint(0, m.shape[1], (S,), device=dev, generator=gen)])
    Pk, Qk = E
    P, Q = Pk, Qk
    for _ in range(K):
      Pk, Qk = torch.sparse.mm(A, Qk), torch.sparse.mm(At, Pk)
      P, Q = P + Pk, Q + Qk
    a, b = Fn.normalize(P[u] / (K + 1), dim=-1), Fn.normalize(Q[cand] / (K + 1), dim=-1)
    logits = a @ b.T / tau
    dup = (cand[None, :] == i[:, None])
    dup[target, target] = False
    loss = Fn.cross_entropy(logits.masked_fill(dup, float("-inf")), target)
    loss = loss + 0.5 * reg * (E[0][u].pow(2).sum() + E[1][cand].pow(2).sum()) / T
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
  return one


def step_lines(m, name, h, K, T, S, steps, reps, out):
  import torch
  from recoder_amd import als, bpr, directau, lightgcn, simgcl, ssm
  dev = torch.device("cuda")
  graph = lightgcn.Graph(*als.csr_pair(m, m.shape[0], m.shape[1], dev))
  lr, reg, tau = 0.01, REG, 0.1
  rec = {"bench": "ssm_step", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h,
         "num_layers": K, "batch_size": T, "num_negatives": S, "steps": steps, "repetitions": reps, "temperature": tau}
  X, Y = xavier_tables(m.shape[0], m.shape[1], h, dev)
  state = ssm.new_state(X, Y, K)
  ws = ssm.Workspace(m.shape[0], m.shape[1], T, h, dev, num_negatives=S)
  hyper = (tau, S, "cosine", 0.0)
  rec["hip_ms_per_step"], rec["hip_ms_per_step_max"] = loop_ms(
      lambda s: ssm.step(X, Y, graph, state, ws, 0, s, lr, reg, *hyper), steps, reps)
  rec["slots_per_s"] = round(T / (rec["hip_ms_per_step"] * 1e-3))
  b = ws.bpr
  bpr.sample(graph.ucsr, 0, 0, b.users, b.pos, b.neg)
  grad = lambda s=0: ssm.grad(b.users, b.pos, S, 0, s, X, Y, tau, "cosine", None, ws.raw, ws.cand, b.D, ws.DC, b.g,
                              ws.cvalid, ws.loss, ws.valid_count)
  rec["ssm_grad_ms"], rec["ssm_grad_ms_max"] = loop_ms(grad, steps, reps)
  if S == 0:
    lstate, lws = lightgcn.new_state(X, Y, K), lightgcn.Workspace(m.shape[0], m.shape[1], T, h, dev)
    if K >= 1:
      rec["lightgcn_ms_per_step"], rec["lightgcn_ms_per_step_max"] = loop_ms(
          lambda s: lightgcn.step(X, Y, graph, lstate, lws, 0, s, lr, reg), steps, reps)
      rec["over_lightgcn_step"] = round(rec["hip_ms_per_step"] / rec["lightgcn_ms_per_step"], 3)
    draw = torch.empty(directau.grad_workspace_bytes(T, h), dtype=torch.uint8, device=dev)
    dloss, dcount = torch.zeros(3, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    DI = torch.empty_like(b.D)
    rec["dau_grad_ms"], rec["dau_grad_ms_max"] = loop_ms(
        lambda s: directau.grad(b.users, b.pos, X, Y, 1.0, draw, b.D, DI, b.g, dloss, dcount), steps, reps)
    craw = torch.empty(simgcl.contrast_workspace_bytes(T, h), dtype=torch.uint8, device=dev)
    closs, ccount = torch.zeros(2, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    keys = (torch.sort(b.users)[0], torch.sort(b.pos)[0])
    X2, Y2 = X + 0.01, Y + 0.01

    def pair(s):
      for side, (V1, V2) in enumerate(((X, X2), (Y, Y2))):
        simgcl.contrast(keys[side], V1, V2, 0.2, 0.5, ws.G[side], ws.G[side], craw, closs[side:side + 1],
                        ccount[side:side + 1])
    rec["contrast_pair_ms"], rec["contrast_pair_ms_max"] = loop_ms(pair, steps, reps)
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
    for side, (ids, g, V) in enumerate(((b.users, b.g, b.D), (ws.cand, ws.cvalid, ws.DC))):
      k, o = ssm.sorted_keys(ids, g, ws.G[side].shape[0])
      lightgcn.scatter(k, o, 1, g, V, -1.0, ws.G[side], ws.count[side])

  def adam_both():
    state["step"] += 1
    for side in (0, 1):
      lightgcn.adam(state["E0"][side], ws.H[side], ws.count[side], reg / T, state["M"][side], state["V"][side], lr,
                    state["step"])
  for s in range(10000, 10000 + steps):
    timed("propagate_forward", lambda: lightgcn.forward(graph, state["E0"], K, ws.layers, (X, Y)))
    timed("sample", lambda: bpr.sample(graph.ucsr, 0, s, b.users, b.pos, b.neg))
    timed("ssm_grad", lambda: grad(s))
    timed("sorts_zero_scatters", sums)
    timed("propagate_backward", lambda: lightgcn.forward(graph, ws.G, K, ws.layers, ws.H))
    timed("adam", adam_both)
  torch.cuda.synchronize()
  rec["split_ms"] = {k: round(sum(a.elapsed_time(z) for a, z in v) / steps, 4) for k, v in parts.items()}
  rec["ssm_grad_share_of_step"] = round(rec["split_ms"]["ssm_grad"] / sum(rec["split_ms"].values()), 4)
  rec["losses_last_step"] = [round(v, 4) for v in ws.loss.cpu().tolist()]
  t = guarded(lambda: loop_ms(torch_step(m, graph, h, K, T, S, lr, reg, tau), steps, reps))
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
  d = {k: p.default for k, p in inspect.signature(Recoder.train_ssm).parameters.items()
       if p.default is not inspect.Parameter.empty}
  torch.manual_seed(0)
  rec = Recoder(model=MatrixFactorization(H), optimizer_type="adam")
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  hist = rec.train_ssm(RecommendationDataset(x))
  e1.record()
  torch.cuda.synchronize()
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  r20, n100 = (float(np.nanmean(np.asarray(v, dtype=np.float64))) for v in res.values())
  emit(dict({k: d[k] for k in ("num_layers", "temperature", "num_negatives", "logq_weight", "lr", "similarity", "reg",
                               "batch_size", "num_epochs")},
            bench="ssm_quality", h=H, recall20=round(r20, 4), ndcg100=round(n100, 4), loss=round(hist[-1][0], 4),
            positive_probability=round(hist[-1][1], 6), fit_ms=round(e0.elapsed_time(e1), 1),
            source="Recoder.train_ssm, MI355X"), out)


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
  ap.add_argument("--lrs", default=",".join(str(v) for v in LRS))
  ap.add_argument("--checkpoints", default=",".join(str(v) for v in CHECKPOINTS))
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    return run_cpu_grid(args.jobs, tuple(float(v) for v in args.lrs.split(",")),
                        tuple(int(v) for v in args.checkpoints.split(",")),
                        args.out or os.path.join(ROOT, "profiles", "ssm_quality.jsonl"))
  import torch
  if not torch.cuda.is_available():
    sys.exit("ssm_bench.py measures on the GPU (only --cpu-grid runs without one)")
  out = args.out or os.path.join(ROOT, "profiles", "ssm_bench.jsonl")
  for name in ("slice", "c2"):
    m, _ = load(name)
    for S in (0, args.batch):
      step_lines(m, name, args.h, args.layers, args.batch, S, args.steps, args.reps, out)
  if args.quality:
    quality(out)


if __name__ == "__main__":
  main()
