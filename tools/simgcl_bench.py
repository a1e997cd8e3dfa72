#!/usr/bin/env python
"""SimGCL step throughput and quality (recoder_amd/simgcl.py, the rk_als_gcl_* part of include/recoder_als.h), one
JSON line per measurement:

    python tools/simgcl_bench.py [--h H] [--layers K] [--batch T] [--steps N] [--quality] [--out FILE]
    python tools/simgcl_bench.py --cpu-grid [--jobs J] [--out FILE]

  step       ms per simgcl.step on the ML-20M slice and on the C2-shaped matrix (HIP events over N steps after a
             warm-up) and the split of N instrumented steps: the clean forward, both views, the two contrasts (and
             their share of the step), the backward propagation, and the rest (sample, grad, sorts, zeroing,
             scatters, Adam); beside it a lightgcn.step at the same shape, and the same step in torch ops
             (torch.sparse.mm, autograd through sign / normalize / logsumexp, torch.optim.Adam) with the noise
             drawn by torch.rand
  propagate  rk_als_gcl_propagate beside rk_als_lgcn_propagate followed by a separate torch perturbation of its
             output (rand, norm, sign, add) and of the accumulate, both orientations of both matrices
  quality    (--quality, on the ML-20M slice) Recall@20 / NDCG@100 of Recoder.train_simgcl at QUALITY_POINTS
  cpu-grid   (--cpu-grid, no GPU) the float64 restatement of tests/simgcl_util.py on the ML-20M slice over GRID at
             h = 64 and temperature 0.2, evaluated at the epochs of CHECKPOINTS; appends to
             profiles/simgcl_quality.jsonl

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915, 118 k nnz); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz).  Writes profiles/simgcl_bench.jsonl unless --out says otherwise.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_util import cpu_grid, emit, event_ms, guarded, load, loop_ms, xavier_tables  # noqa: E402

H, BATCH, TAU = 64, 1024, 0.2
# (num_layers, cl_weight, cl_eps, lr, reg): layers x weight x eps x lr at LightGCN's reg, the paper's own lr and reg,
# two more weights, and the weight 0 (BPR at the layer-0-free mean)
GRID = [(K, w, eps, lr, 1e-3) for K in (2, 3) for w in (0.1, 0.5) for eps in (0.1, 0.2) for lr in (0.002, 0.01)] + \
    [(2, 0.5, 0.1, 0.001, 1e-4), (3, 0.5, 0.1, 0.001, 1e-4), (2, 0.05, 0.1, 0.01, 1e-3), (2, 0.2, 0.1, 0.01, 1e-3),
     (2, 0.0, 0.1, 0.01, 1e-3), (3, 0.0, 0.1, 0.01, 1e-3)]
CHECKPOINTS = (5, 10, 20)
# (num_layers, cl_weight, cl_eps, lr, reg, epochs); the first: the defaults
QUALITY_POINTS = [(2, 0.1, 0.2, 0.002, 1e-3, 10), (2, 0.5, 0.1, 0.01, 1e-3, 10)]


# ----------------------------------------------------------------- cpu grid
def _grid_point(args):
  K, w, eps, lr, reg = args
  from tests import bpr_util, simgcl_util as sg
  x, y = bpr_util.load_slice()
  Eu, Ei, _ = bpr_util.xavier_tables(x.shape[0], x.shape[1], H, 0)
  rows = []

  def on_epoch(ep, state):
    if ep in CHECKPOINTS:
      P, Q = sg.forward(x, *state["E0"], K)
      r, n = sg.quality(P, Q, x, y)
      rows.append((ep, float(r), float(n)))
  _, _, _, hist = sg.fit(x, Eu, Ei, K, max(CHECKPOINTS), BATCH, lr, reg, w, eps, TAU, seed=0, on_epoch=on_epoch)
  return [{"bench": "simgcl_quality", "num_layers": K, "cl_weight": w, "cl_eps": eps, "cl_temperature": TAU, "lr": lr,
           "reg": reg, "h": H, "batch_size": BATCH, "num_epochs": ep, "recall20": round(r, 4), "ndcg100": round(n, 4),
           "bpr_loss": round(hist[ep - 1][0], 4), "cl_loss": round(hist[ep - 1][1], 4),
           "source": "float64 restatement (tests/simgcl_util.py), CPU"} for ep, r, n in rows]


# ------------------------------------------------------------------ timing
def propagate_lines(name, graph, h, eps, reps, out):
  """The noise in the epilogue beside rk_als_lgcn_propagate and a separate torch pass over its output."""
  import torch
  from recoder_amd import lightgcn, simgcl
  dev = graph.su.device
  for side, (label, csr, rs, cs) in enumerate((("user-major", graph.ucsr, graph.su, graph.si),
                                               ("item-major", graph.icsr, graph.si, graph.su))):
    rows, cols = csr.shape
    torch.manual_seed(1)
    F = torch.randn(cols, h, device=dev)
    acc, nxt = torch.randn(rows, h, device=dev), torch.empty(rows, h, device=dev)
    rec = {"bench": "simgcl_propagate", "data": name, "orientation": label, "rows": rows, "cols": cols, "nnz": csr.nnz,
           "h": h, "cl_eps": eps}
    rec["gcl_ms"] = round(event_ms(lambda: simgcl.propagate(csr, rs, cs, F, nxt, acc, 0.5, eps, 0, 3, 1, 2, side), reps), 4)
    rec["lgcn_ms"] = round(event_ms(lambda: lightgcn.propagate(csr, rs, cs, F, nxt, acc, 0.5), reps), 4)

    def separate():
      lightgcn.propagate(csr, rs, cs, F, nxt, None)
      u = torch.rand_like(nxt)
      nxt.add_(torch.sign(nxt) * u * (eps / u.norm(dim=1, keepdim=True)))
      acc.add_(nxt).mul_(0.5)
    rec["lgcn_then_torch_noise_ms"] = round(event_ms(separate, reps), 4)
    rec["gcl_over_lgcn"] = round(rec["gcl_ms"] / rec["lgcn_ms"], 3)
    rec["gcl_over_separate"] = round(rec["gcl_ms"] / rec["lgcn_then_torch_noise_ms"], 3)
    emit(rec, out)


def torch_step_ms(m, graph, h, K, T, steps, lr, reg, w, eps, tau):
  """ms per step of the same step in torch ops on the same draws: torch.sparse.mm for the 6 K forward
  propagations, torch.rand noise, autograd for the backward pass, torch.optim.Adam on the base tables."""
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

  def tables(noisy):
    Pk, Qk = E
    P, Q = 0, 0
    for _ in range(K):
      Pk, Qk = torch.sparse.mm(A, Qk), torch.sparse.mm(At, Pk)
      if noisy:
        Pk = Pk + torch.sign(Pk) * Fn.normalize(torch.rand_like(Pk), dim=1) * eps
        Qk = Qk + torch.sign(Qk) * Fn.normalize(torch.rand_like(Qk), dim=1) * eps
      P, Q = P + Pk, Q + Qk
    return P / K, Q / K

  def one(s):
    bpr.sample(graph.ucsr, 0, s, users, pos, neg)
    ok = neg >= 0
    u, i, j = users[ok].long(), pos[ok].long(), neg[ok].long()
    P, Q = tables(False)
    x = (P[u] * (Q[i] - Q[j])).sum(1)
    l2 = E[0][u].pow(2).sum() + E[1][i].pow(2).sum() + E[1][j].pow(2).sum()
    loss = (Fn.softplus(-x).sum() + 0.5 * reg * l2) / T
    (P1, Q1), (P2, Q2) = tables(True), tables(True)
    for V1, V2, ids in ((P1, P2, torch.unique(u)), (Q1, Q2, torch.unique(i))):
      S = Fn.normalize(V1[ids], dim=1) @ Fn.normalize(V2[ids], dim=1).T / tau
      loss = loss + w * (torch.logsumexp(S, 1) - torch.diagonal(S)).mean()
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
  return loop_ms(one, steps)[0]


def step_lines(m, name, h, K, T, steps, out):
  import torch
  from recoder_amd import als, bpr, lightgcn, simgcl
  dev = torch.device("cuda")
  graph = lightgcn.Graph(*als.csr_pair(m, m.shape[0], m.shape[1], dev))
  lr, reg, w, eps, tau = 0.01, 1e-3, 0.5, 0.1, TAU
  rec = {"bench": "simgcl_step", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h,
         "num_layers": K, "batch_size": T, "steps": steps, "cl_weight": w, "cl_eps": eps, "cl_temperature": tau}
  X, Y = xavier_tables(m.shape[0], m.shape[1], h, dev)
  state = simgcl.new_state(X, Y, K)
  ws = simgcl.Workspace(m.shape[0], m.shape[1], T, h, dev)
  rec["hip_ms_per_step"] = loop_ms(lambda s: simgcl.step(X, Y, graph, state, ws, 0, s, lr, reg, w, eps, tau), steps)[0]
  rec["triples_per_s"] = round(T / (rec["hip_ms_per_step"] * 1e-3))
  rec["hip_ms_per_step_cl_weight_0"] = loop_ms(
      lambda s: simgcl.step(X, Y, graph, state, ws, 0, s, lr, reg, 0.0, eps, tau), steps)[0]
  lstate, lws = lightgcn.new_state(X, Y, K), lightgcn.Workspace(m.shape[0], m.shape[1], T, h, dev)
  rec["lightgcn_ms_per_step"] = loop_ms(lambda s: lightgcn.step(X, Y, graph, lstate, lws, 0, s, lr, reg), steps)[0]
  rec["over_lightgcn_step"] = round(rec["hip_ms_per_step"] / rec["lightgcn_ms_per_step"], 3)
  # the split: the step's calls one by one between events
  b, parts = ws.bpr, {}
  E0 = state["E0"]

  def timed(key, fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    z.record()
    parts.setdefault(key, []).append((a, z))
    return r

  def draw(s):
    bpr.sample(graph.ucsr, 0, s, b.users, b.pos, b.neg)
    bpr.grad(b.users, b.pos, b.neg, X, Y, ws.zero_bias, b.g, b.loss, b.D, b.P)
    keys = bpr.sorted_keys(b.users, b.pos, b.neg, X.shape[0], Y.shape[0])
    for t in ws.G + ws.count:
      t.zero_()
    lightgcn.scatter(*keys[0], 1, b.g, b.D, 1.0 / T, ws.G[0], ws.count[0])
    lightgcn.scatter(*keys[1], 2, b.g, b.P, 1.0 / T, ws.G[1], ws.count[1])
    return keys[0][0], torch.sort(torch.where(b.neg >= 0, b.pos, torch.full_like(b.pos, Y.shape[0])))[0]

  def adam_both():
    state["step"] += 1
    for side in (0, 1):
      lightgcn.adam(E0[side], ws.H[side], ws.count[side], reg / T, state["M"][side], state["V"][side], lr, state["step"])
  for s in range(100, 100 + steps):
    timed("propagate_clean", lambda: simgcl.forward(graph, E0, K, ws.layers, (X, Y)))
    uk, pk = timed("sample_grad_sorts_zero_scatters", lambda: draw(s))
    for a in (0, 1):
      timed("propagate_views", lambda: simgcl.forward(graph, E0, K, ws.layers, ws.views[a], eps, 0, s, a + 1))
    for side, keys in enumerate((uk, pk)):
      timed("contrast", lambda: simgcl.contrast(keys, ws.views[0][side], ws.views[1][side], tau, w, ws.G[side],
                                                ws.G[side], ws.raw, ws.cl_loss[side:side + 1],
                                                ws.cl_count[side:side + 1]))
    timed("propagate_backward", lambda: simgcl.forward(graph, ws.G, K, ws.layers, ws.H))
    timed("adam", adam_both)
  torch.cuda.synchronize()
  rec["split_ms"] = {k: round(sum(a.elapsed_time(z) for a, z in v) / steps, 4) for k, v in parts.items()}
  rec["contrast_share_of_step"] = round(rec["split_ms"]["contrast"] / sum(rec["split_ms"].values()), 4)
  rec["distinct_users_items_last_step"] = ws.cl_count.cpu().tolist()
  rec["gathered_bytes_per_step"] = 2 * 4 * K * int(m.nnz) * h * 4
  rec["torch_ops_step_ms"] = guarded(lambda: torch_step_ms(m, graph, h, K, T, steps, lr, reg, w, eps, tau))
  emit(rec, out)
  propagate_lines(name, graph, h, eps, max(5, steps // 2), out)


def quality(out):
  import torch
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  x, y = load("slice")
  for K, w, eps, lr, reg, epochs in QUALITY_POINTS:
    torch.manual_seed(0)
    rec = Recoder(model=MatrixFactorization(H), optimizer_type="adam")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    hist = rec.train_simgcl(RecommendationDataset(x), num_layers=K, num_epochs=epochs, batch_size=BATCH, lr=lr,
                            reg=reg, cl_weight=w, cl_eps=eps, cl_temperature=TAU, seed=0)
    e1.record()
    torch.cuda.synchronize()
    res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                       metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
    r20, n100 = (float(np.nanmean(np.asarray(v, dtype=np.float64))) for v in res.values())
    emit({"bench": "simgcl_quality", "num_layers": K, "cl_weight": w, "cl_eps": eps, "cl_temperature": TAU, "lr": lr,
          "reg": reg, "h": H, "batch_size": BATCH, "num_epochs": epochs, "recall20": round(r20, 4),
          "ndcg100": round(n100, 4), "bpr_loss": round(hist[-1][0], 4), "cl_loss": round(hist[-1][1], 4),
          "fit_ms": round(e0.elapsed_time(e1), 1), "source": "Recoder.train_simgcl, MI355X"}, out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--h", type=int, default=H)
  ap.add_argument("--layers", type=int, default=2)
  ap.add_argument("--batch", type=int, default=2048)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--jobs", type=int, default=16)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    return cpu_grid(_grid_point, GRID, args.jobs,
                    args.out or os.path.join(ROOT, "profiles", "simgcl_quality.jsonl"))
  import torch
  if not torch.cuda.is_available():
    sys.exit("simgcl_bench.py measures on the GPU (only --cpu-grid runs without one)")
  out = args.out or os.path.join(ROOT, "profiles", "simgcl_bench.jsonl")
  for name in ("slice", "c2"):
    m, _ = load(name)
    step_lines(m, name, args.h, args.layers, args.batch, args.steps, out)
  if args.quality:
    quality(out)


if __name__ == "__main__":
  main()
