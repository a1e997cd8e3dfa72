#!/usr/bin/env python
"""LightGCN step throughput and quality (recoder_amd/lightgcn.py, the rk_als_lgcn_* part of include/recoder_als.h),
one JSON line per measurement:

    python tools/lightgcn_bench.py [--h H] [--layers K] [--batch T] [--steps N] [--quality] [--out FILE]
    python tools/lightgcn_bench.py --cpu-grid [--jobs J] [--out FILE]

  step       ms per lightgcn.step on the ML-20M slice and on the C2-shaped matrix (HIP events over N steps after a
             warm-up), triples/s, and the per-kernel split of N instrumented steps: the 4 K propagations, sample,
             grad, sort (torch.sort: plumbing), the zeroing, the two scatters, the two Adam passes; beside it the
             same step in torch ops (torch.sparse.mm, autograd, torch.optim.Adam)
  propagate  one propagation with the layer-mean accumulate on both orientations of both matrices: ms and the
             gathered bytes/s (nnz h 4 bytes over the time); beside it, on the same matrix and width, the
             existing kernel it would otherwise be built from -- rk_svd_spmm over a CSR with a value array
             (s_u s_i per entry) followed by the torch add and scale of the layer mean -- and torch.sparse.mm
             with the same add and scale
  quality    (--quality, on the ML-20M slice) Recall@20 / NDCG@100 of Recoder.train_lightgcn at QUALITY_POINTS
  cpu-grid   (--cpu-grid, no GPU) the float64 restatement of tests/lightgcn_util.py on the ML-20M slice over GRID at
             h = 64, evaluated at the epochs of CHECKPOINTS; appends to profiles/lightgcn_quality.jsonl

Data: slice = tests/golden/real_ml20m_slice.npz (10 000 x 7 915, 118 k nnz); c2 = synthetic.ml20m_like(seed=0)
(116 677 x 20 108, 6.32 M nnz).  Writes profiles/lightgcn_bench.jsonl unless --out says otherwise.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_util import cpu_grid, emit, event_ms, guarded, load, loop_ms, xavier_tables  # noqa: E402

H, BATCH = 64, 1024
# (num_layers, lr, reg): num_layers x lr x reg, and one larger lr at two layers
GRID = [(K, lr, reg) for K in (1, 2, 3) for lr in (0.002, 0.01) for reg in (1e-4, 1e-3)] + \
    [(2, 0.05, 1e-4), (2, 0.05, 1e-3)]
CHECKPOINTS = (5, 10, 20)
QUALITY_POINTS = [(3, 0.01, 1e-3, 10), (1, 0.002, 1e-3, 20)]     # (num_layers, lr, reg, epochs); the first: the defaults


# ----------------------------------------------------------------- cpu grid
def _grid_point(args):
  K, lr, reg = args
  from tests import bpr_util, lightgcn_util as lg
  x, y = bpr_util.load_slice()
  Eu, Ei, _ = bpr_util.xavier_tables(x.shape[0], x.shape[1], H, 0)
  rows = []

  def on_epoch(ep, state):
    if ep in CHECKPOINTS:
      P, Q = lg.forward(x, *state["E0"], K)
      r, n = lg.quality(P, Q, x, y)
      rows.append((ep, float(r), float(n)))
  _, _, _, hist = lg.fit(x, Eu, Ei, K, max(CHECKPOINTS), BATCH, lr, reg, seed=0, on_epoch=on_epoch)
  return [{"bench": "lightgcn_quality", "num_layers": K, "lr": lr, "reg": reg, "h": H, "batch_size": BATCH,
           "num_epochs": ep, "recall20": round(r, 4), "ndcg100": round(n, 4), "loss": round(hist[ep - 1], 4),
           "source": "float64 restatement (tests/lightgcn_util.py), CPU"} for ep, r, n in rows]


# ------------------------------------------------------------------ timing
def propagate_lines(name, graph, h, reps, out):
  """The fused propagate beside rk_svd_spmm + add + scale and torch.sparse.mm + add + scale, both orientations."""
  import torch
  from recoder_amd import als, lightgcn, svd
  import scipy.sparse as sp
  dev = graph.su.device
  for side, csr, rs, cs in (("user-major", graph.ucsr, graph.su, graph.si), ("item-major", graph.icsr, graph.si, graph.su)):
    rows, cols = csr.shape
    torch.manual_seed(1)
    F = torch.randn(cols, h, device=dev)
    acc, nxt = torch.randn(rows, h, device=dev), torch.empty(rows, h, device=dev)
    gathered = csr.nnz * h * 4
    lens = np.diff(csr.indptr.cpu().numpy())
    rec = {"bench": "lightgcn_propagate", "data": name, "orientation": side, "rows": rows, "cols": cols,
           "nnz": csr.nnz, "h": h, "longest_row": int(lens.max()), "rows_at_or_above_long_row": int((lens >= lightgcn.LONG_ROW).sum())}
    ms = event_ms(lambda: lightgcn.propagate(csr, rs, cs, F, nxt, acc, 0.5), reps)
    rec["fused_ms"] = round(ms, 4)
    rec["fused_gathered_GBps"] = round(gathered / (ms * 1e-3) / 1e9, 1)
    ms_last = event_ms(lambda: lightgcn.propagate(csr, rs, cs, F, None, acc, 0.5), reps)
    rec["fused_last_layer_ms"] = round(ms_last, 4)
    # the comparator: the same operator as a CSR with values, the existing spmm, then the layer mean in torch
    indptr, indices = csr.indptr.cpu().numpy(), csr.indices.cpu().numpy()[:csr.nnz]
    r_of = np.repeat(np.arange(rows), lens)
    vals = (rs.cpu().numpy()[r_of].astype(np.float64) * cs.cpu().numpy()[indices]).astype(np.float32)
    vals[vals == 1.0] = np.nextafter(np.float32(1), np.float32(0))          # (AlsCSR drops an all-ones value array)
    wcsr = als.AlsCSR(sp.csr_matrix((vals, indices, indptr), shape=(rows, cols)), dev)

    def spmm_seq():
      svd.spmm(wcsr, F, nxt)
      acc.add_(nxt).mul_(0.5)
    ms2 = event_ms(spmm_seq, reps)
    rec["svd_spmm_add_scale_ms"] = round(ms2, 4)
    rec["svd_spmm_alone_ms"] = round(event_ms(lambda: svd.spmm(wcsr, F, nxt), reps), 4)
    rec["fused_over_svd_spmm_sequence"] = round(ms / ms2, 3)

    def sparse_mm():
      A = torch.sparse_csr_tensor(wcsr.indptr, wcsr.indices[:csr.nnz].long(), wcsr.data, size=(rows, cols))
      t = event_ms(lambda: acc.add_(torch.sparse.mm(A, F)).mul_(0.5), reps)
      return round(t, 4)
    rec["torch_sparse_mm_add_scale_ms"] = guarded(sparse_mm)
    emit(rec, out)


def torch_step_ms(m, graph, h, K, T, steps, lr, reg):
  """ms per step of the same step in torch ops on the same draws: torch.sparse.mm for the 2 K propagations,
  autograd for the backward pass, torch.optim.Adam on the base tables."""
  import torch
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

  def one(s):
    bpr.sample(graph.ucsr, 0, s, users, pos, neg)
    ok = neg >= 0
    u, i, j = users[ok].long(), pos[ok].long(), neg[ok].long()
    Pk, Qk = E
    P, Q = Pk, Qk
    for _ in range(K):
      Pk, Qk = torch.sparse.mm(A, Qk), torch.sparse.mm(At, Pk)
      P, Q = P + Pk, Q + Qk
    P, Q = P / (K + 1), Q / (K + 1)
    x = (P[u] * (Q[i] - Q[j])).sum(1)
    l2 = E[0][u].pow(2).sum() + E[1][i].pow(2).sum() + E[1][j].pow(2).sum()
    loss = (torch.nn.functional.softplus(-x).sum() + 0.5 * reg * l2) / T
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
  return loop_ms(one, steps)[0]


def step_lines(m, name, h, K, T, steps, out):
  import torch
  from recoder_amd import als, bpr, lightgcn
  dev = torch.device("cuda")
  graph = lightgcn.Graph(*als.csr_pair(m, m.shape[0], m.shape[1], dev))
  X, Y = xavier_tables(m.shape[0], m.shape[1], h, dev)
  state = lightgcn.new_state(X, Y, K)
  ws = lightgcn.Workspace(m.shape[0], m.shape[1], T, h, dev)
  rec = {"bench": "lightgcn_step", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h,
         "num_layers": K, "batch_size": T, "steps": steps}
  lr, reg = 0.01, 1e-3
  rec["hip_ms_per_step"] = loop_ms(lambda s: lightgcn.step(X, Y, graph, state, ws, 0, s, lr, reg), steps)[0]
  rec["triples_per_s"] = round(T / (rec["hip_ms_per_step"] * 1e-3))
  # the split: the step's calls one by one between events
  b, parts = ws.bpr, {}

  def timed(key, fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    z.record()
    parts.setdefault(key, []).append((a, z))
    return r
  for s in range(3 + steps, 3 + 2 * steps):
    timed("propagate_forward", lambda: lightgcn.forward(graph, state["E0"], K, ws.layers, (X, Y)))
    timed("sample", lambda: bpr.sample(graph.ucsr, 0, s, b.users, b.pos, b.neg))
    timed("grad", lambda: bpr.grad(b.users, b.pos, b.neg, X, Y, ws.zero_bias, b.g, b.loss, b.D, b.P))
    (uk, uo), (ik, io) = timed("sort", lambda: bpr.sorted_keys(b.users, b.pos, b.neg, X.shape[0], Y.shape[0]))
    timed("zero", lambda: [t.zero_() for t in ws.G + ws.count])
    timed("scatter_users", lambda: lightgcn.scatter(uk, uo, 1, b.g, b.D, 1.0 / T, ws.G[0], ws.count[0]))
    timed("scatter_items", lambda: lightgcn.scatter(ik, io, 2, b.g, b.P, 1.0 / T, ws.G[1], ws.count[1]))
    timed("propagate_backward", lambda: lightgcn.forward(graph, ws.G, K, ws.layers, ws.H))
    state["step"] += 1
    for side, key in ((0, "adam_users"), (1, "adam_items")):
      timed(key, lambda: lightgcn.adam(state["E0"][side], ws.H[side], ws.count[side], reg / T, state["M"][side],
                                       state["V"][side], lr, state["step"]))
  torch.cuda.synchronize()
  rec["split_ms"] = {k: round(sum(a.elapsed_time(z) for a, z in v) / steps, 4) for k, v in parts.items()}
  # a forward (and a backward) gathers nnz rows of h floats per orientation and layer
  rec["gathered_bytes_per_step"] = 2 * 2 * K * int(m.nnz) * h * 4
  rec["torch_sparse_mm_step_ms"] = guarded(lambda: torch_step_ms(m, graph, h, K, T, steps, lr, reg))
  emit(rec, out)
  propagate_lines(name, graph, h, max(5, steps // 2), out)


def quality(out):
  import torch
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  x, y = load("slice")
  for K, lr, reg, epochs in QUALITY_POINTS:
    torch.manual_seed(0)
    rec = Recoder(model=MatrixFactorization(H), optimizer_type="adam")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    hist = rec.train_lightgcn(RecommendationDataset(x), num_layers=K, num_epochs=epochs, batch_size=BATCH, lr=lr,
                              reg=reg, seed=0)
    e1.record()
    torch.cuda.synchronize()
    res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                       metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
    r20, n100 = (float(np.nanmean(np.asarray(v, dtype=np.float64))) for v in res.values())
    emit({"bench": "lightgcn_quality", "num_layers": K, "lr": lr, "reg": reg, "h": H, "batch_size": BATCH,
          "num_epochs": epochs, "recall20": round(r20, 4), "ndcg100": round(n100, 4), "loss": round(hist[-1], 4),
          "fit_ms": round(e0.elapsed_time(e1), 1), "source": "Recoder.train_lightgcn, MI355X"}, out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--h", type=int, default=H)
  ap.add_argument("--layers", type=int, default=3)
  ap.add_argument("--batch", type=int, default=4096)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--jobs", type=int, default=16)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    return cpu_grid(_grid_point, GRID, args.jobs,
                    args.out or os.path.join(ROOT, "profiles", "lightgcn_quality.jsonl"))
  import torch
  if not torch.cuda.is_available():
    sys.exit("lightgcn_bench.py measures on the GPU (only --cpu-grid runs without one)")
  out = args.out or os.path.join(ROOT, "profiles", "lightgcn_bench.jsonl")
  for name in ("slice", "c2"):
    m, _ = load(name)
    step_lines(m, name, args.h, args.layers, args.batch, args.steps, out)
  if args.quality:
    quality(out)


if __name__ == "__main__":
  main()
