"""CCL (recoder_amd/ccl.py, rk_als_ccl_grad, rk_als_ccl_scatter): speed on the GPU and quality on the CPU.

    python tools/ccl_bench.py [--quality] [--batch T] [--steps N] [--reps R]
    python tools/ccl_bench.py --cpu-grid [--jobs N] [--margins ..] [--weights ..] [--negatives ..] [--lrs ..]
                                         [--layers ..] [--checkpoints ..]
    python tools/ccl_bench.py --test-reference

default      ms per CCL step (the minimum of R timed loops after a warm-up, the largest beside it) and its split per
             kernel at R = 64 and 512, on the slice and on the C2-shaped matrix, beside a ``train_ultragcn`` step at
             the same R and K = 0, a ``train_bpr`` step and the same CCL step in torch ops; the share of live
             negatives, and the item-side scatter with the sentinel keys against the same scatter fed every entry
             (the keys are ``cand``: the dead entries carry coefficient 0 and are gathered all the same).
             --quality adds Recall / NDCG of the default fit through the kernels.  -> profiles/ccl_bench.jsonl
--cpu-grid   (no GPU) the float64 restatement (tests/ccl_util.py) on the slice over margin x negative_weight x R x lr
             x layers, Recall@20 / NDCG@100 ranked by the cosine at every checkpoint -> profiles/ccl_quality.jsonl.
             The options restrict the grid (what the records then cover is what was run).
--test-reference  (no GPU) the float64 fit that tests/test_ccl.py compares against -> profiles/ccl_quality.jsonl
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
MARGINS, WEIGHTS, NEGATIVES, LRS, LAYERS = (0.0, 0.2, 0.4, 0.6, 0.8), (16.0, 64.0, 256.0), (64, 256, 1024), \
    (0.003, 0.01), (0, 2)
CHECKPOINTS = (5, 10, 20)
TEST_CELL, TEST_EPOCHS = (0.4, 64.0, 64, 0.01, 0), 2             # the fit of tests/test_ccl.py on the slice


# ----------------------------------------------------------------- cpu grid
def _grid_point(args):
  (margin, nw, R, lr, K), checkpoints, seed, cosine = args
  from tests import bpr_util, ccl_util as cu
  x, y = bpr_util.load_slice()
  Eu, Ei, _ = bpr_util.xavier_tables(x.shape[0], x.shape[1], H, seed)
  rows = []

  def on_epoch(ep, state):
    if ep in checkpoints:
      P, Q = cu.lg.forward(x, *state["E0"], K)
      if cosine:
        P, Q = cu.unit_rows(P), cu.unit_rows(Q)
      rows.append((ep,) + tuple(float(v) for v in cu.quality(P, Q, x, y)))
  _, _, _, hist, stats = cu.fit(x, Eu, Ei, K, max(checkpoints), BATCH, lr, REG, R, nw, margin, seed=seed,
                                on_epoch=on_epoch)
  return [{"bench": "ccl_quality", "margin": margin, "negative_weight": nw, "num_negatives": R, "lr": lr,
           "num_layers": K, "reg": REG, "h": H, "batch_size": BATCH, "seed": seed, "num_epochs": ep,
           "ranked_by": "cosine" if cosine else "dot", "recall20": round(r, 4), "ndcg100": round(n, 4),
           "loss": [round(float(v), 5) for v in hist[ep - 1]], "live_share": round(float(stats[ep - 1]), 5),
           "source": "float64 restatement (tests/ccl_util.py), CPU"} for ep, r, n in rows]


def run_cpu_grid(jobs, cells, checkpoints, out):
  cpu_grid(_grid_point, [(c, checkpoints, 0, True) for c in cells], jobs, out)


def run_test_reference(out):
  """The float64 restatement of the end-to-end fit of tests/test_ccl.py (ranked by the dot product, as the test
  ranks): the figure its constant copies."""
  for rec in _grid_point((TEST_CELL, (TEST_EPOCHS,), 0, False)):
    emit(dict(rec, bench="ccl_test_reference"), out)


# ------------------------------------------------------------------ timing
def torch_step(m, graph, h, T, R, lr, reg, nw, margin):
  """The same step in torch ops on the same slots: private uniform negatives from torch's generator."""
  import torch
  import torch.nn.functional as Fn
  from recoder_amd import bpr
  dev = graph.su.device
  E = [torch.nn.Parameter(t) for t in xavier_tables(m.shape[0], m.shape[1], h, dev)]
  opt = torch.optim.Adam(E, lr=lr)
  users, pos, neg = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(3))
  gen = torch.Generator(device=dev)

  def one(s):
    bpr.sample(graph.ucsr, 0, s, users, pos, neg)
    u, i = users.long(), pos.long()
    j = torch.randint(0, m.shape[1], (T, R), device=dev, generator=gen)
    cand = torch.cat([i[:, None], j], 1)
    p = Fn.embedding(u, E[0])
    c = torch.bmm(Fn.normalize(Fn.embedding(cand, E[1]), dim=2), Fn.normalize(p, dim=1)[:, :, None])[:, :, 0]
    loss = (1 - c[:, 0]).sum() + (nw / R) * torch.relu(c[:, 1:] - margin).sum()
    loss = loss / T + 0.5 * reg * (p.pow(2).sum() + E[1][i].pow(2).sum()) / T
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
  return one


def step_lines(m, name, h, T, R, steps, reps, out):
  import torch
  from recoder_amd import als, bpr, ccl, lightgcn, ultragcn
  dev = torch.device("cuda")
  graph = lightgcn.Graph(*als.csr_pair(m, m.shape[0], m.shape[1], dev))
  lr, reg, nw, margin = 0.01, REG, 64.0, 0.4
  E = 1 + R
  rec = {"bench": "ccl_step", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h,
         "batch_size": T, "num_negatives": R, "margin": margin, "negative_weight": nw, "steps": steps,
         "repetitions": reps}
  X, Y = xavier_tables(m.shape[0], m.shape[1], h, dev)
  state = ccl.new_state(X, Y, 0)
  ws = ccl.Workspace(m.shape[0], m.shape[1], T, h, dev, num_negatives=R)
  # a few hundred steps first: at the Xavier start almost no cosine exceeds the margin, a trained table is the case
  for s in range(300):
    ccl.step(X, Y, graph, state, ws, 0, s, lr, reg, R, nw, margin)
  rec["hip_ms_per_step"], rec["hip_ms_per_step_max"] = loop_ms(
      lambda s: ccl.step(X, Y, graph, state, ws, 0, 300 + s, lr, reg, R, nw, margin), steps, reps)
  rec["live_share"] = round(float(ws.live.sum()) / (float(ws.bpr.g.sum()) * R), 5)
  UX, UY = X.clone(), Y.clone()
  ustate = ultragcn.new_state(UX, UY, 0)
  uws = ultragcn.Workspace(m.shape[0], m.shape[1], T, h, dev, num_negatives=R, neighbours=0)
  uhyper = (R, float(R), 0, 0.0, (1e-7, 1.0, 1e-7, 1.0))
  rec["ultragcn_ms_per_step"], rec["ultragcn_ms_per_step_max"] = loop_ms(
      lambda s: ultragcn.step(UX, UY, graph, ustate, uws, 0, s, 0.001, reg, *uhyper), steps, reps)
  BX, BY = X.clone(), Y.clone()
  bws = bpr.Workspace(T, h, dev)
  zero_bias = torch.zeros(m.shape[1], device=dev)
  rec["bpr_ms_per_step"], rec["bpr_ms_per_step_max"] = loop_ms(
      lambda s: bpr.step(BX, BY, zero_bias, graph.ucsr, bws, 0, s, 0.05, reg), steps, reps)
  rec["over_ultragcn_step"] = round(rec["hip_ms_per_step"] / rec["ultragcn_ms_per_step"], 3)
  rec["over_bpr_step"] = round(rec["hip_ms_per_step"] / rec["bpr_ms_per_step"], 3)
  rec["cheaper_than_ultragcn_step"] = rec["hip_ms_per_step"] < rec["ultragcn_ms_per_step"]
  b, parts, sorted_ = ws.bpr, {}, {}

  def timed(key, fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    parts.setdefault(key, []).append((a, z))

  def sorts():
    for t in ws.G + ws.count:
      t.zero_()
    sorted_["u"] = torch.sort(bpr.masked_keys(b.users, b.g > 0, X.shape[0]), stable=True)
    sorted_["i"] = torch.sort(ws.key.view(-1), stable=True)

  def adam_both():
    state["step"] += 1
    for side in (0, 1):
      lightgcn.adam(state["E0"][side], ws.G[side], ws.count[side], reg / T, state["M"][side], state["V"][side], lr,
                    state["step"])
  for s in range(10000, 10000 + steps):
    timed("sample", lambda: bpr.sample(graph.ucsr, 0, s, b.users, b.pos, b.neg))
    timed("ccl_grad", lambda: ccl.grad(b.users, b.pos, R, 0, s, X, Y, margin, nw, ws.cand, ws.key, ws.coef, ws.self_,
                                       b.D, b.g, ws.loss, ws.live))
    timed("sorts_zero", sorts)
    timed("lgcn_scatter_users", lambda: lightgcn.scatter(*sorted_["u"], 1, b.g, b.D, -1.0 / T, ws.G[0], ws.count[0]))
    timed("ccl_scatter_sentinel_keys", lambda: ccl.scatter(*sorted_["i"], E, b.users, ws.coef, ws.self_, X, Y,
                                                           1.0 / T, ws.G[1], ws.count[1]))
    every = torch.sort(ws.cand.view(-1), stable=True)
    timed("ccl_scatter_every_entry", lambda: ccl.scatter(*every, E, b.users, ws.coef, ws.self_, X, Y, 1.0 / T,
                                                         ws.G[1], ws.count[1]))
    timed("adam", adam_both)
  torch.cuda.synchronize()
  rec["split_ms"] = {k: round(sum(a.elapsed_time(z) for a, z in v) / steps, 4) for k, v in parts.items()}
  t = guarded(lambda: loop_ms(torch_step(m, graph, h, T, R, lr, reg, nw, margin), steps, reps))
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
  d = {k: p.default for k, p in inspect.signature(Recoder.train_ccl).parameters.items()
       if p.default is not inspect.Parameter.empty}
  torch.manual_seed(0)
  rec = Recoder(model=MatrixFactorization(H), optimizer_type="adam")
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  hist = rec.train_ccl(RecommendationDataset(x), normalize=True)
  e1.record()
  torch.cuda.synchronize()
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  r20, n100 = (float(np.nanmean(np.asarray(v, dtype=np.float64))) for v in res.values())
  emit(dict({k: d[k] for k in ("num_layers", "num_epochs", "batch_size", "lr", "reg", "num_negatives",
                               "negative_weight", "margin")},
            bench="ccl_quality", normalize=True, h=H, recall20=round(r20, 4), ndcg100=round(n100, 4),
            loss=[round(v, 5) for v in hist[-1]], live_share=round(rec.ccl_stats[-1], 5),
            fit_ms=round(e0.elapsed_time(e1), 1), source="Recoder.train_ccl, MI355X"), out)


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
  for name, values in (("margins", MARGINS), ("weights", WEIGHTS), ("negatives", NEGATIVES), ("lrs", LRS),
                       ("layers", LAYERS), ("checkpoints", CHECKPOINTS)):
    ap.add_argument("--" + name, default=",".join(str(v) for v in values))
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  quality_out = args.out or os.path.join(ROOT, "profiles", "ccl_quality.jsonl")
  if args.test_reference:
    return run_test_reference(quality_out)
  if args.cpu_grid:
    f = lambda s, t: tuple(t(v) for v in s.split(","))
    cells = [(mg, nw, R, lr, K) for K in f(args.layers, int) for lr in f(args.lrs, float)
             for R in f(args.negatives, int) for nw in f(args.weights, float) for mg in f(args.margins, float)]
    return run_cpu_grid(args.jobs, cells, f(args.checkpoints, int), quality_out)
  import torch
  if not torch.cuda.is_available():
    sys.exit("ccl_bench.py measures on the GPU (only --cpu-grid and --test-reference run without one)")
  out = args.out or os.path.join(ROOT, "profiles", "ccl_bench.jsonl")
  for name in ("slice", "c2"):
    m, _ = load(name)
    for R in (64, 512):
      step_lines(m, name, args.h, args.batch, R, args.steps, args.reps, out)
  if args.quality:
    quality(out)


if __name__ == "__main__":
  main()
