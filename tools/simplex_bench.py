"""SimpleX (recoder_amd/simplex.py, rk_als_sx_forward, rk_als_sx_backward): speed on the GPU and quality on the CPU.

    python tools/simplex_bench.py [--quality] [--batch T] [--steps N] [--reps R]
    python tools/simplex_bench.py --cpu-grid [--jobs N] [--gammas ..] [--margins ..] [--checkpoints ..]
    python tools/simplex_bench.py --test-reference

default      ms per SimpleX step at gamma = 0.5 (the minimum of R timed loops after a warm-up, the largest beside it)
             and its split per launch, on the slice and on the C2-shaped matrix, beside a ``train_ccl`` step at
             ``num_layers = 0`` and at ``num_layers = 1`` (the full-graph substitute the pooling replaces) with the
             same T and R, and the same step in torch ops.  --quality adds Recall / NDCG of the default fit through the
             kernels.  -> profiles/simplex_bench.jsonl
--cpu-grid   (no GPU) the float64 restatement (tests/simplex_util.py) on the slice over gamma x margin at h = 64,
             batch 1024, R = 64, weight 16, lr 0.01, Recall@20 / NDCG@100 ranked by the cosine at every checkpoint
             -> profiles/simplex_quality.jsonl.  The options restrict the grid (the records cover what was run).
--test-reference  (no GPU) the float64 fit that tests/test_simplex.py compares against -> profiles/simplex_quality.jsonl
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_util import cpu_grid, emit, guarded, load, loop_ms, xavier_tables  # noqa: E402

H, BATCH, REG, R, NW, LR, MAX_HISTORY = 64, 1024, 1e-3, 64, 16.0, 0.01, 256
GAMMAS, MARGINS, CHECKPOINTS = (0.0, 0.25, 0.5, 0.75, 1.0), (0.0, 0.4), (5, 10)
TEST_CELL, TEST_EPOCHS = (0.5, 0.0), 2                          # the fit of tests/test_simplex.py on the slice


# ----------------------------------------------------------------- cpu grid
def _grid_point(args):
  (gamma, margin), checkpoints, seed, cosine = args
  from tests import bpr_util, ccl_util as cu, simplex_util as su
  x, y = bpr_util.load_slice()
  P, Q, _ = bpr_util.xavier_tables(x.shape[0], x.shape[1], H, seed)
  rows = []

  def on_epoch(ep, state):
    if ep in checkpoints:
      X, Y = su.tables64(x, *state["E0"], gamma, MAX_HISTORY)
      if cosine:
        X, Y = cu.unit_rows(X), cu.unit_rows(Y)
      rows.append((ep,) + tuple(float(v) for v in su.quality(X, Y, x, y)))
  _, _, _, hist, stats = su.fit(x, P, Q, gamma, MAX_HISTORY, max(checkpoints), BATCH, LR, REG, R, NW, margin, seed=seed,
                                on_epoch=on_epoch)
  return [{"bench": "simplex_quality", "gamma": gamma, "max_history": MAX_HISTORY, "margin": margin,
           "negative_weight": NW, "num_negatives": R, "lr": LR, "reg": REG, "h": H, "batch_size": BATCH, "seed": seed,
           "num_epochs": ep, "ranked_by": "cosine" if cosine else "dot", "recall20": round(r, 4),
           "ndcg100": round(n, 4), "loss": [float(v) for v in hist[ep - 1]],
           "live_share": round(float(stats[ep - 1]), 5),
           "source": "float64 restatement (tests/simplex_util.py), CPU"} for ep, r, n in rows]


def run_test_reference(out):
  """The float64 restatement of the end-to-end fit of tests/test_simplex.py (ranked by the dot product, as the test
  ranks): the figures its constants copy."""
  for rec in _grid_point((TEST_CELL, tuple(range(1, TEST_EPOCHS + 1)), 0, False)):
    emit(dict(rec, bench="simplex_test_reference"), out)


# ------------------------------------------------------------------ timing
def torch_step(m, graph, h, T, lr, reg, margin, gamma, L):
  """The same step in torch ops on the same slots: the histories as one padded [users, E] index table, private
  uniform negatives from torch's generator."""
  import torch
  import torch.nn.functional as Fn
  from recoder_amd import bpr, simplex
  dev = graph.su.device
  lens = np.diff(m.indptr)
  E = simplex.entry_width(lens, L)
  pad = np.full((m.shape[0], E), m.shape[1], np.int64)
  for u in range(m.shape[0]):
    row = m.indices[m.indptr[u]:m.indptr[u + 1]]
    pos = simplex.history_positions(len(row), L)
    pad[u, :len(pos)] = row[pos]
  pad = torch.as_tensor(pad, device=dev)
  inv = torch.as_tensor(1.0 / np.maximum(np.minimum(lens, L), 1), dtype=torch.float32, device=dev)
  P, Q = (torch.nn.Parameter(t) for t in xavier_tables(m.shape[0], m.shape[1], h, dev))
  W = torch.nn.Parameter(torch.eye(h, device=dev))
  opt = torch.optim.Adam([P, Q, W], lr=lr)
  users, pos, neg = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(3))
  gen = torch.Generator(device=dev)

  def one(s):
    bpr.sample(graph.ucsr, 0, s, users, pos, neg)
    u, i = users.long(), pos.long()
    j = torch.randint(0, m.shape[1], (T, R), device=dev, generator=gen)
    cand = torch.cat([i[:, None], j], 1)
    Qp = torch.cat([Q, torch.zeros(1, h, device=dev)])
    b = Fn.embedding(pad[u], Qp).sum(1) * inv[u][:, None]
    p = gamma * Fn.embedding(u, P) + (1 - gamma) * b @ W.T
    c = torch.bmm(Fn.normalize(Fn.embedding(cand, Q), dim=2), Fn.normalize(p, dim=1)[:, :, None])[:, :, 0]
    loss = (1 - c[:, 0]).sum() + (NW / R) * torch.relu(c[:, 1:] - margin).sum()
    loss = loss / T + 0.5 * reg * (P[u].pow(2).sum() + Q[i].pow(2).sum()) / T
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
  return one


def step_lines(m, name, h, T, steps, reps, out):
  import torch
  from recoder_amd import als, bpr, ccl, lightgcn, simplex
  dev = torch.device("cuda")
  graph = lightgcn.Graph(*als.csr_pair(m, m.shape[0], m.shape[1], dev))
  lr, reg, margin, gamma, L = LR, REG, 0.0, 0.5, MAX_HISTORY
  E = simplex.entry_width(np.diff(m.indptr), L)
  rec = {"bench": "simplex_step", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz), "h": h,
         "batch_size": T, "num_negatives": R, "margin": margin, "negative_weight": NW, "gamma": gamma,
         "max_history": L, "entries": E, "steps": steps, "repetitions": reps}
  X, Y = xavier_tables(m.shape[0], m.shape[1], h, dev)
  state = simplex.new_state(X, Y, (gamma, L))
  ws = simplex.Workspace(m.shape[0], m.shape[1], T, h, dev, num_negatives=R, entries=E, pooled=True)
  one = lambda s: simplex.step(X, Y, graph, state, ws, 0, s, lr, reg, R, NW, margin)
  for s in range(300):                                        # (a trained table is the case, as tools/ccl_bench.py)
    one(s)
  rec["hip_ms_per_step"], rec["hip_ms_per_step_max"] = loop_ms(lambda s: one(300 + s), steps, reps)
  rec["live_share"] = round(float(ws.live.sum()) / (float(ws.bpr.g.sum()) * R), 5)
  for K in (0, 1):                                            # train_ccl's step: the tables themselves; one full-graph layer
    CX, CY = xavier_tables(m.shape[0], m.shape[1], h, dev)
    cstate = ccl.new_state(CX, CY, K)
    cws = ccl.Workspace(m.shape[0], m.shape[1], T, h, dev, num_negatives=R)
    cone = lambda s: ccl.step(CX, CY, graph, cstate, cws, 0, s, lr, reg, R, NW, margin)
    for s in range(50):
      cone(s)
    key = "ccl_layers%d_ms_per_step" % K
    rec[key], rec[key + "_max"] = loop_ms(lambda s: cone(50 + s), steps, reps)
    rec["over_ccl_layers%d_step" % K] = round(rec["hip_ms_per_step"] / rec[key], 3)
  b, parts, sorted_ = ws.bpr, {}, {}
  P, Q, W = state["E0"]

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

  def history_sort():
    ws.H[1].zero_(), ws.count2.zero_()
    sorted_["h"] = torch.sort(ws.hkey.view(-1), stable=True)

  def adam_all():
    state["step"] += 1
    for k, (g, c) in enumerate(((ws.G[0], ws.count[0]), (ws.G[1], ws.count[1]), (ws.dW, ws.zero_h))):
      lightgcn.adam(state["E0"][k], g, c, reg / T, state["M"][k], state["V"][k], lr, state["step"])
  for s in range(10000, 10000 + steps):
    timed("sample", lambda: bpr.sample(graph.ucsr, 0, s, b.users, b.pos, b.neg))
    timed("sx_forward", lambda: simplex.forward(b.users, graph.ucsr, Q, P, W, gamma, L, X, B=ws.B, hkey=ws.hkey,
                                                hcoef=ws.hcoef))
    timed("ccl_grad", lambda: ccl.grad(b.users, b.pos, R, 0, s, X, Q, margin, NW, ws.cand, ws.key, ws.coef, ws.self_,
                                       b.D, b.g, ws.loss, ws.live))
    timed("sorts_zero", sorts)
    timed("lgcn_scatter_users", lambda: lightgcn.scatter(*sorted_["u"], 1, b.g, b.D, -gamma / T, ws.G[0], ws.count[0]))
    timed("ccl_scatter_candidates", lambda: ccl.scatter(*sorted_["i"], 1 + R, b.users, ws.coef, ws.self_, X, Q,
                                                        1.0 / T, ws.G[1], ws.count[1]))
    timed("sx_backward", lambda: simplex.backward(b.D, b.g, ws.B, W, (1.0 - gamma) / T, ws.dB, ws.part, ws.dW))
    timed("history_sort_zero", history_sort)
    timed("ccl_scatter_history", lambda: ccl.scatter(*sorted_["h"], E, ws.slots, ws.hcoef, ws.zero_self, ws.dB, Q, 1.0,
                                                     ws.H[1], ws.count2))
    timed("history_add", lambda: ws.G[1].add_(ws.H[1]))
    timed("adam", adam_all)
  timed("sx_forward_all_users", lambda: simplex._all_users(X, graph.ucsr, state, ws.all_users))
  torch.cuda.synchronize()
  rec["split_ms"] = {k: round(sum(a.elapsed_time(z) for a, z in v) / len(v), 4) for k, v in parts.items()}
  t = guarded(lambda: loop_ms(torch_step(m, graph, h, T, lr, reg, margin, gamma, L), steps, reps))
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
  d = {k: p.default for k, p in inspect.signature(Recoder.train_simplex).parameters.items()
       if p.default is not inspect.Parameter.empty}
  torch.manual_seed(0)
  rec = Recoder(model=MatrixFactorization(H), optimizer_type="adam")
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  hist = rec.train_simplex(RecommendationDataset(x), normalize=True)
  e1.record()
  torch.cuda.synchronize()
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  r20, n100 = (float(np.nanmean(np.asarray(v, dtype=np.float64))) for v in res.values())
  emit(dict({k: d[k] for k in ("gamma", "max_history", "num_epochs", "batch_size", "lr", "reg", "num_negatives",
                               "negative_weight", "margin")},
            bench="simplex_quality", normalize=True, h=H, recall20=round(r20, 4), ndcg100=round(n100, 4),
            loss=[round(v, 5) for v in hist[-1]], live_share=round(rec.simplex_stats[-1], 5),
            fit_ms=round(e0.elapsed_time(e1), 1), source="Recoder.train_simplex, MI355X"), out)


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
  for name, values in (("gammas", GAMMAS), ("margins", MARGINS), ("checkpoints", CHECKPOINTS)):
    ap.add_argument("--" + name, default=",".join(str(v) for v in values))
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  quality_out = args.out or os.path.join(ROOT, "profiles", "simplex_quality.jsonl")
  if args.test_reference:
    return run_test_reference(quality_out)
  if args.cpu_grid:
    f = lambda s, t: tuple(t(v) for v in s.split(","))
    cells = [(g, mg) for mg in f(args.margins, float) for g in f(args.gammas, float)]
    return cpu_grid(_grid_point, [(c, f(args.checkpoints, int), 0, True) for c in cells], args.jobs, quality_out)
  import torch
  if not torch.cuda.is_available():
    sys.exit("simplex_bench.py measures on the GPU (only --cpu-grid and --test-reference run without one)")
  out = args.out or os.path.join(ROOT, "profiles", "simplex_bench.jsonl")
  for name in ("slice", "c2"):
    m, _ = load(name)
    step_lines(m, name, args.h, args.batch, args.steps, args.reps, out)
  if args.quality:
    quality(out)


if __name__ == "__main__":
  main()
