"""NeuMF (recoder_amd/ncf.py, rk_als_ncf_*): speed on the GPU and quality on the CPU.

    python tools/ncf_bench.py [--quality] [--steps N] [--reps R]
    python tools/ncf_bench.py --cpu-grid [--jobs N] [--lrs ..] [--negatives ..] [--checkpoints ..]

default      ms per ``ncf.step`` (the minimum of R timed loops after a warm-up, the largest beside it) and its split per
             launch, on the ML-20M slice at batch 1024 and on the C2-shaped matrix at batch 4096, at the default sizes and
             4 negatives, beside the same step in torch ops (embedding gathers, three linear layers, BCE-with-logits,
             autograd, Adam on every parameter); rk_als_ncf_item_part and rk_als_ncf_scores for 500 users over the
             catalogue beside the same scoring in torch ops (the layer-1 split too, so that no [B, n, 2 dm] tensor is
             formed).  --quality adds Recall@20 / NDCG@100 of ``Recoder.train_ncf`` at its defaults on the slice.
             -> profiles/ncf_bench.jsonl
--cpu-grid   (no GPU) the float64 restatement (tests/ncf_util.py) on the slice from ``train_ncf``'s own start, over
             lr x num_negatives x sizes at batch 1024, reg 0, Recall@20 / NDCG@100 at every checkpoint
             -> profiles/ncf_quality.jsonl.  The options restrict the grid (the records cover what was run); the file
             holds this grid and ``--cpu-grid --lrs 0.001 --checkpoints 15,20`` behind it (the cells that still rose).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_util import cpu_grid, emit, event_ms, guarded, load, loop_ms  # noqa: E402

DEFAULT = (32, 32, (64, 32, 16))
SIZES = (DEFAULT, (16, 16, (32, 16, 8)))
LRS, NEGATIVES, CHECKPOINTS = (1e-3, 3e-3), (4, 8), (2, 5, 10)
BATCH, REG = 1024, 0.0


# ----------------------------------------------------------------- cpu grid
def _grid_point(args):
  sizes, lr, R, checkpoints, seed = args
  from tests import bpr_util, ncf_util as nu, rp3_util
  x, y = bpr_util.load_slice()
  state, recs, done, hist = None, [], 0, []
  p0 = nu.start_params(sizes, x.shape[0], x.shape[1], seed)
  for ep in sorted(checkpoints):
    state, h = nu.fit(x, p0, sizes, ep - done, BATCH, lr, REG, R, seed=seed, state=state)
    done, hist = ep, hist + h
    S = nu.scores_blocked(nu.state_params(state), np.arange(x.shape[0]))
    r, n = rp3_util.metric_means(rp3_util.top_k(S, x, 100), y)
    recs.append({"bench": "ncf_quality", "embedding_size": sizes[0], "mlp_embedding_size": sizes[1],
                 "mlp_layers": list(sizes[2]), "lr": lr, "num_negatives": R, "reg": REG, "batch_size": BATCH,
                 "seed": seed, "num_epochs": ep, "recall20": round(r, 4), "ndcg100": round(n, 4),
                 "loss": round(hist[-1], 5), "source": "float64 restatement (tests/ncf_util.py), CPU"})
  return recs


# ------------------------------------------------------------------ timing
def torch_model(model):
  """The model's parameters as leaves torch's autograd and Adam own."""
  import torch
  P = {k: torch.nn.Parameter(getattr(model, k).data.clone()) for k in ("Pg", "Qg", "Pm", "Qm", "w", "b0")}
  Ws = [torch.nn.Parameter(W.data.clone()) for W in model.mlp_weights]
  cs = [torch.nn.Parameter(c.data.clone()) for c in model.mlp_biases]
  return P, Ws, cs


def torch_step(model, ucsr, T, R, lr):
  import torch
  import torch.nn.functional as Fn
  from recoder_amd import bpr
  dev = model.Pg.device
  P, Ws, cs = torch_model(model)
  opt = torch.optim.Adam(list(P.values()) + Ws + cs, lr=lr)
  users, pos, neg = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(3))
  gen = torch.Generator(device=dev)
  y = torch.zeros(T, 1 + R, device=dev)
  y[:, 0] = 1.0
  dg = P["Pg"].shape[1]

  def one(s):
    bpr.sample(ucsr, 0, s, users, pos, neg)
    u = users.long()[:, None].expand(T, 1 + R).reshape(-1)
    i = torch.cat([pos.long()[:, None], torch.randint(0, P["Qg"].shape[0], (T, R), device=dev, generator=gen)],
                  1).reshape(-1)
    x = torch.cat([Fn.embedding(u, P["Pm"]), Fn.embedding(i, P["Qm"])], 1)
    for W, c in zip(Ws, cs):
      x = torch.relu(Fn.linear(x, W, c))
    z = (Fn.embedding(u, P["Pg"]) * Fn.embedding(i, P["Qg"])) @ P["w"][:dg] + x @ P["w"][dg:] + P["b0"]
    loss = Fn.binary_cross_entropy_with_logits(z, y.reshape(-1))
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
  return one


def torch_scores(model, users):
  """The same scores in torch ops with layer 1 split into halves: the [B, n, d1] block is its largest tensor."""
  import torch
  with torch.no_grad():
    return model.torch_forward(None, input_users=users)


def bench_lines(m, name, T, R, steps, reps, out):
  import torch
  from recoder_amd import bpr, lightgcn, ncf
  from recoder_amd.nn import NeuralMatrixFactorization
  dev = torch.device("cuda")
  model = NeuralMatrixFactorization(*DEFAULT)
  model.init_model(m.shape[1], m.shape[0])
  model = model.to(dev)
  sizes, lr = model.sizes(), 1e-3
  ucsr = bpr.user_csr(m, m.shape[0], m.shape[1], dev)
  rec = {"bench": "ncf_step", "data": name, "users": m.shape[0], "items": m.shape[1], "nnz": int(m.nnz),
         "sizes": [sizes[0], sizes[1], list(sizes[2])], "batch_size": T, "num_negatives": R, "entries": T * (1 + R),
         "steps": steps, "repetitions": reps}
  state = ncf.new_state(model)
  ws = ncf.Workspace(m.shape[0], m.shape[1], T, R, sizes, dev)
  one = lambda s: ncf.step(ucsr, state, ws, 0, s, lr, REG)
  for s in range(100):                                        # (a table that has moved is the case)
    one(s)
  rec["hip_ms_per_step"], rec["hip_ms_per_step_max"] = loop_ms(lambda s: one(100 + s), steps, reps)
  parts, sorted_ = {}, {}
  U, I, theta, dg = state["U"], state["I"], state["theta"], sizes[0]

  def timed(key, fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    parts.setdefault(key, []).append((a, z))

  def sorts():
    for t in ws.G + ws.count:
      t.zero_()
    sorted_["u"], sorted_["i"] = torch.sort(ws.ukey, stable=True), torch.sort(ws.ikey, stable=True)

  def adams():
    state["step"] += 1
    for side, table in enumerate((U, I)):
      lightgcn.adam(table, ws.G[side], ws.count[side], REG / ws.E, state["M"][side], state["V"][side], lr,
                    state["step"])
  for s in range(10000, 10000 + steps):
    timed("bpr_sample", lambda: bpr.sample(ucsr, 0, s, ws.users, ws.pos, ws.neg))
    timed("ncf_step", lambda: ncf.step_kernel(ws.users, ws.pos, R, 0, s, U[:, :dg], I[:, :dg], U[:, dg:], I[:, dg:],
                                              theta, sizes, ws.ukey, ws.ikey, ws.GU, ws.GI, ws.slabs))
    timed("sorts_zero", sorts)
    timed("lgcn_scatter_users", lambda: lightgcn.scatter(*sorted_["u"], 1, ws.ones, ws.GU, -1.0 / ws.E, ws.G[0],
                                                         ws.count[0]))
    timed("lgcn_scatter_items", lambda: lightgcn.scatter(*sorted_["i"], 1, ws.ones, ws.GI, -1.0 / ws.E, ws.G[1],
                                                         ws.count[1]))
    timed("lgcn_adam_both", adams)
    timed("ncf_dense_adam", lambda: ncf.dense_adam(theta, state["M"][2], state["V"][2], ws.slabs, ws.E, sizes, lr, REG,
                                                   state["step"], ws.loss))
  torch.cuda.synchronize()
  rec["split_ms"] = {k: round(sum(a.elapsed_time(z) for a, z in v) / len(v), 4) for k, v in parts.items()}
  t = guarded(lambda: loop_ms(torch_step(model, ucsr, T, R, lr), steps, reps))
  if isinstance(t, tuple):
    rec["torch_ops_step_ms"], rec["torch_ops_step_ms_max"] = t
    rec["step_faster_than_torch_ops"] = rec["hip_ms_per_step"] < rec["torch_ops_step_ms"]
  else:
    rec["torch_ops_step_ms"] = t
  emit(rec, out)
  # ---- scoring: 500 users over the catalogue
  ncf.unpack(model, U, I, theta)
  B, n = min(500, m.shape[0]), m.shape[1]
  users = torch.arange(B, dtype=torch.int32, device=dev)
  outbuf = torch.empty(B, n, dtype=torch.float32, device=dev)
  srec = {"bench": "ncf_scores", "data": name, "users": B, "items": n, "sizes": rec["sizes"]}
  th = ncf.pack(model)[2]
  srec["item_part_ms"] = round(event_ms(lambda: ncf.item_part(model.Qm.data, th, sizes), reps), 4)
  model._weights_written()
  model.user_scores(users, 0, n, outbuf, n)
  srec["scores_ms"] = round(event_ms(lambda: model.user_scores(users, 0, n, outbuf, n), reps), 4)
  srec["pairs_per_us"] = round(B * n / (1e3 * srec["scores_ms"]), 1)
  t = guarded(lambda: event_ms(lambda: torch_scores(model, users.long()), reps))
  srec["torch_ops_scores_ms"] = None if t is None else round(t, 4)
  if t is not None:
    srec["scores_faster_than_torch_ops"] = srec["scores_ms"] < t
    ref = torch_scores(model, users.long())
    srec["max_abs_difference_to_torch_ops"] = float((ref - outbuf).abs().max())
  emit(srec, out)


def quality(out):
  import inspect
  import torch
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import NeuralMatrixFactorization
  x, y = load("slice")
  d = {k: p.default for k, p in inspect.signature(Recoder.train_ncf).parameters.items()
       if p.default is not inspect.Parameter.empty}
  rec = Recoder(model=NeuralMatrixFactorization(), use_cuda=True, user_based=True)
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  hist = rec.train_ncf(RecommendationDataset(x))
  e1.record()
  torch.cuda.synchronize()
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
  r20, n100 = (float(np.nanmean(np.asarray(v, dtype=np.float64))) for v in res.values())
  emit(dict({k: d[k] for k in ("num_epochs", "batch_size", "lr", "reg", "num_negatives", "seed")},
            bench="ncf_quality", sizes=[DEFAULT[0], DEFAULT[1], list(DEFAULT[2])], recall20=round(r20, 4),
            ndcg100=round(n100, 4), loss=round(hist[-1], 5), fit_ms=round(e0.elapsed_time(e1), 1),
            source="Recoder.train_ncf, MI355X"), out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--jobs", type=int, default=8)
  for name, values in (("lrs", LRS), ("negatives", NEGATIVES), ("checkpoints", CHECKPOINTS)):
    ap.add_argument("--" + name, default=",".join(str(v) for v in values))
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    f = lambda s, t: tuple(t(v) for v in s.split(","))
    out = args.out or os.path.join(ROOT, "profiles", "ncf_quality.jsonl")
    work = [(sizes, lr, R, f(args.checkpoints, int), 0) for sizes in SIZES for lr in f(args.lrs, float)
            for R in f(args.negatives, int)]
    return cpu_grid(_grid_point, work, args.jobs, out)
  import torch
  if not torch.cuda.is_available():
    sys.exit("ncf_bench.py measures on the GPU (only --cpu-grid runs without one)")
  out = args.out or os.path.join(ROOT, "profiles", "ncf_bench.jsonl")
  for name, T in (("slice", 1024), ("c2", 4096)):
    m, _ = load(name)
    bench_lines(m, name, T, 4, args.steps, args.reps, out)
  if args.quality:
    quality(out)


if __name__ == "__main__":
  main()
