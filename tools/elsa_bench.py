#!/usr/bin/env python
"""ELSA quality grid, step and kernel times (recoder_amd/elsa.py, rk_ease_elsa_* in librecoder_ease.so), one JSON line
per record:

    python tools/elsa_bench.py --cpu-grid [--out FILE]       (no GPU)
    python tools/elsa_bench.py --quality [--out FILE]

  --cpu-grid  the float64 restatement (tests/elsa_util.py, the Gram form) on the ML-20M slice, into
          profiles/elsa_quality.jsonl: embedding_size {64, 256} x lr {0.03, 0.1, 0.3} at batch 1024, seed 0, each run
          read after 5, 10 and 20 epochs (Recall@20, NDCG@100, the epoch's mean loss).  Then the test's point
          (embedding_size 64, 5 epochs, lr 0.1, batch 1024) for the seeds 0..4 in float64 and, beside it, the
          published dense formulation in float32; the float64 values go to tests/golden/elsa_slice.json with the
          interval tests/test_elsa.py checks and whether the float32 runs lie inside it.
  --quality   on the GPU, into profiles/elsa_bench.jsonl, on the slice and on the C2-shaped synthetic matrix at
          embedding_size 256, batch 1024:
          elsa_step     ms per step (the smallest and the largest of 5 timed loops of 20 steps after a warm-up), and per
                        launch of the chain, each timed alone with its operands made beforehand (the smallest and the largest of 5
                        timed loops of 10 launches after three warm ones), beside the
                        published dense step (X_b A A^T - X_b, the loss, autograd, torch.optim.Adam) in torch f32 ops
                        on the same device
          elsa_quality  on the slice: Recall@20 / NDCG@100 of train_elsa at the model's defaults and at the test's point
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_util import emit, guarded, load, loop_ms  # noqa: E402

HS, LRS, READ_AT, BATCH = (64, 256), (0.03, 0.1, 0.3), (5, 10, 20), 1024
POINT = dict(embedding_size=64, num_epochs=5, lr=0.1, batch_size=1024)     # (the point of tests/test_elsa.py)
SEEDS = (0, 1, 2, 3, 4)
GOLDEN = os.path.join(ROOT, "tests", "golden", "elsa_slice.json")


# ------------------------------------------------------------------ the CPU cells
def cpu_grid(out):
  from tests import elsa_util as eu
  x, y = load("slice")
  src = "float64 restatement (tests/elsa_util.py, Gram form), CPU"
  for h in HS:
    for lr in LRS:
      t0 = time.perf_counter()
      _, hist, reads = eu.fit(x, h, max(READ_AT), BATCH, lr, 0, read_at=READ_AT)
      for e in READ_AT:
        r20, n100 = eu.quality(x, y, reads[e])
        emit(dict(bench="elsa_quality", embedding_size=h, lr=lr, batch_size=BATCH, seed=0, epochs=e,
                  recall20=round(r20, 6), ndcg100=round(n100, 6), loss=hist[e - 1],
                  seconds=round(time.perf_counter() - t0, 1), source=src), out)
  lr, batch = POINT["lr"], POINT["batch_size"]
  h, epochs = POINT["embedding_size"], POINT["num_epochs"]
  got = {"f64": [], "f32": []}
  for seed in SEEDS:
    for form, key in (("gram", "f64"), ("dense32", "f32")):
      W, hist, _ = eu.fit(x, h, epochs, batch, lr, seed, form=form)
      r20, n100 = eu.quality(x, y, W)
      got[key].append((r20, n100))
      emit(dict(bench="elsa_point", form=form, embedding_size=h, lr=lr, batch_size=batch, seed=seed, epochs=epochs,
                recall20=round(r20, 6), ndcg100=round(n100, 6), loss=hist[-1]), out)
  golden = dict(point=dict(embedding_size=h, num_epochs=epochs, lr=lr, batch_size=batch), seeds=list(SEEDS),
                recall20=[v[0] for v in got["f64"]], ndcg100=[v[1] for v in got["f64"]])
  inside = True
  for i, name in enumerate(("recall20", "ndcg100")):
    lo, hi = min(golden[name]), max(golden[name])
    golden[name + "_interval"] = [lo - (hi - lo), hi + (hi - lo)]
    inside = inside and all(lo - (hi - lo) <= v[i] <= hi + (hi - lo) for v in got["f32"])
  golden["float32_inside"] = bool(inside)
  golden["float32_recall20"] = [v[0] for v in got["f32"]]
  golden["float32_ndcg100"] = [v[1] for v in got["f32"]]
  with open(GOLDEN, "w") as f:
    json.dump(golden, f, indent=1, sort_keys=True)
    f.write("\n")


# ------------------------------------------------------------------ the GPU runs
def _launch_ms(fn, reps=10, loops=5):
  """[the smallest, the largest] ms per call of ``loops`` timed loops of ``reps`` calls, after three warm calls."""
  return list(loop_ms(lambda s: fn(), reps, reps=loops))


def step_times(name, x, h, out):
  import torch
  from types import SimpleNamespace
  from recoder_amd import als, elsa
  from recoder_amd.admm import gemm
  from recoder_amd.ease import scores
  dev = "cuda"
  U, n = x.shape
  ucsr, _ = als.csr_pair(x, U, n, dev)
  W = torch.from_numpy(elsa.initial_factors(n, h, 0)).to(dev)
  st = elsa.State(W, BATCH)
  order = torch.from_numpy(elsa.epoch_order(U, 0, 0).astype(np.int64)).to(dev)
  t2 = elsa.row_squares(ucsr)[order]
  pair_ms = _launch_ms(lambda: elsa.permuted_pair(ucsr, order), 3)
  pair = elsa.permuted_pair(ucsr, order)
  nb = U // BATCH
  acc = torch.zeros(1, dtype=torch.float64, device=dev)
  run = lambda s: st.step(pair, t2, (s % nb) * BATCH, (s % nb) * BATCH + BATCH, 0.01, acc)
  lo_ms, hi_ms = loop_ms(run, 20, reps=5)
  # the chain, launch by launch, on the first batch
  pu, pt = pair
  b = BATCH
  Z, Q, E, F = st.Z, st.Q, st.E, st.F
  batch = SimpleNamespace(indptr=pu.indptr, indices=pu.indices, data=pu.data, shape=(b, n))
  S, Zt = als.gram(st.A, 0.0, None, st.gws)[0], Z.t().contiguous()       # (operands of the products, made beforehand)
  parts = dict(
      scores_Z=lambda: scores(batch, st.A, 0, h, out=Z, ld=h, n_rows=b),
      gram_S=lambda: als.gram(st.A, 0.0, None, st.gws),
      gemm_Q=lambda: gemm(Z, S, Q),
      rows=lambda: elsa.rows(Z, Q, t2[:b], n, E, F, st.row_loss, acc),
      scatter=lambda: elsa.scatter(pt, 0, b, E, st.dA),
      transpose_Z=lambda: Z.t().contiguous(),
      gemm_M=lambda: gemm(Zt, F, st.Mm),
      gemm_dA=lambda: gemm(st.A, st.Mm, st.dA, 1.0, 1.0, E=st.dA),
      adam=lambda: elsa.adam(st.W, st.dA, st.A, st.norms, st.M, st.V, 0.01, 1000))
  ms = {k: _launch_ms(f) for k, f in parts.items()}
  flop = 2.0 * (2 * n * h * h + 2 * b * h * h) + 4.0 * x.nnz / U * b * h
  rec = dict(bench="elsa_step", data=name, n_users=U, n=n, nnz=int(x.nnz), embedding_size=h, batch_size=b,
             step_ms_min=lo_ms, step_ms_max=hi_ms, loops=5, steps_per_loop=20, permuted_pair_ms=pair_ms, launch_ms=ms,
             dense_flop_per_step=flop, tflops=round(flop / (lo_ms * 1e-3) / 1e12, 3))

  def dense():
    Wd = torch.nn.Parameter(torch.from_numpy(elsa.initial_factors(n, h, 0)).to(dev))
    opt = torch.optim.Adam([Wd], lr=0.01)
    xs = [torch.from_numpy(np.asarray(x[order.cpu().numpy()[i * b:(i + 1) * b]].todense(), np.float32)).to(dev)
          for i in range(min(nb, 4))]

    def one(s):
      X = xs[s % len(xs)]
      A = torch.nn.functional.normalize(Wd, dim=-1)
      P = (X @ A) @ A.t() - X
      loss = torch.nn.functional.mse_loss(torch.nn.functional.normalize(P, dim=-1),
                                          torch.nn.functional.normalize(X, dim=-1))
      opt.zero_grad(set_to_none=True)
      loss.backward()
      opt.step()
    return loop_ms(one, 20, reps=5)
  d = guarded(dense)
  if d is not None:
    rec.update(torch_dense_ms_min=d[0], torch_dense_ms_max=d[1], speedup=round(d[0] / lo_ms, 2))
  emit(rec, out)


def quality(x, y, out):
  import torch
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall
  from recoder_amd.model import Recoder
  from recoder_amd.nn import LowRankShallowAutoencoder
  for label, h, kw in (("defaults", 256, {}), ("point", POINT["embedding_size"], {k: v for k, v in POINT.items() if k != "embedding_size"})):
    rec = Recoder(model=LowRankShallowAutoencoder(h))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = rec.train_elsa(RecommendationDataset(x), **kw)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                       metrics=[Recall(k=20, normalize=True), NDCG(k=100)], batch_size=500)
    got = {str(k): float(np.nanmean(np.asarray(v, np.float64))) for k, v in res.items()}
    emit(dict(bench="elsa_quality", cell=label, embedding_size=h, epochs=len(hist), loss=hist,
              fit_seconds=round(fit_s, 3), recall20=round(got[str(Recall(k=20))], 6),
              ndcg100=round(got[str(NDCG(k=100))], 6), source="kernels, MI355X"), out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--cpu-grid", action="store_true")
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if args.cpu_grid:
    cpu_grid(args.out or os.path.join(ROOT, "profiles", "elsa_quality.jsonl"))
  if args.quality:
    import torch
    if not torch.cuda.is_available():
      raise SystemExit("--quality needs an MI355X: there is no CPU path for the kernels")
    out = args.out or os.path.join(ROOT, "profiles", "elsa_bench.jsonl")
    x, y = load("slice")
    step_times("slice", x, 256, out)
    step_times("c2", load("c2")[0], 256, out)
    quality(x, y, out)


if __name__ == "__main__":
  main()
