#!/usr/bin/env python
"""VariationalAutoencoder against DynamicAutoencoder on the fused HIP step, one JSON line per run:

    python tools/vae_bench.py [--epochs N] [--only vae600,...] [--quality] [--out FILE]

  step     ms per step and users/s over N whole epochs of Recoder.train (after a warm one) on the
           ML-20M-like synthetic CSR (C2's generator, synthetic.ml20m_like), B = 500, logloss, dense
           Adam, noise 0.5: VAE [600, 200], DAE [600, 200], VAE [200, 200], DAE [200, 200]
  quality  (--quality) VAE [600, 200] logloss on tests/golden/real_ml20m_slice.npz: Recall@20 / @50,
           NDCG@100 on the held-out part, against a popularity ranking

The share of the rk_vae_* kernels in a step comes from a separate kernel-trace run of this script
(rocprofv3 --kernel-trace --stats -- python tools/vae_bench.py --epochs 1 --only vae600).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from recoder_amd import synthetic  # noqa: E402
from recoder_amd.data import RecommendationDataset  # noqa: E402
from recoder_amd.model import Recoder  # noqa: E402
from recoder_amd.nn import DynamicAutoencoder, VariationalAutoencoder  # noqa: E402

RUNS = {
  "vae600": lambda: VariationalAutoencoder([600, 200], activation_type="tanh", noise_prob=0.5, kl_cap=0.2,
                                           anneal_steps=200000),
  "dae600": lambda: DynamicAutoencoder([600, 200], activation_type="tanh", noise_prob=0.5),
  "vae200": lambda: VariationalAutoencoder([200, 200], activation_type="tanh", noise_prob=0.5, kl_cap=0.2,
                                           anneal_steps=200000),
  "dae200": lambda: DynamicAutoencoder([200, 200], activation_type="tanh", noise_prob=0.5),
}


def emit(rec, out):
  line = json.dumps(rec)
  print(line, flush=True)
  if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
      f.write(line + "\n")


def step_run(name, csr, epochs, B=500):
  torch.manual_seed(0)
  rec = Recoder(model=RUNS[name](), optimizer_type="adam", loss="logloss")
  ds = RecommendationDataset(csr)
  kw = dict(batch_size=B, lr=1e-3, weight_decay=0.0, negative_sampling=True)
  rec.train(ds, num_epochs=1, **kw)
  torch.cuda.synchronize()
  k0 = len(rec.loss_history)
  t0 = time.perf_counter()
  rec.train(ds, num_epochs=epochs, **kw)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  steps = sum(len(x) for x in rec.loss_history[k0:])
  users = steps * B
  last = rec.loss_history[-1]
  return dict(kind="step", run=name, hidden=rec.model.hidden_layers, B=B, epochs=epochs, steps=steps,
              ms_per_step=round(1e3 * dt / steps, 4), users_per_s=round(users / dt, 1),
              loss_last=float(last[-1]), graph=getattr(rec, "_graph_stepper", None) is not None,
              anneal_step=int(getattr(rec.model, "anneal_step", 0)))


def quality_run(epochs):
  sys.path.insert(0, ROOT)
  from tests import vae_util
  from recoder_amd.metrics import NDCG, Recall
  x, y = vae_util.load_slice()
  torch.manual_seed(0)
  m = VariationalAutoencoder([600, 200], activation_type="tanh", noise_prob=0.5, kl_cap=0.2, anneal_steps=200)
  rec = Recoder(model=m, optimizer_type="adam", loss="logloss")
  rec.train(RecommendationDataset(x), batch_size=500, lr=1e-3, num_epochs=epochs, negative_sampling=True)
  res = rec.evaluate(RecommendationDataset(x, y), num_recommendations=100,
                     metrics=[Recall(20), Recall(50), NDCG(100)], batch_size=500)
  out = {str(k): round(float(np.nanmean(np.asarray(v, dtype=np.float64))), 4) for k, v in res.items()}
  return dict(kind="quality", run="vae600_slice", epochs=epochs, **out,
              popularity_recall20=round(vae_util.popularity_recall(x, y, 20), 4))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--epochs", type=int, default=3)
  ap.add_argument("--only", default=",".join(RUNS))
  ap.add_argument("--quality", action="store_true")
  ap.add_argument("--quality-epochs", type=int, default=15)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  names = [n for n in a.only.split(",") if n]
  if names:
    csr = synthetic.ml20m_like(seed=0)
    for n in names:
      emit(step_run(n, csr, a.epochs), a.out)
  if a.quality:
    emit(quality_run(a.quality_epochs), a.out)


if __name__ == "__main__":
  main()
