"""What the side libraries' bench tools (tools/*_bench.py) share: the JSON line, the two data sets, the
guarded torch step, the event timers, the start tables of the graph-trained methods and the grid of CPU jobs."""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emit(rec, out):
  line = json.dumps(rec)
  print(line, flush=True)
  if out:
    with open(out, "a") as f:
      f.write(line + "\n")


def load(name):
  """(x, y): c2 = synthetic.ml20m_like(seed=0), no held-out part; else the ML-20M slice and its held-out part."""
  if name == "c2":
    from recoder_amd import synthetic
    return sp.csr_matrix(synthetic.ml20m_like(seed=0)), None
  z = np.load(os.path.join(ROOT, "tests", "golden", "real_ml20m_slice.npz"))
  shape = tuple(int(v) for v in z["shape"])
  mk = lambda p: sp.csr_matrix((z[p + "/data"], z[p + "/indices"], z[p + "/indptr"]), shape=shape)
  return mk("x"), mk("y")


def guarded(fn):
  try:
    return fn()
  except Exception as e:          # (an op this torch build lacks, or no room for the dense matrix: reported, not fatal)
    print("torch restatement step not available: %s: %s" % (type(e).__name__, e), file=sys.stderr)
    return None


def event_ms(fn, reps):
  """ms of one ``fn()`` by HIP events: the mean of ``reps`` calls after a warm one."""
  import torch
  fn()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(reps):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / reps


def loop_ms(run, steps, reps=1):
  """(the smallest ms per step of ``reps`` timed loops of ``steps`` calls ``run(s)`` after a warm-up of three, the
  largest); s counts on from 0."""
  import torch
  for s in range(3):
    run(s)
  torch.cuda.synchronize()
  got = []
  for r in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(3 + r * steps, 3 + (r + 1) * steps):
      run(s)
    e1.record()
    torch.cuda.synchronize()
    got.append(e0.elapsed_time(e1) / steps)
  return round(min(got), 4), round(max(got), 4)


def xavier_tables(n_users, n_items, h, dev):
  """(X, Y) on ``dev``: Xavier-uniform under torch seed 0."""
  import torch
  torch.manual_seed(0)
  X, Y = torch.empty(n_users, h), torch.empty(n_items, h)
  torch.nn.init.xavier_uniform_(X)
  torch.nn.init.xavier_uniform_(Y)
  return X.to(dev), Y.to(dev)


def cpu_grid(job, work, jobs, out):
  """Emits the records of ``job(w)`` for every w of ``work``, in order, from a spawn pool of ``jobs`` single-threaded
  processes (``job`` is a module-level function of the tool)."""
  import multiprocessing as mp
  for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[var] = "1"                                # (the spawned workers read it when they import numpy)
  with mp.get_context("spawn").Pool(min(jobs, len(work))) as pool:
    for recs in pool.imap(job, work):
      for rec in recs:
        emit(rec, out)
