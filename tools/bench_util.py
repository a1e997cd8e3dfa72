"""What the side libraries' bench tools (tools/*_bench.py) share: the JSON line, the two data sets, the
guarded torch step and the event timer."""
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
