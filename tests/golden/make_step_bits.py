#!/usr/bin/env python
"""The bits of the one-call training step (rk_ae_train_step, sequenced by FusedEngine._c_train_step): three steps of
DynamicAutoencoder([h]) through Recoder.train per case, and the SHA-256 over every parameter, both Adam moments of
every parameter and the three losses.

    python tests/golden/make_step_bits.py           # writes tests/golden/step_bits.json (needs the GPU)
    python tests/golden/make_step_bits.py --modes   # writes tests/golden/step_modes.json (host only)

tests/test_step_bits.py recomputes digests() and compares; tests/test_step_route.py recomputes modes(words()).  Both files
were written at commit 660bd50 ("Pin encoder forward, noise draw and row kernels to float64 references"), the last one
whose rk_ae_train_step decided its kernels with a set of interdependent locals: this script uses only names that exist
there, so checking that commit out beside this file and running it reproduces the fixtures.  A digest that moves
means the step launched other kernels, or the same ones with other arguments or in another order.  Every case is run
twice and is written only when the two runs agree.

Each case trains on the first 3 B users of one synthetic matrix (N_USERS x N_ITEMS, negative sampling on):
  eager   one block of 3 B users, three batches of it: row_off = 0, B, 2 B
  graph   three blocks of B users replayed as one HIP graph (a replayed block is one batch: row_off = 0 throughout)
h: 36 (h % 32 != 0: the ones-column bias path), 64, 96 (inside the fused dZ, outside the register-resident decode),
260 (outside both); B: 40, 200 (four row tiles: the first size at which gb_part has room for the bias gradient's K
slabs, so that the ones-column path is taken), 1056 (>= 1024: the pipelined kernels, three row segments), 1504 (item
parallel only: dW as two K slabs); tanh (bounded) and relu (rk_amax + rk_split_z); the three losses; tied
and untied tables; input noise 0.5 and 0.  RK_GEMM_PREC=f32 / bf16 cases run in a child process each (the library
reads the variable once); the one-rank data-parallel cases (RK_FORCE_DP=1, plus RK_DP_ZERO=force or
RK_DP_ITEMSETS=local) and the one-rank item-parallel ones (RK_PARALLEL=items) under a one-rank RCCL group."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "step_bits.json")
MODES_OUT = os.path.join(HERE, "step_modes.json")

N_USERS, N_ITEMS = 4512, 300
PRECS = ("", "f32", "bf16")


def _case(h, B, act, loss, tied=False, noise=0.5, graph=False, par="", prec=""):
  name = "%s%sh%d_B%d_%s_%s_%s_n%d_%s" % (prec and prec + "_", par and par + "_", h, B, act, loss,
                                         "tied" if tied else "untied", int(noise * 10), "graph" if graph else "eager")
  return name, dict(h=h, B=B, act=act, loss=loss, tied=tied, noise=noise, graph=graph, par=par, prec=prec)


CASES = dict([
  # whole single-process steps, split operands
  _case(36, 40, "tanh", "mse"),
  _case(36, 40, "tanh", "logistic", noise=0.0, graph=True),
  _case(36, 200, "tanh", "mse"),
  _case(36, 200, "tanh", "logistic", noise=0.0, graph=True),
  _case(64, 40, "tanh", "mse", noise=0.0, graph=True),
  _case(64, 40, "relu", "logistic"),
  _case(96, 40, "tanh", "mse"),
  _case(96, 40, "relu", "mse", noise=0.0, graph=True),
  _case(260, 40, "tanh", "mse", noise=0.0),
  _case(260, 40, "relu", "logistic", graph=True),
  _case(64, 1056, "tanh", "logistic"),
  _case(36, 1056, "relu", "mse", noise=0.0, graph=True),
  _case(260, 1056, "tanh", "mse"),
  _case(64, 40, "tanh", "logloss"),
  _case(260, 1056, "relu", "logloss", noise=0.0, graph=True),
  _case(64, 40, "tanh", "mse", tied=True),
  _case(36, 1056, "relu", "logistic", tied=True, noise=0.0, graph=True),
  _case(260, 40, "tanh", "logloss", tied=True),
  # RK_GEMM_PREC
  _case(36, 40, "tanh", "mse", prec="f32"),
  _case(64, 1056, "relu", "logistic", noise=0.0, graph=True, prec="f32"),
  _case(260, 40, "tanh", "logloss", prec="f32"),
  _case(64, 40, "tanh", "mse", tied=True, graph=True, prec="f32"),
  _case(36, 40, "tanh", "mse", prec="bf16"),
  _case(36, 200, "tanh", "mse", prec="bf16"),
  _case(64, 40, "tanh", "mse", noise=0.0, graph=True, prec="bf16"),
  _case(260, 1056, "relu", "logistic", prec="bf16"),
  _case(64, 40, "tanh", "logloss", prec="bf16"),
  # one rank, users sharded: the phased step
  _case(64, 40, "tanh", "mse", par="dp"),
  _case(36, 40, "tanh", "logistic", noise=0.0, graph=True, par="dp"),
  _case(96, 40, "tanh", "mse", par="dp"),
  _case(260, 1056, "relu", "mse", par="dp"),
  _case(64, 40, "tanh", "mse", tied=True, par="dp"),
  _case(64, 40, "tanh", "logloss", noise=0.0, par="dp"),
  _case(64, 40, "tanh", "mse", par="dp_zero"),
  _case(64, 40, "tanh", "mse", noise=0.0, graph=True, par="dp_zero"),
  _case(64, 40, "tanh", "mse", par="dp_local"),
  _case(36, 1056, "relu", "logistic", noise=0.0, par="dp_local"),
  # one rank, items sharded
  _case(64, 40, "tanh", "mse", par="ip"),
  _case(36, 40, "relu", "logistic", tied=True, noise=0.0, par="ip"),
  _case(260, 1056, "tanh", "mse", par="ip"),
  _case(64, 1504, "tanh", "mse", noise=0.0, par="ip"),
])

PAR_ENV = {"": {}, "dp": {"RK_FORCE_DP": "1", "RK_PARALLEL": "users"},
           "dp_zero": {"RK_FORCE_DP": "1", "RK_PARALLEL": "users", "RK_DP_ZERO": "force"},
           "dp_local": {"RK_FORCE_DP": "1", "RK_PARALLEL": "users", "RK_DP_ITEMSETS": "local"},
           "ip": {"RK_FORCE_DP": "1", "RK_PARALLEL": "items"}}
ENV_KEYS = ("RK_FORCE_DP", "RK_PARALLEL", "RK_DP_ZERO", "RK_DP_ITEMSETS", "RK_GRAPH")


def matrix():
  """implicit feedback, popularity ~ 1 / rank, 1 to 75 items per user"""
  import scipy.sparse as sp
  rng = np.random.RandomState(7)
  pop = 1.0 / np.arange(1, N_ITEMS + 1)
  pop /= pop.sum()
  deg = np.clip(rng.lognormal(np.log(20) - 0.5, 1.0, N_USERS).astype(int), 1, N_ITEMS // 4)
  rows = np.repeat(np.arange(N_USERS), deg)
  cols = rng.choice(N_ITEMS, size=int(deg.sum()), p=pop)
  m = sp.coo_matrix((np.ones(len(cols), np.float32), (rows, cols)), shape=(N_USERS, N_ITEMS)).tocsr()
  m.sum_duplicates()
  m.data[:] = 1.0
  m.sort_indices()
  return m


def run_case(c, csr):
  """(digest, route word of the last step or None where the engine does not publish one, bits 0-4 of
  rk_ae_step_uses_pg as the engine saw them or None)"""
  import torch
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder
  B = c["B"]
  for k in ENV_KEYS:
    os.environ.pop(k, None)
  os.environ.update(PAR_ENV[c["par"]])
  os.environ["RK_GRAPH"] = "1" if c["graph"] else "0"
  torch.manual_seed(5)
  model = DynamicAutoencoder([c["h"]], activation_type=c["act"], noise_prob=c["noise"], sparse=False,
                             is_constrained=c["tied"])
  rec = Recoder(model=model, use_cuda=True, optimizer_type="adam", loss=c["loss"])
  rec.user_order_hook = lambda epoch, n: np.arange(n, dtype=np.int64)
  rec.train(RecommendationDataset(csr[:3 * B]), batch_size=B, lr=1e-3, weight_decay=2e-5, num_epochs=1,
            negative_sampling=True, num_sampling_users=B if c["graph"] else 3 * B)
  eng = rec._engine()
  assert (getattr(rec, "_graph_stepper", None) is not None) == c["graph"], "graph replay"
  assert (getattr(rec, "_dp", None) is not None) == c["par"].startswith("dp"), "data parallel"
  assert (getattr(rec, "_ip", None) is not None) == (c["par"] == "ip"), "item parallel"
  assert bool(getattr(eng, "zero_adam", False)) == (c["par"] == "dp_zero")
  assert bool(getattr(getattr(rec, "_dp", None), "local_sets", False)) == (c["par"] == "dp_local")
  losses = np.ascontiguousarray(np.concatenate(rec.loss_history), dtype=np.float32)
  assert losses.shape == (3,) and np.all(np.isfinite(losses)), losses
  torch.cuda.synchronize()
  sha = hashlib.sha256()
  for k, p in sorted(model.named_parameters()):
    s = eng.states[k]
    for t in (p, s.m, s.v):
      sha.update(t.detach().cpu().numpy().tobytes())
  sha.update(losses.tobytes())
  flags = getattr(eng, "_step_flags", None)
  return sha.hexdigest(), getattr(eng, "_step_route", None), (None if flags is None else int(flags) & 31)


def digests(prec=""):
  """{case: {"sha256", "mode", "route"}} of the cases of one RK_GEMM_PREC value, which this process must have."""
  import torch
  import torch.distributed as dist
  assert os.environ.get("RK_GEMM_PREC", "") == prec, "RK_GEMM_PREC is read once per process"
  csr = matrix()
  saved = {k: os.environ.get(k) for k in ENV_KEYS}
  out = {}
  try:
    for group in (False, True):                   # the cases under the one-rank RCCL group last
      cases = {n: c for n, c in CASES.items() if c["prec"] == prec and bool(c["par"]) == group}
      if group and cases:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29731")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
      try:
        for name, c in cases.items():
          sha, route, mode = run_case(c, csr)
          out[name] = {"sha256": sha, "mode": mode, "route": route}
      finally:
        if group and cases:
          dist.destroy_process_group()
  finally:
    for k, v in saved.items():
      os.environ.pop(k, None)
      if v is not None:
        os.environ[k] = v
  return out


def child_digests(prec):
  """digests(prec) in a fresh process with RK_GEMM_PREC=prec"""
  env = dict(os.environ, RK_GEMM_PREC=prec)
  r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", prec], env=env, stdout=subprocess.PIPE,
                     check=True, timeout=600)
  return json.loads(r.stdout.decode().strip().splitlines()[-1])


# ---- rk_ae_step_uses_pg on synthetic step structs (host only: the call reads no device memory)
MODE_HS, MODE_BS = (36, 64, 96, 260), (40, 200, 1056)
MODE_OFFERS = ("planes", "do_scales", "ws", "ws_dw", "dw", "zt_planes", "gb_part", "cursor")
MODE_PHASES = (7, 1, 2, 4, 3, 8, 16, 32)                       # recorded in step_modes.json
ROUTE_PHASES = MODE_PHASES + (0, 5, 6, 24, 40, 48, 56)         # every mask tests/test_step_route.py compares


def mode_configs():
  """(key, fields): the grid of shapes and configurations x the sets of resources a caller may leave out"""
  offers = [set(MODE_OFFERS)] + [set(MODE_OFFERS) - {o} for o in MODE_OFFERS] + [{"ws"}, {"ws", "planes", "zt_planes"}]
  for h in MODE_HS:
    for B in MODE_BS:
      for act in ("tanh", "relu"):
        for loss in (0, 1, 2):
          for tied in (0, 1):
            # (a pruned cross product: every pair (loss, tied) at every shape, the offers rotating through them)
            for i, offer in enumerate(offers):
              if (i + h + B + loss + tied + (act == "relu")) % 3 and i:
                continue
              for row_off in ((0, B) if i == 0 else (0,)):
                yield ("h%d_B%d_%s_l%d_t%d_o%d_r%d" % (h, B, act, loss, tied, i, row_off),
                       dict(h=h, B=B, act=act, loss=loss, tied=tied, offer=offer, row_off=row_off))


def synthetic_step(f, phase):
  """an rk_ae_step_t with dummy non-null pointers for what `offer` holds; (step, the objects it points to)"""
  import ctypes
  from recoder_amd._lib import ACT, RkAeStep, RkBlock
  blk = RkBlock()
  blk.n_cap, blk.n_items, blk.S_cap = 320, N_ITEMS, 3 * f["B"]
  st = RkAeStep()
  st.blk = ctypes.pointer(blk)
  st.row_off, st.B, st.h, st.act, st.loss_kind, st.tied = f["row_off"], f["B"], f["h"], ACT[f["act"]], f["loss"], f["tied"]
  st.phase = phase
  dummy = ctypes.create_string_buffer(64)
  p = ctypes.addressof(dummy)
  for name in ("planes", "do_scales", "ws", "ws_dw", "zt_planes", "gb_part", "cursor"):
    setattr(st, name, p if name in f["offer"] else None)
  if "dw" in f["offer"]:
    st.dw_stream = st.dw_fork = st.dw_join = p
  return st, (blk, dummy)


def words():
  """{key: [rk_ae_step_uses_pg for the phases of ROUTE_PHASES]} for this process's RK_GEMM_PREC"""
  import ctypes
  from recoder_amd import _lib
  lib = _lib.load()
  out = {}
  for key, f in mode_configs():
    row = []
    for phase in ROUTE_PHASES:
      st, keep = synthetic_step(f, phase)
      row.append(int(lib.rk_ae_step_uses_pg(ctypes.byref(st))))
    out[key] = row
  return out


def modes(w):
  """what step_modes.json holds of words(): bits 0-4 for the phases of MODE_PHASES"""
  return {k: [x & 31 for x in row[:len(MODE_PHASES)]] for k, row in w.items()}


def child_words(prec):
  """words() in a fresh process with RK_GEMM_PREC=prec"""
  env = dict(os.environ, RK_GEMM_PREC=prec)
  r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-modes", prec], env=env,
                     stdout=subprocess.PIPE, check=True, timeout=600)
  return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
  sys.path.insert(0, ROOT)
  if sys.argv[1:2] == ["--child"]:
    print(json.dumps(digests(sys.argv[2])))
    return
  if sys.argv[1:2] == ["--child-modes"]:
    print(json.dumps(words()))
    return
  if sys.argv[1:2] == ["--modes"]:
    d = {prec or "split": modes(child_words(prec)) for prec in PRECS}
    with open(MODES_OUT, "w") as f:
      json.dump(d, f, indent=0, sort_keys=True)
      f.write("\n")
    print("wrote %d x %d configurations to %s" % (len(d), len(d["split"]), MODES_OUT))
    return
  runs = []
  for rep in range(2):
    d = {}
    for prec in PRECS:
      d.update(child_digests(prec))
      print("run %d: RK_GEMM_PREC=%s done, %d cases" % (rep, prec or "(unset)", len(d)), flush=True)
    runs.append(d)
  assert sorted(runs[0]) == sorted(CASES)
  bad = [n for n in CASES if runs[0][n]["sha256"] != runs[1][n]["sha256"]]
  assert not bad, "not repeatable: %s" % bad
  d = {n: {"sha256": v["sha256"], "mode": v["mode"]} for n, v in runs[0].items()}
  with open(OUT, "w") as f:
    json.dump(d, f, indent=0, sort_keys=True)
    f.write("\n")
  print("wrote %d digests to %s" % (len(d), OUT))


if __name__ == "__main__":
  main()
