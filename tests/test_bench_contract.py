"""bench.py's contract with the driver: ONE JSON line, last on stdout, with the agreed keys; also for
the multi-rank code path (two processes on one GPU over gloo -- marked INVALID, a code-path test).
The roofline, Recall@20 and the CPU baseline are --full's; a plain run prints the lean line and, with
--dump-outputs, the same outputs as a --full run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEYS = {"metric": str, "value": float, "unit": str, "n_gpus": int, "steps": int, "warmup": int,
        "ms_per_step": float, "higher_is_better": bool, "scaling": str, "dtype": str, "data": str,
        "config": dict}


def check_line(out, n_gpus, steps, warmup, full=True):
  lines = [l for l in out.strip().splitlines() if l.strip()]
  d = json.loads(lines[-1])                        # the LAST line of stdout
  for k, t in dict(KEYS, **({"roofline": dict} if full else {})).items():
    assert k in d and isinstance(d[k], t), (k, d.get(k))
  assert "vs_baseline" in d and d["vs_baseline"] is None
  assert d["metric"] == "train_users_per_sec" and d["unit"] == "users/s"
  assert (d["n_gpus"], d["steps"], d["warmup"]) == (n_gpus, steps, warmup)
  assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic"
  assert "workload" in d["config"] and "model" not in d["config"]
  assert abs(d["value"] - d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
  if not full:
    return d
  r = d["roofline"]
  for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernels", "step"):
    assert k in r, k
  assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
  # (the lazy dense Adam delivers SURVEY 8(d)'s dense-sweep bytes while moving fewer: its own bytes are priced in
  # roofline.lazy_sweep, whose fraction is the one bounded by 1)
  assert 0.0 < r["frac"] and len(r["kernels"]) >= 5
  own = r.get("lazy_sweep")
  assert (own is None and r["frac"] < 1.0) or (0.0 < own["frac"] < 1.0 and own["own_bytes"] < r["achieved"] * 1e9 * r["avg_launch_ms"] * 1e-3 * 1.001)
  return d


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
  """(stdout, dump directory) of one --full run on one GPU."""
  dump = str(tmp_path_factory.mktemp("full_outputs"))
  r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "4", "--cpu-seconds", "2",
                      "--full", "--dump-outputs", dump], cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  return r.stdout, dump


def test_single_gpu_line(full_run):
  d = check_line(full_run[0], 1, 8, 4)
  c = d["cpu_baseline"]
  assert c["kind"] == "port" and c["cores"] >= 1 and c["host_cores"] >= c["cores"] and c["value"] > 0
  assert d["config"]["api"] == "Recoder.train" and d["config"]["graph_replay"] is True
  # Recall@20 of the trained state next to the throughput it qualifies: product == oracle to 4 decimals
  assert d["recall_match_4dp"] is True and 0.0 <= d["recall_at_20"] <= 1.0, d.get("recall")
  assert abs(d["recall"]["value"] - d["recall"]["oracle"]) < 5e-5
  assert d["roofline"]["traffic"] is None or "NOT collected in this run" in d["roofline"]["traffic_source"]


def test_plain_line_and_dumped_outputs(full_run, tmp_path):
  """Without --full: the lean line, nothing of the roofline / Recall / CPU baseline.  --dump-outputs: the
  parameters after the last timed step and the timed steps' losses, float32, at most 64 MB, bit for bit
  what the --full run of the same arguments wrote (seeded inputs, deterministic steps)."""
  dump = str(tmp_path / "outputs")
  r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "4", "--dump-outputs", dump],
                     cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  d = check_line(r.stdout, 1, 8, 4, full=False)
  assert not {"roofline", "recall", "recall_at_20", "cpu_baseline"} & set(d), sorted(d)
  assert d["config"]["graph_replay"] is True
  files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(dump, "*.npy")))
  want = sorted(os.path.basename(f) for f in glob.glob(os.path.join(full_run[1], "*.npy")))
  assert files == want and "losses.npy" in files and "en_embedding_layer.weight.npy" in files, (files, want)
  assert sum(os.path.getsize(os.path.join(dump, f)) for f in files) <= 64 << 20
  for f in files:
    a, b = np.load(os.path.join(dump, f)), np.load(os.path.join(full_run[1], f))
    assert a.dtype == np.float32 and np.all(np.isfinite(a)), f
    np.testing.assert_array_equal(a, b, err_msg=f)
  losses = np.load(os.path.join(dump, "losses.npy"))
  assert losses.shape == (8,) and float(losses[-1]) == d["config"]["last_loss"]


@pytest.mark.parametrize("abandon_alt", [False, True])
def test_two_rank_code_path_on_one_gpu(abandon_alt):
  """abandon_alt: the extra item-parallel run behind the graded one is cut off by its watchdog
  (as if it hung): the graded line must still come out, last on stdout, and every rank exit 0."""
  env = dict(os.environ, MASTER_ADDR="127.0.0.1")
  cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", "29598" if abandon_alt else "29597", "bench.py",
         "--gpus", "2", "--steps", "6", "--warmup", "3", "--one-gpu-gloo", "--full"]
  if abandon_alt:
    cmd += ["--alt-timeout", "0.05"]
  r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
  assert r.returncode == 0, r.stderr[-3000:]
  d = check_line(r.stdout, 2, 6, 3)
  assert d["config"]["global_batch"] == 2 * d["config"]["batch_size_per_gpu"]
  assert "INVALID" in d and d["config"]["parallelism"].startswith("dp2")
  alt = d["config"]["alt_item_parallel"]
  if abandon_alt:
    assert alt and "abandoned" in alt["error"]
  else:
    assert alt and "error" not in alt and alt["value"] > 0 and alt["parallelism"].startswith("ip2")
