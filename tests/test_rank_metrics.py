"""GPU: rk_als_rank_metrics against its numpy restatement (tests/rank_metrics_util.py, itself held to the per-user
functions of recoder_amd.metrics by tests/test_rank_metrics_host.py).

Recall is one integer division and must be equal bit for bit.  NDCG and AveragePrecision are float64 sums the kernel
and the restatement add in the same ascending rank order: the bound asserted is still the derived one for two
different orders, 2 K 2^-53 max(a, b).  ``sums`` is added in the same fixed order on both sides (256 strided partials,
a halving tree) from values inside that bound: K 2^-53-relative differences of the terms carry through, so the same
bound times B; ``count`` is an integer."""
import functools

import numpy as np
import pytest
import torch

from recoder_amd import metrics as M

from . import rank_metrics_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(K, B):
  recs, tm = U.make_case(K, B, seed=1000 * B + K)
  return recs, tm, tuple((tuple(g), U.rank_metrics(recs, tm, g)) for g in U.metric_set(K))


def _device_recs(recs, strided):
  B, K = recs.shape
  if not strided:
    return torch.as_tensor(recs, device=DEV).contiguous(), K
  buf = torch.full((B, 3 * K), -7, dtype=torch.int64, device=DEV)      # (what lies between the rows is never read)
  buf[:, :K] = torch.as_tensor(recs, device=DEV)
  return buf[:, :K], 3 * K


@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("K", U.K_CASES)
def test_kernel_against_the_restatement(K, B):
  recs, tm, groups = _case(K, B)
  target = M.DeviceTarget(tm, DEV)
  for strided in (False, True):
    dev, ld = _device_recs(recs, strided)
    for group, (want, want_sums, want_count) in groups:
      values, (sums, count) = M.device_batch_metrics(dev, ld, target, list(group))
      again, (sums2, count2) = M.device_batch_metrics(dev, ld, target, list(group))
      got, got_sums, got_count = values.cpu().numpy(), sums.cpu().numpy(), int(count.cpu())
      assert got.tobytes() == again.cpu().numpy().tobytes()                       # the same bits twice
      assert got_sums.tobytes() == sums2.cpu().numpy().tobytes() and got_count == int(count2.cpu())
      assert np.array_equal(np.isnan(got), np.isnan(want))
      assert got_count == want_count
      ok = ~np.isnan(want[:, 0])
      for j, m in enumerate(group):
        a, b = got[ok, j], want[ok, j]
        if isinstance(m, M.Recall):
          assert np.array_equal(a, b), (str(m), strided)
        else:
          assert (np.abs(a - b) <= 2.0 * K * 2.0 ** -53 * np.maximum(a, b)).all(), (str(m), strided)
        assert abs(got_sums[j] - want_sums[j]) <= B * U.bound(K, got_sums[j], want_sums[j]), (str(m), strided)


def test_a_target_longer_than_the_batch_and_an_empty_one():
  import scipy.sparse as sp
  recs, tm, _ = _case(20, 3)
  metrics = [M.Recall(20), M.NDCG(20)]
  tall = sp.vstack([tm, tm]).tocsr()                     # more target rows than lists: the first B are read
  a, _ = M.device_batch_metrics(torch.as_tensor(recs, device=DEV), 20, M.DeviceTarget(tall, DEV), metrics)
  b, _ = M.device_batch_metrics(torch.as_tensor(recs, device=DEV), 20, M.DeviceTarget(tm, DEV), metrics)
  assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
  empty = sp.csr_matrix(tm.shape, dtype=np.float32)
  v, (s, c) = M.device_batch_metrics(torch.as_tensor(recs, device=DEV), 20, M.DeviceTarget(empty, DEV), metrics)
  assert np.isnan(v.cpu().numpy()).all() and not s.cpu().numpy().any() and int(c.cpu()) == 0
  with pytest.raises(ValueError, match="target holds"):
    M.device_batch_metrics(torch.as_tensor(recs, device=DEV), 20, M.DeviceTarget(tm[:2], DEV), metrics)
