"""rk_als_rank_metrics without a GPU: the export and its binding, and the kernel's arithmetic as restated in
tests/rank_metrics_util.py against the per-user functions of recoder_amd.metrics (the reference's, pinned by the
known-answer tests of tests/test_host_logic.py).

Recall is one integer division: equal bit for bit.  NDCG and AveragePrecision are sums of at most K non-negative
terms, each at most 1, added in another order than numpy's pairwise sum: |a - b| <= 2 K 2^-53 max(a, b), derived from
the (K - 1) 2^-53 relative error of either order, not measured."""
import os

import numpy as np
import pytest

from recoder_amd import metrics as M

from . import rank_metrics_util as U
from .abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)


def test_library_exports_and_binds_rank_metrics(built):
  from recoder_amd import _als_lib
  assert "rk_als_rank_metrics" in exports(built.ALS_LIB)
  assert "rk_als_rank_metrics" in declared([os.path.join(INC, "recoder_als.h")])
  assert "rk_als_rank_metrics" in _als_lib.SIGNATURES
  lib = _als_lib.load()
  assert lib.rk_als_rank_metrics.restype is _als_lib.SIGNATURES["rk_als_rank_metrics"][0]
  assert _als_lib.RANK_METRICS_MAX == M.MAX_DEVICE_METRICS == 8


def test_entry_point_refuses_bad_arguments(built):
  """K < 1, more than 8 metrics, k < 1 and null pointers return the library's error code before any launch; the
  binding's ``check`` raises on it."""
  from ctypes import c_int32
  from recoder_amd import _als_lib
  from recoder_amd._lib import RecoderHipError
  lib = _als_lib.load()
  one, zero, nine = (c_int32 * 1)(1), (c_int32 * 1)(0), (c_int32 * 9)(*[1] * 9)
  p = 4096                                               # (never dereferenced: every case is refused first)
  good = [p, 4, 10, 10, p, p, 1, 1, zero, one, one, p, p, p, p, p, None]

  def call(**change):
    a = list(good)
    for i, v in change.items():
      a[int(i[1:])] = v
    return lib.rk_als_rank_metrics(*a)
  assert call(_2=0) == -2                                # K < 1
  assert call(_3=9) == -2                                # ld < K
  assert call(_7=9, _8=nine, _9=nine, _10=nine) == -2    # more than 8 metrics
  assert call(_7=0) == -2
  assert call(_9=zero) == -2                             # k < 1
  assert call(_8=(c_int32 * 1)(3)) == -2                 # no such kind
  for i in (0, 4, 8, 9, 10, 11, 12, 13, 14, 15):
    assert call(**{"_%d" % i: None}) == -2, i            # null pointers
  assert call(_5=None) == -2                             # (indices may be NULL only with tgt_nnz == 0)
  with pytest.raises(RecoderHipError, match="rk_als_rank_metrics"):
    _als_lib.check(call(_2=0), "rk_als_rank_metrics")


def _per_user(metric, x, y):
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.float64(metric.evaluate(x, y))


@pytest.mark.parametrize("K", U.K_CASES)
def test_restatement_against_the_per_user_functions(K):
  recs, tm = U.make_case(K, 2 * len(U.ROW_KINDS), seed=K)
  dense_rows = [tm.indices[tm.indptr[u]:tm.indptr[u + 1]][tm.data[tm.indptr[u]:tm.indptr[u + 1]] != 0]
                for u in range(recs.shape[0])]
  lengths = {len(y) for y in dense_rows}
  assert {0, 1, 3, 2000} <= lengths
  for group in U.metric_set(K):
    values, _, _ = U.rank_metrics(recs, tm, group)
    for u, y in enumerate(dense_rows):
      for j, m in enumerate(group):
        want, got = _per_user(m, recs[u], y), values[u, j]
        if len(y) == 0:
          assert np.isnan(want) and np.isnan(got), (u, str(m))
        elif isinstance(m, M.Recall):
          assert got == want, (u, str(m), got, want)
        else:
          assert abs(got - want) <= U.bound(K, got, want), (u, str(m), got, want)
  # every recommendation a hit / none: the values are known
  values, _, _ = U.rank_metrics(recs, tm, [M.Recall(K, normalize=True), M.NDCG(K), M.AveragePrecision(K)])
  assert np.array_equal(values[U.ROW_KINDS.index("all")], [1.0, 1.0, 1.0])
  assert np.array_equal(values[U.ROW_KINDS.index("none")], [0.0, 0.0, 0.0])


@pytest.mark.parametrize("K", U.K_CASES)
def test_restatement_sums_against_batch_metrics(K):
  B = 300
  recs, tm = U.make_case(K, B, seed=100 + K)
  for group in U.metric_set(K):
    values, sums, count = U.rank_metrics(recs, tm, group)
    host = M.batch_metrics(recs, tm, group)
    ny = np.diff(tm.indptr) - np.bincount(np.repeat(np.arange(B), np.diff(tm.indptr))[tm.data == 0], minlength=B)
    assert count == int((ny > 0).sum())
    for j, m in enumerate(group):
      col = np.asarray(host[m], dtype=np.float64)
      assert np.array_equal(np.isnan(col), np.isnan(values[:, j]))
      assert np.array_equal(np.isnan(col), ny == 0)
      want = np.nansum(col)
      assert abs(sums[j] - want) <= B * U.bound(K, sums[j], want), (str(m), sums[j], want)


def test_k_above_the_list_reads_the_list():
  recs, tm = U.make_case(20, 16, seed=7)
  a, _, _ = U.rank_metrics(recs, tm, [M.NDCG(25), M.AveragePrecision(25, normalize=False)])
  b = M.batch_metrics(recs, tm, [M.NDCG(25), M.AveragePrecision(25, normalize=False)])
  for j, col in enumerate(b.values()):
    col = np.asarray(col)
    ok = ~np.isnan(col)
    assert (np.abs(a[ok, j] - col[ok]) <= 2 * 20 * 2.0 ** -53 * np.maximum(a[ok, j], col[ok])).all()


def test_device_metrics_ok():
  assert M.device_metrics_ok([M.Recall(20), M.NDCG(1), M.AveragePrecision(5, normalize=False)])
  assert not M.device_metrics_ok([])
  assert not M.device_metrics_ok([M.Recall(1)] * 9)
  assert not M.device_metrics_ok([M.Recall(0)])
  assert not M.device_metrics_ok([M.Recall(2.5)])

  class Mine(M.Recall):
    pass
  assert not M.device_metrics_ok([Mine(3)])
