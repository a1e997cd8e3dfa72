"""CPU: the host side of fsSLIM (``candidates=M`` of recoder_amd/slim.py and ``Recoder.train_slim``) -- the memory
arithmetic without the n x n Gram, the restated size queries, the refusals -- and the comparator of
tests/fsslim_util.py against ``slim_util.cd_f32`` where the candidates restrict nothing."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import fsslim_util, slim_util
from tests.test_closed_form_host import _no_gpu, _untouched


def test_a_million_items_pass_with_candidates_and_not_without():
  from recoder_amd import slim
  from recoder_amd.device import DEVICE_HBM_BYTES
  args = (100_000, 1_000_000, 200, 10_000_000)
  with pytest.raises(ValueError, match="n x n fp32 Gram"):
    slim.check_memory(*args, free_bytes=DEVICE_HBM_BYTES)
  need = slim.check_memory(*args, free_bytes=DEVICE_HBM_BYTES, candidates=100)
  assert need == slim.required_bytes(*args, candidates=100) < 10 ** 6 * 10 ** 6 * 4
  assert need >= 10 ** 6 * (200 + 100) * 8                  # (the model and the candidate lists are counted)
  with pytest.raises(ValueError, match=r"1000000 items with 200 neighbours, 100 candidates.*1000 are free"):
    slim.check_memory(*args, free_bytes=1000, candidates=100)


def test_size_restatements_are_monotone_and_refuse_a_bad_m():
  from recoder_amd import slim
  ws = [slim.sparse_workspace_bytes(M) for M in range(1, slim.MAX_CANDIDATES + 1)]
  need = [slim.required_bytes(1000, 5000, 50, 20000, candidates=M) for M in range(1, slim.MAX_CANDIDATES + 1)]
  assert all(b >= a for a, b in zip(ws, ws[1:])) and all(b > a for a, b in zip(need, need[1:]))
  lds = slim.SPARSE_LDS_CANDIDATES
  assert ws[0] == ws[lds - 1] == 256 and ws[lds] == 256 + 768 * (128 * 128 + 7 * 128) * 4
  assert ws[-1] == 256 + 768 * (1024 * 1024 + 7 * 1024) * 4
  for bad in (0, -1, slim.MAX_CANDIDATES + 1, 1.5, True, None, "8"):
    with pytest.raises(ValueError, match="candidates"):
      slim.sparse_workspace_bytes(bad)
  for bad in (0, slim.MAX_CANDIDATES + 1, 1.5, True):
    with pytest.raises(ValueError, match="candidates"):
      slim.check_memory(10, 10, 5, 10, free_bytes=float("inf"), candidates=bad)


@pytest.mark.parametrize("bad", [0, 1025, 1.5, True])
def test_train_slim_refuses_bad_candidates_and_changes_nothing(monkeypatch, bad):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import SparseLinearModel
  _no_gpu(monkeypatch)
  X = sp.random(20, 15, density=0.3, format="csr", dtype=np.float32, random_state=np.random.RandomState(4))
  X.data[:] = 1.0
  rec = Recoder(model=SparseLinearModel())
  before = rec.model.model_params()
  with pytest.raises(ValueError, match="candidates"):
    rec.train_slim(RecommendationDataset(X), l1_reg=2.0, candidates=bad)
  _untouched(rec, before)
  assert rec.model.candidates is None
  for kw, match in ((dict(candidate_similarity="pearson"), "candidate_similarity"),
                    (dict(candidate_shrink=-1.0), "candidate_shrink")):
    with pytest.raises(ValueError, match=match):
      rec.train_slim(RecommendationDataset(X), l1_reg=2.0, candidates=5, **kw)
    _untouched(rec, before)


def test_candidates_travel_in_model_params_only_when_set():
  from recoder_amd.nn import SparseLinearModel
  m = SparseLinearModel()
  assert m.candidates is None and sorted(m.model_params()) == ["l1_reg", "l2_reg", "neighbours"]
  m.candidates, m.candidate_shrink = 64, 300.0
  p = m.model_params()
  assert (p["candidates"], p["candidate_similarity"], p["candidate_shrink"]) == (64, "cosine", 300.0)
  m2 = SparseLinearModel()
  m2.load_model_params(p)
  assert m2.model_params() == p
  m2.load_model_params({"l1_reg": 1.0, "l2_reg": 2.0, "neighbours": 3})
  assert m2.candidates is None and m2.model_params() == {"l1_reg": 1.0, "l2_reg": 2.0, "neighbours": 3}


def test_full_candidates_are_the_unrestricted_restatement():
  """M >= n - 1 on a binary 120 x 37 matrix: every item that shares a user with j is a candidate of j, the others
  have G[j, k] = 0 <= l1, and the masked restatement is ``slim_util.cd_f32`` on the full Gram bit for bit."""
  rng = np.random.RandomState(11)
  X = sp.csr_matrix((rng.rand(120, 37) < 0.15).astype(np.float32))
  G = slim_util.gram_f64(X)
  inv = slim_util.inv_denom_f64(G, 5.0).astype(np.float32)
  want = slim_util.cd_f32(G.astype(np.float32), inv, 1.0, 6, 50, 1e-5)
  assert want[2].max() == 6 and want[4].max() > 6, "the cut must bind"
  for M in (36, 50):
    cand, cnt = fsslim_util.select(X, M)
    assert cand.shape == (37, M) and cnt.max() <= 36
    got = fsslim_util.cd_f32(G.astype(np.float32), inv, cand, cnt, 1.0, 6, 50, 1e-5)
    for g, t in zip(got, want):
      assert g.dtype == t.dtype and np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                                                   t.view(np.uint32) if t.dtype == np.float32 else t)
  cand, cnt = fsslim_util.all_candidates(37)
  got = fsslim_util.cd_f32(G.astype(np.float32), inv, cand, cnt, 1.0, 6, 50, 1e-5)
  assert all(np.array_equal(g, t) for g, t in zip(got, want))
  # (a restriction that binds gives another model: the comparison above is not vacuous)
  cand, cnt = fsslim_util.select(X, 4)
  assert not np.array_equal(fsslim_util.cd_f32(G.astype(np.float32), inv, cand, cnt, 1.0, 6, 50, 1e-5)[1], want[1])


def test_the_drivers_diagonal_is_the_ascending_chain_on_values_that_round():
  """``slim.diagonal`` on values in (0, 2), where every step of the chain rounds: bit for bit the per-item chain
  acc = fmaf(a, a, acc) over the item's users in ascending order, made with ``ease_util.fmaf`` (itself held to exact
  rational arithmetic in tests/test_ease_host.py); summed in descending order the bits differ, so the order is pinned."""
  import types

  import torch

  from recoder_amd import slim
  from tests import ease_util
  rng = np.random.RandomState(3)
  m = (rng.rand(400, 23) < 0.3).astype(np.float32) * rng.uniform(0.05, 1.95, (400, 23)).astype(np.float32)
  m[:, 4] = 0.0
  Xt = sp.csr_matrix(m).T.tocsr()
  Xt.sort_indices()
  icsr = types.SimpleNamespace(indptr=torch.from_numpy(Xt.indptr.astype(np.int64)), data=torch.from_numpy(Xt.data))
  want, back = np.zeros(23, np.float32), np.zeros(23, np.float32)
  for k in range(23):
    vals = Xt.data[Xt.indptr[k]:Xt.indptr[k + 1]]
    for a in vals:
      want[k] = ease_util.fmaf(a, a, want[k]).ravel()[0]
    for a in vals[::-1]:
      back[k] = ease_util.fmaf(a, a, back[k]).ravel()[0]
  got = slim.diagonal(icsr)
  assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)) and got[4] == 0
  assert (want != back).any(), "the data must tell the two orders apart"
  icsr.data = None
  assert np.array_equal(slim.diagonal(icsr), np.diff(Xt.indptr).astype(np.float32))


def test_the_drivers_fmaf_is_the_comparators():
  """``slim._fmaf32`` against ``ease_util.fmaf`` on random operands and on sums that sit on an f32 rounding midpoint
  in float64 without being exact (where a plain float64 sum rounded to f32 is off by one ulp)."""
  from recoder_amd import slim
  from tests import ease_util
  rng = np.random.RandomState(0)
  a, b, c = (rng.uniform(-2, 2, 200000).astype(np.float32) for _ in range(3))
  assert np.array_equal(slim._fmaf32(a, b, c).view(np.uint32), ease_util.fmaf(a, b, c).view(np.uint32))
  # a * b = (1 + 2^-23)(2^-24 - 2^-47) = 2^-24 - 2^-70 and c = 1 + 2^-23 (an odd last bit): the float64 sum rounds to the
  # midpoint 1 + 2^-23 + 2^-24, which rounds to even, up; the true sum lies just below it and rounds down
  a = np.array([1.0 + 2.0 ** -23], np.float32)
  b = np.array([2.0 ** -24 - 2.0 ** -47], np.float32)
  c = np.array([1.0 + 2.0 ** -23], np.float32)
  twice = (a.astype(np.float64) * b + c).astype(np.float32)
  got = slim._fmaf32(a, b, c)
  assert got[0] == c[0] and twice[0] == np.float32(1.0 + 2.0 ** -22), "the case must sit on the midpoint"
  assert np.array_equal(got, ease_util.fmaf(a, b, c))
