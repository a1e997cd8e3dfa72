"""CPU: what UserKNN (recoder_amd/userknn.py, UserNeighbourhoodModel) decides without a device -- the
parameter and memory checks, the workspace arithmetic against the library's query, the declared and
bound symbols -- and the f32 restatement of tests/userknn_util.py against brute-force float64 on the ML-20M
slice.

The float64 bounds.  Both restatements are given the SAME f32 norms (exact in float64), as the kernel is.
A similarity is then three f32 roundings away from float64 (product, sum, quotient): within 3 * 2^-24
relative to first order.  A score is an fmaf chain over m kept neighbours of positive terms (the slice is
binary): m further roundings of partial sums that never exceed the total, so
|s32 - s64| <= (m + 3) 2^-24 * s64 to first order, asserted as (m + 4) 2^-24."""
import os

import numpy as np
import pytest

from tests import userknn_util as uu
from tests.abi_util import built, declared  # noqa: F401  (built: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RP3_HEADER = os.path.join(ROOT, "include", "recoder_rp3.h")
NEW = ("rk_rp3_user_workspace_bytes", "rk_rp3_user_neighbours", "rk_rp3_user_scores")


def test_parameter_checks():
  from recoder_amd import userknn
  from recoder_amd.nn import RandomWalkItemModel, UserNeighbourhoodModel
  assert userknn.check_params(100, 0) == (100, 0.0)
  assert userknn.check_params(np.int64(7), np.float32(2.5)) == (7, 2.5)
  assert userknn.check_params(userknn.MAX_NEIGHBOURS, 1e9)[0] == userknn.MAX_NEIGHBOURS
  for bad in (0, -1, userknn.MAX_NEIGHBOURS + 1, 2.0, True, None, "3"):
    with pytest.raises(ValueError, match=r"neighbours must be an integer in \[1, %d\]" % userknn.MAX_NEIGHBOURS):
      userknn.check_params(bad, 0.0)
  for bad in (-0.5, float("inf"), float("nan"), True, None, "1"):
    with pytest.raises(ValueError, match="shrink must be finite and >= 0"):
      userknn.check_params(10, bad)
  m = UserNeighbourhoodModel()
  assert m.model_params() == {"neighbours": m.neighbours, "shrink": m.shrink, "num_users": None, "nnz": 0}
  assert userknn.check_config(m, 5, 1) == (5, 1.0)
  with pytest.raises(ValueError, match="train_userknn fits a UserNeighbourhoodModel, not RandomWalkItemModel"):
    userknn.check_config(RandomWalkItemModel(), 5, 1)
  with pytest.raises(ValueError, match="neighbours"):
    UserNeighbourhoodModel(neighbours=0)
  with pytest.raises(ValueError, match="shrink"):
    UserNeighbourhoodModel(shrink=-1.0)


def test_memory_check_names_the_sizes():
  from recoder_amd import userknn
  from recoder_amd.device import DEVICE_HBM_BYTES
  need = userknn.required_bytes(100000, 1000000, 100, 5 * 10 ** 6)
  assert need == (100001 + 1000001) * 8 + 3 * 5 * 10 ** 6 * 4 + 100000 * 4 + userknn.SERVING_ROWS * 808 + \
      userknn.workspace_bytes(100000)
  assert userknn.check_memory(100000, 1000000, 100, 5 * 10 ** 6, free_bytes=float("inf")) == need
  with pytest.raises(ValueError, match=r"100000 users x 1000000 items with 100 neighbours and 5000000 entries needs "
                                       r"%d bytes of device memory, 1000 are free" % need):
    userknn.check_memory(100000, 1000000, 100, 5 * 10 ** 6, free_bytes=1000)
  big = DEVICE_HBM_BYTES // 12 + 1
  with pytest.raises(ValueError, match=r"UserKNN over 1000 users x 1000 items with 10 neighbours and %d entries needs "
                                       r"\d+ bytes: more than one device's memory" % big):
    userknn.check_memory(1000, 1000, 10, big, free_bytes=float("inf"))
  with pytest.raises(ValueError, match="at least one user and one item"):
    userknn.check_memory(0, 10, 10, 0, free_bytes=float("inf"))


def test_workspace_bytes_is_the_librarys_query(built):
  from recoder_amd import _rp3_lib, userknn
  lib = _rp3_lib.load()
  cap = lib.rk_rp3_lds_items()
  assert cap == userknn.LDS_USERS
  for U in (1, 37, cap, cap + 1, 10 ** 6):
    assert lib.rk_rp3_user_workspace_bytes(U) == userknn.workspace_bytes(U) > 0
  assert lib.rk_rp3_user_workspace_bytes(cap) < lib.rk_rp3_user_workspace_bytes(cap + 1)
  assert lib.rk_rp3_user_workspace_bytes(0) < 0 and userknn.workspace_bytes(0) < 0
  assert b"n_users" in lib.rk_rp3_last_error()


def test_new_symbols_are_declared_and_bound(built):
  from recoder_amd import _rp3_lib
  import recoder_amd
  names = declared([RP3_HEADER])
  for name in NEW:
    assert name in names and name in _rp3_lib.SIGNATURES
    assert hasattr(_rp3_lib.load(), name)
  assert "user-neighbourhood" in built.__doc__
  assert recoder_amd.UserNeighbourhoodModel is __import__("recoder_amd.nn").nn.UserNeighbourhoodModel
  assert "UserNeighbourhoodModel" in recoder_amd.__all__


def test_train_refuses_the_model():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import UserNeighbourhoodModel
  rec = Recoder(model=UserNeighbourhoodModel())
  with pytest.raises(ValueError, match="train_userknn"):
    rec.train(RecommendationDataset(uu.random_matrix(20, 15, 0.3, seed=1)))


def test_torch_forward_on_the_host_is_the_model():
  import torch
  from recoder_amd.nn import UserNeighbourhoodModel
  X = uu.random_matrix(40, 31, 0.2, seed=5, values=True)
  Q = uu.random_matrix(9, 31, 0.25, seed=6)
  N, shrink = 6, 2.0
  m = UserNeighbourhoodModel(N, shrink)
  m.nnz = X.nnz
  m.init_model(num_items=31, num_users=40)
  Xt = X.T.tocsr()
  Xt.sort_indices()
  m.user_indptr.copy_(torch.from_numpy(X.indptr.astype(np.int64)))
  m.user_indices.copy_(torch.from_numpy(X.indices.astype(np.int32)))
  m.item_indptr.copy_(torch.from_numpy(Xt.indptr.astype(np.int64)))
  m.item_indices.copy_(torch.from_numpy(Xt.indices.astype(np.int32)))
  m.interaction_values.data.copy_(torch.from_numpy(X.data))
  m.user_norms.copy_(torch.from_numpy(uu.norms_f32(X)))
  assert sorted(m.state_dict()) == ["interaction_values", "item_indices", "item_indptr", "user_indices",
                                    "user_indptr", "user_norms"]
  got = m(torch.from_numpy(Q.toarray())).numpy()
  kept, S = uu.neighbours_f64(X, Q, N, shrink)
  want = uu.scores_f64(X, kept, S)
  # (no cut falls on a near-tie here: the f32 and float64 neighbour sets agree)
  ids32, _, cnt32 = uu.neighbours_f32(X, Q, N, shrink)
  assert all(np.array_equal(ids32[q, :cnt32[q]], kept[q]) for q in range(Q.shape[0]))
  assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
  cols = torch.tensor([3, 0, 17])
  assert np.array_equal(m(torch.from_numpy(Q.toarray()), target_items=cols).numpy(), got[:, [3, 0, 17]])


@pytest.fixture(scope="module")
def slice_case():
  """500 query rows of the slice (every 20th training user) against the whole slice, at the defaults."""
  from recoder_amd.nn import UserNeighbourhoodModel
  X, _ = uu.load_slice()
  m = UserNeighbourhoodModel()
  N, shrink = m.neighbours, m.shrink
  rows = np.arange(0, X.shape[0], 20)
  Q = X[rows]
  un, qn = uu.norms_f32(X), uu.norms_f32(Q)
  ids, sim, count = uu.neighbours_f32(X, Q, N, shrink, un=un, qn=qn)
  kept, S = uu.neighbours_f64(X, Q, N, np.float64(np.float32(shrink)), un=un, qn=qn)
  return X, Q, N, (ids, sim, count), kept, S


def test_f32_neighbours_against_float64_on_the_slice(slice_case):
  X, Q, N, (ids, sim, count), kept, S = slice_case
  differ = near = 0
  worst = 0.0
  for q in range(Q.shape[0]):
    got = ids[q, :count[q]]
    assert len(got) == len(kept[q]) == min(N, int((S[q] > 0).sum()))
    rel = np.abs(sim[q, :count[q]].astype(np.float64) - S[q, got]) / S[q, got]
    worst = max(worst, float(rel.max()) if len(rel) else 0.0)
    if not np.array_equal(got, kept[q]):
      # the sets may differ only where the float64 similarities at the cut are within one f32 ulp
      differ += 1
      cut = S[q, kept[q]].min()
      odd = np.setxor1d(got, kept[q])
      assert np.all(np.abs(S[q, odd] - cut) <= cut * 2.0 ** -23), (q, S[q, odd], cut)
    nxt = np.sort(S[q])[::-1][N] if (S[q] > 0).sum() > N else 0.0
    near += bool(len(kept[q]) == N and abs(S[q, kept[q]].min() - nxt) <= nxt * 2.0 ** -23)
  print("slice: %d of %d rows differ from float64 (%d rows have a cut within one f32 ulp); "
        "max rel err of a similarity %.3g = %.2f * 2^-24" % (differ, Q.shape[0], near, worst, worst * 2 ** 24))
  assert worst <= 3.5 * 2.0 ** -24


def test_f32_scores_against_float64_on_the_slice(slice_case):
  X, Q, N, (ids, sim, count), kept, S = slice_case
  assert np.all(X.data == 1.0)
  s32 = uu.scores_f32(X, ids, sim, count)
  # float64 scores of the f32 restatement's OWN neighbour sets (they differ from float64's only at near-ties)
  s64 = uu.scores_f64(X, [ids[q, :count[q]] for q in range(Q.shape[0])], S)
  B = X.astype(np.float64)
  m = np.zeros(s64.shape)
  for q in range(Q.shape[0]):
    m[q] = np.asarray(B[ids[q, :count[q]]].sum(0)).ravel()          # how many kept neighbours reach the item
  assert np.array_equal(s32 == 0, s64 == 0)
  live = s64 > 0
  ratio = np.abs(s32.astype(np.float64) - s64)[live] / ((m[live] + 4) * 2.0 ** -24 * s64[live])
  print("slice scores: max |s32 - s64| / ((m + 4) 2^-24 s64) = %.3f, max m %d" % (ratio.max(), m.max()))
  assert ratio.max() <= 1.0
  for lo, hi in ((0, 1), (100, 1357), (X.shape[1] - 1, X.shape[1])):
    part = uu.scores_f32(X, ids, sim, count, lo, hi)
    assert np.array_equal(part.view(np.uint32), s32[:, lo:hi].view(np.uint32))
