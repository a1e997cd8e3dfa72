"""GPU: UserKNN (recoder_amd/userknn.py, the rk_rp3_user_* kernels of librecoder_rp3.so,
UserNeighbourhoodModel) against the f32 restatement of tests/userknn_util.py.  Every kernel comparison is
bit for bit: the neighbour lists (ids, similarities, counts; both accumulator paths; ties; short and empty
lists), the scores (strips, leading dimensions, values, batch positions), and the public path through
``Recoder.train_userknn`` (recommend, evaluate, checkpoints, predict, strips)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import userknn_util as uu

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev_csr(m):
  from recoder_amd.als import AlsCSR
  return AlsCSR(sp.csr_matrix(m), DEV)


def _gpu(X, Q, N, shrink, lo=0, hi=None, fill=(7, 3.0, 9), want_scores=True, ld=None):
  """((ids, sim, count), scores) as numpy from the two kernels."""
  from recoder_amd import als, userknn
  uc, ic = als.csr_pair(X, X.shape[0], X.shape[1], DEV)
  qc = _dev_csr(Q)
  nq = Q.shape[0]
  out = (torch.full((nq, N), fill[0], dtype=torch.int32, device=DEV),
         torch.full((nq, N), fill[1], dtype=torch.float32, device=DEV),
         torch.full((nq,), fill[2], dtype=torch.int32, device=DEV))
  un = torch.from_numpy(uu.norms_f32(X)).to(DEV)
  *nbr, _ = userknn.neighbours(qc, ic, un, N, shrink, out=out)
  s = None
  if want_scores:
    s = userknn.scores(nbr, uc, lo, hi).cpu().numpy()
  return tuple(t.cpu().numpy() for t in nbr), s


def _assert_bitwise(got, want, what=""):
  for g, t, name in zip(got, want, ("ids", "sims", "counts")):
    assert g.dtype == t.dtype and g.shape == t.shape, (what, name)
    same = g.view(np.uint32) == t.view(np.uint32) if g.dtype == np.float32 else g == t
    assert same.all(), "%s %s: %d entries differ, first at %s" % (what, name, (~same).sum(), np.argwhere(~same)[0])


def _same_bits(a, b):
  return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _small():
  """U = 37, n = 29, density ~0.2; 11 queries, 5 of them training rows."""
  X = uu.random_matrix(37, 29, 0.2, seed=3)
  Q = sp.vstack([X[[0, 5, 17, 30, 36]], uu.random_matrix(6, 29, 0.25, seed=4)]).tocsr()
  return X, Q


@pytest.mark.parametrize("shrink", [0.0, 10.0])
def test_small_case_bit_for_bit(shrink):
  X, Q = _small()
  N = 5
  want = uu.neighbours_f32(X, Q, N, shrink)
  nbr, s = _gpu(X, Q, N, shrink)
  _assert_bitwise(nbr, want, "shrink=%g" % shrink)
  assert _same_bits(s, uu.scores_f32(X, *want))
  ids, sim, count = nbr
  live = np.arange(N)[None, :] < count[:, None]
  assert np.all(ids[~live] == -1) and np.all(sim[~live].view(np.uint32) == 0), "padding must be -1 / +0"
  assert np.all(np.diff(ids.astype(np.int64), axis=1)[live[:, 1:]] > 0), "ids ascending inside a row"
  # a training user finds itself: not excluded
  for q, v in enumerate((0, 5, 17, 30, 36)):
    assert X[v].nnz == 0 or v in ids[q, :count[q]]
  again, s2 = _gpu(X, Q, N, shrink, fill=(0, 0.0, 0))
  _assert_bitwise(again, nbr, "second call")
  assert _same_bits(s2, s)


def test_ties_short_lists_and_empty_rows():
  n = 20
  rows = [[1, 2, 3, 4]] * 12 + [[1, 2, 10, 11, 16], [12, 13], [12, 14, 15]]
  X = sp.lil_matrix((15, n), dtype=np.float32)
  for v, items in enumerate(rows):
    X[v, items] = 1.0
  X = X.tocsr()
  queries = [[1, 2, 3, 4],      # 12 identical users tie at 1.0: the 8 lowest ids are kept
             [12],              # shares items with users 13 and 14 only
             [],                # an empty row
             [18, 19],          # items nobody holds
             [1, 2, 10]]        # user 12 is the most similar, then the 12 tie: the cut falls inside the tie
  Q = sp.lil_matrix((len(queries), n), dtype=np.float32)
  for q, items in enumerate(queries):
    if items:
      Q[q, items] = 1.0
  Q = Q.tocsr()
  N = 8
  want = uu.neighbours_f32(X, Q, N, 0.0)
  nbr, s = _gpu(X, Q, N, 0.0)
  _assert_bitwise(nbr, want, "ties")
  ids, sim, count = nbr
  assert list(ids[0]) == list(range(8)) and np.all(sim[0] == 1.0)
  assert count[1] == 2 and list(ids[1]) == [13, 14] + [-1] * 6 and np.all(sim[1, 2:].view(np.uint32) == 0)
  assert count[2] == 0 and count[3] == 0
  assert list(ids[4]) == list(range(7)) + [12] and sim[4, 7] > sim[4, 0]
  assert _same_bits(s, uu.scores_f32(X, *want))
  assert np.all(s[2].view(np.uint32) == 0) and np.all(s[3].view(np.uint32) == 0), "all +0 without neighbours"


def test_workspace_path_and_the_hand_out_counter():
  """U above rk_rp3_lds_items(): counts and the list of touched users live in the workspace; 600 query rows
  are more than the resident workgroups, so rows are taken through the counter."""
  from recoder_amd import _rp3_lib
  U = _rp3_lib.load().rk_rp3_lds_items() + 5
  n, nq, N = 3000, 600, 3
  rng = np.random.RandomState(7)
  per = rng.randint(2, 4, U)
  rows = np.repeat(np.arange(U), per)
  cols = np.concatenate([rng.choice(n, p, replace=False) for p in per])
  X = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(U, n))
  X.sort_indices()
  Q = sp.vstack([X[rng.choice(U, nq - 100, replace=False)], uu.random_matrix(100, n, 0.002, seed=8)]).tocsr()
  want = uu.neighbours_f32(X, Q, N, 1.0)
  assert (want[2] == N).sum() > 400
  nbr, s = _gpu(X, Q, N, 1.0, lo=100, hi=1100)
  _assert_bitwise(nbr, want, "workspace path")
  assert _same_bits(s, uu.scores_f32(X, *want, 100, 1100))
  again, _ = _gpu(X, Q, N, 1.0, want_scores=False, fill=(-7, 9.0, -3))
  _assert_bitwise(again, nbr, "workspace path, second call")


def test_neighbours_at_the_librarys_maximum():
  from recoder_amd import userknn
  U, n, N = 1500, 60, userknn.MAX_NEIGHBOURS
  X = uu.random_matrix(U, n, 0.15, seed=9)
  Q = uu.random_matrix(4, n, 0.3, seed=10)
  want = uu.neighbours_f32(X, Q, N, 0.5)
  assert want[2].max() == N
  nbr, s = _gpu(X, Q, N, 0.5)
  _assert_bitwise(nbr, want, "N = max")
  assert _same_bits(s, uu.scores_f32(X, *want))


def test_strips_and_leading_dimension():
  from recoder_amd import als, userknn
  X, Q = _small()
  n, N = X.shape[1], 5
  want = uu.neighbours_f32(X, Q, N, 0.0)
  full = uu.scores_f32(X, *want)
  uc, _ = als.csr_pair(X, X.shape[0], n, DEV)
  nbr = tuple(torch.from_numpy(a).to(DEV) for a in want)
  for lo, hi in ((0, n), (7, 19), (n - 1, n)):
    part = userknn.scores(nbr, uc, lo, hi).cpu().numpy()
    assert _same_bits(part, np.ascontiguousarray(full[:, lo:hi])), (lo, hi)
    out = torch.full((Q.shape[0], 32), 5.0, device=DEV)
    userknn.scores(nbr, uc, lo, hi, out=out)
    out = out.cpu().numpy()
    assert _same_bits(np.ascontiguousarray(out[:, :hi - lo]), part) and np.all(out[:, hi - lo:] == 5.0), (lo, hi)


def test_values_and_batch_position():
  X = uu.random_matrix(60, 45, 0.2, seed=11, values=True)
  assert not np.all(X.data == 1.0)
  Q = uu.random_matrix(9, 45, 0.25, seed=12, values=True)
  N = 7
  want = uu.neighbours_f32(X, Q, N, 2.0)
  nbr, s = _gpu(X, Q, N, 2.0)
  _assert_bitwise(nbr, want, "values")
  assert _same_bits(s, uu.scores_f32(X, *want))
  alone, s1 = _gpu(X, Q[4], N, 2.0)
  _assert_bitwise(alone, [a[4:5] for a in nbr], "a query alone")
  assert _same_bits(s1, s[4:5])
  _, srev = _gpu(X, Q[::-1], N, 2.0)
  assert _same_bits(np.ascontiguousarray(srev[::-1]), s)


# ---------------------------------------------------------------- end to end
U_PUB, N_PUB = 200, 150


@pytest.fixture(scope="module")
def fitted():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import UserNeighbourhoodModel
  X = uu.random_matrix(U_PUB, N_PUB, 0.08, seed=21, values=True)
  X.data = np.abs(X.data)
  rec = Recoder(model=UserNeighbourhoodModel(neighbours=20, shrink=1.0))
  info = rec.train_userknn(RecommendationDataset(X))
  Q = sp.vstack([X[:40], np.abs(uu.random_matrix(20, N_PUB, 0.1, seed=22, values=True))]).tocsr()
  want = uu.neighbours_f32(X, Q, 20, 1.0)
  return rec, info, X, Q, want, uu.scores_f32(X, *want)


def _inter(Q):
  from recoder_amd.data import UsersInteractions
  return UsersInteractions(np.arange(Q.shape[0]), Q)


def test_train_userknn_info_and_recommendations(fitted):
  rec, info, X, Q, want, S32 = fitted
  assert sorted(info) == ["fit_ms", "n", "n_users", "neighbours", "nnz", "shrink"]
  assert (info["n_users"], info["n"], info["nnz"], info["neighbours"], info["shrink"]) == (U_PUB, N_PUB, X.nnz, 20, 1.0)
  assert info["fit_ms"] >= 0 and rec.userknn_info == info
  m = rec.model
  assert np.array_equal(m.user_indices.cpu().numpy(), X.indices) and np.array_equal(m.user_indptr.cpu().numpy(), X.indptr)
  assert np.array_equal(m.interaction_values.data.cpu().numpy(), X.data)
  assert np.array_equal(m.user_norms.cpu().numpy(), uu.norms_f32(X))
  got = rec.recommend_array(_inter(Q), 10)
  assert np.array_equal(got, uu.top_k(S32.copy(), Q, 10))
  with pytest.raises(ValueError, match="train_userknn"):
    from recoder_amd.data import RecommendationDataset
    rec.train(RecommendationDataset(X))


def test_predict_is_csr_scores_and_the_restatement(fitted):
  rec, _, X, Q, want, S32 = fitted
  out, _ = rec.predict(_inter(Q))
  assert _same_bits(out.cpu().numpy(), S32)
  direct = rec.model.csr_scores(_dev_csr(Q), 0, N_PUB, None, None, Q.shape[0])
  assert torch.equal(out, direct)
  dense = torch.from_numpy(Q.toarray()).to(DEV)
  assert torch.equal(rec.model(dense), direct)


def test_strips_share_one_neighbour_pass(fitted):
  rec, _, X, Q, _, _ = fitted
  one = rec.recommend_array(_inter(Q), 10)
  before = rec.model.neighbour_passes
  rec.eval_strip_items = 40
  try:
    strips = rec.recommend_array(_inter(Q), 10)
  finally:
    del rec.eval_strip_items
  assert -(-N_PUB // 40) > 1 and np.array_equal(strips, one)
  assert rec.model.neighbour_passes == before + 1, "the neighbours of a batch are computed once, not per strip"


def test_checkpoint_round_trip(fitted, tmp_path):
  from recoder_amd.model import Recoder
  from recoder_amd.nn import UserNeighbourhoodModel
  rec, _, X, Q, _, _ = fitted
  f = rec.save_state(str(tmp_path / "userknn"))
  st = torch.load(f, map_location="cpu", weights_only=False)
  assert st["model_params"] == {"neighbours": 20, "shrink": 1.0, "num_users": U_PUB, "nnz": X.nnz}
  rec2 = Recoder(model=UserNeighbourhoodModel(3, 0.0))
  rec2.init_from_model_file(f)
  assert rec2.model.model_params() == rec.model.model_params()
  for name in st["model"]:
    assert torch.equal(getattr(rec2.model, name), getattr(rec.model, name))
  assert np.array_equal(rec.recommend_array(_inter(Q), 10), rec2.recommend_array(_inter(Q), 10))


def test_evaluate_returns_one_value_per_user(fitted):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import Recall
  rec, _, X, _, _, _ = fitted
  Y = uu.random_matrix(U_PUB, N_PUB, 0.05, seed=23)
  Y = Y - Y.multiply(X != 0)
  Y.eliminate_zeros()
  ds = RecommendationDataset(X, sp.csr_matrix(Y))
  res = rec.evaluate(ds, num_recommendations=20, metrics=[Recall(k=20)], batch_size=64)
  (vals,) = res.values()
  assert len(vals) == len(ds.users) == U_PUB
