"""CPU: what ItemKNN (recoder_amd/itemknn.py, ItemNeighbourhoodModel) decides without a device -- the parameter
and memory checks, the workspace arithmetic against the library's query, the declared and bound symbols, the
feature weighting and the denominator's vectors against hand-computed values -- and the f32 restatement of
tests/itemknn_util.py against the float64 one.

The 1e-5 of the last test: a similarity of the f32 restatement is an fmaf (or add) chain of m <= 300 positive
terms, m - 1 roundings of partial sums that never exceed the total, then at most four more roundings
(denominator and quotient), over vectors rounded once: about (m + 7) 2^-24 < 2e-5 at worst to first order, and
n = 37 at density 0.2 shares m of about 12 users per pair (60 for the item every other user holds)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import itemknn_util as iu
from tests import rp3_util
from tests.abi_util import built, declared  # noqa: F401  (built: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RP3_HEADER = os.path.join(ROOT, "include", "recoder_rp3.h")
NEW = ("rk_rp3_item_workspace_bytes", "rk_rp3_item_fit")
DEFAULTS = {"neighbours": 200, "shrink": 300.0, "similarity": "cosine", "feature_weighting": "none",
            "asymmetric_alpha": 0.5, "tversky_alpha": 1.0, "tversky_beta": 1.0}


def test_parameter_checks():
  from recoder_amd import itemknn
  from recoder_amd.nn import ItemNeighbourhoodModel, RandomWalkItemModel
  assert itemknn.check_params(100, 0) == (100, 0.0, "cosine", "none", 0.5, 1.0, 1.0)
  assert itemknn.check_params(np.int64(7), np.float32(2.5), "asymmetric", "bm25", 0.3) == \
      (7, 2.5, "asymmetric", "bm25", 0.3, 1.0, 1.0)
  assert itemknn.check_params(itemknn.MAX_NEIGHBOURS, 1e9, "tversky", "none", 0, 0.25, 3)[4:] == (0.0, 0.25, 3.0)
  for sim in itemknn.SIMILARITIES:
    assert itemknn.check_params(5, 1, sim)[2] == sim
  for fw in itemknn.FEATURE_WEIGHTINGS:
    assert itemknn.check_params(5, 1, "cosine", fw)[3] == fw
  for bad in (0, -1, itemknn.MAX_NEIGHBOURS + 1, 2.0, True, None, "3"):
    with pytest.raises(ValueError, match=r"neighbours must be an integer in \[1, %d\]" % itemknn.MAX_NEIGHBOURS):
      itemknn.check_params(bad, 0.0)
  for bad in (-0.5, float("inf"), float("nan"), True, None, "1"):
    with pytest.raises(ValueError, match="shrink must be finite and >= 0"):
      itemknn.check_params(10, bad)
  for bad in ("pearson", "Cosine", None, 3):
    with pytest.raises(ValueError, match="similarity must be one of cosine, asymmetric, jaccard, dice, tversky"):
      itemknn.check_params(10, 1.0, bad)
  for bad in ("idf", "BM25", None):
    with pytest.raises(ValueError, match="feature_weighting must be one of none, tfidf, bm25"):
      itemknn.check_params(10, 1.0, "cosine", bad)
  for sim in ("jaccard", "dice", "tversky"):
    for fw in ("tfidf", "bm25"):
      with pytest.raises(ValueError, match="the %s similarity is over item sets" % sim):
        itemknn.check_params(10, 1.0, sim, fw)
  for bad in (-0.1, 1.1, float("nan"), None, True):
    with pytest.raises(ValueError, match=r"asymmetric_alpha must be finite and in \[0, 1\]"):
      itemknn.check_params(10, 1.0, "asymmetric", "none", bad)
  for name, args in (("tversky_alpha", (-1.0, 1.0)), ("tversky_beta", (1.0, float("inf")))):
    with pytest.raises(ValueError, match="%s must be finite and >= 0" % name):
      itemknn.check_params(10, 1.0, "tversky", "none", 0.5, *args)
  m = ItemNeighbourhoodModel()
  assert itemknn.check_config(m, 5, 1, "dice", "none") == (5, 1.0, "dice", "none", 0.5, 1.0, 1.0)
  with pytest.raises(ValueError, match="train_itemknn fits an ItemNeighbourhoodModel, not RandomWalkItemModel"):
    itemknn.check_config(RandomWalkItemModel(), 5, 1, "cosine", "none")
  for kw in (dict(neighbours=0), dict(shrink=-1.0), dict(similarity="x"), dict(feature_weighting="x"),
             dict(asymmetric_alpha=2), dict(tversky_beta=-1), dict(similarity="jaccard", feature_weighting="tfidf")):
    with pytest.raises(ValueError):
      ItemNeighbourhoodModel(**kw)


def test_values_must_be_finite_and_non_negative():
  from recoder_amd import itemknn
  X = rp3_util.graph_matrix(6, 5, 0.6, seed=1)
  itemknn.check_values(X)
  for bad in (-1.0, float("nan"), float("inf")):
    Y = X.copy()
    Y.data[2] = bad
    with pytest.raises(ValueError, match="ItemKNN needs finite interaction values >= 0: 1 of the %d" % X.nnz):
      itemknn.check_values(Y)


def test_new_symbols_are_declared_and_bound(built):
  import recoder_amd
  from recoder_amd import _rp3_lib
  names = declared([RP3_HEADER])
  for name in NEW:
    assert name in names and name in _rp3_lib.SIGNATURES
    assert hasattr(_rp3_lib.load(), name)
  assert _rp3_lib.load().rk_rp3_version() == 102
  assert "item-neighbourhood" in built.__doc__
  assert recoder_amd.ItemNeighbourhoodModel is __import__("recoder_amd.nn").nn.ItemNeighbourhoodModel
  assert "ItemNeighbourhoodModel" in recoder_amd.__all__


def test_workspace_bytes_is_the_librarys_query(built):
  from recoder_amd import _rp3_lib, itemknn
  lib = _rp3_lib.load()
  lds = lib.rk_rp3_lds_items()
  assert lds == itemknn.LDS_ITEMS
  for n in (1, 37, lds, lds + 1, 250000, 10 ** 6):
    assert lib.rk_rp3_item_workspace_bytes(n) == itemknn.workspace_bytes(n) == lib.rk_rp3_fit_workspace_bytes(n) > 0
  assert lib.rk_rp3_item_workspace_bytes(lds) < lib.rk_rp3_item_workspace_bytes(lds + 1)
  assert lib.rk_rp3_item_workspace_bytes(0) < 0
  assert b"rk_rp3_item_workspace_bytes: n_items" in lib.rk_rp3_last_error()


def test_memory_check_names_the_sizes():
  from recoder_amd import itemknn, rp3
  from recoder_amd.device import DEVICE_HBM_BYTES
  args = (100000, 1000000, 100, 5 * 10 ** 6)
  need = itemknn.required_bytes(*args)
  assert need == 10 ** 6 * 100 * 8 + 10 ** 6 * 4 + (100001 + 1000001) * 8 + 4 * 5 * 10 ** 6 * 4 + 2 * 10 ** 6 * 4 + \
      itemknn.workspace_bytes(10 ** 6)
  # (RP3beta's, with the two value arrays for its user vector)
  assert need - rp3.required_bytes(*args) == 2 * 5 * 10 ** 6 * 4 - 100000 * 4
  assert itemknn.required_bytes(*args, allocate_model=False) == need - (10 ** 6 * 100 * 8 + 10 ** 6 * 4)
  assert itemknn.check_memory(*args, free_bytes=float("inf")) == need
  with pytest.raises(ValueError, match=r"ItemKNN over 100000 users x 1000000 items with 100 neighbours and 5000000 "
                                       r"entries needs %d bytes of device memory, 1000 are free" % need):
    itemknn.check_memory(*args, free_bytes=1000)
  big = DEVICE_HBM_BYTES // 16 + 1
  with pytest.raises(ValueError, match=r"ItemKNN over 1000 users x 1000 items with 10 neighbours and %d entries needs "
                                       r"\d+ bytes: more than one device's memory" % big):
    itemknn.check_memory(1000, 1000, 10, big, free_bytes=float("inf"))
  with pytest.raises(ValueError, match="at least one item"):
    itemknn.check_memory(10, 0, 10, 0, free_bytes=float("inf"))


# users x items, 4 x 5; user 2 holds every item, item 4 has one user
X45 = sp.csr_matrix(np.array([[1, 0, 2, 0, 0],
                              [0, 3, 1, 0, 0],
                              [2, 1, 1, 4, 5],
                              [1, 0, 0, 1, 0]], np.float32))


def test_feature_weighting_is_the_formula():
  from recoder_amd import itemknn
  log = np.log
  idf = [log(5 / 3), log(5 / 3), max(0.0, log(5 / 6)), log(5 / 3)]          # r = 2, 2, 5, 2
  assert idf[2] == 0.0
  got = itemknn.feature_weighted(X45, "none")
  assert got.dtype == np.float32 and np.array_equal(got, X45.data)
  want = [1 * idf[0], np.sqrt(2) * idf[0], np.sqrt(3) * idf[1], 1 * idf[1], 0, 0, 0, 0, 0, 1 * idf[3], 1 * idf[3]]
  got = itemknn.feature_weighted(X45, "tfidf")
  assert got.dtype == np.float32 and np.array_equal(got, np.asarray(want, np.float64).astype(np.float32))
  length = np.array([4.0, 4.0, 4.0, 5.0, 5.0])                            # len_i = column sums; mean 4.4
  norm = 0.25 + 0.75 * length / 4.4
  bm = lambda x, i, v: x * 2.2 / (1.2 * norm[i] + x) * idf[v]
  want = [bm(1, 0, 0), bm(2, 2, 0), bm(3, 1, 1), bm(1, 2, 1), 0, 0, 0, 0, 0, bm(1, 0, 3), bm(1, 3, 3)]
  got = itemknn.feature_weighted(X45, "bm25")
  assert got.dtype == np.float32 and np.array_equal(got, np.asarray(want, np.float64).astype(np.float32))
  for kind in ("none", "tfidf", "bm25"):
    ref = iu.weighted_f64(X45, kind)
    assert np.array_equal(itemknn.feature_weighted(X45, kind), ref.data.astype(np.float32))


def test_denominator_vectors_are_the_table():
  from recoder_amd import itemknn
  f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
  sq = np.array([1 + 4 + 1, 9 + 1, 4 + 1 + 1, 16 + 1, 25], np.float64)    # column sums of squares
  d = np.array([3, 2, 3, 2, 1], np.float64)
  form, own, oth, g = itemknn.vectors(X45.indices, X45.data, 5, "cosine")
  assert (form, g) == (0, 0.0) and own.dtype == oth.dtype == np.float32
  assert np.array_equal(own, f32(np.sqrt(sq))) and np.array_equal(oth, own)
  form, own, oth, g = itemknn.vectors(X45.indices, X45.data, 5, "asymmetric", 0.3)
  assert (form, g) == (0, 0.0)
  assert np.allclose(own, np.sqrt(sq) ** (2 * 0.7), rtol=2.0 ** -22, atol=0)       # |a|^(2(1 - alpha))
  assert np.array_equal(own, f32(sq ** 0.7)) and np.array_equal(oth, f32(sq ** 0.3))
  form, own, oth, g = itemknn.vectors(X45.indices, None, 5, "cosine")          # (no values: all 1.0)
  assert np.array_equal(own, f32(np.sqrt(d)))
  form, own, oth, g = itemknn.vectors(X45.indices, X45.data, 5, "jaccard")
  assert (form, g) == (1, -1.0) and np.array_equal(own, f32(d)) and np.array_equal(oth, f32(d))
  form, own, oth, g = itemknn.vectors(X45.indices, X45.data, 5, "dice")
  assert (form, g) == (1, 0.0) and np.array_equal(own, f32(d / 2)) and np.array_equal(oth, f32(d / 2))
  form, own, oth, g = itemknn.vectors(X45.indices, X45.data, 5, "tversky", 0.5, 0.3, 0.6)
  assert form == 1 and g == float(np.float32(1.0 - 0.3 - 0.6))
  assert np.array_equal(own, f32(0.6 * d)) and np.array_equal(oth, f32(0.3 * d))
  for sim, extra in (("cosine", ()), ("asymmetric", (0.3,)), ("jaccard", ()), ("tversky", (0.5, 0.3, 0.6))):
    ref = iu.vectors_f64(X45, sim, *extra)
    got = itemknn.vectors(X45.indices, X45.data, 5, sim, *extra)
    assert got[0] == ref[0] and np.array_equal(got[1], f32(ref[1])) and np.array_equal(got[2], f32(ref[2]))
    assert got[3] == float(np.float32(ref[3]))


def test_model_params_round_trip():
  from recoder_amd.nn import ItemNeighbourhoodModel, SparseLinearModel
  m = ItemNeighbourhoodModel()
  assert m.model_params() == DEFAULTS
  assert m.fit_module == "itemknn" and ItemNeighbourhoodModel.dense_weights is SparseLinearModel.dense_weights
  a = ItemNeighbourhoodModel(7, 2, "tversky", "none", 0.25, 0.3, 0.6)
  p = a.model_params()
  assert p == {"neighbours": 7, "shrink": 2.0, "similarity": "tversky", "feature_weighting": "none",
               "asymmetric_alpha": 0.25, "tversky_alpha": 0.3, "tversky_beta": 0.6}
  m.load_model_params(p)
  assert m.model_params() == p
  with pytest.raises(ValueError, match="similarity"):
    m.load_model_params(dict(p, similarity="pearson"))
  m = ItemNeighbourhoodModel(neighbours=3)
  m.init_model(num_items=11)
  assert sorted(m.state_dict()) == ["item_neighbours", "item_weights", "neighbour_counts"]
  assert tuple(m.item_neighbours.shape) == tuple(m.item_weights.shape) == (11, 3)


def test_dense_weights_are_per_column_and_torch_forward_on_the_host_is_the_model():
  import torch
  from recoder_amd.nn import ItemNeighbourhoodModel
  X, _ = _case37()
  A = iu.weighted_f64(X, "none")
  form, own, oth, g, binary = iu.vectors_f64(A, "asymmetric", 0.3)
  ids, w, count = iu.fit_f32(A, form, own, oth, g, 2.0, 5, binary)
  m = ItemNeighbourhoodModel(5, 2.0, "asymmetric", "none", 0.3)
  m.init_model(num_items=37)
  m.item_neighbours.copy_(torch.from_numpy(ids))
  m.item_weights.data.copy_(torch.from_numpy(w))
  m.neighbour_counts.copy_(torch.from_numpy(count))
  W = m.dense_weights().numpy()
  full = iu.dense_f32(A, form, own, oth, g, 2.0, binary)
  for j in range(37):
    assert np.array_equal(np.flatnonzero(W[:, j]), ids[j, :count[j]])
    assert np.array_equal(W[ids[j, :count[j]], j], full[ids[j, :count[j]], j])
  assert not np.array_equal(W, W.T)
  Q = np.asarray(X[:9].todense(), np.float32)
  assert np.allclose(m(torch.from_numpy(Q)).numpy(), Q @ W, rtol=1e-6, atol=0)


def test_train_refuses_the_model_and_train_itemknn_refuses_another():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ItemNeighbourhoodModel, MatrixFactorization
  ds = RecommendationDataset(rp3_util.graph_matrix(20, 15, 0.3, seed=1))
  rec = Recoder(model=ItemNeighbourhoodModel())
  with pytest.raises(ValueError, match=r"train_itemknn\(train_dataset\)"):
    rec.train(ds)
  rec = Recoder(model=MatrixFactorization(embedding_size=8))
  with pytest.raises(ValueError, match="train_itemknn fits an ItemNeighbourhoodModel, not MatrixFactorization"):
    rec.train_itemknn(ds)
  rec = Recoder(model=ItemNeighbourhoodModel())
  with pytest.raises(ValueError, match="shrink must be finite and >= 0"):
    rec.train_itemknn(ds, shrink=-1)
  with pytest.raises(ValueError, match="over item sets"):
    rec.train_itemknn(ds, similarity="jaccard", feature_weighting="bm25")


def _case37():
  X = rp3_util.graph_matrix(300, 37, 0.2, seed=40, empty=(0, 150), full=12, none=18)
  V = X.copy()
  V.data = np.random.RandomState(5).randint(1, 6, X.nnz).astype(np.float32)
  return X, V


COMBOS = [("cosine", "none", 0.0, ()), ("cosine", "none", 10.0, ()), ("cosine", "bm25", 10.0, ()),
          ("cosine", "tfidf", 10.0, ()), ("asymmetric", "none", 10.0, (0.3,)), ("jaccard", "none", 0.0, ()),
          ("dice", "none", 5.0, ()), ("tversky", "none", 2.0, (0.5, 0.3, 0.7))]


@pytest.mark.parametrize("similarity, weighting, shrink, extra", COMBOS)
def test_f32_restatement_is_within_1e_5_of_float64_at_n_37(similarity, weighting, shrink, extra):
  X, V = _case37()
  M = V if weighting != "none" else X
  A64 = iu.weighted_f64(M, weighting)
  A32 = sp.csr_matrix((A64.data.astype(np.float32), A64.indices, A64.indptr), shape=A64.shape)
  form, own, oth, g, binary = iu.vectors_f64(A32, similarity, *extra)
  W32 = iu.dense_f32(A32, form, own, oth, g, shrink, binary)
  W64 = np.asarray(iu.sims_f64(A32, form, own, oth, g, shrink, binary).todense())
  assert np.array_equal(W32 > 0, W64 > 0) and (W64 > 0).sum() > 1000
  assert np.all(np.diag(W32) == 0) and np.all(W32[:, 18] == 0) and np.all(W32[18, :] == 0)
  live = W64 > 0
  rel = np.abs(W32.astype(np.float64) - W64)[live] / W64[live]
  print("%s / %s / shrink %g: max rel err of a similarity %.3g" % (similarity, weighting, shrink, rel.max()))
  assert rel.max() <= 1e-5
  if similarity == "jaccard" and shrink == 0:
    B = (np.asarray(X.todense()) > 0)
    inter = (B[:, 3] & B[:, 7]).sum()
    assert abs(W64[3, 7] - inter / (B[:, 3] | B[:, 7]).sum()) < 1e-12 and W64[3, 7] == W64[7, 3]
  # the cut lists spell the same model: K = 5 by (sim descending, id ascending)
  ids, w, count = iu.fit_f32(A32, form, own, oth, g, shrink, 5, binary)
  for j in (0, 12, 18, 36):
    order = np.lexsort((np.arange(37), -W32[:, j]))
    want = np.sort(np.array([i for i in order[:5] if W32[i, j] > 0], np.int64))
    assert np.array_equal(ids[j, :count[j]], want) and np.array_equal(w[j, :count[j]], W32[want, j])
    assert np.all(ids[j, count[j]:] == -1) and np.all(w[j, count[j]:] == 0)
