"""ExactEmbeddingsIndex on the GPU: the reference's AnnoyEmbeddingsIndex answers (golden fixtures of
tests/golden/make_golden_similarity.py, an exact angular index behind the reference's own class),
float64 numpy, the bitwise invariants of the one-chain-per-score kernels, and the edges."""
import numpy as np
import pytest
import torch

from tests.similarity_util import (CONFIGS, COS_TOL, assert_same_ranking, check_knn, load_fixture, unit64)

pytestmark = pytest.mark.gpu


def _index(emb, id_map=None, **kw):
  from recoder_amd.embedding import ExactEmbeddingsIndex
  index = ExactEmbeddingsIndex(embeddings=emb, id_map=id_map, **kw)
  index.build()
  return index


@pytest.mark.parametrize("name", CONFIGS)
def test_reference_answers(name):
  z, emb, ids, id_map = load_fixture(name)
  U = unit64(emb)
  cos64 = lambda a, b: float(U[id_map[a]] @ U[id_map[b]])
  index = _index(emb, id_map)
  dindex = _index(emb, id_map, include_distances=True)
  for n in (1, 10, 100):
    for i, q in enumerate(z["query_ids"]):
      q = int(q)
      score = lambda k: cos64(q, k)
      assert_same_ranking(index.get_nns_by_id(q, n), z["nns/%d" % n][i], score, what=(name, n, q))
      d = dindex.get_nns_by_id(q, n)
      assert isinstance(d, dict)
      assert_same_ranking(list(d), z["nns_dist_ids/%d" % n][i], score, what=(name, n, q))
      for k, v in d.items():                       # angular distance: cos = 1 - d^2 / 2
        assert abs((1.0 - v * v / 2) - score(k)) <= 2 * COS_TOL
  for i, v in enumerate(z["query_vecs"]):
    u = unit64(v)
    assert_same_ranking(index.get_nns_by_embedding(v, 10), z["nns_vec/10"][i],
                        lambda k: float(U[id_map[k]] @ u), what=(name, "vec", i))
  for (a, b), want in zip(z["sim_pairs"], z["sim"]):
    got = index.get_similarity(int(a), int(b))
    assert isinstance(got, float) and abs(got - want) <= COS_TOL
  for r in (0, 7, len(ids) - 1):
    assert index.get_embedding(int(ids[r])) == emb[r].tolist()


def test_knn_against_float64_and_bitwise_invariants():
  z, emb, ids, id_map = load_fixture("h64")
  index = _index(emb, id_map)
  N = emb.shape[0]
  C64 = unit64(emb) @ unit64(emb).T
  rows = np.arange(0, N, 7)
  idx, cos = index.knn(rows, 100)
  check_knn(idx.cpu().numpy(), cos.cpu().numpy(), C64[rows], 100)
  # a query's row in a batch is the same query alone
  for j in (0, 5, len(rows) - 1):
    i1, c1 = index.knn(rows[j:j + 1], 100)
    assert torch.equal(i1[0], idx[j]) and torch.equal(c1[0], cos[j])
  # many strips give the one-strip answer; two calls give the same answer
  strips = _index(emb, id_map)
  strips.strip_items = 256
  i2, c2 = strips.knn(rows, 100)
  assert torch.equal(i2, idx) and torch.equal(c2, cos)
  i3, c3 = index.knn(rows, 100)
  assert torch.equal(i3, idx) and torch.equal(c3, cos)
  # a vector normalised as a query is bitwise the table row
  dindex = _index(emb, id_map, include_distances=True)
  for r in (3, 99, N - 1):
    i = int(ids[r])
    assert index.get_nns_by_embedding(index.get_embedding(i), 50) == index.get_nns_by_id(i, 50)
    assert dindex.get_nns_by_embedding(dindex.get_embedding(i), 50) == dindex.get_nns_by_id(i, 50)
  nt = index.neighbor_table(10)
  assert nt.shape == (N, 10) and nt is index.neighbor_table(10)
  assert torch.equal(nt[rows], index.knn(rows, 10)[0])


@pytest.mark.parametrize("h", [1, 37, 64, 200, 512])
def test_hidden_sizes_and_strided_tables(h):
  rng = np.random.RandomState(h)
  N = 1037
  big = torch.from_numpy(rng.standard_normal((N, h + 5)).astype(np.float32)).cuda()
  view = big[:, :h]                                # leading dimension h + 5
  assert view.stride(0) == h + 5
  index = _index(view)
  emb = view.cpu().numpy()
  C64 = unit64(emb) @ unit64(emb).T
  q = np.array([0, 500, N - 1])
  n = min(100, N)
  idx, cos = index.knn(q, n)
  if h == 1:                                       # cosines are +-1: all ties, lower rows first
    sign = np.sign(emb[:, 0])
    for j, r in enumerate(q):
      want = np.nonzero(sign == sign[r])[0][:n]
      assert np.array_equal(idx[j].cpu().numpy(), want)
    return
  check_knn(idx.cpu().numpy(), cos.cpu().numpy(), C64[q], n)
  contiguous = _index(view.contiguous())
  i2, c2 = contiguous.knn(q, n)
  assert torch.equal(i2, idx) and torch.equal(c2, cos)


@pytest.mark.parametrize("Q", [1, 3, 4096])
def test_query_batch_sizes(Q):
  rng = np.random.RandomState(Q)
  N, h = 5003, 48
  emb = rng.standard_normal((N, h)).astype(np.float32)
  index = _index(emb)
  U = unit64(emb)
  vecs = rng.standard_normal((Q, h)).astype(np.float32)
  idx, cos = index.knn(vecs, 10)
  check_knn(idx.cpu().numpy(), cos.cpu().numpy(), unit64(vecs) @ U.T, 10)
  rows = rng.randint(0, N, size=Q)
  idx, cos = index.knn(rows, 10)
  check_knn(idx.cpu().numpy(), cos.cpu().numpy(), U[rows] @ U.T, 10)
  assert np.array_equal(idx[:, 0].cpu().numpy(), rows)       # the item itself first (no duplicates here)


@pytest.mark.parametrize("n", [1, 100, 1024, 1025, 1500])
def test_result_sizes_and_the_sort_path(n):
  z, emb, ids, id_map = load_fixture("h64")
  N = emb.shape[0]
  index = _index(emb)
  C64 = unit64(emb) @ unit64(emb).T
  rows = np.array([0, 1, 777, N - 1])
  idx, cos = index.knn(rows, n)
  check_knn(idx.cpu().numpy(), cos.cpu().numpy(), C64[rows], n)
  strips = _index(emb)
  strips.strip_items = 256
  i2, c2 = strips.knn(rows, n)
  assert torch.equal(i2, idx) and torch.equal(c2, cos)
  assert len(index.get_nns_by_id(3, n + 10)) == min(n + 10, N)     # at most N results


def test_zero_rows_and_duplicates():
  rng = np.random.RandomState(5)
  emb = rng.standard_normal((700, 40)).astype(np.float32)
  emb[5] = 0
  emb[20] = emb[10]
  emb[30] = emb[10]
  index = _index(emb)
  assert torch.count_nonzero(index.normalized()[5]) == 0
  idx, cos = index.knn(np.array([5]), 50)          # cosine 0 against everything: rows in order
  assert np.array_equal(idx[0].cpu().numpy(), np.arange(50)) and torch.count_nonzero(cos) == 0
  assert index.get_similarity(5, 5) == 0.5 and index.get_similarity(5, 123) == 0.5
  idx, cos = index.knn(np.array([20, 30, 10]), 3)  # equal rows: equal cosines, the lower row first
  for j in range(3):
    assert idx[j].tolist() == [10, 20, 30]
    assert cos[j, 0] == cos[j, 1] == cos[j, 2]
  assert index.get_nns_by_id(30, 1) == [10]


def test_build_index(tmp_path):
  """The reference's tests/test_embedding.py::test_build_index, on this index."""
  from recoder_amd.embedding import ExactEmbeddingsIndex
  embeddings_mat = np.random.rand(1000, 128)
  index = ExactEmbeddingsIndex(embeddings=embeddings_mat)
  f = str(tmp_path / "test_embeddings")
  index.build(index_file=f)
  index_loaded = ExactEmbeddingsIndex()
  index_loaded.load(index_file=f)
  assert index_loaded.embedding_size == index.embedding_size and index.embedding_size == 128
  test_item = np.random.randint(1000)
  assert index.get_embedding(test_item) == index_loaded.get_embedding(test_item)
  assert index.get_nns_by_id(test_item, 100) == index_loaded.get_nns_by_id(test_item, 100)
  test_item_1 = np.random.randint(0, 1000)
  test_item_2 = np.random.randint(0, 1000)
  assert index.get_similarity(test_item_1, test_item_2) == index_loaded.get_similarity(test_item_1, test_item_2)


@pytest.mark.parametrize("kind", ["ae", "mf"])
def test_from_recoder_reads_the_trained_tables(kind):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.embedding import ExactEmbeddingsIndex
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder, MatrixFactorization
  from tests.test_hip_parity import synth_csr
  csr = synth_csr(600, 800, 10, seed=91)
  torch.manual_seed(4)
  model = DynamicAutoencoder([32], activation_type="tanh", sparse=False) if kind == "ae" else \
      MatrixFactorization(16, activation_type="none", sparse=False)
  rec = Recoder(model=model, use_cuda=True, optimizer_type="adam", loss="mse")
  rec.train(RecommendationDataset(csr), batch_size=64, lr=1e-3, weight_decay=2e-5, num_epochs=2, negative_sampling=True)
  layers = [("encoder", "en_embedding_layer"), ("decoder", "de_embedding_layer")] if kind == "ae" else \
      [("encoder", "item_embedding_layer")]
  for layer, attr in layers:
    W = getattr(model, attr).weight.detach()
    index = ExactEmbeddingsIndex.from_recoder(rec, layer=layer)
    Wh = W.cpu().numpy()
    for r in range(W.shape[0]):
      assert index.get_embedding(r) == Wh[r].tolist(), (layer, r)
    rows = np.arange(0, W.shape[0], 37)
    idx, cos = index.knn(rows, 20)
    check_knn(idx.cpu().numpy(), cos.cpu().numpy(), unit64(Wh[rows]) @ unit64(Wh).T, 20)
