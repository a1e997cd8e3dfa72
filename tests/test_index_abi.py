"""CPU: librecoder_index.so is built beside the training library, exports exactly what
include/recoder_index.h declares (each bound in _index_lib.SIGNATURES), leaves the training
library's exports alone; ExactEmbeddingsIndex builds, saves and loads without a GPU and fails
loudly when asked to search without one."""
import os
import pickle

import numpy as np
import pytest

from tests.abi_util import built  # noqa: F401  (built: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_library_produces_both_libraries(built):
  for path in (built.LIB, built.INDEX_LIB):
    assert os.path.exists(path), path


def test_build_load_round_trip_without_gpu(tmp_path):
  from recoder_amd.embedding import ExactEmbeddingsIndex
  rng = np.random.RandomState(0)
  emb = rng.rand(300, 24)                                  # float64 in, float32 stored (as Annoy stores it)
  id_map = {1000 + 3 * r: r for r in range(300)}
  index = ExactEmbeddingsIndex(embeddings=emb, id_map=id_map, n_trees=5, search_k=100)
  f = str(tmp_path / "index")
  index.build(index_file=f)
  with open(f, "rb") as fh:
    state = pickle.load(fh)
  assert state == {"embedding_size": 24, "id_map": id_map}
  with open(f + ".embeddings", "rb") as fh:
    raw = np.load(fh)
  assert raw.dtype == np.float32 and np.array_equal(raw, emb.astype(np.float32))
  loaded = ExactEmbeddingsIndex()
  loaded.load(index_file=f)
  assert loaded.embedding_size == index.embedding_size == 24
  assert loaded.id_map == id_map and loaded.inverse_id_map == index.inverse_id_map
  for i in (1000, 1003, 1000 + 3 * 299):
    e = index.get_embedding(i)
    assert isinstance(e, list) and e == loaded.get_embedding(i)
    assert e == emb[id_map[i]].astype(np.float32).tolist()


def test_loading_a_foreign_embeddings_file_fails_clearly(tmp_path):
  from recoder_amd.embedding import ExactEmbeddingsIndex
  f = str(tmp_path / "annoy_index")
  with open(f, "wb") as fh:
    pickle.dump({"embedding_size": 8, "id_map": {0: 0}}, fh)
  with open(f + ".embeddings", "wb") as fh:
    fh.write(b"\x00\x01\x02\x03" * 64)                     # not an np.save file (e.g. an Annoy index)
  with pytest.raises(ValueError, match="not an embeddings file"):
    ExactEmbeddingsIndex().load(f)


def test_search_without_gpu_raises():
  import torch
  if torch.cuda.is_available():
    pytest.skip("GPU present")
  from recoder_amd._lib import RecoderHipError
  from recoder_amd.embedding import ExactEmbeddingsIndex
  index = ExactEmbeddingsIndex(embeddings=np.eye(5, dtype=np.float32))
  index.build()
  assert index.get_embedding(2) == [0.0, 0.0, 1.0, 0.0, 0.0]
  with pytest.raises(RecoderHipError):
    index.get_nns_by_id(0, 3)
  with pytest.raises(RecoderHipError):
    index.knn(np.arange(5), 2)
