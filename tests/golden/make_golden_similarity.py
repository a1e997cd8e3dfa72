"""Golden vectors of the reference's item-embedding API (build container only).

Imports amoussawi/recoder from /root/reference (read-only) the way make_golden.py does, replaces
the ``annoy.AnnoyIndex`` its ``recoder.embedding`` uses with ``ExactAngularIndex`` below -- an
EXACT in-memory angular index (float32 storage as Annoy's, float64 arithmetic, ties to the lower
item) -- and records what the reference's own ``AnnoyEmbeddingsIndex``, ``MemCacheEmbeddingsIndex``
and ``SimilarityRecommender`` return through it on seeded embeddings with a non-identity id map.

Only data goes to ``tests/golden/similarity_*.npz``.  The embeddings are small integers / 32
(exact in float32) stored as int8, which keeps the files small.

    python tests/golden/make_golden_similarity.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

CONFIGS = [("h64", 1500, 64, 11), ("h200", 1000, 200, 12), ("h37", 400, 37, 13)]
QUERY_NS = (1, 10, 100)
REC_CASES = ((1, 1), (5, 1), (5, 2))
NUM_RECOMMENDATIONS = 20
EMB_SCALE = 32.0


class ExactAngularIndex(object):
  """The part of ``annoy.AnnoyIndex`` the reference calls, answered exactly."""

  def __init__(self, f, metric="angular"):
    assert metric == "angular"
    self.f = f
    self.items = {}
    self.X = None

  def add_item(self, i, v):
    self.items[int(i)] = np.asarray(v, dtype=np.float32).copy()

  def build(self, n_trees):
    X = np.zeros((max(self.items) + 1, self.f), dtype=np.float32)
    for i, v in self.items.items():
      X[i] = v
    self._set(X)

  def _set(self, X):
    self.X = X
    x = X.astype(np.float64)
    nrm = np.linalg.norm(x, axis=1, keepdims=True)
    self.Xn = np.divide(x, nrm, out=np.zeros_like(x), where=nrm > 0)

  def save(self, fn):
    with open(fn, "wb") as f:
      np.save(f, self.X)

  def load(self, fn):
    with open(fn, "rb") as f:
      self._set(np.load(f))

  def get_item_vector(self, i):
    return self.X[i].tolist()

  def _nns(self, q, n, include_distances):
    cos = self.Xn @ q
    order = np.lexsort((np.arange(len(cos)), -cos))[:n]
    ids = [int(i) for i in order]
    if not include_distances:
      return ids
    return ids, [float(np.sqrt(max(2.0 - 2.0 * cos[i], 0.0))) for i in order]

  def get_nns_by_item(self, i, n, search_k=-1, include_distances=False):
    return self._nns(self.Xn[i], n, include_distances)

  def get_nns_by_vector(self, v, n, search_k=-1, include_distances=False):
    q = np.asarray(v, dtype=np.float32).astype(np.float64)
    nrm = np.linalg.norm(q)
    return self._nns(q / nrm if nrm > 0 else q, n, include_distances)

  def get_distance(self, i, j):
    return float(np.sqrt(max(2.0 - 2.0 * float(self.Xn[i] @ self.Xn[j]), 0.0)))


def import_similarity():
  from make_golden import import_reference
  import_reference()
  import recoder.embedding as remb
  import recoder.recommender as rrec
  remb.an.AnnoyIndex = ExactAngularIndex
  return remb, rrec


def make(name, N, h, seed, remb, rrec):
  rng = np.random.RandomState(seed)
  centers = rng.randint(-60, 61, size=(24, h))
  q = np.clip(centers[rng.randint(0, 24, size=N)] + rng.randint(-40, 41, size=(N, h)), -127, 127).astype(np.int8)
  q[(np.abs(q).sum(axis=1) == 0), 0] = 1
  emb = q.astype(np.float32) / EMB_SCALE
  ids = 100000 + 7 * rng.permutation(N)                  # original id of row r: ids[r]
  id_map = {int(ids[r]): r for r in range(N)}
  out = {"emb_q": q, "emb_scale": np.float64(EMB_SCALE), "ids": ids.astype(np.int64)}

  index = remb.AnnoyEmbeddingsIndex(embeddings=emb, id_map=id_map)
  index.build()
  dist_index = remb.AnnoyEmbeddingsIndex(embeddings=emb, id_map=id_map, include_distances=True)
  dist_index.build()
  qids = ids[rng.choice(N, 20, replace=False)]
  out["query_ids"] = qids.astype(np.int64)
  for n in QUERY_NS:
    out["nns/%d" % n] = np.array([index.get_nns_by_id(int(i), n) for i in qids], dtype=np.int64)
    d = [dist_index.get_nns_by_id(int(i), n) for i in qids]
    out["nns_dist_ids/%d" % n] = np.array([list(x.keys()) for x in d], dtype=np.int64)
    out["nns_dist/%d" % n] = np.array([list(x.values()) for x in d], dtype=np.float64)
  vecs = (rng.randint(-100, 101, size=(10, h)) / EMB_SCALE).astype(np.float32)
  out["query_vecs"] = vecs
  out["nns_vec/10"] = np.array([index.get_nns_by_embedding(v, 10) for v in vecs], dtype=np.int64)
  pairs = ids[rng.randint(0, N, size=(50, 2))]
  out["sim_pairs"] = pairs.astype(np.int64)
  out["sim"] = np.array([index.get_similarity(int(a), int(b)) for a, b in pairs], dtype=np.float64)

  # the recommender: 50 users, histories of 1-30 original ids
  lens = rng.randint(1, 31, size=50)
  hist = [ids[rng.choice(N, L, replace=False)] for L in lens]
  out["hist_ptr"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  out["hist"] = np.concatenate(hist).astype(np.int64)
  users = [types.SimpleNamespace(items=list(int(i) for i in x)) for x in hist]
  for n, scale in REC_CASES:
    rec = rrec.SimilarityRecommender(index, NUM_RECOMMENDATIONS, n=n, scale=scale)
    cached = rrec.SimilarityRecommender(remb.MemCacheEmbeddingsIndex(index), NUM_RECOMMENDATIONS, n=n, scale=scale)
    lists = []
    for u in users:
      pool = set(j for i in u.items for j in index.get_nns_by_id(i, n)) - set(u.items)
      if not pool:
        # (the reference raises on an empty pool -- normalize() of a 1-D empty array; recorded as an empty list)
        lists.append(np.zeros(0, dtype=np.int64))
        continue
      got = rec.recommend([u])[0]
      assert np.array_equal(got, cached.recommend([u])[0])
      lists.append(got)
    key = "rec/n%d_s%d" % (n, scale)
    out[key + "/ptr"] = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    out[key + "/ids"] = np.concatenate(lists).astype(np.int64)
  path = os.path.join(HERE, "similarity_%s.npz" % name)
  np.savez_compressed(path, **out)
  print(path, os.path.getsize(path), "bytes")


def main():
  remb, rrec = import_similarity()
  for name, N, h, seed in CONFIGS:
    make(name, N, h, seed, remb, rrec)


if __name__ == "__main__":
  main()
