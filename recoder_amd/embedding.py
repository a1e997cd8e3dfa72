"""Item-embedding indices with the reference's API (recoder/embedding.py).

``EmbeddingsIndex`` is the reference's interface.  ``ExactEmbeddingsIndex`` takes the place of its
``AnnoyEmbeddingsIndex``: the same constructor keywords, ``build`` / ``load`` and return values, but
the search is EXACT cosine similarity on the GPU (include/recoder_index.h) instead of Annoy's
approximate trees:

  * the table is normalised once (``rk_ix_normalize``; a zero row stays zero: cosine 0 against
    everything, itself included),
  * queries are scored against strips of ``strip_items`` items (``rk_ix_scores``, f32-input MFMA,
    one k-ascending f32 chain per score) and each strip's best n are kept with ``rk_topk_masked``,
    then merged with one more top-n pass -- ties go to the lower row at both levels.  Above
    ``rk_topk_max_k()`` results a stable descending ``torch.sort`` takes its place.

Neighbour lists are ordered by cosine descending, ties to the lower row, and include the queried
item (as Annoy's ``get_nns_by_item`` does).  Distances are Annoy's angular distance
sqrt(2 - 2 cos).  ``MemCacheEmbeddingsIndex`` is the reference's per-item cache.
"""
import math
import pickle

import numpy as np
import torch

from . import _index_lib
from .device import current_stream, require_gpu


class EmbeddingsIndex(object):
  """An index over item embeddings: fetch an item's embedding and search its nearest neighbours
  (recoder/embedding.py).  Every ``EmbeddingsIndex`` implements these four methods."""

  def get_embedding(self, embedding_id):
    """The embedding of item ``embedding_id``."""
    raise NotImplementedError

  def get_nns_by_id(self, embedding_id, n):
    """The ``n`` nearest neighbours of item ``embedding_id``."""
    raise NotImplementedError

  def get_nns_by_embedding(self, embedding, n):
    """The ``n`` nearest neighbours of the vector ``embedding``."""
    raise NotImplementedError

  def get_similarity(self, id1, id2):
    """The similarity of items ``id1`` and ``id2``."""
    raise NotImplementedError


_SCORE_BYTES = 128 << 20        # the [queries, strip] score buffer of one launch


class ExactEmbeddingsIndex(EmbeddingsIndex):
  """Exact cosine-similarity index on the GPU, a drop-in for the reference's ``AnnoyEmbeddingsIndex``.

  Args:
    embeddings (numpy.array or torch.Tensor, optional): the [items, embedding size] matrix (numpy,
      CPU or CUDA tensor; stored as float32, as Annoy stores it).  Required to build the index.
    id_map (dict, optional): original item id -> row of ``embeddings``; identity if not given.
    n_trees (int, optional): accepted for compatibility; no effect (the search is exact).
    search_k (int, optional): accepted for compatibility; no effect (the search is exact).
    include_distances (bool, optional): ``get_nns_by_*`` return ``{id: angular distance}``.

  The raw rows are kept; the upload and the normalisation happen on the first search, so ``build``,
  ``load`` and ``get_embedding`` work without a GPU.  ``build(index_file)`` writes ``index_file``
  (the reference's pickle: ``embedding_size``, ``id_map``) and ``index_file + '.embeddings'`` (the
  raw float32 matrix in ``np.save`` format -- not Annoy's file format, which ``load`` rejects).
  """

  strip_items = 65536           # items scored per launch (tests lower it to force many strips)

  def __init__(self, embeddings=None, id_map=None, n_trees=10, search_k=-1, include_distances=False):
    self.embeddings = embeddings
    self.id_map = id_map
    self.n_trees = n_trees
    self.search_k = search_k
    self.include_distances = include_distances
    self._raw = None
    self._En = None
    self._tables = {}

  # ---- construction -------------------------------------------------------------------
  @classmethod
  def from_recoder(cls, recoder, layer="encoder", id_map=None, **kwargs):
    """An index over a trained ``Recoder``'s item table: the encoder's ``en_embedding_layer`` (what the
    reference's scripts/build_embeddings.py indexes) or the decoder's ``de_embedding_layer``; a
    MatrixFactorization model has one table, ``item_embedding_layer``.  The table is copied as it
    stands when this is called (``Recoder.train`` returns with every lazy Adam sweep applied)."""
    if layer not in ("encoder", "decoder"):
      raise ValueError("layer must be 'encoder' or 'decoder', not %r" % (layer,))
    model = recoder.model
    table = getattr(model, "item_embedding_layer", None)
    if table is None:
      table = model.en_embedding_layer if layer == "encoder" else model.de_embedding_layer
    index = cls(embeddings=table.weight.detach().clone(), id_map=id_map, **kwargs)
    index.build()
    return index

  @staticmethod
  def _as_raw(embeddings):
    if isinstance(embeddings, torch.Tensor):
      t = embeddings.detach()
      if t.dim() != 2:
        raise ValueError("embeddings must be a 2-D matrix")
      if t.is_cuda:
        t = t.float()
        return t if t.stride(1) == 1 else t.contiguous()
      return np.ascontiguousarray(t.numpy(), dtype=np.float32)
    a = np.ascontiguousarray(embeddings, dtype=np.float32)
    if a.ndim != 2:
      raise ValueError("embeddings must be a 2-D matrix")
    return a

  def build(self, index_file=None):
    """Builds the index over ``embeddings`` and stores it in ``index_file`` if given (plus
    ``index_file + '.embeddings'``, the raw matrix, in the same directory)."""
    if self.embeddings is None:
      raise ValueError("no embeddings to build the index from")
    raw = self._as_raw(self.embeddings)
    if raw.shape[0] >= 2 ** 31 or raw.shape[1] >= 2 ** 31:
      raise ValueError("the index holds fewer than 2^31 items of fewer than 2^31 dimensions")
    self._set(raw, self.id_map)
    if index_file:
      host = raw if isinstance(raw, np.ndarray) else raw.cpu().numpy()
      with open(index_file + ".embeddings", "wb") as f:
        np.save(f, np.ascontiguousarray(host, dtype=np.float32), allow_pickle=False)
      with open(index_file, "wb") as f:
        pickle.dump({"embedding_size": self.embedding_size, "id_map": self.id_map}, f)

  def load(self, index_file):
    """Loads an index stored by ``build(index_file)``."""
    with open(index_file, "rb") as f:
      state = pickle.load(f)
    emb_file = index_file + ".embeddings"
    with open(emb_file, "rb") as f:
      try:
        raw = np.load(f, allow_pickle=False)
      except (ValueError, OSError, EOFError) as e:
        raise ValueError("%s is not an embeddings file written by ExactEmbeddingsIndex.build (an Annoy index "
                         "file cannot be read: its format is not supported): %s" % (emb_file, e))
    if raw.dtype != np.float32 or raw.ndim != 2 or raw.shape[1] != state["embedding_size"]:
      raise ValueError("%s: expected a float32 [items, %d] matrix, found %s %s"
                       % (emb_file, state["embedding_size"], raw.dtype, raw.shape))
    self.embeddings = raw
    self._set(raw, state["id_map"])

  def _set(self, raw, id_map):
    n_items = raw.shape[0]
    self.embedding_size = int(raw.shape[1])
    self.id_map = id_map if id_map is not None else {i: i for i in range(n_items)}
    self.inverse_id_map = {v: k for k, v in self.id_map.items()}
    self._ids = [self.inverse_id_map.get(r, r) for r in range(n_items)]
    self._raw = raw
    self._En = None
    self._tables = {}

  def _ensure_built(self):
    if self._raw is None:
      self.build()

  def __len__(self):
    self._ensure_built()
    return int(self._raw.shape[0])

  # ---- device side ----------------------------------------------------------------------
  def normalized(self):
    """The normalised table [items, embedding size] on the GPU (computed on first use)."""
    self._ensure_built()
    if self._En is None:
      dev = require_gpu()
      lib = _index_lib.load()
      raw = self._raw
      src = torch.from_numpy(raw).to(dev) if isinstance(raw, np.ndarray) else raw
      N, h = src.shape
      En = torch.empty(N, h, dtype=torch.float32, device=src.device)
      _index_lib.check(lib.rk_ix_normalize(src.data_ptr(), N, h, src.stride(0), En.data_ptr(), h,
                                           current_stream()), "rk_ix_normalize")
      self._En = En
    return self._En

  def _queries(self, rows_or_vectors):
    """[Q, h] normalised query rows: a table row is copied, a vector goes through the same
    normalisation as the table (so the two come out bitwise equal)."""
    En = self.normalized()
    x = rows_or_vectors
    if not isinstance(x, torch.Tensor):
      x = np.asarray(x)
      if x.dtype.kind in "iu":
        x = torch.from_numpy(x.astype(np.int64))
      else:
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if not x.dtype.is_floating_point:
      rows = x.reshape(-1).to(En.device, torch.int64)
      if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= En.shape[0]):
        raise IndexError("row out of range [0, %d)" % En.shape[0])
      return En.index_select(0, rows)
    v = x.to(En.device, torch.float32)
    if v.dim() == 1:
      v = v.reshape(1, -1)
    if v.dim() != 2 or v.shape[1] != En.shape[1]:
      raise ValueError("query vectors must have %d components" % En.shape[1])
    if v.stride(1) != 1:
      v = v.contiguous()
    out = torch.empty(v.shape[0], v.shape[1], dtype=torch.float32, device=En.device)
    _index_lib.check(_index_lib.load().rk_ix_normalize(v.data_ptr(), v.shape[0], v.shape[1], v.stride(0),
                                                       out.data_ptr(), v.shape[1], current_stream()),
                     "rk_ix_normalize")
    return out

  def scores(self, Qn, lo, hi, out=None):
    """out[q, c] = cosine of normalised query q with row lo + c (``rk_ix_scores``)."""
    En = self.normalized()
    Q, h = Qn.shape
    if out is None:
      out = torch.empty(Q, hi - lo, dtype=torch.float32, device=En.device)
    _index_lib.check(_index_lib.load().rk_ix_scores(Qn.data_ptr(), Q, Qn.stride(0), En.data_ptr(), h, h, lo, hi,
                                                    out.data_ptr(), out.stride(0), current_stream()),
                     "rk_ix_scores")
    return out

  def _strips(self, N, n):
    """[lo, hi) item ranges of ``strip_items`` (at least n) items each."""
    strip = max(n, 1, min(N, int(self.strip_items)))
    bounds = [(lo, min(N, lo + strip)) for lo in range(0, N, strip)]
    if len(bounds) > 1 and bounds[-1][1] - bounds[-1][0] < n:     # a last strip shorter than n: merge it
      bounds = bounds[:-2] + [(bounds[-2][0], N)]
    return bounds

  def knn(self, rows_or_vectors, n):
    """The n nearest rows of each query, exactly: (rows int64 [Q, n], cosines float32 [Q, n]) on the GPU,
    cosine descending, ties to the lower row.  Queries are table rows (an integer array) or vectors
    ([Q, embedding size] floats).  n is capped at the number of items."""
    from . import _lib
    Qn = self._queries(rows_or_vectors)
    En = self._En
    N = En.shape[0]
    Q = Qn.shape[0]
    n = min(int(n), N)
    dev = En.device
    idx = torch.empty(Q, max(n, 0), dtype=torch.int64, device=dev)
    val = torch.empty(Q, max(n, 0), dtype=torch.float32, device=dev)
    if Q == 0 or n <= 0:
      return idx, val
    lib = _lib.load()
    use_topk = n <= lib.rk_topk_max_k()
    bounds = self._strips(N, n if use_topk else 1)
    ns = len(bounds)
    width = max(hi - lo for lo, hi in bounds)
    ld = -(-width // 32) * 32
    qc = max(1, min(Q, _SCORE_BYTES // (4 * ld)))
    scores = torch.empty(qc * ld, dtype=torch.float32, device=dev)
    stream = current_stream()
    for q0 in range(0, Q, qc):
      q1 = min(Q, q0 + qc)
      B = q1 - q0
      S = scores[:B * ld].view(B, ld)
      if use_topk:
        cand_idx = torch.empty(B, ns * n, dtype=torch.int64, device=dev)
        cand_val = torch.empty(B, ns * n, dtype=torch.float32, device=dev)
        for s, (lo, hi) in enumerate(bounds):
          self.scores(Qn[q0:q1], lo, hi, S)
          _lib.check(lib.rk_topk_masked(S.data_ptr(), B, hi - lo, ld, None, 0, n, lo, 1,
                                        cand_idx[:, s * n:].data_ptr(), cand_val[:, s * n:].data_ptr(), ns * n,
                                        stream), "rk_topk_masked")
        if ns == 1:
          idx[q0:q1], val[q0:q1] = cand_idx, cand_val
          continue
        # merge: the strips' lists side by side, each sorted (cosine desc, row asc) -- equal cosines keep
        # ascending rows
        pos = torch.empty(B, n, dtype=torch.int64, device=dev)
        _lib.check(lib.rk_topk_masked(cand_val.data_ptr(), B, ns * n, ns * n, None, 0, n, 0, 1, pos.data_ptr(),
                                      val[q0:q1].data_ptr(), n, stream), "rk_topk_masked")
        idx[q0:q1] = torch.gather(cand_idx, 1, pos)
      else:
        # above the top-k kernel's limit: stable descending sorts (torch.topk's tie order is not defined
        # on the GPU), strip by strip, then over the strips' lists laid side by side
        ci, cv = [], []
        for lo, hi in bounds:
          self.scores(Qn[q0:q1], lo, hi, S)
          v, i = torch.sort(S[:, :hi - lo], dim=1, descending=True, stable=True)
          m = min(n, hi - lo)
          cv.append(v[:, :m])
          ci.append(i[:, :m] + lo)
        cv, ci = torch.cat(cv, 1), torch.cat(ci, 1)
        v, p = torch.sort(cv, dim=1, descending=True, stable=True)
        val[q0:q1] = v[:, :n]
        idx[q0:q1] = torch.gather(ci, 1, p[:, :n])
    return idx, val

  def neighbor_table(self, n):
    """[items, n] rows of every item's n nearest neighbours (itself included), on the GPU; cached per n."""
    t = self._tables.get(int(n))
    if t is None:
      self._ensure_built()
      t = self.knn(torch.arange(self._raw.shape[0], dtype=torch.int64), n)[0]
      self._tables[int(n)] = t
    return t

  # ---- the reference's interface ---------------------------------------------------------
  def get_embedding(self, embedding_id):
    """The raw (not normalised) embedding as a list of floats, as Annoy's ``get_item_vector``."""
    self._ensure_built()
    row = self._raw[self.id_map[embedding_id]]
    return (row if isinstance(row, np.ndarray) else row.cpu().numpy()).tolist()

  def _result(self, idx, cos):
    ids = [self._ids[r] for r in idx.tolist()]
    if not self.include_distances:
      return ids
    return dict(zip(ids, [math.sqrt(max(2.0 - 2.0 * c, 0.0)) for c in cos.tolist()]))

  def get_nns_by_id(self, embedding_id, n):
    self._ensure_built()
    idx, cos = self.knn(np.array([self.id_map[embedding_id]], dtype=np.int64), n)
    return self._result(idx[0].cpu(), cos[0].cpu())

  def get_nns_by_embedding(self, embedding, n):
    self._ensure_built()
    idx, cos = self.knn(np.asarray(embedding, dtype=np.float32).reshape(1, -1), n)
    return self._result(idx[0].cpu(), cos[0].cpu())

  def get_similarity(self, id1, id2):
    """(cosine + 1) / 2, in [0, 1]."""
    self._ensure_built()
    r2 = self.id_map[id2]
    s = self.scores(self._queries(np.array([self.id_map[id1]], dtype=np.int64)), r2, r2 + 1)
    return float(((s + 1.0) * 0.5).item())


class MemCacheEmbeddingsIndex(EmbeddingsIndex):
  """Caches the nearest-neighbour lists of ``get_nns_by_id`` per item in memory, as the reference's
  does (the first ``n`` asked for an item is the one cached).

  Args:
    embedding_index (EmbeddingsIndex): the index to hit on cache misses.
  """

  def __init__(self, embedding_index):
    self.embedding_index = embedding_index
    self.__nns_cache = {}

  def get_embedding(self, embedding_id):
    return self.embedding_index.get_embedding(embedding_id)

  def get_nns_by_embedding(self, embedding, n):
    return self.embedding_index.get_nns_by_embedding(embedding, n)

  def get_nns_by_id(self, embedding_id, n):
    if embedding_id not in self.__nns_cache:
      self.__nns_cache[embedding_id] = self.embedding_index.get_nns_by_id(embedding_id, n)
    return self.__nns_cache[embedding_id]

  def get_similarity(self, id1, id2):
    return self.embedding_index.get_similarity(id1, id2)
