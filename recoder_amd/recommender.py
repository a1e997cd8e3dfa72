"""Recommenders (recoder/recommender.py).

``InferenceRecommender`` ranks a ``Recoder``'s predictions.  ``SimilarityRecommender`` is the
reference's item-kNN recommender (Aiolli 2013) over an ``EmbeddingsIndex``
(recoder_amd/embedding.py): with an ``ExactEmbeddingsIndex`` (or a ``MemCacheEmbeddingsIndex``
around one) a whole batch of users runs on the GPU -- one exact kNN over the batch's history
items, the candidate pools built with torch ops, ``rk_ix_pool_scores`` and ``rk_topk_masked``;
with any other index, a per-user host loop restates the reference.
"""
import numpy as np
import torch


class Recommender(object):
  def recommend(self, users_hist):
    raise NotImplementedError


class SimilarityRecommender(Recommender):
  """Recommends the items most similar to a user's history (reference recommender.py; Fabio Aiolli,
  Efficient top-n recommendation for very large scale binary rated datasets, RecSys 2013).

  For every user: the pool is the sorted union of the ``n`` nearest neighbours of each history item,
  minus the history; pool item j scores sum over history items t of ((cos(j, t) + 1) / 2) ^ scale;
  at most ``num_recommendations`` pool items are returned, score descending, ties to the lower pool
  position.  A user with an empty pool gets an empty array.

  Args:
    embeddings_index (EmbeddingsIndex): the index used to fetch embeddings and neighbours.
    num_recommendations (int): the most items recommended to a user (fewer if the pool is smaller).
    n (int, optional): neighbours retrieved per history item.
    scale (float, optional): the exponent applied to each similarity.

  ``recommend(users_hist)`` takes either the reference's input -- a list of objects whose ``.items``
  hold original item ids, answered with a list of numpy arrays of original ids -- or a
  ``UsersInteractions`` batch (what ``RecommenderEvaluator`` passes): the history of a user is the
  stored non-zero columns of its row, taken as rows of the index, and the answer is in rows too.
  """

  max_users_per_call = 4096     # users scored per kernel launch

  def __init__(self, embeddings_index, num_recommendations, n=1, scale=1):
    self.embeddings_index = embeddings_index
    self.num_recommendations = num_recommendations
    self.n = n
    self.scale = scale

  def _exact_index(self):
    from .embedding import ExactEmbeddingsIndex, MemCacheEmbeddingsIndex
    index = self.embeddings_index
    if isinstance(index, MemCacheEmbeddingsIndex):
      index = index.embedding_index
    return index if isinstance(index, ExactEmbeddingsIndex) else None

  def recommend(self, users_hist):
    from .data import UsersInteractions
    exact = self._exact_index()
    if isinstance(users_hist, UsersInteractions):
      m = users_hist.interactions_matrix.tocsr()
      hists = []
      for u in range(m.shape[0]):
        lo, hi = m.indptr[u], m.indptr[u + 1]
        hists.append(m.indices[lo:hi][m.data[lo:hi] != 0].astype(np.int64))
      if exact is not None:
        return self._recommend_rows(exact, hists)
      return [self._recommend_single(h) for h in hists]
    if exact is None:
      return [self._recommend_single(np.asarray(uh.items)) for uh in users_hist]
    id_map = exact.id_map
    hists = [np.array([id_map[i] for i in uh.items], dtype=np.int64) for uh in users_hist]
    ids = np.asarray(exact._ids)
    return [ids[rows] for rows in self._recommend_rows(exact, hists)]

  # ---- the GPU path ----------------------------------------------------------------------
  def _recommend_rows(self, index, hists):
    out = []
    step = int(self.max_users_per_call)
    for u0 in range(0, len(hists), step):
      out.extend(self._recommend_rows_batch(index, hists[u0:u0 + step]))
    return out

  def _recommend_rows_batch(self, index, hists):
    from . import _index_lib, _lib
    from .device import current_stream
    U = len(hists)
    k_max = int(self.num_recommendations)
    empty = np.zeros(0, dtype=np.int64)
    lens = np.array([len(h) for h in hists], dtype=np.int64)
    if U == 0 or lens.sum() == 0 or k_max <= 0:
      return [empty.copy() for _ in range(U)]
    En = index.normalized()
    N = En.shape[0]
    dev = En.device
    hist_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(dev)
    hist_idx = torch.from_numpy(np.concatenate(hists).astype(np.int64)).to(dev)
    if int(hist_idx.min()) < 0 or int(hist_idx.max()) >= N:
      raise IndexError("history item out of range [0, %d)" % N)
    user_of = torch.repeat_interleave(torch.arange(U, device=dev), torch.from_numpy(lens).to(dev))
    # 1. one exact kNN over the batch's distinct history items
    uniq, inv = torch.unique(hist_idx, sorted=True, return_inverse=True)
    nn = index.knn(uniq, self.n)[0]                             # [|uniq|, n]
    # 2. pools: sorted unique (user, row) keys of every history item's neighbours, minus the history
    cand = nn[inv]                                              # [nnz, n]
    keys = (user_of[:, None] * N + cand).reshape(-1)
    keys = torch.unique(keys, sorted=True)
    hkeys = torch.unique(user_of * N + hist_idx, sorted=True)
    keys = keys[~torch.isin(keys, hkeys)]
    pool_user = keys // N
    pool_row = keys - pool_user * N
    pool_cnt = torch.bincount(pool_user, minlength=U)
    pool_ld = int(pool_cnt.max()) if keys.numel() else 0
    if pool_ld == 0:
      return [empty.copy() for _ in range(U)]
    start = torch.cumsum(pool_cnt, 0) - pool_cnt
    pool_idx = torch.zeros(U, pool_ld, dtype=torch.int64, device=dev)      # (padding: row 0, never read)
    pool_idx[pool_user, torch.arange(keys.numel(), device=dev) - start[pool_user]] = pool_row
    # 3. scores: -inf past each user's pool
    scores = torch.empty(U, pool_ld, dtype=torch.float32, device=dev)
    _index_lib.check(_index_lib.load().rk_ix_pool_scores(
        En.data_ptr(), En.stride(0), En.shape[1], hist_ptr.data_ptr(), hist_idx.data_ptr(), U, pool_idx.data_ptr(),
        pool_cnt.data_ptr(), pool_ld, float(self.scale), scores.data_ptr(), current_stream()), "rk_ix_pool_scores")
    # 4. the best k per user (score descending, ties to the lower pool position); the -inf padding sorts
    #    last and every list is cut to its pool's size
    k = min(k_max, pool_ld)
    lib = _lib.load()
    if k <= lib.rk_topk_max_k():
      pos = torch.empty(U, k, dtype=torch.int64, device=dev)
      _lib.check(lib.rk_topk_masked(scores.data_ptr(), U, pool_ld, pool_ld, None, 0, k, 0, 1, pos.data_ptr(), None,
                                    k, current_stream()), "rk_topk_masked")
    else:
      pos = torch.sort(scores, dim=1, descending=True, stable=True)[1][:, :k]
    rows = torch.gather(pool_idx, 1, pos).cpu().numpy()
    cnt = pool_cnt.cpu().numpy()
    return [rows[u, :min(k, int(cnt[u]))].copy() for u in range(U)]

  # ---- any other EmbeddingsIndex: the reference's per-user loop ---------------------------
  def _recommend_single(self, user_items):
    user_items = np.asarray(user_items)
    if len(user_items) == 0:
      return np.zeros(0, dtype=np.int64)
    pool = np.unique(np.concatenate([list(self.embeddings_index.get_nns_by_id(i, self.n))    # (list: a dict
                                     for i in user_items]))                                     # of distances too)
    pool = pool[np.isin(pool, user_items, invert=True)]
    if len(pool) == 0:
      return pool
    P = self._unit_rows(pool)
    H = self._unit_rows(user_items)
    scores = np.power((P @ H.T + 1) / 2, self.scale).sum(axis=1)
    order = np.argsort(-scores, kind="stable")[:int(self.num_recommendations)]
    return pool[order]

  def _unit_rows(self, ids):
    x = np.array([self.embeddings_index.get_embedding(i) for i in ids], dtype=np.float64)
    nrm = np.linalg.norm(x, axis=1, keepdims=True)
    return np.divide(x, nrm, out=np.zeros_like(x), where=nrm > 0)


class InferenceRecommender(Recommender):
  """Recommends from the predictions of a ``Recoder`` (recommender.py:104-118)."""

  def __init__(self, model, num_recommendations):
    self.model = model
    self.num_recommendations = num_recommendations

  def recommend(self, users_hist):
    return self.model.recommend(users_hist, self.num_recommendations)

  def recommend_array(self, users_hist):
    """The same lists as one [users, k] integer array (metrics.RecommenderEvaluator's fast path)."""
    return self.model.recommend_array(users_hist, self.num_recommendations)

  def recommend_device(self, users_hist):
    """The same lists left on the device: (int64 tensor [users, k], its row stride), what
    ``RecommenderEvaluator.evaluate(on_device=True)`` hands to rk_als_rank_metrics."""
    return self.model._recommend_device(users_hist, self.num_recommendations)


class FoldInRecommender(Recommender):
  """Recommends to users a ``Recoder``'s MatrixFactorization has not seen: every batch's user rows are folded in
  from the users' histories (``Recoder.fold_in`` at ``alpha``, ``reg``; recoder_amd/foldin.py) and scored like
  ``InferenceRecommender``'s.  ``users_hist.users`` is ignored.  With ``RecommenderEvaluator`` this evaluates strong
  generalisation (held-out users), on its host path and with ``on_device=True``."""

  def __init__(self, model, num_recommendations, alpha=30.0, reg=100.0):
    self.model = model
    self.num_recommendations = num_recommendations
    self.alpha = alpha
    self.reg = reg

  def recommend(self, users_hist):
    return self.recommend_array(users_hist).tolist()

  def recommend_array(self, users_hist):
    return self.model.recommend_folded(users_hist, self.num_recommendations, alpha=self.alpha, reg=self.reg)

  def recommend_device(self, users_hist):
    """(int64 device tensor [users, k], its row stride), as ``InferenceRecommender.recommend_device``."""
    rows = self.model.fold_in(users_hist.interactions_matrix, self.alpha, self.reg)
    return self.model._recommend_device(users_hist, self.num_recommendations, user_rows=rows)


class FilteredRecommender(Recommender):
  """``InferenceRecommender`` under the filters of ``Recoder.recommend_filtered`` (recoder_amd/serve.py).
  ``user_allow`` / ``user_deny`` are scipy sparse [num_users, n_items] and are row-indexed with every batch's
  ``users_hist.users``; the other arguments are passed as they are.  A user with fewer than ``num_recommendations``
  eligible items gets id -1 in the last positions, which no metric counts as a hit.  With ``RecommenderEvaluator``
  and ``metrics.sampled_candidates`` as ``user_allow`` this is the sampled-negatives protocol, on the host path and
  with ``on_device=True``."""

  def __init__(self, model, num_recommendations, filter_seen=True, allow_items=None, deny_items=None, user_allow=None,
               user_deny=None, route="auto"):
    self.model = model
    self.num_recommendations = num_recommendations
    self.user_allow = None if user_allow is None else user_allow.tocsr()
    self.user_deny = None if user_deny is None else user_deny.tocsr()
    self.kw = dict(filter_seen=filter_seen, allow_items=allow_items, deny_items=deny_items, route=route)

  def _filters(self, users_hist):
    users = np.asarray(users_hist.users).astype(np.int64).reshape(-1)
    rows = lambda m: None if m is None else m[users]
    return dict(self.kw, user_allow=rows(self.user_allow), user_deny=rows(self.user_deny))

  def recommend(self, users_hist):
    return self.recommend_array(users_hist).tolist()

  def recommend_array(self, users_hist):
    return self.model.recommend_filtered(users_hist, self.num_recommendations, **self._filters(users_hist))

  def recommend_device(self, users_hist):
    """(int64 device tensor [users, k], its row stride), as ``InferenceRecommender.recommend_device``."""
    from . import serve
    ids, _ = serve.recommend_filtered_device(self.model, users_hist, self.num_recommendations,
                                             **self._filters(users_hist))
    return ids, int(ids.stride(0))
