"""Constrained serving: item filters, candidate reranking and scores for every model a ``Recoder`` serves, on
rk_als_serve_mask, rk_als_pair_scores and rk_als_pairs_topk of librecoder_als.so (include/recoder_als.h).

For row r of a batch and item c, ``eligible(r, c)`` is the conjunction of

  * not ``filter_seen``, or (r, c) is not a stored entry of the users' interactions with a POSITIVE value (the
    rule of ``recommend``: a stored value <= 0 does not mask),
  * ``allow_items`` is None, or c is in it;  c is not in ``deny_items``  (catalogue-wide),
  * ``user_allow`` is None, or (r, c) is in its pattern;  (r, c) is not in the pattern of ``user_deny``  (per row),

and the result of row r is its eligible items by (score descending, item id ascending) in ``rk_topk_masked``'s
order, cut at k.  A row with e < k eligible items returns them and then id -1 with score -inf: the padding is
decided by a count of eligible items taken on the device, never by the score values, and nothing is read back
before the result's own copy.  Scores are expected finite: an eligible item that scores -inf or a negative NaN
ties with, or falls below, what the mask holds at -inf on the "mask" route.

Two routes rank the same set by the same rule:

  "mask"   the filters become a deny bitmap over the catalogue (rk_als_serve_mask) that the strip decode, the
           per-strip ``rk_topk_masked`` and the merge of ``Recoder._recommend_device`` read in place of the users'
           own input block.  Every model.
  "pairs"  with ``user_allow``: every candidate is scored by one gather and one f32 dot product
           (rk_als_pair_scores) and the lists go through a ragged top-k (rk_als_pairs_topk).  Only a
           MatrixFactorization with activation 'none' on the fused engine (the state ``fold_in`` accepts, at any
           embedding size the kernel takes), rows of at most ``PAIRS_MAX_ROW`` candidates.

Their score BITS may differ: the strip decode multiplies split fp16 planes, the pair kernel plain f32.  On
near-ties the ids may therefore differ between the routes.  ``route="auto"`` takes "pairs" whenever it is legal.

``Recoder.recommend_filtered``, ``Recoder.rerank`` and ``recommender.FilteredRecommender`` are the public entry
points.  The checks in ``check_serving`` and ``Filters`` run on the host before any GPU work.
"""
import ctypes
import numbers

import numpy as np
import scipy.sparse as sp
import torch

from . import _als_lib
from ._lib import RkBlock, ptr
from .device import cdiv, current_stream
from .nn import MatrixFactorization

PAIRS_MAX_ROW = _als_lib.PAIRS_TOPK_MAX_ROW      # rk_als_pairs_topk_max_row()
TOPK_MAX_K = 1024                                # rk_topk_max_k()
ROUTES = ("auto", "mask", "pairs")


def _catalogue_bits(name, items, n_items):
  """``allow_items`` / ``deny_items`` as a bool array [n_items] (None stays None): a boolean array of that length,
  or a 1-D integer array of ids in [0, n_items), duplicates allowed."""
  if items is None:
    return None
  a = np.asarray(items)
  if a.ndim != 1:
    raise ValueError("%s must be a 1-D array of item ids or a boolean array of length %d (got shape %r)"
                     % (name, n_items, a.shape))
  if a.dtype == np.bool_:
    if a.shape[0] != n_items:
      raise ValueError("a boolean %s must have one entry per item: %d (got %d)" % (name, n_items, a.shape[0]))
    return a.copy()
  if a.size == 0:
    return np.zeros(n_items, dtype=bool)
  if not np.issubdtype(a.dtype, np.integer):
    raise ValueError("%s must hold integer item ids or booleans (got dtype %s)" % (name, a.dtype))
  if a.min() < 0 or a.max() >= n_items:
    raise ValueError("%s holds an id outside [0, %d) (got %d .. %d)" % (name, n_items, a.min(), a.max()))
  out = np.zeros(n_items, dtype=bool)
  out[a] = True
  return out


def pack_bits(flags):
  """bool [n] -> uint32 [ceil(n / 32)]: item c is bit c & 31 of word c >> 5, zeros past n."""
  n = len(flags)
  padded = np.zeros(cdiv(max(n, 1), 32) * 32, dtype=np.uint8)
  padded[:n] = flags
  return np.packbits(padded, bitorder="little").view(np.uint32).copy()


def _row_lists(name, matrix, rows, n_items):
  """``user_allow`` / ``user_deny`` as (indptr int64 [rows + 1], ids int32), sorted and unique within a row: only the
  pattern counts, an explicit zero is present."""
  if matrix is None:
    return None
  if not sp.issparse(matrix):
    raise ValueError("%s must be a scipy sparse matrix [%d, %d]" % (name, rows, n_items))
  if tuple(matrix.shape) != (rows, n_items):
    raise ValueError("%s must have shape (%d, %d): one row per user of the batch, one column per item (got %r)"
                     % (name, rows, n_items, tuple(matrix.shape)))
  m = sp.csr_matrix(matrix, copy=True)
  if m.nnz and (m.indices.min() < 0 or m.indices.max() >= n_items):
    raise ValueError("%s holds a column outside [0, %d)" % (name, n_items))
  m.data = np.ones(m.nnz, dtype=np.int8)               # (before the duplicates are summed: a zero stays an entry)
  m.sum_duplicates()
  m.sort_indices()
  return m.indptr.astype(np.int64), m.indices.astype(np.int32)


class Filters(object):
  """The five filters of a call, checked and canonicalised on the host for a batch of ``rows`` users over
  ``n_items`` items (ValueError: a wrong shape or type, an id out of range)."""

  def __init__(self, rows, n_items, filter_seen=True, allow_items=None, deny_items=None, user_allow=None,
               user_deny=None):
    self.rows, self.n_items = int(rows), int(n_items)
    self.filter_seen = bool(filter_seen)
    self.allow = _catalogue_bits("allow_items", allow_items, self.n_items)
    self.deny = _catalogue_bits("deny_items", deny_items, self.n_items)
    self.user_allow = _row_lists("user_allow", user_allow, self.rows, self.n_items)
    self.user_deny = _row_lists("user_deny", user_deny, self.rows, self.n_items)
    self.max_row = 0
    if self.user_allow is not None and self.rows:
      self.max_row = int(np.diff(self.user_allow[0]).max())

  def only_candidates(self):
    """True when ``user_allow`` is the one filter set: the pair route then needs no bitmap."""
    return not self.filter_seen and self.allow is None and self.deny is None and self.user_deny is None


def pairs_legal(recoder, filters):
  """None when ``route="pairs"`` can serve the call, else the reason it cannot."""
  model = recoder.model
  if filters.user_allow is None:
    return "route='pairs' ranks the candidates of user_allow, which is not given"
  if not isinstance(model, MatrixFactorization) or model.activation_type != "none":
    return "route='pairs' serves a MatrixFactorization with activation_type='none', not %s" % (
        type(model).__name__ if not isinstance(model, MatrixFactorization)
        else "activation %r" % (model.activation_type,))
  if recoder._use_generic():
    return "route='pairs' needs the fused HIP engine (optimizer_type='adam', an embedding size that is a multiple of 4)"
  h = model.embedding_size
  if isinstance(h, bool) or not isinstance(h, numbers.Integral) or h < 4 or h % 4 or h > _als_lib.IALS_MAX_H:
    return "route='pairs' takes embedding sizes that are multiples of 4 in [4, %d] (got %r)" % (_als_lib.IALS_MAX_H, h)
  if filters.max_row > PAIRS_MAX_ROW:
    return "route='pairs' ranks at most %d candidates a user (a row of user_allow has %d)" % (
        PAIRS_MAX_ROW, filters.max_row)
  return None


def check_serving(recoder, k, route):
  """What ``recommend_filtered`` refuses whatever the filters are; returns k as an int."""
  if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
    raise ValueError("num_recommendations must be an integer >= 1 (got %r)" % (k,))
  if route not in ROUTES:
    raise ValueError("route must be one of %s (got %r)" % (", ".join(repr(r) for r in ROUTES), route))
  if k > TOPK_MAX_K:
    raise ValueError("recommend_filtered takes at most %d recommendations (got %d): there is no dense fallback"
                     % (TOPK_MAX_K, k))
  own_scores = recoder._scores_from_csr_rows() or recoder._scores_from_user_ids()
  if recoder._use_generic() and not own_scores:
    raise ValueError("recommend_filtered serves on the fused HIP engine (optimizer_type='adam', a first hidden / "
                     "embedding size that is a multiple of 4, a fused activation and loss), not on the generic "
                     "torch-autograd engine: there is no dense fallback")
  return int(k)


def pick_route(recoder, filters, route):
  reason = pairs_legal(recoder, filters)
  if route == "pairs" and reason is not None:
    raise ValueError(reason)
  return "pairs" if route != "mask" and reason is None else "mask"


class MaskBlock(object):
  """A deny bitmap [rows, ldw] (int32 words) dressed as the unsampled ``rk_block_t`` that ``rk_topk_masked`` reads:
  ``bits_rc`` with ``implicit`` set, so that a set bit masks whatever values the users' own block stores."""

  def __init__(self, bits, rows, n_items, ldw):
    self.bits = bits
    self.c = RkBlock(S_cap=rows, n_cap=n_items, n_items=n_items, ldw_rc=ldw, implicit=1, bits_rc=ptr(bits))
    self.ref = ctypes.byref(self.c)


def _dev(a, device):
  return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def build_mask(filters, dcsr, device):
  """(bits int32 [rows, ldw], eligible int32 [rows], ldw) on the device: rk_als_serve_mask over the filters and,
  with ``filter_seen``, the batch's ``DeviceCSR``."""
  B, n = filters.rows, filters.n_items
  ldw = cdiv(n, 32)
  bits = torch.empty((max(B, 1), ldw), dtype=torch.int32, device=device)
  eligible = torch.empty(max(B, 1), dtype=torch.int32, device=device)
  allow = None if filters.allow is None else _dev(pack_bits(filters.allow).view(np.int32), device)
  deny = None if filters.deny is None else _dev(pack_bits(filters.deny).view(np.int32), device)
  ua = None if filters.user_allow is None else tuple(_dev(a, device) for a in filters.user_allow)
  ud = None if filters.user_deny is None else tuple(_dev(a, device) for a in filters.user_deny)
  seen = dcsr if filters.filter_seen else None
  lists = lambda p: (None, None, 0) if p is None else (ptr(p[0]), ptr(p[1]), int(p[1].numel()))
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_serve_mask(
      B, n, ldw, ptr(seen.indptr) if seen is not None else None, ptr(seen.indices) if seen is not None else None,
      ptr(seen.data) if seen is not None else None, seen.nnz if seen is not None else 0, ptr(allow), ptr(deny),
      *lists(ua), *lists(ud), ptr(bits), ptr(eligible), current_stream()), "rk_als_serve_mask")
  return bits, eligible, ldw


def pair_scores(indptr, ids, max_row, z, Y, bias, deny=None, ldw=0, out=None):
  """rk_als_pair_scores: f32 [nnz] scores of the ragged lists (int64 ``indptr`` [B + 1], int32 ``ids``, on the
  device) of the rows of ``z`` [B, h] against ``Y`` [n, h] and ``bias`` [n] or None."""
  B, h = int(z.shape[0]), int(z.shape[1])
  nnz = int(ids.numel())
  assert z.dtype == Y.dtype == torch.float32 and z.stride(1) == 1 and Y.stride(1) == 1 and Y.shape[1] == h
  assert indptr.dtype == torch.int64 and indptr.numel() == B + 1 and ids.dtype == torch.int32
  if z.stride(0) % 4 or z.data_ptr() % 16:
    z = z.contiguous().clone()
  out = torch.empty(max(nnz, 1), dtype=torch.float32, device=Y.device) if out is None else out
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_pair_scores(ptr(indptr), ptr(ids), nnz, B, int(max_row), ptr(z), z.stride(0) if B else h,
                                        ptr(Y), Y.stride(0), Y.shape[0], h, ptr(bias), ptr(deny), int(ldw), ptr(out),
                                        current_stream()), "rk_als_pair_scores")
  return out[:nnz]


def pairs_topk(indptr, ids, scores, max_row, n_items, k, deny=None, ldw=0):
  """rk_als_pairs_topk: (ids int64 [B, k], scores f32 [B, k], count int32 [B]) on the device."""
  B = int(indptr.numel()) - 1
  dev = indptr.device
  out_idx = torch.empty((B, k), dtype=torch.int64, device=dev)
  out_val = torch.empty((B, k), dtype=torch.float32, device=dev)
  count = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
  lib = _als_lib.load()
  _als_lib.check(lib.rk_als_pairs_topk(ptr(indptr), ptr(ids), ptr(scores), int(ids.numel()), B, int(max_row),
                                       int(n_items), ptr(deny), int(ldw), int(k), ptr(out_idx), ptr(out_val), k,
                                       ptr(count), current_stream()), "rk_als_pairs_topk")
  return out_idx, out_val, count[:B]


def recommend_filtered_device(recoder, users_interactions, k, filter_seen=True, allow_items=None, deny_items=None,
                              user_allow=None, user_deny=None, route="auto", user_rows=None, ws=None):
  """``Recoder.recommend_filtered`` before its copy to the host: (ids int64 [B, k], scores f32 [B, k]) on the
  device, nothing synchronised."""
  k = check_serving(recoder, k, route)
  m = users_interactions.interactions_matrix
  B = int(m.shape[0])
  n_items = int(recoder.num_items if recoder.num_items is not None else m.shape[1])
  if k > n_items:
    raise ValueError("num_recommendations (%d) exceeds the number of items (%d)" % (k, n_items))
  filters = Filters(B, n_items, filter_seen, allow_items, deny_items, user_allow, user_deny)
  route = pick_route(recoder, filters, route)
  if user_rows is not None and (recoder._scores_from_csr_rows() or recoder._scores_from_user_ids()):
    raise ValueError("user_rows are scored against an item table: %s has none" % type(recoder.model).__name__)
  recoder.model.eval()
  recoder._check_ranges()
  blk, B, n_items = recoder._input_block(users_interactions, ws, lookup_users=user_rows is None)
  ws = recoder._eval_ws if ws is None else ws
  dcsr = ws["dcsr"]
  device = recoder.device
  if route == "pairs":
    engine = recoder._engine()
    if user_rows is None:
      h = engine.h[0]
      z = engine.encode_eval(blk, 0, B).reshape(-1)[:B * h].view(B, h)      # (the engine's flat buffer: rows h apart)
    else:
      assert tuple(user_rows.shape) == (B, engine.h[0]) and user_rows.dtype == torch.float32
      z = user_rows.contiguous()
    deny, ldw = None, 0
    if not filters.only_candidates():
      deny, _, ldw = build_mask(filters, dcsr, device)
    indptr, ids = (_dev(a, device) for a in filters.user_allow)
    model = recoder.model
    scores = pair_scores(indptr, ids, filters.max_row, z, model.item_embedding_layer.weight.data, model.bias.data,
                         deny, ldw)
    out_idx, out_val, _ = pairs_topk(indptr, ids, scores, filters.max_row, n_items, k, deny, ldw)
    return out_idx, out_val
  bits, eligible, ldw = build_mask(filters, dcsr, device)
  mask = MaskBlock(bits, B, n_items, ldw)
  ids, _, vals = recoder._recommend_device(users_interactions, k, ws=ws, inputs=(blk, B, n_items, dcsr),
                                           user_rows=user_rows, seen=mask, with_scores=True)
  # the padding, from the device's count of eligible items: rank i of row r is real when i < eligible[r]
  pad = torch.arange(k, device=device)[None, :] >= eligible[:B, None]
  return ids.masked_fill(pad, -1), vals.masked_fill(pad, float("-inf"))


def recommend_filtered(recoder, users_interactions, k, return_scores=False, **kw):
  ids, vals = recommend_filtered_device(recoder, users_interactions, k, **kw)
  ids = ids.cpu().numpy().copy()
  if return_scores:
    return ids, vals.cpu().numpy().copy()
  return ids
