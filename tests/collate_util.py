"""What a collation leaves in a ``rk_block_t`` (include/recoder_hip.h), restated in numpy, and the inputs the
collation tests feed it.

* collate_ref: every array of the block after ``rk_collate`` / ``rk_collate_at`` / ``rk_collate_at_multi`` of one
  batch of user rows -- the item set in ``np.unique`` order, the rows in batch order (a user may appear more than
  once), the entries in the order the CSR stores them, the two bitmaps and the prefix popcounts, and the header's
  truncated form when the block is smaller than the batch: the first ``n_cap`` items of the set are kept, an entry
  of any other item has column 0 and value 0 and no bit; the row pointers are clamped at ``nnz_cap`` and a row keeps
  the first entries its clamped range has room for.  The item set is that of ALL stored entries of the rows either way.
  ``gcols`` is the stored item id of every kept entry (== ``items[cols]`` in a block that is large enough).
* need_lists_ref / densify_ref: ``rk_lazy_need_lists`` for one pair of pos maps and ``rk_densify``.
* the case builders: matrices with given rows, the item ids on both sides of every scan boundary, the batch that
  mixes empty, light and heavy rows, and the two wide-bitmap matrices.

Nothing here touches torch.cuda: tests/test_collate_host.py holds collate_ref to oracle.recoder_oracle.collate and to
its own invariants before tests/test_collate.py judges a kernel by it.
"""
import numpy as np
import scipy.sparse as sp

SCAN_CHUNK = 2048            # RK_SCAN_CHUNK: items per workgroup of the chunked scans
SCAN_ROUND = 4096            # items per round of the one-workgroup scan
SMALL_SCAN_MAX = 1 << 16     # catalogues up to here take the one-workgroup (or look-back) scan
BUILD_HEAVY = 512            # rows past this many entries are built by four waves
SEG_WORDS = 2048             # bitmap words a wave assembles at a time
COLLATE_MULTI = 8            # RK_COLLATE_MULTI
NEED_LIST_MAX_ITEMS = 64 * SCAN_CHUNK


def cdiv(a, b):
  return -(-a // b)


def _pack_rows(dense):
  """[rows, 32 * words] bool -> [rows, words] uint32, bit c & 31 of word c >> 5 = dense[:, c]."""
  return np.ascontiguousarray(np.packbits(dense, axis=1, bitorder="little")).view("<u4").astype(np.uint32)


def collate_ref(indptr, indices, data, users, negative_sampling, S_cap, nnz_cap, n_cap, n_items, implicit=False,
                ldw_rc=None, ldw_cr=None):
  """The block after collating rows `users` of the CSR (indptr, indices, data); see the module docstring.

  Returns a dict: S, n_b, nnz, wr (bitmap words in use), counts [72] (slots 4 and 7 are not collation's: 0 here),
  indptr [S + 1], cols / gcols / vals [nnz], items [n_b], pos [n_items], bits_rc / pref_rc [S, wr],
  bits_cr [n_cap, ldw_cr]."""
  indptr = np.asarray(indptr, dtype=np.int64)
  indices = np.asarray(indices, dtype=np.int64)
  users = np.asarray(users, dtype=np.int64).reshape(-1)
  S = len(users)
  assert 1 <= S <= S_cap
  ldw_rc = cdiv(n_cap, 32) if ldw_rc is None else ldw_rc
  ldw_cr = cdiv(S_cap, 32) if ldw_cr is None else ldw_cr
  deg = indptr[users + 1] - indptr[users]
  true_nnz = int(deg.sum())
  ptr_b = np.minimum(np.concatenate([[0], np.cumsum(deg)]), nnz_cap)
  kept = np.diff(ptr_b)
  nnz = int(ptr_b[-1])
  src = np.concatenate([indptr[u] + np.arange(k) for u, k in zip(users, kept)] + [np.zeros(0, np.int64)])
  src = src.astype(np.int64)
  rows = np.repeat(np.arange(S), kept)
  gitem = indices[src]
  vals = np.ones(nnz, np.float32) if implicit or data is None else np.asarray(data, dtype=np.float32)[src]
  if negative_sampling:
    stored = np.concatenate([indices[indptr[u]:indptr[u + 1]] for u in users] + [np.zeros(0, np.int64)])
    item_set = np.unique(stored)
  else:
    item_set = np.arange(n_items, dtype=np.int64)
  n_all = len(item_set)
  n_b = min(n_all, n_cap)
  items = item_set[:n_b]
  pos = np.full(n_items, -1, dtype=np.int64)
  pos[items] = np.arange(n_b)
  col = pos[gitem]
  live = col >= 0
  wr = cdiv(n_b, 32)
  dense = np.zeros((S, wr * 32), dtype=bool)
  dense[rows[live], col[live]] = True
  bits_rc = _pack_rows(dense).reshape(S, wr)
  per_word = dense.reshape(S, wr, 32).sum(axis=2)
  pref_rc = np.cumsum(per_word, axis=1) - per_word
  dense_t = np.zeros((n_cap, ldw_cr * 32), dtype=bool)
  dense_t[:n_b, :S] = dense[:, :n_b].T
  counts = np.zeros(72, dtype=np.int32)
  counts[0], counts[1], counts[2], counts[3] = n_b, nnz, cdiv(n_b, 32) * 32, S
  counts[5] = n_all if n_all > n_cap else 0
  counts[6] = true_nnz if true_nnz > nnz_cap else 0
  return dict(S=S, n_b=n_b, nnz=nnz, wr=wr, counts=counts, indptr=ptr_b.astype(np.int32),
              cols=np.where(live, col, 0).astype(np.int32), gcols=gitem.astype(np.int32),
              vals=np.where(live, vals, np.float32(0)).astype(np.float32),
              items=items.astype(np.int32), pos=pos.astype(np.int32), bits_rc=bits_rc,
              pref_rc=pref_rc.astype(np.int32), bits_cr=_pack_rows(dense_t).reshape(n_cap, ldw_cr))


def need_lists_ref(pos_a, pos_b):
  """The ascending ids that either pos map holds (rk_lazy_need_lists, one pair of consecutive blocks)."""
  return np.nonzero((np.asarray(pos_a) >= 0) | (np.asarray(pos_b) >= 0))[0].astype(np.int32)


def densify_ref(ref, row_off, B, n):
  """Rows [row_off, row_off + B) of a collate_ref block as a dense [B, n] float32 matrix (rk_densify)."""
  out = np.zeros((B, n), dtype=np.float32)
  for r in range(B):
    a, b = ref["indptr"][row_off + r], ref["indptr"][row_off + r + 1]
    out[r, ref["cols"][a:b]] = ref["vals"][a:b]
  return out


# ------------------------------------------------------------------ case builders
def ratings(rng, n):
  """n nonzero float32 values in (-5, 5): negative and non-integer ones among them."""
  v = (rng.rand(n) * 10 - 5).astype(np.float32)
  v[np.abs(v) < 0.05] = np.float32(0.375)
  return v


def csr_from_rows(rows, n_items, seed=0, implicit=False):
  """A [len(rows), n_items] scipy CSR whose row u stores the item ids rows[u] (distinct; sorted here), with
  ratings() values, or 1.0 throughout."""
  rng = np.random.RandomState(seed)
  rows = [np.unique(np.asarray(r, dtype=np.int64)) for r in rows]
  indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
  indices = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)
  assert len(indices) == 0 or (indices.min() >= 0 and indices.max() < n_items)
  data = np.ones(len(indices), np.float32) if implicit else ratings(rng, len(indices))
  return sp.csr_matrix((data, indices, indptr), shape=(len(rows), n_items))


def random_rows(rng, lengths, n_items):
  return [np.sort(rng.choice(n_items, size=int(n), replace=False)) for n in lengths]


def boundary_items(n_items):
  """Item 0, item n_items - 1 and both sides of every 2048 and 4096 boundary of the catalogue."""
  ids = {0, n_items - 1}
  for b in range(SCAN_CHUNK, n_items + 1, SCAN_CHUNK):
    ids.update((b - 1, b))
  return np.array(sorted(i for i in ids if 0 <= i < n_items), dtype=np.int64)


def scan_case(n_items, seed=0, n_rows=5):
  """A handful of rows over a catalogue of n_items whose stored ids cover boundary_items(n_items): (csr, users)."""
  rng = np.random.RandomState(seed + n_items)
  edge = boundary_items(n_items)
  rows = [[] for _ in range(n_rows)]
  for k, it in enumerate(edge):
    rows[k % (n_rows - 1)].append(it)              # (the last row takes random ids only)
    if k % 3 == 0:
      rows[(k + 2) % n_rows].append(it)            # (an id in two rows)
  extra = min(n_items, 40)
  for r in range(n_rows):
    rows[r].extend(rng.choice(n_items, size=rng.randint(0, extra + 1), replace=False))
  csr = csr_from_rows(rows, n_items, seed)
  users = rng.permutation(n_rows).astype(np.int64)
  assert np.isin(edge, csr.indices).all()
  return csr, users


# the mixed batch (tests/test_collate.py, rows): one entry per batch row, a row length or a user name
MIX_ROWS = [
    0, 1, 63, 64,                       # workgroup 0: an empty row first
    65, 511, 513, 512,                  # workgroup 1: exactly one heavy row, in wave 2
    1100, 600, 513, "heavy",            # workgroup 2: four heavy rows
    0, 0, "light", "heavy",             # workgroup 3: two empty rows side by side
    "light", 2, "light", "heavy",       # workgroup 4
    5, 9, 0,                            # workgroup 5: three rows, the last one empty
]
MIX_NAMED = {"light": 20, "heavy": 700}
MIX_ITEMS = 3000


def mix_case(seed=0):
  """(csr, users): batch row r is a user of MIX_ROWS[r] entries, or the named user (three times each: one light,
  one heavy).  User ids are scattered over a larger matrix with other rows in between."""
  rng = np.random.RandomState(seed)
  n_users = 2 * len(MIX_ROWS)
  ids = rng.permutation(n_users)
  named = {name: int(ids[-1 - k]) for k, name in enumerate(MIX_NAMED)}
  lengths = np.zeros(n_users, dtype=np.int64)
  users = []
  for r, what in enumerate(MIX_ROWS):
    if isinstance(what, str):
      u = named[what]
      lengths[u] = MIX_NAMED[what]
    else:
      u = int(ids[r])
      lengths[u] = what
    users.append(u)
  for u in ids[len(MIX_ROWS):n_users - len(MIX_NAMED)]:     # (rows of the matrix that the batch leaves out)
    lengths[u] = rng.randint(0, 30)
  rows = random_rows(rng, lengths, MIX_ITEMS)
  rows[users[1]] = np.array([MIX_ITEMS - 1])                # (the one-entry row holds the last item)
  rows[users[2]][0] = 0                                     # (item 0 is stored, too)
  return csr_from_rows(rows, MIX_ITEMS, seed), np.array(users, dtype=np.int64)


WIDE_ITEMS = 72000


def wide_case(n_rows, own, stripe, extra, seed=0):
  """n_rows rows over WIDE_ITEMS items: row r stores `own` ids of its stripe [r * stripe, (r + 1) * stripe) and
  `extra` ids from anywhere, so the batch's item set is wider than 65 536 ids (SEG_WORDS bitmap words)."""
  rng = np.random.RandomState(seed)
  assert n_rows * stripe <= WIDE_ITEMS and own <= stripe
  rows = []
  for r in range(n_rows):
    mine = r * stripe + rng.choice(stripe, size=own, replace=False)
    rows.append(np.union1d(mine, rng.choice(WIDE_ITEMS, size=extra, replace=False)))
  return csr_from_rows(rows, WIDE_ITEMS, seed), rng.permutation(n_rows).astype(np.int64)


def degrees(csr, users):
  return np.diff(csr.indptr)[np.asarray(users)]
