"""Recoder.recommend's three kernels restated in numpy, and the inputs their tests feed them.

* order_key / key_value: the total order of csrc/topk.hip (f2key / key2f) -- float32 by value, both zeros
  ONE value, the canonical quiet NaN (0x7fc00000) above +inf as torch.topk ranks it.  NaNs with the sign
  bit set are outside the contract; no generator here makes one.
* masked_topk: rk_topk_masked -- seen items (stored value > 0) at -inf, order (key descending, item id
  ascending).  The values it returns are the keys' values: a selected -0.0 reads +0.0.
* pairs_topk: rk_topk_pairs -- the same order over a row's first cnt (score, id) pairs, with the two status
  bits and the rows they leave unwritten.
* filter_survivors: the epilogue of rk_decode_filter_planes -- what reaches the row's threshold (IEEE >=)
  and is not seen, as a set of (item id, score bits).

Nothing here touches torch.cuda: tests/test_recommend_host.py holds these restatements to numpy's stable
argsort and to torch.topk on the CPU, and runs every generator's own assertions.
"""
import numpy as np
import scipy.sparse as sp

CANON_NAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]
CHUNK, WAVE = 256, 64              # columns per pass of rk_topk_masked's collection / per wave of it
KEY_TOP = np.uint32(0xffffffff)


def bits(x):
  return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def order_key(x):
  """float32 array -> uint32 keys: a < b (by value) <=> key(a) < key(b); -0.0 and +0.0 share one key."""
  u = bits(x).copy()
  u[u == np.uint32(0x80000000)] = 0
  neg = (u & np.uint32(0x80000000)) != 0
  return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_value(key):
  """The float32 a key stands for (+0.0 for the zeros)."""
  key = np.ascontiguousarray(key, dtype=np.uint32)
  pos = (key & np.uint32(0x80000000)) != 0
  return np.where(pos, key & np.uint32(0x7fffffff), ~key).astype(np.uint32).view(np.float32)


def seen_mask(seen, items):
  """[rows, len(items)] bool: the stored values > 0 of `seen` (scipy CSR over the whole catalogue)."""
  return np.asarray(sp.csr_matrix(seen)[:, np.asarray(items)].todense()) > 0


def masked_keys(scores, seen=None, col_off=0, col_stride=1):
  scores = np.asarray(scores, dtype=np.float32)
  if seen is not None:
    items = col_off + np.arange(scores.shape[1], dtype=np.int64) * col_stride
    scores = np.where(seen_mask(seen, items), np.float32(-np.inf), scores)
  return order_key(scores)


def masked_topk(scores, k, seen=None, col_off=0, col_stride=1):
  """ids [B, k] int64 and values [B, k] float32 of rk_topk_masked: score column c is item
  col_off + c * col_stride, row r of `seen` masks row r of `scores`."""
  key = masked_keys(scores, seen, col_off, col_stride)
  cols = np.argsort(KEY_TOP - key, axis=1, kind="stable")[:, :k]      # key descending, column ascending
  return col_off + cols.astype(np.int64) * col_stride, key_value(np.take_along_axis(key, cols, 1))


def pairs_topk(val, idx, cnt, cap, k):
  """ids [B, k] int64 (-1 in unwritten rows), written [B] bool, status: a row with cnt > cap sets bit 1,
  one with cnt < k bit 2; neither is written."""
  val = np.asarray(val, dtype=np.float32).reshape(len(cnt), -1)
  idx = np.asarray(idx).reshape(len(cnt), -1)
  B = len(cnt)
  ids = np.full((B, k), -1, dtype=np.int64)
  written = np.zeros(B, dtype=bool)
  status = 0
  for r in range(B):
    c = int(cnt[r])
    if c > cap:
      status |= 1
    elif c < k:
      status |= 2
    else:
      order = np.lexsort((idx[r, :c], KEY_TOP - order_key(val[r, :c])))   # key descending, then id ascending
      ids[r] = idx[r, :c][order[:k]]
      written[r] = True
  return ids, written, status


def filter_survivors(S, thr, seen=None, col_off=0, row_off=0):
  """Per row of S [B, n] the set {(item id, score bits)} with S >= thr[row] and item col_off + c not a
  seen item of row row_off + r of `seen`."""
  S = np.asarray(S, dtype=np.float32)
  B, n = S.shape
  keep = S >= np.asarray(thr, dtype=np.float32)[:, None]              # (a NaN on either side: False)
  if seen is not None:
    keep &= ~seen_mask(sp.csr_matrix(seen)[row_off:row_off + B], col_off + np.arange(n))
  u = bits(S)
  return [set(zip((col_off + np.nonzero(keep[r])[0]).tolist(), u[r][keep[r]].tolist())) for r in range(B)]


# ----------------------------------------------------------------------------------------- inputs
def threshold_ties(key_row, k):
  """Columns holding the k-th largest key of a row, and how many of them (the lowest columns) a top k takes."""
  key_row = np.asarray(key_row, dtype=np.uint32)
  T = np.sort(key_row)[::-1][k - 1]
  cols = np.nonzero(key_row == T)[0]
  return cols, k - int((key_row > T).sum())


def tie_straddles(key_row, k):
  """(chunk, wave): do the TAKEN ties of the threshold key lie on both sides of a 256-column chunk boundary /
  of a 64-lane wave boundary (at least two of them, one on each side)?"""
  cols, need = threshold_ties(key_row, k)
  taken = cols[:need]
  return len(set((taken // CHUNK).tolist())) >= 2, len(set((taken // WAVE).tolist())) >= 2


TIE_COLUMNS = (62, 63, 64, 65, 254, 255, 256, 257)
SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39, 3.4028235e38,
                     -3.4028235e38, 1.17549435e-38], dtype=np.float32)
FAMILIES = ("normal", "normal", "eighths", "eighths", "constant", "few_unseen", "specials", "ties")
FEW, SPEC, TIES = FAMILIES.index("few_unseen"), FAMILIES.index("specials"), FAMILIES.index("ties")


def tie_row(rng, n, k):
  """A row whose threshold key is tied at TIE_COLUMNS (and at the row's last two columns): the top k takes the
  ties up to column 256 and leaves the later ones, wherever n and k leave room for that."""
  cols = np.array(sorted(set(c for c in TIE_COLUMNS + (n - 2, n - 1) if 0 <= c < n)))
  need = min(k, int((cols <= CHUNK).sum()))
  need = max(need, k - (n - len(cols)))                               # (k close to n: more of them are taken)
  row = rng.uniform(-1.0, 0.5, size=n).astype(np.float32)
  row[cols] = 1.0
  free = np.setdiff1d(np.arange(n), cols)
  above = rng.choice(free, size=k - need, replace=False)
  row[above] = (2.0 + rng.permutation(k - need)).astype(np.float32)
  got_cols, got_need = threshold_ties(order_key(row), k)
  assert np.array_equal(got_cols, cols) and got_need == need
  chunk, wave = tie_straddles(order_key(row), k)
  if n > CHUNK + 1 and k >= 7:
    assert chunk and need >= 2
    assert k == n or cols.max() <= CHUNK or need < len(cols)          # (the cut falls INSIDE the ties)
  if n > WAVE + 1 and k >= 3:
    assert wave
  return row


def topk_case(n, k, seen_kind, col_off=0, col_stride=1, row_off=0, seed=0):
  """One launch of rk_topk_masked: scores [B, n] with one row (or two) of every data family and the seen matrix
  (None, or scipy CSR [row_off + B + 2, catalogue]; "explicit" stores negatives and values > 1 too).  Row FEW has
  max(k - 2, 0) unseen items where there is a seen matrix (-inf scores stand in for the seen ones without)."""
  rng = np.random.RandomState(1000003 * seed + 7919 * n + k)
  B = len(FAMILIES)
  sc = rng.randn(B, n).astype(np.float32)
  for r, fam in enumerate(FAMILIES):
    if fam == "eighths":
      sc[r] = rng.randint(-12, 12, size=n) / 8.0                      # (both zeros' neighbourhood, many ties)
    elif fam == "constant":
      sc[r] = 0.375
    elif fam == "specials":
      m = min(n, 3 * len(SPECIALS))
      where = np.sort(rng.choice(n, size=m, replace=False))
      sc[r, where] = np.resize(SPECIALS, m)[rng.permutation(m)]
      if n >= 2:                                                      # -0.0 at a LOWER column than a +0.0
        a, b = np.sort(rng.choice(n, size=2, replace=False))
        sc[r, a], sc[r, b] = -0.0, 0.0
    elif fam == "ties":
      sc[r] = tie_row(rng, n, k)
  n_cat = col_off + (n - 1) * col_stride + 1 + 5
  items = col_off + np.arange(n) * col_stride
  unseen_few = max(k - 2, 0)
  hidden = np.sort(rng.choice(n, size=n - unseen_few, replace=False))  # row FEW: the columns that are masked
  if seen_kind is None:
    sc[FEW, hidden] = -np.inf
    assert int((sc[FEW] > -np.inf).sum()) < k
    seen = None
  else:
    rows_total = row_off + B + 2
    dens = min(0.3, 60.0 / n_cat)
    m = sp.random(rows_total, n_cat, density=dens, random_state=rng, format="coo", dtype=np.float32)
    # (row FEW is written below; row TIES keeps its ties and what ranks above them unseen: the cut stays where it is)
    tied = items[sc[TIES] >= 1.0]
    keep = (m.row != row_off + FEW) & ~((m.row == row_off + TIES) & np.isin(m.col, tied))
    m = sp.coo_matrix((m.data[keep], (m.row[keep], m.col[keep])), shape=m.shape)
    rows = np.concatenate([m.row, np.full(len(hidden), row_off + FEW)])
    cols = np.concatenate([m.col, items[hidden]])
    if seen_kind == "implicit":
      vals = np.ones(len(rows), np.float32)
    else:
      vals = rng.choice([-2.0, 1.0, 3.0], size=len(rows)).astype(np.float32)   # negatives: stored, NOT masked
      vals[len(m.row):] = rng.choice([1.0, 3.0], size=len(hidden))
      free = np.setdiff1d(np.arange(n), hidden)                       # stored negatives on row FEW's unseen items
      rows = np.concatenate([rows, np.full(len(free), row_off + FEW)])
      cols = np.concatenate([cols, items[free]])
      vals = np.concatenate([vals, np.full(len(free), -2.0, np.float32)])
    seen = sp.coo_matrix((vals, (rows, cols)), shape=(rows_total, n_cat)).tocsr()
    seen.sum_duplicates()
    seen.eliminate_zeros()
    seen.sort_indices()
    few = seen_mask(seen[row_off + FEW], items)[0]
    assert int((~few).sum()) == unseen_few < k                        # the row really has fewer than k unseen items
  keys = masked_keys(sc, None if seen is None else seen[row_off:row_off + B], col_off, col_stride)
  if n > CHUNK + 1 and 7 <= k < n:
    assert tie_straddles(keys[TIES], k)[0]                            # (also after the mask; k == n takes all)
  return sc, seen


def pairs_case(cap, k, kind, seed=0):
  """One launch of rk_topk_pairs: val / idx [B, cap], cnt [B].  Rows with cnt == k, cnt == cap and counts in
  between; `kind` adds the rows that set a status bit ("over": cnt == cap + 1, "under": cnt == k - 1, "both").
  Scores are quantised (equal scores under different ids); entries at and past cnt are NaN / -1."""
  rng = np.random.RandomState(7 * cap + 31 * k + 1009 * seed + len(kind))
  cnts = [k, cap, (k + cap) // 2, int(rng.randint(k, cap + 1))]
  bad = []
  if kind in ("over", "both"):
    bad.append(len(cnts))
    cnts.append(cap + 1)
  if kind in ("under", "both"):
    bad.append(len(cnts))
    cnts.append(k - 1)
  cnts += [k, cap]
  cnt = np.asarray(cnts, dtype=np.int32)
  B = len(cnt)
  n_ids = 3 * cap + 10
  val = np.full((B, cap), np.nan, dtype=np.float32)
  idx = np.full((B, cap), -1, dtype=np.int32)
  for r in range(B):
    c = min(int(cnt[r]), cap)
    val[r, :c] = rng.randint(-6, 6, size=c) / 4.0
    idx[r, :c] = rng.choice(n_ids, size=c, replace=False)
  want = 0 if kind == "good" else {"over": 1, "under": 2, "both": 3}[kind]
  assert pairs_topk(val, idx, cnt, cap, k)[2] == want
  assert (~pairs_topk(val, idx, cnt, cap, k)[1]).sum() == len(bad)
  return val, idx, cnt, n_ids


# (B, h, n) of the filter tests: every B of {1, 37, 130}, h of {4, 36, 64, 200} and n of {97, 700, 2049}
FILTER_SHAPES = [(1, 4, 97), (37, 36, 700), (130, 64, 2049), (1, 200, 700), (37, 64, 97), (130, 4, 700),
                 (37, 200, 2049), (130, 36, 97)]
ORDER_STATS = (1, 5, 40, 100)


def filter_operands(B, h, n, seed=0):
  """Z [B, h], W [n, h], b [n] inside the documented split range (|Z| < 2048 at scale 32, |W| < 512 at 128)."""
  rng = np.random.RandomState(97 * B + 13 * h + n + seed)
  Z = np.tanh(rng.randn(B, h)).astype(np.float32)
  W = (0.2 * rng.randn(n, h)).astype(np.float32)
  b = (0.1 * rng.randn(n)).astype(np.float32)
  assert np.abs(Z).max() < 2048 and np.abs(W).max() < 512
  return Z, W, b


def filter_thresholds(S, rot=0):
  """thr [B]: row r + rot == 0 at -inf, 1 at +inf, 2 at NaN, every other row at an order statistic of ITS row of
  S (the q-th largest, q through ORDER_STATS and n // 2), so that a score equal to the threshold occurs."""
  S = np.asarray(S, dtype=np.float32)
  B, n = S.shape
  thr = np.empty(B, dtype=np.float32)
  for r in range(B):
    kind = r + rot
    if kind < 3:
      thr[r] = (-np.inf, np.inf, np.nan)[kind]
    else:
      q = min(n, (ORDER_STATS + (n // 2,))[kind % 5])
      thr[r] = np.sort(S[r])[::-1][q - 1]
      assert (S[r] == thr[r]).any()
  return thr


def seen_matrix(rows, n_cat, kind, seed=0, density=0.05):
  """scipy CSR [rows, n_cat] of seen items: "implicit" stores ones, "explicit" negatives (NOT seen) and values
  above one as well; None: no matrix."""
  if kind is None:
    return None
  rng = np.random.RandomState(31 * rows + n_cat + seed)
  density = min(1.0, max(density, 8.0 / (rows * n_cat)))              # (a handful of entries at the least)
  m = sp.random(rows, n_cat, density=density, random_state=rng, format="csr", dtype=np.float32)
  m.data[:] = 1.0 if kind == "implicit" else rng.choice([-2.0, 1.0, 3.0], size=m.nnz)
  if kind == "explicit":
    assert m.nnz >= 3
    m.data[:3] = (-2.0, 1.0, 3.0)                                       # (whatever the draw: it IS explicit)
  m.sort_indices()
  return m


# the (n, k) and the layouts (col_off, col_stride, row_off) of the rk_topk_masked cases
NK = [(5, 3), (5, 5), (255, 1), (256, 256), (257, 20), (1024, 1024), (3000, 1024), (3000, 25)]
LAYOUTS = {"tight": (0, 1, 0), "padded": (0, 1, 5), "strided": (3, 7, 5)}
