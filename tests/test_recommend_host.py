"""CPU: what stands behind tests/test_recommend_kernels.py without a GPU.

* tests/recommend_util.masked_topk -- the restatement rk_topk_masked is held to -- against numpy's stable argsort
  and torch.topk on data where the three agree by definition (no NaN, no signed zero).
* order_key is monotone over float32's bit patterns from -inf to +inf through the subnormals, and maps the two zeros
  to one key; the canonical NaN ranks on top, as torch.topk ranks it.
* pairs_topk depends on the SET of a row's first cnt pairs only.
* filter_survivors at the k-th value of masked_topk contains masked_topk's ids: the property the fused
  recommend path rests on.
* every input generator of the GPU tests runs here with the seeds the GPU tests use: their own assertions (a row
  with fewer than k unseen items, threshold ties on both sides of a chunk boundary) hold for every case.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import recommend_util as ru

NK, LAYOUTS = ru.NK, ru.LAYOUTS


def _plain_scores(seed, B, n, quantised):
  rng = np.random.RandomState(seed)
  if quantised:
    return (rng.randint(1, 40, size=(B, n)) / 8.0).astype(np.float32)          # ties, no zero
  return rng.randn(B, n).astype(np.float32)


def _seen(seed, B, n_cat, explicit):
  return ru.seen_matrix(B, n_cat, "explicit" if explicit else "implicit", seed)


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("n,k", [(5, 5), (300, 1), (300, 25), (1000, 1000)])
@pytest.mark.parametrize("col_off,col_stride", [(0, 1), (3, 7)])
def test_masked_topk_is_stable_argsort_and_torch_topk(n, k, col_off, col_stride, quantised):
  B = 9
  sc = _plain_scores(n + k, B, n, quantised)
  n_cat = col_off + n * col_stride
  seen = _seen(n, B, n_cat, explicit=True)
  ids, vals = ru.masked_topk(sc, k, seen, col_off, col_stride)
  items = col_off + np.arange(n) * col_stride
  masked = sc.copy()
  masked[np.asarray(seen.todense())[:, items] > 0] = -np.inf                  # (stored negatives stay)
  want = np.argsort(-masked, axis=1, kind="stable")[:, :k]
  assert np.array_equal(ids, items[want])
  tv = torch.topk(torch.from_numpy(masked), k, dim=1, sorted=True)[0].numpy()
  assert np.array_equal(ru.bits(vals), ru.bits(tv))
  assert ids.dtype == np.int64 and vals.dtype == np.float32
  # without a seen matrix: the plain rows
  ids0, _ = ru.masked_topk(sc, k)
  assert np.array_equal(ids0, np.argsort(-sc, axis=1, kind="stable")[:, :k])


def test_order_key_is_monotone_and_the_zeros_are_one_key():
  # float32 bit patterns in ascending VALUE order: -inf ... -subnormals, -0.0, +0.0, subnormals ... +inf
  step = 65521                                                                 # (a prime: every exponent is met)
  pos = np.concatenate([np.arange(0, 0x00800000 + 64, 1 << 14), np.arange(0, 0x7f800000, step),
                        [1, 2, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000]]).astype(np.uint32)
  pos = np.unique(pos)
  neg = (pos | np.uint32(0x80000000))[::-1]
  sweep = np.concatenate([neg, pos]).view(np.float32)
  assert np.isneginf(sweep[0]) and np.isposinf(sweep[-1]) and not np.isnan(sweep).any()
  assert np.all(np.diff(sweep.astype(np.float64)) >= 0)
  key = ru.order_key(sweep)
  d = np.diff(key.astype(np.int64))
  zero = len(neg) - 1                                                          # -0.0 sits here, +0.0 next to it
  assert ru.bits(sweep[zero:zero + 2]).tolist() == [0x80000000, 0]
  assert d[zero] == 0 and np.all(np.delete(d, zero) > 0)
  assert ru.order_key(np.float32(-0.0).reshape(1))[0] == ru.order_key(np.float32(0.0).reshape(1))[0] == 0x80000000
  # the canonical NaN: above +inf, where torch.topk puts it
  assert ru.order_key(np.array([ru.CANON_NAN]))[0] > key[-1]
  x = np.array([[1.0, np.inf, ru.CANON_NAN, -np.inf, 0.0]], dtype=np.float32)
  assert ru.masked_topk(x, 3)[0].tolist() == torch.topk(torch.from_numpy(x), 3, dim=1)[1].tolist() == [[2, 1, 0]]
  # key_value inverts the keys (the zeros read +0.0)
  back = ru.key_value(key)
  want = sweep.copy()
  want[zero] = 0.0
  assert np.array_equal(ru.bits(back), ru.bits(want))
  # equal zeros of either sign: the lower column first
  z = np.array([[-1.0, 0.0, -0.0, -0.0, 0.0, -2.0]], dtype=np.float32)
  assert ru.masked_topk(z, 4)[0].tolist() == [[1, 2, 3, 4]]
  assert ru.bits(ru.masked_topk(z, 4)[1]).tolist() == [[0, 0, 0, 0]]


@pytest.mark.parametrize("cap,k", [(1, 1), (2, 1), (64, 1), (64, 17), (64, 64), (4096, 100)])
def test_pairs_topk_depends_on_the_set_of_the_first_cnt_pairs(cap, k):
  val, idx, cnt, _ = ru.pairs_case(cap, k, "both", seed=3)
  ids, written, status = ru.pairs_topk(val, idx, cnt, cap, k)
  assert status == 3 and written.sum() == len(cnt) - 2
  rng = np.random.RandomState(cap + k)
  val2, idx2 = val.copy(), idx.copy()
  for r in range(len(cnt)):
    c = min(int(cnt[r]), cap)
    p = rng.permutation(c)
    val2[r, :c], idx2[r, :c] = val[r, :c][p], idx[r, :c][p]
    val2[r, c:], idx2[r, c:] = 1e30, 5                                        # (entries at and past cnt: other garbage)
  ids2, written2, status2 = ru.pairs_topk(val2, idx2, cnt, cap, k)
  assert np.array_equal(ids, ids2) and np.array_equal(written, written2) and status2 == 3
  # against masked_topk over the dense scatter of the pairs (ids are unique inside a row)
  for r in np.nonzero(written)[0]:
    c = int(cnt[r])
    dense = np.full((1, 3 * cap + 10), -np.inf, dtype=np.float32)
    dense[0, idx[r, :c]] = val[r, :c]
    assert np.array_equal(ru.masked_topk(dense, k)[0][0], ids[r])
  assert (ids[~written] == -1).all()


@pytest.mark.parametrize("B,n,k", [(9, 300, 5), (4, 97, 20), (6, 700, 1)])
def test_filter_survivors_at_the_kth_value_contain_the_topk(B, n, k):
  sc = _plain_scores(B + n, B + 5, n, quantised=True)[5:]
  seen = _seen(n + 1, B + 5, n, explicit=True)
  ids, vals = ru.masked_topk(sc, k, seen[5:5 + B])
  surv = ru.filter_survivors(sc, vals[:, k - 1], seen, 0, 5)
  dense_seen = np.asarray(seen.todense())[5:5 + B] > 0
  for r in range(B):
    got = {i for i, _ in surv[r]}
    assert set(ids[r].tolist()) <= got
    assert not dense_seen[r, sorted(got)].any()
    assert all(u == ru.bits(sc[r, i:i + 1])[0] for i, u in surv[r])
    # and nothing below the k-th value: the candidates rk_topk_pairs sorts are the top k and its ties
    assert all(sc[r, i] >= vals[r, k - 1] for i in got)
  # a strip: item ids carry the column offset; a NaN threshold keeps nothing, -inf everything unseen
  thr = np.array([-np.inf, np.nan, np.inf] + [0.5] * (B - 3), dtype=np.float32)
  strip = ru.filter_survivors(sc[:, 40:], thr, seen, 40, 5)
  assert {i for i, _ in strip[0]} == set((40 + np.nonzero(~dense_seen[0, 40:])[0]).tolist())
  assert strip[1] == set() and strip[2] == set()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("seen_kind", [None, "implicit", "explicit"])
@pytest.mark.parametrize("n,k", NK)
def test_topk_cases_hold_what_they_promise(n, k, seen_kind, layout):
  """The generator's own assertions (row FEW has fewer than k unseen items, row TIES has its taken ties on both sides
  of column 256 wherever n > 257 and k >= 7) for every case of the GPU test, and the properties the restatement must
  show on them."""
  col_off, col_stride, row_off = LAYOUTS[layout]
  sc, seen = ru.topk_case(n, k, seen_kind, col_off, col_stride, row_off)
  B = sc.shape[0]
  rows = None if seen is None else seen[row_off:row_off + B]
  ids, vals = ru.masked_topk(sc, k, rows, col_off, col_stride)
  assert ids.shape == (B, k) and all(len(set(r.tolist())) == k for r in ids)
  key = ru.order_key(vals)
  assert np.all(key[:, 1:] <= key[:, :-1])
  # row FEW: max(k - 2, 0) finite winners, then masked items lowest id first
  u = max(k - 2, 0)
  assert np.isneginf(vals[ru.FEW, u:]).all() and np.all(np.diff(ids[ru.FEW, u:]) > 0)
  if u:
    assert np.isfinite(vals[ru.FEW, :u]).all()
  if seen_kind == "explicit":
    assert (seen.data < 0).any() and (seen.data > 1).any()
  if seen is not None:
    assert seen.shape[0] > row_off + B                                          # (a block with more rows than B)
  # the specials row holds what it says
  spec = sc[ru.SPEC]
  if n >= 256:
    for s in ru.SPECIALS:
      assert (ru.bits(spec) == ru.bits(np.array([s]))[0]).any()
  assert (ru.bits(spec) == 0x80000000).any() and (ru.bits(spec) == 0).any()
  assert not (ru.bits(sc) > 0xff800000).any()                                   # no NaN with the sign bit set


@pytest.mark.parametrize("kind", ["good", "over", "under", "both"])
@pytest.mark.parametrize("cap", [1, 2, 64, 4096, 8192])
def test_pairs_cases_hold_what_they_promise(cap, kind):
  for k in sorted({1, max(1, cap // 3), cap}):
    val, idx, cnt, n_ids = ru.pairs_case(cap, k, kind)
    assert (cnt == k).any() and (cnt == cap).any()
    assert ((cnt == cap + 1).any(), (cnt == k - 1).any()) == (kind in ("over", "both"), kind in ("under", "both"))
    for r in range(len(cnt)):
      c = min(int(cnt[r]), cap)
      assert np.isnan(val[r, c:]).all() and (idx[r, c:] == -1).all()
      assert len(set(idx[r, :c].tolist())) == c and (idx[r, :c] >= 0).all() and (idx[r, :c] < n_ids).all()
      if c > 12:
        assert len(set(val[r, :c].tolist())) < c                                # equal scores under different ids


@pytest.mark.parametrize("B,h,n", ru.FILTER_SHAPES)
def test_filter_inputs_hold_what_they_promise(B, h, n):
  assert {s[0] for s in ru.FILTER_SHAPES} == {1, 37, 130}
  assert {s[1] for s in ru.FILTER_SHAPES} == {4, 36, 64, 200}
  assert {s[2] for s in ru.FILTER_SHAPES} == {97, 700, 2049}
  Z, W, b = ru.filter_operands(B, h, n)
  S = (Z.astype(np.float64) @ W.astype(np.float64).T + b).astype(np.float32)
  kinds = set()
  for rot in range(4 if B == 1 else 1):
    thr = ru.filter_thresholds(S, rot)
    surv = ru.filter_survivors(S, thr)
    for r in range(B):
      kind = r + rot
      kinds.add(min(kind, 3))
      if kind == 0:
        assert len(surv[r]) == n
      elif kind in (1, 2):
        assert len(surv[r]) == 0
      else:
        assert (S[r] == thr[r]).any() and 1 <= len(surv[r]) <= n
  assert kinds == {0, 1, 2, 3}
