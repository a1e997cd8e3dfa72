"""GPU: the constrained-serving kernels against the numpy restatements of tests/serve_util.py, bit for bit, and
Recoder.recommend_filtered / rerank / FilteredRecommender against a float64 brute force (an integer-valued
MatrixFactorization, where every route is exact) and against recommend_util.masked_topk over the strip scorer's own
output (an autoencoder, an EASE fit, NeuMF)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import recommend_util as RU
from tests import serve_util as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
  return None if t is None else t.data_ptr()


def _stream():
  from recoder_amd.device import current_stream
  return current_stream()


# ---------------------------------------------------------------------------------------------------- the mask
def _run_mask(B, n, ldw, seen=None, allow=None, deny=None, ua=None, ud=None):
  """rk_als_serve_mask on raw arrays: seen = (indptr, ids, vals or None), allow / deny bool [n], ua / ud scipy CSR."""
  from recoder_amd import _als_lib, serve
  lib = _als_lib.load()
  bits = torch.full((B, ldw), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
  elig = torch.full((B,), -7, dtype=torch.int32, device=DEV)
  keep = []

  def csr(m):
    if m is None:
      return None, None, 0
    a, b = _t(m.indptr.astype(np.int64)), _t(np.concatenate([m.indices, [0]]).astype(np.int32))
    keep.extend([a, b])
    return _p(a), _p(b), int(m.nnz)
  s = (None, None, None, 0)
  if seen is not None:
    st = [_t(seen[0].astype(np.int64)), _t(np.concatenate([seen[1], [0]]).astype(np.int32)),
          None if seen[2] is None else _t(np.concatenate([seen[2], [0]]).astype(np.float32))]
    keep.extend(st)
    s = (_p(st[0]), _p(st[1]), _p(st[2]), len(seen[1]))
  words = [None if f is None else _t(serve.pack_bits(f).view(np.int32)) for f in (allow, deny)]
  _als_lib.check(lib.rk_als_serve_mask(B, n, ldw, *s, _p(words[0]), _p(words[1]), *csr(ua), *csr(ud), _p(bits),
                                       _p(elig), _stream()), "rk_als_serve_mask")
  return bits.cpu().numpy().view(np.uint32), elig.cpu().numpy()


def _raw_csr(rows, n, rng, density, values):
  """(indptr, ids, vals) with sorted unique ids and the given value pool, not canonicalised: zeros stay stored."""
  indptr, ids, vals = [0], [], []
  for r in range(rows):
    c = int(rng.binomial(n, density)) if r != 1 else 0          # (row 1, where there is one: empty)
    row = np.sort(rng.choice(n, size=c, replace=False))
    ids.append(row)
    vals.append(rng.choice(values, size=c))
    indptr.append(indptr[-1] + c)
  return (np.asarray(indptr, np.int64), np.concatenate(ids).astype(np.int32), np.concatenate(vals).astype(np.float32))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 2049])
def test_mask_kernel_equals_the_definition_bit_for_bit(n, B):
  rng = np.random.RandomState(100 * n + B)
  nw = -(-n // 32)
  seen = _raw_csr(B, n, rng, 0.3, [-2.0, 0.0, 1.0, 3.0])       # stored zeros and negatives: they stay eligible
  seen[2][:1] = 0.0
  if len(seen[2]) > 1:
    seen[2][1] = -2.0
  seen_m = sp.csr_matrix((seen[2], seen[1], seen[0]), shape=(B, n))
  rnd = lambda d: sp.random(B, n, density=d, random_state=rng, format="csr", dtype=np.float32)
  empty, full = sp.csr_matrix((B, n), dtype=np.float32), sp.csr_matrix(np.ones((B, n), dtype=np.float32))
  allow, deny = rng.rand(n) > 0.3, np.concatenate([rng.randint(0, n, size=5), rng.randint(0, n, size=5)])
  cases = [
      dict(),                                                    # filter_seen=False, nothing else: all eligible
      dict(seen=True),
      dict(seen=True, implicit=True),
      dict(seen=True, allow_items=allow, deny_items=deny, user_allow=rnd(0.5), user_deny=rnd(0.2)),
      dict(allow_items=np.zeros(0, dtype=np.int64)),             # an empty allow list: nothing is eligible
      dict(deny_items=deny),
      dict(user_allow=empty), dict(user_allow=full), dict(user_deny=empty),
      dict(user_deny=full),                                      # every item denied
      dict(seen=True, user_allow=full, user_deny=rnd(0.4), deny_items=np.ones(n, dtype=bool)),
  ]
  for i, c in enumerate(cases):
    ldw = nw + (i % 3)                                          # (words past the catalogue: all-ones)
    has_seen, implicit = c.pop("seen", False), c.pop("implicit", False)
    seen_ref = None if not has_seen else seen_m if not implicit else sp.csr_matrix(
        (np.ones_like(seen[2]), seen[1], seen[0]), shape=(B, n))
    ok = S.eligible_dense(B, n, seen_ref, filter_seen=has_seen, **c)
    want_bits, want_elig = S.mask_words(ok, ldw)
    flags = lambda x: None if x is None else S.catalogue(x, n)
    got_bits, got_elig = _run_mask(B, n, ldw, (seen[0], seen[1], None if implicit else seen[2]) if has_seen else None,
                                   flags(c.get("allow_items")), flags(c.get("deny_items")), c.get("user_allow"),
                                   c.get("user_deny"))
    assert np.array_equal(got_bits, want_bits), (i, n, B)
    assert np.array_equal(got_elig, want_elig), (i, n, B)


def test_mask_kernel_skips_ids_out_of_range():
  n, B = 40, 2
  bad = sp.csr_matrix((np.ones(4, np.float32), np.array([3, 39, 7, 20], np.int32), np.array([0, 2, 4])), shape=(B, n))
  raw = sp.csr_matrix(bad)
  raw.indices = np.array([3, 40, -1, 20], np.int32)             # (past the catalogue and below it)
  bits, elig = _run_mask(B, n, 2, ud=raw)
  ok = np.ones((B, n), dtype=bool)
  ok[0, 3] = ok[1, 20] = False
  want_bits, want_elig = S.mask_words(ok, 2)
  assert np.array_equal(bits, want_bits) and np.array_equal(elig, want_elig)


# -------------------------------------------------------------------------------------------------- pair scores
PAIR_COUNTS = [0, 1, 63, 64, 65, 8192]
PAIR_N = 8200


@pytest.fixture(scope="module")
def pair_lists():
  rng = np.random.RandomState(7)
  return S.csr_lists(len(PAIR_COUNTS), PAIR_N, PAIR_COUNTS, rng, must=(0, PAIR_N - 1))


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("h", [4, 64, 68, 520])
def test_pair_scores_meet_their_summation_order_bit_for_bit(pair_lists, h, with_bias):
  from recoder_amd import serve
  rng = np.random.RandomState(h)
  B, cand = len(PAIR_COUNTS), pair_lists
  assert 0 in cand.indices and PAIR_N - 1 in cand.indices
  z = rng.randn(B, h).astype(np.float32)
  Y = rng.randn(PAIR_N, h).astype(np.float32)
  b = rng.randn(PAIR_N).astype(np.float32) if with_bias else None
  wide = torch.zeros(B, h + 4, dtype=torch.float32, device=DEV)         # (a row stride that is not h)
  wide[:, :h] = _t(z)
  indptr, ids = _t(cand.indptr.astype(np.int64)), _t(cand.indices.astype(np.int32))
  got = serve.pair_scores(indptr, ids, max(PAIR_COUNTS), wide[:, :h], _t(Y), _t(b)).cpu().numpy()
  short = serve.pair_scores(indptr, ids, 1, wide[:, :h], _t(Y), _t(b)).cpu().numpy()       # (another launch shape)
  assert np.array_equal(got.view(np.uint32), short.view(np.uint32))
  for r in range(B):
    lo, hi = cand.indptr[r], cand.indptr[r + 1]
    rows = cand.indices[lo:hi]
    bias = None if b is None else b[rows]
    want = S.pair_scores(z[r], Y[rows], bias)
    assert np.array_equal(got[lo:hi].view(np.uint32), want.view(np.uint32)), (h, r)
    exact = Y[rows].astype(np.float64) @ z[r].astype(np.float64) + (0.0 if bias is None else bias.astype(np.float64))
    assert (np.abs(got[lo:hi].astype(np.float64) - exact) <= S.forward_bound(z[r], Y[rows], bias)).all()


def test_a_denied_entry_is_never_scored_nor_ranked(pair_lists):
  from recoder_amd import serve
  rng = np.random.RandomState(9)
  B, cand, h, k = len(PAIR_COUNTS), pair_lists, 8, 20
  z, Y = rng.randn(B, h).astype(np.float32), rng.randn(PAIR_N, h).astype(np.float32)
  ok = np.ones((B, PAIR_N), dtype=bool)
  ok[:, rng.choice(PAIR_N, size=PAIR_N // 3, replace=False)] = False
  ok[3] = False                                                           # (a row whose candidates are all denied)
  ldw = -(-PAIR_N // 32)
  deny = _t(S.mask_words(ok, ldw)[0].view(np.int32))
  indptr, ids = _t(cand.indptr.astype(np.int64)), _t(cand.indices.astype(np.int32))
  sc = serve.pair_scores(indptr, ids, 8192, _t(z), _t(Y), None, deny, ldw)
  rows = np.repeat(np.arange(B), PAIR_COUNTS)
  entry_ok = ok[rows, cand.indices]
  host = sc.cpu().numpy()
  assert np.isneginf(host[~entry_ok]).all() and np.isfinite(host[entry_ok]).all()
  got = [t.cpu().numpy() for t in serve.pairs_topk(indptr, ids, sc, 8192, PAIR_N, k, deny, ldw)]
  want = S.ragged_topk(cand.indptr, cand.indices, host, k, entry_ok)
  for g, w in zip(got, want):
    assert np.array_equal(g, w, equal_nan=True)
  assert (got[0][3] == -1).all() and got[2][3] == 0


# ------------------------------------------------------------------------------------------------ ragged top-k
@pytest.mark.parametrize("k", [1, 20, 1024])
def test_ragged_topk_equals_the_ordering_key(k):
  from recoder_amd import serve
  rng = np.random.RandomState(k)
  n = 9000
  counts = [0, k - 1, k, k + 1, min(8192, 4 * k + 3), 8192, 5]
  cand = S.csr_lists(len(counts), n, counts, rng, must=(0, n - 1))
  sc = (rng.randint(-6, 6, size=cand.nnz) / 4.0).astype(np.float32)       # quantised: equal scores, different ids
  lo = cand.indptr[3]
  sc[lo:lo + k + 1] = 1.0                                                  # count k + 1, all tied: the highest id is cut
  lo = cand.indptr[4]
  sc[lo:cand.indptr[5]] = -3.0
  sc[lo:lo + k - 1] = 2.0
  sc[lo + k - 1:lo + k + 2] = 0.5                                          # equal scores straddling position k
  lo = cand.indptr[6]
  sc[lo:lo + 5] = [0.0, -0.0, np.inf, RU.CANON_NAN, -np.inf]
  indptr, ids = _t(cand.indptr.astype(np.int64)), _t(cand.indices.astype(np.int32))
  got = [t.cpu().numpy() for t in serve.pairs_topk(indptr, ids, _t(sc), 8192, n, k)]
  want = S.ragged_topk(cand.indptr, cand.indices, sc, k)
  assert np.array_equal(got[0], want[0])
  assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
  assert np.array_equal(got[2], counts)
  if k >= 3:
    zeros = [int(i) for i, v in zip(got[0][6], got[1][6]) if v == 0.0]
    assert zeros == sorted(zeros) and len(zeros) == 2 and np.isnan(got[1][6][0])


# --------------------------------------------------------------------------------------- through the public call
N_ITEMS, N_USERS, K, STRIP = 200, 12, 10, 64
BOUNDS = [(0, 64), (64, 128), (128, 200)]        # (192, 200) is shorter than K: merged into the strip before it


def _interactions(seed=0):
  rng = np.random.RandomState(seed)
  m = sp.random(N_USERS, N_ITEMS, density=0.08, random_state=rng, format="csr", dtype=np.float32)
  m.data[:] = 1.0
  return m


def _batch(m, users=None):
  from recoder_amd.data import UsersInteractions
  users = np.arange(m.shape[0]) if users is None else np.asarray(users)
  return UsersInteractions(users, m[users])


def _filter_cases(m):
  """name -> keyword arguments; rows 0, 1, 2 of the per-row cases have 0, K - 1 and K eligible items."""
  rng = np.random.RandomState(4)
  B = m.shape[0]
  counts = [0, K - 1, K] + [60] * (B - 3)
  ua = S.csr_lists(B, N_ITEMS, counts, rng, must=(0, 63, 64, N_ITEMS - 1))
  ud = sp.csr_matrix(1.0 - np.asarray(S.csr_lists(B, N_ITEMS, [0, K - 1, K] + [150] * (B - 3), rng).todense()))
  allow = rng.rand(N_ITEMS) > 0.5
  deny = np.concatenate([rng.randint(0, N_ITEMS, 30), rng.randint(0, N_ITEMS, 30)])
  # all five: the per-row lists drawn from what the other three leave, so that rows 0..2 keep their counts
  ok3 = S.eligible_dense(B, N_ITEMS, m, True, allow, deny)
  ua5 = sp.lil_matrix((B, N_ITEMS), dtype=np.float32)
  ud5 = sp.lil_matrix((B, N_ITEMS), dtype=np.float32)
  for r, c in enumerate([0, K - 1, K] + [40] * (B - 3)):
    free, taken = np.nonzero(ok3[r])[0], np.nonzero(~ok3[r])[0]
    pick = rng.choice(free, size=c + 5 if r else 0, replace=False)       # c + 5 allowed, 5 of them denied again
    ua5[r, pick] = 1.0
    ua5[r, rng.choice(taken, size=10, replace=False)] = 1.0             # (allowed here, ineligible elsewhere)
    if r:
      ud5[r, pick[:5]] = 1.0
  return {
      "seen": dict(),
      "allow": dict(filter_seen=False, allow_items=allow),
      "deny": dict(filter_seen=False, deny_items=deny),
      "user_allow": dict(filter_seen=False, user_allow=ua),
      "user_deny": dict(filter_seen=False, user_deny=ud),
      "all": dict(filter_seen=True, allow_items=allow, deny_items=deny, user_allow=ua5.tocsr(), user_deny=ud5.tocsr()),
  }


def _ok(m, kw):
  kw = dict(kw)
  return S.eligible_dense(m.shape[0], N_ITEMS, m, kw.pop("filter_seen", True), **kw)


@pytest.fixture(scope="module")
def int_mf():
  """A MatrixFactorization whose tables are small integers: every product and sum is exact in f32 and in the fp16
  hi / lo split, so both routes give the float64 scores exactly."""
  from recoder_amd.model import Recoder
  from recoder_amd.nn import MatrixFactorization
  rng = np.random.RandomState(1)
  rec = Recoder(model=MatrixFactorization(16), use_cuda=True, optimizer_type="adam", loss="mse",
                loss_params={"confidence": 10.0}, num_items=N_ITEMS, num_users=N_USERS)
  rec._Recoder__init_model()
  X, Y, b = (rng.randint(-8, 9, size=s).astype(np.float32) for s in ((N_USERS, 16), (N_ITEMS, 16), (N_ITEMS,)))
  Y[64], b[64] = Y[63], b[63]                                    # a tie across a strip boundary, in every row
  Y[128], b[128] = Y[0], b[0]
  md = rec.model
  md.user_embedding_layer.weight.data.copy_(_t(X))
  md.item_embedding_layer.weight.data.copy_(_t(Y))
  md.bias.data.copy_(_t(b))
  rec._sync_ranges()
  rec.eval_strip_items = STRIP
  scores = X.astype(np.float64) @ Y.astype(np.float64).T + b.astype(np.float64)
  return rec, scores


@pytest.mark.parametrize("case", ["seen", "allow", "deny", "user_allow", "user_deny", "all"])
def test_integer_mf_gives_the_brute_force_on_both_routes(int_mf, case):
  rec, scores = int_mf
  m = _interactions()
  kw = _filter_cases(m)[case]
  ok = _ok(m, kw)
  if case in ("user_allow", "user_deny", "all"):
    assert ok.sum(axis=1)[:3].tolist() == [0, K - 1, K]
  want_ids, want_val = S.brute_force(scores, ok, K)
  routes = ["mask", "pairs", "auto"] if "user_allow" in kw else ["mask", "auto"]
  for route in routes:
    ids, val = rec.recommend_filtered(_batch(m), K, return_scores=True, route=route, **kw)
    assert ids.dtype == np.int64 and val.dtype == np.float32 and ids.shape == val.shape == (N_USERS, K)
    assert np.array_equal(ids, want_ids), (case, route)
    assert np.array_equal(val.astype(np.float64), want_val), (case, route)
    assert np.array_equal(rec.recommend_filtered(_batch(m), K, route=route, **kw), want_ids)
  if "user_allow" not in kw:
    with pytest.raises(ValueError, match="route='pairs'"):
      rec.recommend_filtered(_batch(m), K, route="pairs", **kw)


def _strip_scores(rec, ui):
  """[B, N_ITEMS] f32: the output of the strip scorer recommend() runs, strip by strip over BOUNDS."""
  from recoder_amd.device import Block
  rec.model.eval()
  rec._check_ranges()
  blk, B, n = rec._input_block(ui)
  dcsr = rec._eval_ws["dcsr"]
  out = np.zeros((B, n), dtype=np.float32)
  ld = 96
  buf = torch.empty(B * ld, dtype=torch.float32, device=DEV)
  engine = rec._engine()
  z = None
  if not (rec._scores_from_csr_rows() or rec._scores_from_user_ids()):
    z = engine.encode_eval(blk, 0, B)
  for lo, hi in BOUNDS:
    if rec._scores_from_user_ids():
      rec.model.user_scores(rec._user_ids(ui), lo, hi, buf, ld)
    elif rec._scores_from_csr_rows():
      rec.model.csr_scores(dcsr, lo, hi, buf, ld, B)
    else:
      sblk = Block(B, 1, n, DEV, negative_sampling=True, need_bits_cr=False, n_cap=hi - lo)
      sblk.set_items(torch.arange(lo, hi, dtype=torch.int32, device=DEV), hi - lo, B)
      engine.decode_scores(z, B, sblk, buf, ld)
    out[:, lo:hi] = buf.view(B, ld)[:, :hi - lo].cpu().numpy()
  return out


def _autoencoder():
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder
  torch.manual_seed(3)
  rec = Recoder(model=DynamicAutoencoder(hidden_layers=[16], activation_type="tanh"), use_cuda=True,
                optimizer_type="adam", loss="mse", num_items=N_ITEMS, num_users=N_USERS)
  rec._Recoder__init_model()
  return rec


def _ease():
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.model import Recoder
  from recoder_amd.nn import ShallowAutoencoder
  rec = Recoder(model=ShallowAutoencoder(5.0))
  rec.train_ease(RecommendationDataset(_interactions(seed=8)))
  return rec


def _neumf():
  from recoder_amd.model import Recoder
  from recoder_amd.nn import NeuralMatrixFactorization
  from tests import ncf_util as nu
  torch.manual_seed(4)
  rec = Recoder(NeuralMatrixFactorization(*nu.MID), use_cuda=True, user_based=True, num_users=N_USERS,
                num_items=N_ITEMS)
  rec._Recoder__init_model()
  return rec


@pytest.fixture(scope="module")
def strip_models():
  out = {}
  for name, make in (("autoencoder", _autoencoder), ("ease", _ease), ("neumf", _neumf)):
    rec = make()
    rec.eval_strip_items = STRIP
    out[name] = rec
  return out


@pytest.mark.parametrize("name", ["autoencoder", "ease", "neumf"])
def test_every_scoring_route_takes_the_filters_through_its_strips(strip_models, name):
  rec = strip_models[name]
  m = _interactions()
  ui = _batch(m)
  scores = _strip_scores(rec, ui)
  assert np.isfinite(scores).all() and len(np.unique(scores)) > K
  for case, kw in _filter_cases(m).items():
    ok = _ok(m, kw)
    want_ids, want_val = S.masked_topk_padded(scores, ok, K)
    ids, val = rec.recommend_filtered(ui, K, return_scores=True, **kw)
    assert np.array_equal(ids, want_ids), (name, case)
    assert np.array_equal(val.view(np.uint32), want_val.view(np.uint32)), (name, case)
    if "user_allow" in kw:
      with pytest.raises(ValueError, match="route='pairs'"):
        rec.recommend_filtered(ui, K, route="pairs", **kw)


@pytest.mark.parametrize("strip", [STRIP, 65536], ids=["strips", "one_strip"])
def test_the_default_call_is_recommend_array(int_mf, strip_models, strip):
  m = _interactions()
  ui = _batch(m)
  for rec in (int_mf[0], strip_models["autoencoder"], strip_models["ease"]):
    rec.eval_strip_items = strip
    try:
      want = rec.recommend_array(ui, K)
      assert np.array_equal(rec.recommend_filtered(ui, K), want)
      assert np.array_equal(rec.recommend_filtered(ui, K, route="mask"), want)
    finally:
      rec.eval_strip_items = STRIP


def test_rerank_is_recommend_filtered_over_the_candidates(int_mf):
  rec, scores = int_mf
  m = _interactions()
  cand = _filter_cases(m)["user_allow"]["user_allow"]
  a = rec.rerank(_batch(m), cand, K, return_scores=True)
  b = rec.recommend_filtered(_batch(m), K, filter_seen=False, user_allow=cand, return_scores=True)
  assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
  assert np.array_equal(a[0], S.brute_force(scores, S.pattern(cand, N_USERS, N_ITEMS), K)[0])
  assert np.array_equal(rec.rerank(_batch(m), cand, K), a[0])


def test_user_rows_are_recommend_folded_when_no_filter_is_set(int_mf):
  rec, _ = int_mf
  m = _interactions()
  ui = _batch(m, np.arange(N_USERS)[::-1])
  want = rec.recommend_folded(ui, K, alpha=10.0, reg=50.0)
  rows = rec.fold_in(ui.interactions_matrix, alpha=10.0, reg=50.0)
  assert np.array_equal(rec.recommend_filtered(ui, K, user_rows=rows), want)
  # with candidates the folded rows go through the pair kernels: the same ranking of that set, up to near-ties
  cand = sp.csr_matrix(np.ones((N_USERS, N_ITEMS), dtype=np.float32))
  ids, val = rec.recommend_filtered(ui, K, user_rows=rows, user_allow=cand, route="pairs", return_scores=True)
  ids_m, val_m = rec.recommend_filtered(ui, K, user_rows=rows, user_allow=cand, route="mask", return_scores=True)
  assert ids.shape == ids_m.shape and (ids >= 0).all() and np.abs(val - val_m).max() <= 1e-3 * np.abs(val_m).max()


def test_filtered_recommender_under_the_evaluator_and_the_sampled_protocol(int_mf):
  from recoder_amd.data import RecommendationDataset
  from recoder_amd.metrics import NDCG, Recall, RecommenderEvaluator, sampled_candidates
  from recoder_amd.recommender import FilteredRecommender
  rec, scores = int_mf
  m = _interactions()
  rng = np.random.RandomState(6)
  target = sp.lil_matrix(m.shape, dtype=np.float32)
  dense = np.asarray(m.todense()) > 0
  for u in range(N_USERS):
    target[u, rng.choice(np.nonzero(~dense[u])[0], size=2, replace=False)] = 1.0
  target = target.tocsr()
  cand = sampled_candidates(target, m, 6, seed=2)              # 2 targets + 6 negatives < K: every list is padded
  assert (np.diff(cand.indptr) == 8).all()
  recommender = FilteredRecommender(rec, K, user_allow=cand)
  metrics = [Recall(k=K, normalize=True), NDCG(k=K)]
  ds = RecommendationDataset(m, target)
  torch.manual_seed(5)                                         # (the evaluator's user order: the same for both)
  host = RecommenderEvaluator(recommender, metrics).evaluate(ds, batch_size=5)
  torch.manual_seed(5)
  dev = RecommenderEvaluator(recommender, metrics).evaluate(ds, batch_size=5, on_device=True)
  for metric in metrics:
    a, d = np.asarray(host[metric], np.float64), np.asarray(dev[metric], np.float64)
    assert a.shape == d.shape == (N_USERS,) and np.array_equal(a, d) and a.mean() > 0
  users = np.array([7, 2, 9])
  lists = recommender.recommend_array(_batch(m, users))
  pat = S.pattern(cand, N_USERS, N_ITEMS)
  for row, u in zip(lists, users):
    real = row[row >= 0]
    assert len(real) == 8 and (row[8:] == -1).all() and pat[u, real].all()       # a subset of the candidate set
  assert np.array_equal(lists, S.brute_force(scores[users], pat[users] & ~dense[users], K)[0])
  assert recommender.recommend(_batch(m, users)) == lists.tolist()
  ids, ld = recommender.recommend_device(_batch(m, users))
  assert ld >= K and np.array_equal(ids.cpu().numpy(), lists)


def test_rank_metrics_count_the_padding_id_as_a_miss():
  from recoder_amd.metrics import DeviceTarget, Recall, NDCG, batch_metrics, device_batch_metrics
  recs = np.array([[-1, -1, -1], [4, -1, -1], [-1, 0, -1]], dtype=np.int64)
  target = sp.csr_matrix(np.array([[1, 0, 0, 0, 0], [0, 0, 0, 0, 1], [1, 1, 0, 0, 0]], dtype=np.float32))
  metrics = [Recall(k=3, normalize=True), NDCG(k=3)]
  values, _ = device_batch_metrics(_t(recs), 3, DeviceTarget(target, DEV), metrics)
  got = values.cpu().numpy()
  assert got[0].tolist() == [0.0, 0.0] and got[1, 0] == 1.0 and got[2, 0] == 0.5
  host = batch_metrics(recs, target, metrics)
  for j, metric in enumerate(metrics):
    assert np.array_equal(np.asarray(host[metric], np.float64), got[:, j])
