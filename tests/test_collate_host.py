"""CPU: tests/collate_util.collate_ref -- the restatement tests/test_collate.py judges csrc/collate.hip by -- against
oracle.recoder_oracle.collate (the reference's BatchCollator restated, pinned to the reference's goldens) and against
the invariants include/recoder_hip.h states for a block, worked out here by other means than collate_ref's own."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import recoder_oracle as orc
from tests import collate_util as cu


def _random_csr(seed, n_users=60, n_items=500):
  """Ratings (negative and non-integer ones), a third of the rows empty, a few long rows."""
  rng = np.random.RandomState(seed)
  lengths = rng.randint(0, 40, size=n_users)
  lengths[rng.rand(n_users) < 0.33] = 0
  lengths[rng.randint(n_users, size=3)] = rng.randint(100, 300, size=3)
  return cu.csr_from_rows(cu.random_rows(rng, lengths, n_items), n_items, seed)


def _ref(csr, users, ns, S_cap=None, nnz_cap=None, n_cap=None, **kw):
  S_cap = S_cap or len(users) + 3
  nnz_cap = nnz_cap or int(cu.degrees(csr, users).sum()) + 5
  n_cap = n_cap or (min(csr.shape[1], nnz_cap) if ns else csr.shape[1])
  return cu.collate_ref(csr.indptr, csr.indices, csr.data, users, ns, S_cap, nnz_cap, n_cap, csr.shape[1], **kw)


def _bit(words, c):
  """Bit c of each row of [rows, words] uint32, one shift and mask per row."""
  return np.array([(int(w) >> (c & 31)) & 1 for w in words[:, c >> 5]], dtype=bool)


def _unpack(words, n):
  return np.stack([_bit(words, c) for c in range(n)], axis=1) if n else np.zeros((len(words), 0), dtype=bool)


def _popcount(words):
  return np.array([[bin(int(w)).count("1") for w in row] for row in words], dtype=np.int64).reshape(words.shape)


CASES = [(seed, ns, dup) for seed in range(4) for ns in (True, False) for dup in (False, True)]


@pytest.mark.parametrize("seed,ns,dup", CASES)
def test_collate_ref_agrees_with_the_oracle(seed, ns, dup):
  csr = _random_csr(seed)
  rng = np.random.RandomState(100 + seed)
  users = rng.choice(csr.shape[0], size=23, replace=dup).astype(np.int64)
  if dup:
    users[[3, 11, 19]] = users[0]
  assert (cu.degrees(csr, users) == 0).any() and (csr.data < 0).any() and (csr.data != np.round(csr.data)).any()
  ref = _ref(csr, users, ns)
  want = orc.collate(orc.extract_rows(csr, users), users, len(users), ns)[0]
  rows = np.repeat(np.arange(ref["S"]), np.diff(ref["indptr"]))
  assert ref["nnz"] == want.indices.shape[1] and ref["indptr"][0] == 0
  assert np.array_equal(rows, want.indices[0])
  assert np.array_equal(ref["cols"], want.indices[1])
  assert np.array_equal(ref["vals"].view(np.uint32), want.values.view(np.uint32))
  if ns:
    assert np.array_equal(ref["items"], want.items) and ref["n_b"] == len(want.items)
  else:
    assert np.array_equal(ref["items"], np.arange(csr.shape[1])) and ref["n_b"] == csr.shape[1]
  c = ref["counts"]
  assert tuple(c[:4]) == (ref["n_b"], ref["nnz"], -(-ref["n_b"] // 32) * 32, len(users))
  assert not c[4:].any()


@pytest.mark.parametrize("seed,ns,dup", CASES)
def test_collate_ref_keeps_the_header_invariants(seed, ns, dup):
  csr = _random_csr(seed, n_users=40, n_items=400)
  rng = np.random.RandomState(200 + seed)
  users = rng.choice(csr.shape[0], size=37, replace=dup).astype(np.int64)
  ref = _ref(csr, users, ns, S_cap=41)
  S, n_b, wr = ref["S"], ref["n_b"], ref["wr"]
  deg = cu.degrees(csr, users)
  # gcols = items[cols]; pos inverts items and is -1 elsewhere
  assert np.array_equal(ref["items"][ref["cols"]], ref["gcols"])
  assert np.array_equal(ref["pos"][ref["items"]], np.arange(n_b))
  assert (ref["pos"] >= 0).sum() == n_b and ref["pos"].min() >= -1
  # the bitmap against the dense matrix scipy makes of the same rows
  dense = np.asarray(csr[users][:, ref["items"]].todense()) != 0
  got = _unpack(ref["bits_rc"], n_b)
  assert np.array_equal(got, dense)
  assert np.array_equal(_popcount(ref["bits_rc"]).sum(axis=1), deg)
  assert not _unpack(ref["bits_rc"], wr * 32)[:, n_b:].any()             # (no bit past n_b in the last word)
  # bits_cr is its transpose over the whole capacity, zero outside [n_b, S)
  got_t = _unpack(ref["bits_cr"], ref["bits_cr"].shape[1] * 32)
  assert ref["bits_cr"].shape[0] >= n_b and ref["bits_cr"].shape[1] == 2          # ([n_cap, ceil(41 / 32)])
  assert np.array_equal(got_t[:n_b, :S], dense.T)
  assert not got_t[n_b:].any() and not got_t[:, S:].any()
  # pref_rc: the exclusive cumulative popcount, which is what finds an entry (header, rk_block_t.pref_rc)
  pc = _popcount(ref["bits_rc"])
  assert np.array_equal(ref["pref_rc"], np.cumsum(pc, axis=1) - pc)
  for j in rng.choice(ref["nnz"], size=50):
    r = np.searchsorted(ref["indptr"], j, side="right") - 1
    c = int(ref["cols"][j])
    w = int(ref["bits_rc"][r, c >> 5])
    assert j == ref["indptr"][r] + ref["pref_rc"][r, c >> 5] + bin(w & ((1 << (c & 31)) - 1)).count("1")


def test_collate_ref_truncated_forms_by_hand():
  # rows: u0 = {1: 2.5, 4: -1, 7: 3}, u1 = {}, u2 = {0: .5, 4: 2, 9: -3.5}
  csr = sp.csr_matrix((np.array([2.5, -1, 3, .5, 2, -3.5], np.float32), np.array([1, 4, 7, 0, 4, 9]),
                       np.array([0, 3, 3, 6])), shape=(3, 10))
  users = np.array([2, 0, 1, 0])
  # too few item slots: the set {0, 1, 4, 7, 9} keeps {0, 1, 4}
  ref = cu.collate_ref(csr.indptr, csr.indices, csr.data, users, True, 5, 12, 3, 10)
  assert list(ref["counts"][:8]) == [3, 9, 32, 4, 0, 5, 0, 0]
  assert list(ref["items"]) == [0, 1, 4]
  assert list(ref["pos"]) == [0, 1, -1, -1, 2, -1, -1, -1, -1, -1]
  assert list(ref["indptr"]) == [0, 3, 6, 6, 9]
  assert list(ref["cols"]) == [0, 2, 0, 1, 2, 0, 1, 2, 0]
  assert list(ref["gcols"]) == [0, 4, 9, 1, 4, 7, 1, 4, 7]
  assert list(ref["vals"]) == [.5, 2, 0, 2.5, -1, 0, 2.5, -1, 0]
  assert ref["bits_rc"].tolist() == [[0b101], [0b110], [0], [0b110]]
  assert ref["pref_rc"].tolist() == [[0], [0], [0], [0]]
  assert ref["bits_cr"].tolist() == [[0b0001], [0b1010], [0b1011]]
  # too few entry slots: 9 stored entries into 5 -- row 1 keeps two of its three, rows 2 and 3 nothing; the
  # item set is still that of every stored entry
  ref = cu.collate_ref(csr.indptr, csr.indices, csr.data, users, True, 5, 5, 7, 10)
  assert list(ref["counts"][:8]) == [5, 5, 32, 4, 0, 0, 9, 0]
  assert list(ref["items"]) == [0, 1, 4, 7, 9]
  assert list(ref["indptr"]) == [0, 3, 5, 5, 5]
  assert list(ref["cols"]) == [0, 2, 4, 1, 2] and list(ref["gcols"]) == [0, 4, 9, 1, 4]
  assert list(ref["vals"]) == [.5, 2, -3.5, 2.5, -1]
  assert ref["bits_rc"].tolist() == [[0b10101], [0b00110], [0], [0]]
  assert ref["bits_cr"].shape == (7, 1)
  assert ref["bits_cr"][:, 0].tolist() == [0b01, 0b10, 0b11, 0, 0b01, 0, 0]
  # implicit data: every value reads 1.0
  ref = cu.collate_ref(csr.indptr, csr.indices, None, users, True, 5, 12, 7, 10, implicit=True)
  assert ref["nnz"] == 9 and np.all(ref["vals"] == 1.0) and not ref["counts"][4:].any()


def test_need_lists_and_densify_refs_by_hand():
  a = np.array([-1, 0, -1, 1, -1, -1])
  b = np.array([-1, -1, 0, 1, -1, 2])
  assert list(cu.need_lists_ref(a, b)) == [1, 2, 3, 5]
  assert len(cu.need_lists_ref(a[:1], b[:1])) == 0
  csr = sp.csr_matrix((np.array([2.5, -1, 3, .5], np.float32), np.array([1, 4, 7, 4]), np.array([0, 3, 3, 4])),
                      shape=(3, 10))
  ref = cu.collate_ref(csr.indptr, csr.indices, csr.data, np.array([0, 1, 2]), True, 3, 4, 4, 10)
  assert cu.densify_ref(ref, 0, 3, 3).tolist() == [[2.5, -1, 3], [0, 0, 0], [0, .5, 0]]
  assert cu.densify_ref(ref, 1, 2, 3).tolist() == [[0, 0, 0], [0, .5, 0]]
  want = orc.densify(orc.collate(csr, np.arange(3), 3, True)[0]).numpy()
  assert np.array_equal(cu.densify_ref(ref, 0, 3, 3), want)


def test_case_builders_reach_what_they_are_built_for():
  for n_items in (1, 3, 4095, 4097, 67585):
    csr, users = cu.scan_case(n_items)
    assert csr.shape[1] == n_items and np.isin(cu.boundary_items(n_items), csr[users].indices).all()
  assert list(cu.boundary_items(4097)) == [0, 2047, 2048, 4095, 4096]
  csr, users = cu.mix_case()
  deg = cu.degrees(csr, users)
  want = [cu.MIX_NAMED.get(x, x) for x in cu.MIX_ROWS]
  assert list(deg) == want and len(users) % 4 != 0 and len(users) % 32 != 0
  assert deg[0] == 0 and deg[-1] == 0 and (deg[12], deg[13]) == (0, 0)
  assert (deg[8:12] > cu.BUILD_HEAVY).all()                                    # four heavy rows in one workgroup
  assert list(deg[4:8] > cu.BUILD_HEAVY) == [False, False, True, False]        # one heavy row, in wave 2
  for name in cu.MIX_NAMED:
    r = [i for i, x in enumerate(cu.MIX_ROWS) if x == name]
    assert len(r) == 3 and len(set(users[r])) == 1
  assert 0 in csr[users].indices and cu.MIX_ITEMS - 1 in csr[users].indices
  for n_rows, own, stripe, extra in ((64, 1060, 1125, 40), (160, 430, 450, 30)):
    csr, users = cu.wide_case(n_rows, own, stripe, extra)
    n_b = len(np.unique(csr[users].indices))
    assert n_b > cu.SMALL_SCAN_MAX and -(-n_b // 32) > cu.SEG_WORDS and csr.nnz <= 75000
