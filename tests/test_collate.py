"""GPU: every kernel of csrc/collate.hip against tests/collate_util.collate_ref (need_lists_ref, densify_ref), the
numpy restatement of what include/recoder_hip.h says a collation leaves in a block -- EXACTLY, values as bit
patterns, at the smallest shapes that reach each path: the three scan routes and their round / chunk tails, the
one-wave and the four-wave row build, bitmaps wider than one LDS segment, the cursor forms with more roles than
workgroups and a look-back over several chunks, truncated blocks, a reused block.

Every output tensor of the block is filled with a sentinel before each collation: what the restatement does not
define (the tails past nnz / n_b / S / the words in use, counts[4] and counts[7], svals) must still hold it
afterwards.  scan_tmp, the scans' scratch, starts from all-ones: a collation may not depend on what it finds there.
Each case asserts the property of its own input that takes it down the path it is named for."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from recoder_amd import _lib
from recoder_amd._lib import RecoderHipError, RkBlock, check, ptr
from recoder_amd.device import Block, DeviceCSR, current_stream
from tests import collate_util as cu

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
OUTPUTS = ("counts", "indptr", "cols", "gcols", "vals", "svals", "items", "pos", "bits_rc", "bits_cr", "pref_rc")


def dev_t(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
  return t.cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.int32)


def fill(blk):
  for name in OUTPUTS:
    t = getattr(blk, name)
    (t.view(torch.int32) if t.dtype == torch.float32 else t).fill_(SENT)
  blk.scan_tmp.fill_(-1)


def make_block(csr, S_cap, nnz_cap, ns=True, n_cap=None):
  return Block(S_cap, nnz_cap, csr.shape[1], torch.device("cuda"), negative_sampling=ns, n_cap=n_cap)


def ref_of(csr, implicit, users, blk, ns=None):
  return cu.collate_ref(csr.indptr, csr.indices, None if implicit else csr.data, users,
                        blk.negative_sampling if ns is None else ns, blk.S_cap, blk.nnz_cap, blk.n_cap, blk.n_items,
                        implicit=implicit, ldw_rc=blk.ldw_rc, ldw_cr=blk.ldw_cr)


def same(what, got, want):
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
  if not np.array_equal(got, want):
    bad = np.argwhere(got != want)
    i = tuple(bad[0])
    raise AssertionError("%s: %d of %d differ, first at %s: got %d, expected %d"
                         % (what, len(bad), got.size, i, got[i], want[i]))


def kept(what, got):
  same(what + " (sentinel)", got, np.full(np.shape(got), SENT, dtype=np.int64))


def check_block(blk, ref):
  """Every tensor of the block against the restatement, and the sentinel everywhere else."""
  S, n_b, nnz, wr = ref["S"], ref["n_b"], ref["nnz"], ref["wr"]
  want = ref["counts"].copy()
  want[4] = want[7] = SENT
  same("counts", host(blk.counts), want)
  same("indptr", host(blk.indptr)[:S + 1], ref["indptr"])
  kept("indptr past S", host(blk.indptr)[S + 1:])
  for name in ("cols", "gcols"):
    same(name, host(getattr(blk, name))[:nnz], ref[name])
    kept(name + " past nnz", host(getattr(blk, name))[nnz:])
  same("vals (bits)", host(blk.vals)[:nnz], ref["vals"].view(np.uint32))
  kept("vals past nnz", host(blk.vals)[nnz:])
  kept("svals", host(blk.svals))
  same("items", host(blk.items)[:n_b], ref["items"])
  kept("items past n_b", host(blk.items)[n_b:])
  same("pos", host(blk.pos), ref["pos"])
  for name in ("bits_rc", "pref_rc"):
    got = host(getattr(blk, name)).reshape(blk.S_cap, blk.ldw_rc)
    same(name, got[:S, :wr].view(np.uint32), ref[name].view(np.uint32))
    kept(name + " words past wr", got[:S, wr:])
    kept(name + " rows past S", got[S:])
  same("bits_cr", host(blk.bits_cr).reshape(blk.n_cap, blk.ldw_cr).view(np.uint32), ref["bits_cr"])


def collate_and_check(csr, dcsr, users, blk, phases=(0,)):
  fill(blk)
  u = dev_t(np.asarray(users, dtype=np.int64))
  for p in phases:
    blk.collate(dcsr, u, phase=p)
  torch.cuda.synchronize()
  ref = ref_of(csr, dcsr.data is None, users, blk)
  check_block(blk, ref)
  return ref


def nnz_of(csr, users):
  return int(cu.degrees(csr, users).sum())


@functools.lru_cache(maxsize=None)
def mix():
  return cu.mix_case()


# ------------------------------------------------------------------ scan routes, rk_collate phase 0
@pytest.mark.parametrize("n_items", [1, 3, 4095, 4096, 4097, 65535, 65536, 65537, 67584, 67585])
def test_scan_routes(n_items):
  """collate_scan_small_kernel up to 65 536 items (round and int4 tails), collate_count_kernel +
  collate_assign_kernel above (chunk tails, n_items not a multiple of 8); collate_phase1_kernel and
  collate_build_kernel (one-wave rows) on the way."""
  csr, users = cu.scan_case(n_items)
  stored = np.unique(csr[users].indices)
  assert np.isin(cu.boundary_items(n_items), stored).all() and stored[0] == 0 and stored[-1] == n_items - 1
  blk = make_block(csr, len(users) + 2, nnz_of(csr, users) + 7)
  assert (blk.n_items > cu.SMALL_SCAN_MAX) == (n_items >= 65537) and blk.n_chunks == cu.cdiv(n_items, cu.SCAN_CHUNK)
  ref = collate_and_check(csr, DeviceCSR(csr), users, blk)
  assert ref["n_b"] == len(stored) and not ref["counts"][5] and not ref["counts"][6]


# ------------------------------------------------------------------ rows
MIX_SLICES = {"S_cap": (0, len(cu.MIX_ROWS)), "S1": (5, 1), "S3": (5, 3), "S4": (5, 4), "S5": (5, 5),
              "only_empty_rows": (12, 2)}


@pytest.mark.parametrize("which", list(MIX_SLICES))
def test_rows(which):
  """The row build: empty rows (first, last, two side by side), rows of 1, 63, 64, 65, 511, 512 entries on one wave,
  513, 600, 700, 1100 on four; a workgroup of four heavy rows, one with its only heavy row in wave 2; a light and a
  heavy user three times each; S = 1, 3, 4, 5 and S_cap = 23."""
  csr, users_all = mix()
  first, S = MIX_SLICES[which]
  users = users_all[first:first + S]
  deg = cu.degrees(csr, users)
  S_cap = len(users_all)
  assert S_cap % 4 != 0 and S_cap % 32 != 0
  if which == "S_cap":
    assert S == S_cap and list(deg) == [cu.MIX_NAMED.get(x, x) for x in cu.MIX_ROWS]
    assert (deg[8:12] > cu.BUILD_HEAVY).all() and list(deg[4:8] > cu.BUILD_HEAVY) == [False, False, True, False]
    assert len(set(users)) == S - 4                     # (two users three times each)
  elif which == "only_empty_rows":
    assert not deg.any()
  else:
    assert deg[0] == 511 and (S < 3 or list(deg[1:3]) == [513, 512])
  blk = make_block(csr, S_cap, nnz_of(csr, users_all) + 7)
  ref = collate_and_check(csr, DeviceCSR(csr), users, blk)
  assert ref["nnz"] == deg.sum() and (which != "S_cap" or ref["wr"] > 64)     # (two 64-word rounds of pref_rc)


# ------------------------------------------------------------------ bitmaps wider than one LDS segment
@pytest.mark.parametrize("n_rows,own,stripe,extra", [(64, 1060, 1125, 40), (160, 430, 450, 30)],
                         ids=["heavy_rows", "one_wave_rows"])
def test_wide_bitmap(n_rows, own, stripe, extra):
  """More than 65 536 items in the set: both w0 loops of collate_build_body take two turns and pref_rc carries the
  row's count over the segment boundary -- by four waves (rows of ~1100 entries) and by one (rows of <= 512)."""
  csr, users = cu.wide_case(n_rows, own, stripe, extra)
  deg = cu.degrees(csr, users)
  assert (deg > cu.BUILD_HEAVY).all() if own > cu.BUILD_HEAVY else (deg <= cu.BUILD_HEAVY).all()
  assert csr.nnz <= 75000
  blk = make_block(csr, n_rows + 1, csr.nnz + 7)
  ref = collate_and_check(csr, DeviceCSR(csr), users, blk)
  assert ref["n_b"] > cu.SMALL_SCAN_MAX and ref["wr"] > cu.SEG_WORDS
  crossing = (ref["pref_rc"][:, cu.SEG_WORDS] > 0) & (ref["bits_rc"][:, cu.SEG_WORDS:] != 0).any(axis=1)
  assert crossing.sum() >= n_rows // 2                  # (rows with entries on both sides of the boundary)


# ------------------------------------------------------------------ the whole catalogue as the item set
@pytest.mark.parametrize("n_items", [97, 65537])
def test_without_negative_sampling(n_items):
  csr, users = cu.scan_case(n_items)
  blk = make_block(csr, len(users) + 2, nnz_of(csr, users) + 7, ns=False)
  ref = collate_and_check(csr, DeviceCSR(csr), users, blk)
  assert ref["n_b"] == n_items == blk.n_cap and np.array_equal(ref["cols"], ref["gcols"])
  assert n_items == 97 or ref["wr"] == cu.SEG_WORDS + 1     # (a second segment of one word)


def test_implicit_data():
  csr, users_all = mix()
  csr = csr.copy()
  csr.data[:] = 1.0
  dcsr = DeviceCSR(csr)
  assert dcsr.data is None                              # (the null data pointer)
  users = users_all[4:13]
  ref = collate_and_check(csr, dcsr, users, make_block(csr, 11, nnz_of(csr, users) + 7))
  assert ref["nnz"] > 0 and np.all(ref["vals"] == 1.0)


# ------------------------------------------------------------------ phases
@pytest.mark.parametrize("case", ["mix", "count_assign"])
def test_phase_1_then_2_leaves_what_phase_0_leaves(case):
  csr, users = mix() if case == "mix" else cu.scan_case(67585)
  assert (csr.shape[1] > cu.SMALL_SCAN_MAX) == (case == "count_assign")
  blk = make_block(csr, len(users) + 1, nnz_of(csr, users) + 7)
  dcsr = DeviceCSR(csr)
  collate_and_check(csr, dcsr, users, blk, phases=(1, 2))
  collate_and_check(csr, dcsr, users[::-1].copy(), blk, phases=(0,))
  collate_and_check(csr, dcsr, users, blk, phases=(1, 2))


# ------------------------------------------------------------------ a reused block
@pytest.mark.parametrize("case", ["mix", "count_assign"])
def test_reused_block_holds_nothing_of_the_batch_before(case):
  """A large batch, then a small one at the next stamp: the stamps of the first batch stay in `mark` and must not
  count; pos is -1 outside the small set and bits_cr is zero over the whole capacity."""
  csr, users = mix() if case == "mix" else cu.scan_case(67585)
  small = users[:4] if case == "mix" else users[:1]
  blk = make_block(csr, len(users) + 1, nnz_of(csr, users) + 7)
  dcsr = DeviceCSR(csr)
  big = collate_and_check(csr, dcsr, users, blk)
  ref = collate_and_check(csr, dcsr, small, blk)
  assert 0 < ref["n_b"] < big["n_b"] and (ref["pos"] >= 0).sum() == ref["n_b"]
  assert not ref["bits_cr"][ref["n_b"]:].any() and big["bits_cr"][ref["n_b"]:].any()


# ------------------------------------------------------------------ the cursor forms
def _at(lib, dcsr, order, S, ns, cursor, off0, blks, form, phases=(0,)):
  st = current_stream()
  for blk in blks:
    blk.c.implicit = 1 if dcsr.data is None else 0
  args = (ptr(dcsr.indptr), ptr(dcsr.indices), ptr(dcsr.data), ptr(order), S, 1 if ns else 0, ptr(cursor))
  if form == "at":
    for g, blk in enumerate(blks):
      check(lib.rk_collate_at(*args, off0 + g, blk.ref, st), "rk_collate_at")
    return
  arr = (ctypes.POINTER(RkBlock) * len(blks))(*[ctypes.pointer(blk.c) for blk in blks])
  for p in phases:
    check(lib.rk_collate_at_multi(*args, off0, arr, len(blks), p, st), "rk_collate_at_multi")


@functools.lru_cache(maxsize=None)
def cursor_case(name):
  """csr, order, S, [step, epoch_base], off0 of a case; the order covers two passes of 8 blocks."""
  rng = np.random.RandomState(len(name))
  n_items, S, step, base, off0, heavy = {
      "epoch_base": (700, 5, 7, 4, 0, 0),
      "step_above_2p31": (700, 5, 2 ** 31 + 9, 2 ** 31 + 6, 2, 0),
      "129_rows_4_chunks": (3 * cu.SCAN_CHUNK + 5, 129, 3, 0, 1, 600),
      "300_rows": (700, 300, 1, 1, 0, 600),
      "count_assign": (67585, 5, 2, 0, 3, 0),
  }[name]
  if name == "count_assign":
    csr, _ = cu.scan_case(n_items)
    n_users = csr.shape[0]
  else:
    n_users = 200
    lengths = rng.randint(0, 26, size=n_users)
    lengths[0], lengths[1] = heavy, 0
    csr = cu.csr_from_rows(cu.random_rows(rng, lengths, n_items), n_items, seed=len(name))
  n_blocks = step - base + off0 + 2 * cu.COLLATE_MULTI
  order = rng.randint(0, n_users, size=n_blocks * S).astype(np.int64)      # (a user may come twice in a block)
  if heavy:
    # a heavy and an empty row in every block: the heavy one in the first turn of its workgroup's role loop where a
    # second turn follows (129 rows: row 1, then row 128 by the same workgroup), in a later turn at 300 rows
    order.reshape(n_blocks, S)[:, 1 if S == 129 else 162] = 0
    order.reshape(n_blocks, S)[:, 6] = 1
  return csr, order, S, step, base, off0


@pytest.mark.parametrize("form,G", [("at", 3), ("multi", 1), ("multi", 3), ("multi", 8)])
@pytest.mark.parametrize("name", ["epoch_base", "step_above_2p31", "129_rows_4_chunks", "300_rows", "count_assign"])
def test_cursor_forms(name, form, G):
  """rk_collate_at and rk_collate_at_multi: block g holds rows order[(step - epoch_base + off0 + g) * S ...], every
  block against the restatement of its own slice; then the same blocks again at a later cursor."""
  lib = _lib.load()
  csr, order, S, step, base, off0 = cursor_case(name)
  n_items = csr.shape[1]
  if name == "129_rows_4_chunks":
    assert cu.cdiv(n_items, cu.SCAN_CHUNK) >= 3 and n_items <= cu.SMALL_SCAN_MAX and cu.cdiv(S, 4) > 32
  if name == "300_rows":
    assert cu.cdiv(S, 4) > 2 * 32
  if name == "count_assign":
    assert n_items > cu.SMALL_SCAN_MAX
  dcsr = DeviceCSR(csr)
  slices = order.reshape(-1, S)
  nnz_cap = max(nnz_of(csr, s) for s in slices) + 3
  blks = [make_block(csr, S + 1, nnz_cap) for _ in range(G)]
  order_d = dev_t(order)
  for rep in range(2):
    cursor = dev_t(np.array([step + rep * G, base], dtype=np.int64))
    for blk in blks:
      fill(blk)
    _at(lib, dcsr, order_d, S, True, cursor, off0, blks, form)
    torch.cuda.synchronize()
    for g, blk in enumerate(blks):
      users = slices[step + rep * G - base + off0 + g]
      ref = ref_of(csr, False, users, blk)
      if name in ("129_rows_4_chunks", "300_rows"):
        deg = cu.degrees(csr, users)
        assert deg.max() > cu.BUILD_HEAVY and deg.min() == 0
        # (marked items in every chunk that another one looks back at)
        assert name == "300_rows" or all((ref["items"] // cu.SCAN_CHUNK == c).any() for c in range(3))
      check_block(blk, ref)
      blk.check()


def test_cursor_set_writes_the_two_words_a_collation_reads():
  """rk_cursor_set (cursor_set_kernel): [step, epoch_base] and nothing behind them; rk_collate_at then takes its
  rows from that cursor."""
  lib = _lib.load()
  csr, order, S, _, _, off0 = cursor_case("step_above_2p31")
  step, base = 2 ** 33 + 5, 2 ** 33 + 1
  cursor = torch.full((4,), -7, dtype=torch.int64, device="cuda")
  check(lib.rk_cursor_set(ptr(cursor), step, base, current_stream()), "rk_cursor_set")
  blk = make_block(csr, S + 1, max(nnz_of(csr, s) for s in order.reshape(-1, S)) + 3)
  fill(blk)
  _at(lib, DeviceCSR(csr), dev_t(order), S, True, cursor, off0, [blk], "at")
  torch.cuda.synchronize()
  assert cursor.tolist() == [step, base, -7, -7]
  check_block(blk, ref_of(csr, False, order.reshape(-1, S)[step - base + off0], blk))


@pytest.mark.parametrize("name", ["129_rows_4_chunks", "count_assign"])
def test_cursor_multi_phase_1_then_2(name):
  lib = _lib.load()
  csr, order, S, step, base, off0 = cursor_case(name)
  dcsr = DeviceCSR(csr)
  slices = order.reshape(-1, S)
  G = 3
  blks = [make_block(csr, S + 1, max(nnz_of(csr, s) for s in slices) + 3) for _ in range(G)]
  for k, phases in enumerate(((1, 2), (0,), (1, 2))):
    cursor = dev_t(np.array([step + 2 * k, base], dtype=np.int64))
    for blk in blks:
      fill(blk)
    _at(lib, dcsr, dev_t(order), S, True, cursor, off0, blks, "multi", phases)
    torch.cuda.synchronize()
    for g, blk in enumerate(blks):
      check_block(blk, ref_of(csr, False, slices[step + 2 * k - base + off0 + g], blk))


# ------------------------------------------------------------------ truncated blocks
@pytest.mark.parametrize("short", ["n_cap", "nnz_cap"])
@pytest.mark.parametrize("route", ["one_workgroup", "look_back", "count_assign", "count_assign_multi"])
def test_truncated_block(route, short):
  """A block with too few item slots, or too few entry slots, on every scan route: the arrays are the restatement's
  truncated form, nothing beside the block is touched, and Block.check() raises."""
  lib = _lib.load()
  n_items = 67585 if route.startswith("count_assign") else 5000
  rng = np.random.RandomState(n_items)
  lengths = rng.randint(0, 41, size=80)
  csr = cu.csr_from_rows(cu.random_rows(rng, lengths, n_items), n_items, seed=7)
  multi = route in ("look_back", "count_assign_multi")
  G, S = (2, 32) if multi else (1, 64)
  order = rng.randint(0, 80, size=G * S).astype(np.int64)
  slices = order.reshape(G, S)
  n_true = [len(np.unique(csr[s].indices)) for s in slices]
  nnz_true = [nnz_of(csr, s) for s in slices]
  assert (n_items > cu.SMALL_SCAN_MAX) == route.startswith("count_assign") and cu.cdiv(n_items, cu.SCAN_CHUNK) >= 3
  if short == "n_cap":
    nnz_cap, n_cap = max(nnz_true) + 5, min(n_true) - 17
  else:
    nnz_cap, n_cap = min(nnz_true) - 13, max(n_true) + 5
  guards, blks = [torch.full((4096,), 12345, dtype=torch.int32, device="cuda")], []
  for g in range(G):
    blks.append(make_block(csr, S + 1, nnz_cap, n_cap=n_cap))
    guards.append(torch.full((4096,), 12345, dtype=torch.int32, device="cuda"))
  dcsr = DeviceCSR(csr)
  for blk in blks:
    fill(blk)
  if multi:
    _at(lib, dcsr, dev_t(order), S, True, dev_t(np.array([5, 5], dtype=np.int64)), 0, blks, "multi")
  else:
    blks[0].collate(dcsr, dev_t(order))
  torch.cuda.synchronize()
  for g, blk in enumerate(blks):
    ref = ref_of(csr, False, slices[g], blk)
    if short == "n_cap":
      assert ref["counts"][5] == n_true[g] > blk.n_cap == ref["n_b"] and not ref["counts"][6]
      assert (ref["vals"] == 0).any() and (ref["vals"] != 0).any()
    else:
      assert ref["counts"][6] == nnz_true[g] > blk.nnz_cap == ref["nnz"] and not ref["counts"][5]
    check_block(blk, ref)
    with pytest.raises(RecoderHipError):
      blk.check()
  assert all(bool((x == 12345).all()) for x in guards)


# ------------------------------------------------------------------ rk_lazy_need_lists
def _pos_maps(N, rng):
  """Eight pos maps whose consecutive pairs give: an empty list, a full one, one that ends at N - 1, one whose
  last chunk contributes nothing, and random ones."""
  last0 = (cu.cdiv(N, cu.SCAN_CHUNK) - 1) * cu.SCAN_CHUNK          # first id of the last chunk
  ends = np.union1d(rng.choice(N, size=min(N, 50), replace=False), [N - 1])
  front = lambda: rng.choice(last0, size=min(last0, 300), replace=False) if last0 else np.zeros(0, np.int64)
  rand = np.nonzero(rng.rand(N) < 0.3)[0]
  sets = [[], [], np.arange(N), ends, front(), [], rand, front()]
  maps = []
  for ids in sets:
    pos = np.full(N, -1, dtype=np.int32)
    pos[np.asarray(ids, dtype=np.int64)] = np.arange(len(ids), dtype=np.int32)
    maps.append(pos)
  return maps


def _need_lists(lib, maps_dev, N, n_chunks=None):
  n = len(maps_dev)
  blks = [RkBlock() for _ in range(n)]
  for b, pos in zip(blks, maps_dev):
    b.n_items, b.n_chunks, b.pos = N, cu.cdiv(N, cu.SCAN_CHUNK) if n_chunks is None else n_chunks, ptr(pos)
  arr = (ctypes.POINTER(RkBlock) * n)(*[ctypes.pointer(b) for b in blks])
  lists = [torch.full((N + 8,), -7, dtype=torch.int32, device="cuda") for _ in range(n - 1)]
  counts = [torch.full((4,), -7, dtype=torch.int32, device="cuda") for _ in range(n - 1)]
  lp = (ctypes.c_void_p * n)(*[x.data_ptr() for x in lists], None)
  cp = (ctypes.c_void_p * n)(*[x.data_ptr() for x in counts], None)
  rc = lib.rk_lazy_need_lists(arr, n, lp, cp, current_stream())
  torch.cuda.synchronize()
  return rc, lists, counts


@pytest.mark.parametrize("n_blk", [2, 8])
@pytest.mark.parametrize("N", [1, 2047, 2048, 2049, 4097, cu.NEED_LIST_MAX_ITEMS])
def test_need_lists(N, n_blk):
  lib = _lib.load()
  assert cu.NEED_LIST_MAX_ITEMS == 131072
  maps = _pos_maps(N, np.random.RandomState(N))
  # two blocks: the pairs (empty, empty), (full, empty), (ends at N - 1, front), (front, front)
  groups = [maps] if n_blk == 8 else [[maps[0], maps[1]], [maps[2], maps[5]], [maps[3], maps[4]], [maps[4], maps[7]]]
  seen = set()
  for group in groups:
    rc, lists, counts = _need_lists(lib, [dev_t(m) for m in group], N)
    assert rc == 0
    for i in range(len(group) - 1):
      want = cu.need_lists_ref(group[i], group[i + 1])
      got_n = counts[i].cpu().numpy()
      got = lists[i].cpu().numpy()
      assert got_n[0] == len(want) and np.all(got_n[1:] == -7)
      same("need list", got[:len(want)], want)
      assert np.all(got[len(want):] == -7)              # (nothing written past the count)
      last0 = (cu.cdiv(N, cu.SCAN_CHUNK) - 1) * cu.SCAN_CHUNK
      seen.update(["empty"] if len(want) == 0 else
                  [what for what, holds in (("full", len(want) == N), ("ends_at_last_id", want[-1] == N - 1),
                                            ("nothing_in_last_chunk", want[-1] < last0)) if holds])
  assert {"empty", "full", "ends_at_last_id"} <= seen and (N <= cu.SCAN_CHUNK or "nothing_in_last_chunk" in seen)


def test_need_lists_refusals_launch_nothing():
  lib = _lib.load()
  N = cu.NEED_LIST_MAX_ITEMS + 1
  full = [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in range(2)]
  rc, lists, counts = _need_lists(lib, full, N)
  assert rc < 0 and b"RK_NEED_LIST_MAX_ITEMS" in lib.rk_last_error()
  assert bool((lists[0] == -7).all()) and bool((counts[0] == -7).all())
  base = [torch.zeros(104, dtype=torch.int32, device="cuda") for _ in range(2)]
  assert base[0].data_ptr() % 16 == 0
  rc, lists, counts = _need_lists(lib, [base[0][1:101], base[1][:100]], 100)
  assert rc < 0 and b"16-byte aligned" in lib.rk_last_error()
  assert bool((lists[0] == -7).all()) and bool((counts[0] == -7).all())
  rc, lists, counts = _need_lists(lib, [base[0][:100], base[1][:100]], 100)
  assert rc == 0 and int(counts[0][0]) == 100


# ------------------------------------------------------------------ rk_densify
def test_densify():
  lib = _lib.load()
  rng = np.random.RandomState(11)
  lengths = [0, 300, 7, 0, 64, 1, 257, 0, 33]
  csr = cu.csr_from_rows(cu.random_rows(rng, lengths, 600), 600, seed=11)
  users = rng.permutation(len(lengths)).astype(np.int64)
  S = len(users)
  blk = make_block(csr, S + 2, csr.nnz + 7)
  ref = collate_and_check(csr, DeviceCSR(csr), users, blk)
  n = ref["n_b"]
  deg = cu.degrees(csr, users)
  empty = int(np.nonzero(deg == 0)[0][1])                 # (an empty row that is not the first)
  assert n > 256 and deg.max() > 256 and empty > 0        # (more than one pass of a workgroup over columns / entries)
  CANARY = np.float32(-77.25)
  for row_off, B, pad in [(0, S, 0), (empty - 1, 3, 9), (empty, 1, 5), (S - 1, 1, 0), (2, 4, 700)]:
    ld = n + pad
    out = torch.full((B * ld + 64,), float(CANARY), dtype=torch.float32, device="cuda")
    check(lib.rk_densify(blk.ref, row_off, B, n, ptr(out), ld, current_stream()), "rk_densify")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    dense = got[:B * ld].reshape(B, ld)
    want = cu.densify_ref(ref, row_off, B, n)
    same("dense", dense[:, :n].view(np.uint32), want.view(np.uint32))
    assert np.all(dense[:, n:] == CANARY) and np.all(got[B * ld:] == CANARY)
    assert np.array_equal(want, csr[users[row_off:row_off + B]][:, ref["items"]].toarray())
  out = torch.full((64,), float(CANARY), dtype=torch.float32, device="cuda")
  assert lib.rk_densify(blk.ref, 1, 0, n, ptr(out), n, current_stream()) == 0      # B = 0
  assert lib.rk_densify(blk.ref, 1, 2, 0, ptr(out), 8, current_stream()) == 0      # n = 0
  torch.cuda.synchronize()
  assert bool((out == float(CANARY)).all())
