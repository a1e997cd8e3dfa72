"""The encoder forward (csrc/encoder.hip: rk_ae_encode_fwd, _partial, _split_w) and the counter-RNG input
noise (rk_keep_draw of csrc/common.h, also behind rk_dropout) called DIRECTLY, against the float64 / numpy
restatements of tests/encoder_util.py, at the kernel's own edges: a row cut over FW = 8 waves
(q = ceil(n / 8)), the second 64-entry pass from n = 513, the min(..., h - 4) column clamp, hv == 3 on the
HV = 4 instantiation, the ballot walk over dropped entries, and svals as the side product the backward
trusts.  Every tolerance is a counted rounding bound (the count stands next to the assertion)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from recoder_amd import _lib
from recoder_amd._lib import RkPlanes, check, ptr
from recoder_amd.device import Block, DeviceCSR, current_stream
from tests import encoder_util as eu
from tests.encoder_util import ACT_NONE, ACTS, U, gamma

gpu = pytest.mark.gpu

# one row per wave-split / second-pass edge plus an empty user (rows 0..11), and four more rows so that a
# 7-row window at row_off = 5 lies inside a 16-row block
LENS = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1100, 20, 33, 2, 130]
N_USERS, N_ITEMS = 1100, 1300
HS = [4, 8, 36, 64, 200, 256, 260, 512, 516, 600, 768, 772, 1024]
CANARY = 12345.0
TAIL = 1200                  # canary floats behind Z0: more than any lane's column offset (<= 1020 + 4)
SEED_HI = 2 ** 63 + 12345


def user_of(row):
  """the non-identity map of the tests: ids far above the row index"""
  return 1000 + 3 * row


class Case:
  pass


@functools.lru_cache(maxsize=None)
def _case(ratings):
  """The 16-row block (built once per kind; the tests only rewrite svals)."""
  dev = torch.device("cuda")
  c = Case()
  c.users_np = np.array([user_of(r) for r in range(len(LENS))], dtype=np.int64)
  c.csr = eu.csr_with_row_lengths(LENS, c.users_np, N_USERS, N_ITEMS, seed=11 + int(ratings), ratings=ratings)
  c.dcsr = DeviceCSR(c.csr)
  c.users = torch.from_numpy(c.users_np).to(dev)
  c.nnz = int(sum(LENS))
  c.blk = Block(len(LENS), c.nnz, N_ITEMS, dev).collate(c.dcsr, c.users)
  sub = c.csr[c.users_np]
  c.indptr = c.blk.indptr[:len(LENS) + 1].cpu().numpy()
  c.gcols = c.blk.gcols[:c.nnz].cpu().numpy()
  # the block's rows are the CSR's rows, entry for entry
  assert np.array_equal(c.indptr, sub.indptr) and np.array_equal(c.gcols, sub.indices)
  assert list(np.diff(c.indptr)) == LENS
  assert bool(c.blk.c.implicit) == (not ratings)
  if ratings:
    assert np.array_equal(c.blk.vals[:c.nnz].cpu().numpy(), sub.data)
    # a few stored values become 0 (the collation never leaves one; the kernel must still write s = 0 and skip)
    zero = np.random.RandomState(5).choice(c.nnz, size=40, replace=False)
    c.blk.vals[torch.from_numpy(zero).to(dev)] = 0.0
    c.vals = c.blk.vals[:c.nnz].cpu().numpy()
  else:
    c.blk.vals.fill_(float("nan"))          # implicit: vals is not read
    c.vals = np.ones(c.nnz, np.float32)
  c.keep_np = (np.random.RandomState(7).rand(c.nnz) < 0.5).astype(np.uint8)
  c.keep = torch.from_numpy(c.keep_np).to(dev)
  return c


@functools.lru_cache(maxsize=None)
def _params(h, n_items=N_ITEMS):
  rng = np.random.RandomState(1000 + h)
  W = (rng.randn(n_items, h) * 0.1).astype(np.float32)
  b = (rng.randn(h) * 0.05).astype(np.float32)
  dev = torch.device("cuda")
  return W, b, torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev)


def _fwd(blk, row_off, B, Wd, bd, h, keep, p, seed, step, users, act, partial=False, user_norm=None):
  """One launch into a canary-filled buffer: ([B, h] output, the buffer's tail untouched)."""
  lib = _lib.load()
  Z = torch.full((B * h + TAIL,), CANARY, dtype=torch.float32, device=Wd.device)
  if partial:
    check(lib.rk_ae_encode_fwd_partial(blk.ref, row_off, B, ptr(Wd), h, ptr(keep), p, seed, step, ptr(users),
                                       ptr(user_norm), ptr(Z), current_stream()), "rk_ae_encode_fwd_partial")
  else:
    check(lib.rk_ae_encode_fwd(blk.ref, row_off, B, ptr(Wd), ptr(bd), h, ptr(keep), p, seed, step, ptr(users),
                               act, ptr(Z), current_stream()), "rk_ae_encode_fwd")
  torch.cuda.synchronize()
  assert bool((Z[B * h:] == CANARY).all()), "h = %d: the launch wrote behind row B of Z0" % h
  return Z[:B * h].view(B, h)


def _bias_act(X, bd, act):
  lib = _lib.load()
  X = X.clone()
  check(lib.rk_bias_act(ptr(X), ptr(bd), X.shape[0], X.shape[1], act, current_stream()), "rk_bias_act")
  torch.cuda.synchronize()
  return X


# ------------------------------------------------------------------ the restatement alone (no GPU)
def test_keep_draw_restatement_is_a_fair_coin_keyed_by_step():
  n = 200000
  a = np.arange(n, dtype=np.uint64) // np.uint64(500) + np.uint64(1000)
  b = np.arange(n, dtype=np.uint64) % np.uint64(500)
  for p in (0.2, 0.5):
    k1 = eu.keep_draw(SEED_HI, 3, a, b, p)
    k2 = eu.keep_draw(SEED_HI, 4, a, b, p)
    for k in (k1, k2):
      # binomial: mean n (1 - p), standard deviation sqrt(n p (1 - p)); 4 of them
      assert abs(int(k.sum()) - n * (1 - p)) <= 4 * np.sqrt(n * p * (1 - p))
    assert not np.array_equal(k1, k2)
  u = eu.keep_uniform(0, 0, a, b)
  assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
  # wrapping arithmetic: a seed above 2^63 plus the step constant overflows 64 bits
  assert eu.mix64(np.uint64(2 ** 64 - 1)).dtype == np.uint64


# ------------------------------------------------------------------ svals and the accumulation
def _svals_c(n, ratings, p):
  """Roundings between the exact s_j and the kernel's: the square root, the quotient, the product with the
  scale and the scale constant (one each: 4); a rated row adds HALF (the square root halves a relative
  error) the roundings of its sum of squares: ceil(n / 512) strided adds per thread, the 6 steps of the
  wave sum and the 8 combines."""
  c = 4.0
  if ratings:
    c += 0.5 * (-(-n // 512) + 6 + 8)
  return c


@gpu
@pytest.mark.parametrize("h", HS)
def test_svals_and_preactivation_against_float64(h):
  W, b, Wd, bd = _params(h)
  for ratings in (False, True):
    c = _case(ratings)
    for p in (0.0, 0.5):
      tag = "h = %d, %s, p = %g" % (h, "rated" if ratings else "implicit", p)
      c.blk.svals.fill_(CANARY)
      # (keep is passed at p = 0 too: it must be ignored there)
      Z = _fwd(c.blk, 0, len(LENS), Wd, bd, h, c.keep, p, 1, 1, c.users, ACT_NONE).cpu().numpy()
      s = c.blk.svals[:c.nnz].cpu().numpy()
      s64 = eu.svals64(c.indptr, c.vals, c.keep_np, p)
      # zero if and only if dropped or a zero value
      want_zero = (c.vals == 0) | ((c.keep_np == 0) if p > 0 else False)
      assert np.array_equal(s == 0, want_zero), tag
      assert np.array_equal(s64 == 0, want_zero)
      for r, n in enumerate(LENS):
        a, e = c.indptr[r], c.indptr[r + 1]
        err = np.abs(s[a:e].astype(np.float64) - s64[a:e])
        assert np.all(err <= _svals_c(n, ratings, p) * U * np.abs(s64[a:e])), "%s: svals of the row of %d" % (tag, n)
      # the accumulation alone: float64 on the svals the device wrote
      Z64, A = eu.encode64(c.indptr, c.gcols, s, W, b)
      for r, n in enumerate(LENS):
        # the longest wave chain ceil(n / 8) fused multiply-adds, seven combines and the bias add
        k = -(-n // 8) + 8
        err = np.abs(Z[r].astype(np.float64) - Z64[r])
        assert np.all(err <= gamma(k) * A[r]), "%s: row of %d entries, worst column %d" % (tag, n, int(err.argmax()))
      assert np.array_equal(Z[0], b), tag + ": the empty row is act(b)"


@gpu
@pytest.mark.parametrize("h", [4, 36, 260, 600])
def test_activation_equals_partial_then_bias_act_bit_for_bit(h):
  W, b, Wd, bd = _params(h)
  c = _case(False)
  for act in ACTS:
    full = _fwd(c.blk, 0, len(LENS), Wd, bd, h, c.keep, 0.5, 1, 1, c.users, act)
    part = _fwd(c.blk, 0, len(LENS), Wd, None, h, c.keep, 0.5, 1, 1, c.users, ACT_NONE, partial=True)
    assert torch.equal(full, _bias_act(part, bd, act)), "h = %d, act = %d" % (h, act)


@gpu
@pytest.mark.parametrize("h", [36, 516])
def test_row_window_writes_its_rows_only(h):
  W, b, Wd, bd = _params(h)
  row_off, B = 5, 7
  for ratings in (False, True):
    c = _case(ratings)
    whole = _fwd(c.blk, 0, len(LENS), Wd, bd, h, c.keep, 0.5, 1, 1, c.users, 1)
    s_whole = c.blk.svals[:c.nnz].clone()
    c.blk.svals.fill_(CANARY)
    win = _fwd(c.blk, row_off, B, Wd, bd, h, c.keep, 0.5, 1, 1, c.users, 1)       # (checks the canary behind row B)
    assert torch.equal(win, whole[row_off:row_off + B])
    s = c.blk.svals[:c.nnz]
    a, e = int(c.indptr[row_off]), int(c.indptr[row_off + B])
    assert torch.equal(s[a:e], s_whole[a:e])
    assert bool((s[:a] == CANARY).all()) and bool((s[e:] == CANARY).all())
    assert bool((c.blk.svals[c.nnz:] == CANARY).all())


# ------------------------------------------------------------------ the drawn noise
def _drawn_pattern(blk, B, nnz, p, seed, step, users, h=8):
  W, b, Wd, bd = _params(h)
  blk.svals.fill_(CANARY)
  _fwd(blk, 0, B, Wd, bd, h, None, p, seed, step, users, ACT_NONE)
  s = blk.svals[:nnz].cpu().numpy()
  assert not np.any(s == CANARY)
  return s != 0


@gpu
@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("seed", [0, SEED_HI])
def test_drawn_noise_is_keyed_by_seed_step_user_id_and_item_id(p, seed):
  c = _case(False)
  R = len(LENS)
  row_of = np.repeat(np.arange(R), LENS)
  uid_of = c.users_np[row_of]
  got = _drawn_pattern(c.blk, R, c.nnz, p, seed, 7, c.users)
  # every entry: the draw of (seed, step, users[row], global item id)
  assert np.array_equal(got, eu.keep_draw(seed, 7, uid_of, c.gcols, p))
  assert not np.array_equal(got, eu.keep_draw(seed, 7, row_of, c.gcols, p))      # (keyed by row: another pattern)
  # another step: another pattern, again the restatement's
  got8 = _drawn_pattern(c.blk, R, c.nnz, p, seed, 8, c.users)
  assert np.array_equal(got8, eu.keep_draw(seed, 8, uid_of, c.gcols, p))
  assert not np.array_equal(got8, got)
  # users == NULL: the key is the block row
  got_rows = _drawn_pattern(c.blk, R, c.nnz, p, seed, 7, None)
  assert np.array_equal(got_rows, eu.keep_draw(seed, 7, row_of, c.gcols, p))
  # the same users in another block, at other rows with other batch mates: the same pattern per user
  order = [11, 3, 9, 1, 15]
  users2 = torch.from_numpy(c.users_np[order]).to(c.users.device)
  nnz2 = int(sum(LENS[r] for r in order))
  blk2 = Block(len(order), nnz2, N_ITEMS, c.users.device).collate(c.dcsr, users2)
  got2 = _drawn_pattern(blk2, len(order), nnz2, p, seed, 7, users2)
  ip2 = blk2.indptr[:len(order) + 1].cpu().numpy()
  for i, r in enumerate(order):
    assert np.array_equal(got2[ip2[i]:ip2[i + 1]], got[c.indptr[r]:c.indptr[r + 1]]), "user %d" % user_of(r)


@gpu
@pytest.mark.parametrize("ncols", [1, 24, 200])
@pytest.mark.parametrize("p", [0.2, 0.5])
def test_dropout_draw_and_scale(ncols, p):
  lib = _lib.load()
  n = 3 * ncols                           # 3, 72, 600: none a multiple of the 256-thread workgroup
  x = (np.random.RandomState(ncols).randn(n) * 3).astype(np.float32)
  for seed, step in ((0, 1), (SEED_HI, 9)):
    X = torch.full((n + 64,), CANARY, dtype=torch.float32, device="cuda")
    X[:n] = torch.from_numpy(x)
    check(lib.rk_dropout(ptr(X), None, n, ncols, p, seed, step, current_stream()), "rk_dropout")
    torch.cuda.synchronize()
    got = X.cpu().numpy()
    i = np.arange(n, dtype=np.uint64)
    keep = eu.keep_draw(seed, step, i // np.uint64(ncols) + np.uint64(0x51ed270b1), i % np.uint64(ncols), p)
    assert np.array_equal(got[:n] != 0, keep & (x != 0))
    # kept: x * fl(1 / (1 - p)), one fp32 product; dropped: +-0
    assert np.array_equal(got[:n][keep], (x * eu.keep_scale(p))[keep])
    assert np.all(got[:n][~keep] == 0)
    assert np.all(got[n:] == CANARY)


# ------------------------------------------------------------------ column shards (user_norm)
@gpu
@pytest.mark.parametrize("h", [36, 600])
def test_partial_sums_of_two_column_shards_with_whole_row_norms(h):
  c = _case(True)
  dev = c.users.device
  W, b, Wd, bd = _params(h)
  R, cut = len(LENS), 650
  sub = c.csr[c.users_np]
  norm64 = np.sqrt(np.asarray(sub.multiply(sub).sum(axis=1), dtype=np.float64)).ravel()
  tab = np.full(N_USERS, np.nan, np.float32)             # per GLOBAL user id, longer than the batch
  tab[c.users_np] = norm64.astype(np.float32)
  tabd = torch.from_numpy(tab).to(dev)
  Zs, Z64, A, nmax = None, np.zeros((R, h)), np.zeros((R, h)), np.zeros(R, dtype=np.int64)
  for lo, hi in ((0, cut), (cut, N_ITEMS)):
    shard = c.csr[:, lo:hi].tocsr()
    dsh = DeviceCSR(shard)
    nnz = int(shard[c.users_np].nnz)
    blk = Block(R, nnz, hi - lo, dev).collate(dsh, c.users)
    ip = blk.indptr[:R + 1].cpu().numpy()
    gc = blk.gcols[:nnz].cpu().numpy()
    Wsh = Wd[lo:hi].contiguous()
    Zp = _fwd(blk, 0, R, Wsh, None, h, None, 0.0, 1, 1, c.users, ACT_NONE, partial=True, user_norm=tabd)
    s = blk.svals[:nnz].cpu().numpy()
    # two roundings: the norm table's entry and the quotient
    s64 = eu.svals64(ip, blk.vals[:nnz].cpu().numpy(), None, 0.0, norms=norm64)
    assert np.all(np.abs(s - s64) <= 2 * U * np.abs(s64))
    z, a = eu.encode64(ip, gc, s, W[lo:hi])
    Z64 += z
    A += a
    nmax = np.maximum(nmax, np.diff(ip))
    Zs = Zp if Zs is None else Zs + Zp
  Z = _bias_act(Zs, bd, ACT_NONE).cpu().numpy()
  Z64 += b.astype(np.float64)
  A += np.abs(b.astype(np.float64))
  assert nmax.max() > 512 // 2
  for r in range(R):
    # the longer shard's wave chain + seven combines + the bias add, and the add of the two partials
    k = -(-int(nmax[r]) // 8) + 8 + 1
    assert np.all(np.abs(Z[r] - Z64[r]) <= gamma(k) * A[r]), "row of %d entries" % LENS[r]


@gpu
def test_partial_with_sqrt_n_norms_equals_the_implicit_norm_bit_for_bit():
  h = 64
  c = _case(False)
  W, b, Wd, bd = _params(h)
  tab = np.full(N_USERS, np.nan, np.float32)
  tab[c.users_np] = np.sqrt(np.asarray(LENS, dtype=np.float32))        # sqrtf(n_u) in fp32
  tabd = torch.from_numpy(tab).to(c.users.device)
  own = _fwd(c.blk, 0, len(LENS), Wd, None, h, c.keep, 0.5, 1, 1, c.users, ACT_NONE, partial=True)
  s_own = c.blk.svals[:c.nnz].clone()
  ext = _fwd(c.blk, 0, len(LENS), Wd, None, h, c.keep, 0.5, 1, 1, c.users, ACT_NONE, partial=True, user_norm=tabd)
  assert torch.equal(own, ext) and torch.equal(s_own, c.blk.svals[:c.nnz])


# ------------------------------------------------------------------ the launch that also splits W_de
@gpu
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("h", [36, 64])
def test_split_w_launch_equals_the_plain_forward_and_rk_split_wz(B, h):
  lib = _lib.load()
  dev = torch.device("cuda")
  n_items = 300
  rng = np.random.RandomState(B + h)
  lens = rng.randint(1, 40, size=B)
  users_np = np.arange(B, dtype=np.int64) * 2 + 1
  csr = eu.csr_with_row_lengths(lens, users_np, 2 * B + 2, n_items, seed=B, ratings=True)
  users = torch.from_numpy(users_np).to(dev)
  nnz = int(lens.sum())
  blk = Block(B, nnz, n_items, dev).collate(DeviceCSR(csr), users)
  W, b, Wd, bd = _params(h, n_items)
  W_de = torch.from_numpy((rng.randn(n_items, h) * 0.07).astype(np.float32)).to(dev)
  keep = torch.from_numpy((rng.rand(nnz) < 0.5).astype(np.uint8)).to(dev)
  ranges = torch.zeros(128, dtype=torch.int32, device=dev)
  ranges[64:65].copy_(W_de.abs().max().reshape(1).view(torch.int32))
  st = current_stream()

  def planes():
    buf = torch.zeros(lib.rk_planes_bytes(B, h, blk.n_cap) // 4 + 64, dtype=torch.float32, device=dev)
    pl = RkPlanes()
    check(lib.rk_planes_layout(ptr(buf), B, h, blk.n_cap, ctypes.byref(pl)))
    return buf, pl
  plain = _fwd(blk, 0, B, Wd, bd, h, keep, 0.5, 1, 1, users, 1)
  s_plain = blk.svals[:nnz].clone()
  blk.svals.fill_(CANARY)
  buf1, pl1 = planes()
  Z = torch.full((B * h + TAIL,), CANARY, dtype=torch.float32, device=dev)
  check(lib.rk_ae_encode_fwd_split_w(blk.ref, 0, B, ptr(Wd), ptr(bd), h, ptr(keep), 0.5, 1, 1, ptr(users), 1, ptr(Z),
                                     ptr(W_de), ptr(ranges), ctypes.byref(pl1), st), "rk_ae_encode_fwd_split_w")
  buf2, pl2 = planes()
  check(lib.rk_split_wz(ptr(W_de), None, B, h, blk.ref, ptr(ranges), ctypes.byref(pl2), None, st), "rk_split_wz")
  torch.cuda.synchronize()
  assert torch.equal(Z[:B * h].view(B, h), plain) and bool((Z[B * h:] == CANARY).all())
  assert torch.equal(blk.svals[:nnz], s_plain)
  assert torch.equal(buf1.view(torch.int32), buf2.view(torch.int32))        # scales, W image, W^T image
  assert bool((buf2.view(torch.int32) != 0).any())


# ------------------------------------------------------------------ argument checks (no launch)
@gpu
def test_host_refusals_leave_a_message_and_the_next_call_succeeds():
  lib = _lib.load()
  c = _case(False)
  R, st = len(LENS), current_stream()
  W, b, Wd, bd = _params(1024)
  Z = torch.zeros(R * 1024 + 64, dtype=torch.float32, device=Wd.device)
  tab = torch.ones(N_USERS, dtype=torch.float32, device=Wd.device)

  def fwd(row_off=0, B=R, h=8, p=0.0):
    return lib.rk_ae_encode_fwd(c.blk.ref, row_off, B, ptr(Wd), ptr(bd), h, None, p, 1, 1, ptr(c.users), 0, ptr(Z), st)
  refusals = {
    "h = 6": lambda: fwd(h=6),
    "h = 1028": lambda: fwd(h=1028),
    "p = 1": lambda: fwd(p=1.0),
    "row_off + B > S_cap": lambda: fwd(row_off=R - 2, B=3),
    "user_norm without users": lambda: lib.rk_ae_encode_fwd_partial(c.blk.ref, 0, R, ptr(Wd), 8, None, 0.0, 1, 1, None,
                                                                   ptr(tab), ptr(Z), st),
  }
  for name, call in refusals.items():
    assert call() != 0, name
    assert len(lib.rk_last_error()) > 0, name
    assert fwd() == 0, "the valid call after '%s'" % name
  torch.cuda.synchronize()
