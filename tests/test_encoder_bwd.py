"""GPU: the encoder backward (csrc/encoder.hip rk_ae_encode_bwd, bodies in csrc/encoder_bwd.h) called DIRECTLY on
every launch route of its host dispatch -- a wave per column with one or two bitmap words per lane, each in the
eight-deep and in the light form, the recursion over row windows, a workgroup per column -- at HV = 1, 2 and 4,
against float64 of the block's own indptr / cols / svals:

  G_en[c] = sum over the window's rows r of svals[r, c] dZ[r],     gb_en = the column sums of dZ.

Every case is checked twice.  EXACT data (svals in {0, 1/2, 1, 2}, dZ and the accumulate prefill small integers
times 2^-6): every partial sum is fewer than 2^18 units of 2^-7, exact in fp32 in any order, so the result must
equal float64 bit for bit -- a dropped, doubled or misplaced entry cannot hide.  GENERIC data (svals ~ U(0, 1), half
of them exactly 0, dZ ~ 1e-2 N(0, 1)) within the fused-multiply-add chain bound

  |got - want| <= (n_c + 8) 2^-24 sum_r |s[r, c] dZ[r, j]|   (+ 2^-24 |prefill| per add onto the prefilled row)

with n_c the column's stored entries in the window (B for gb_en): n_c roundings of the chain, 8 for the three
wave-combine adds, the accumulate add and one add per further window.  The prefill term is the rounding of
fl(prefill + sum): its magnitude is the prefill's, which the entry sum does not contain.

The blocks are collated from hand-made CSRs (tests/encoder_util.py csr_with_column_rows), so the column populations
are exact: none, 1, 8, 9, 64 (the last one-wave column), 65 (the first one split over the four waves), 301
(quarters that are no multiple of 64), every row, all entries dropped.  The table of cases is checked against the
restated dispatch (encoder_util.bwd_route), so a moved threshold shows as a lost route.

The dZ slab reduces (rk_decode_dz_reduce, rk_fdec_dz_reduce, rk_decode_bwd_dw2_dz_reduce) with act'(Z) folded in
stand at the end of the file."""
import functools
import types

import numpy as np
import pytest
import torch

from recoder_amd import _lib
from recoder_amd._lib import check, ptr
from recoder_amd.device import Block, DeviceCSR, current_stream
from tests import encoder_util as eu
from tests.encoder_util import ACTS, U
from tests.test_hip_parity import synth_csr

gpu = pytest.mark.gpu

CANARY = 12345.0
TAIL = 1200                   # canary floats behind G_en: more than any lane's column offset (<= 1020 + 4)
POPS = (1, 8, 9, 64, 65, 301)


# ------------------------------------------------------------------ the blocks
def _design(name):
  """The hand-made matrix of one block and its capacities (host only).  win: the window the populations are
  counted in; special: name -> item id."""
  d = types.SimpleNamespace(name=name, ratings=False, ns=True)
  kind = name.split("_")[0]
  if kind in ("small", "rated", "one"):
    d.S_cap, d.win, d.n_items, d.n_cap_arg, d.nnz_cap, n_fill, fill_max = 400, (0, 400), 301, None, None, 180, 12
    d.ns = name != "small"           # small: every item is a column (n_b = 301), so a column without any entry exists
    d.ratings = kind == "rated"
  elif kind == "light1":
    d.S_cap, d.win, d.n_items, d.n_cap_arg, d.nnz_cap, n_fill, fill_max = 400, (0, 400), 4200, 4200, 8400, 1501, 3
    d.ns = name != "light1"
  elif kind == "cols2":
    d.S_cap, d.win, d.n_items, d.n_cap_arg, n_fill, fill_max = 2100, (17, 2080), 4200, 4200, 1201, 4
    d.nnz_cap = 8400 if name == "cols2_light" else 9000
  elif kind == "windows":
    d.S_cap, d.win, d.n_items, d.n_cap_arg, n_fill, fill_max = 4110, (5, 4100), 4200, 4200, 1202, 3
    d.nnz_cap = 8400 if name == "windows_light" else 20000
  elif kind == "wg":
    d.S_cap, d.win, d.n_items, d.n_cap_arg, d.nnz_cap, n_fill, fill_max = 2100, (17, 2080), 203, None, None, 150, 40
  else:
    raise KeyError(name)
  rng = np.random.RandomState(sum(map(ord, kind)))
  off, B = d.win
  inside = np.arange(off, off + B)
  outside = np.setdiff1d(np.arange(d.S_cap), inside)
  free = list(rng.permutation(d.n_items))            # item ids in random order: the special columns lie scattered
  d.special, d.col_rows = {}, {}

  def column(tag, rows):
    item = int(free.pop())
    d.special[tag] = item
    if len(rows):
      d.col_rows[item] = np.sort(np.asarray(rows, dtype=np.int64))
  if kind == "one":                                  # a single column (n_b = 1): three of the four waves are dead
    column("p301", rng.choice(inside, 301, replace=False))
  else:
    # (no entry in the window: a row outside it where there is one, else -- every item a column -- no entry at all)
    column("none", outside[:1] if len(outside) else [])
    for p in POPS:
      column("p%d" % p, rng.choice(inside, p, replace=False))
    column("every", inside)
    column("dropped", rng.choice(inside, 20, replace=False))
    # entries on both sides of both ends of the window (the masks of the first and the last bitmap word)
    column("edge", [r for r in (off - 1, off, off + B - 1, off + B) if 0 <= r < d.S_cap])
    if kind == "windows":
      first, second = inside[:eu.BWD_WINDOW], inside[eu.BWD_WINDOW:]
      column("first", rng.choice(first, 70, replace=False))
      column("second", rng.choice(second, 20, replace=False))
      column("both", np.concatenate([rng.choice(first, 40, replace=False), rng.choice(second, 10, replace=False)]))
    if kind == "wg":
      column("p700", rng.choice(inside, 700, replace=False))
      column("p1500", rng.choice(inside, 1500, replace=False))
    for i in range(n_fill):
      column("fill%d" % i, rng.choice(d.S_cap, rng.randint(1, fill_max + 1), replace=False))
  d.nnz = int(sum(len(r) for r in d.col_rows.values()))
  if d.nnz_cap is None:
    d.nnz_cap = d.nnz
  assert d.nnz <= d.nnz_cap
  # (Block's rule for the item capacity)
  d.n_cap = max(1, min(d.n_items, d.n_cap_arg or d.nnz_cap) if d.ns else d.n_items)
  d.n_b = len(d.col_rows) if d.ns else d.n_items
  return d


_design = functools.lru_cache(maxsize=None)(_design)


@functools.lru_cache(maxsize=None)
def _block(name):
  """The collated block of a design (built once; the tests only rewrite svals)."""
  d = _design(name)
  dev = torch.device("cuda")
  csr = eu.csr_with_column_rows(d.S_cap, d.n_items, d.col_rows, seed=3, ratings=d.ratings)
  users = torch.arange(d.S_cap, dtype=torch.int64, device=dev)
  blk = Block(d.S_cap, d.nnz_cap, d.n_items, dev, negative_sampling=d.ns, n_cap=d.n_cap_arg)
  blk.collate(DeviceCSR(csr), users)
  n_b, nnz, ld, S = blk.counts_host()
  assert (n_b, nnz, S) == (d.n_b, d.nnz, d.S_cap) and (blk.n_cap, blk.nnz_cap) == (d.n_cap, d.nnz_cap)
  assert bool(blk.c.implicit) == (not d.ratings)
  c = types.SimpleNamespace(d=d, blk=blk, n_b=n_b, nnz=nnz)
  c.indptr = blk.indptr[:d.S_cap + 1].cpu().numpy()
  c.cols = blk.cols[:nnz].cpu().numpy()
  assert np.array_equal(c.indptr, csr.indptr)            # the block's rows are the matrix's rows, entry for entry
  pos = blk.pos.cpu().numpy()
  c.col_of = {tag: int(pos[item]) for tag, item in d.special.items()}      # (-1: not a column of the block)
  return c


# (block, window, h); the expected route is derived, the coverage test below checks what the table reaches
CASES = []
for _win in ((0, 400), (13, 70), (37, 5), (32, 64)):       # (37, 5): inside one bitmap word; (13, 70): mid-word at both ends
  CASES += [("small", _win, 64), ("small", _win, 260), ("light1", _win, 64), ("light1", _win, 512)]
# the cheapest route across the h - 4 clamp (4, 20), hv == 3 on HV = 4 (600) and the upper limit
CASES += [("small", (13, 70), h) for h in (4, 20, 256, 600, 1024)] + [("light1", (13, 70), 600)]
# item sets shorter than the capacity (rows >= n_b stay untouched), n_b = 1, explicit ratings
CASES += [("small_s", (0, 400), 64), ("small_s", (13, 70), 260), ("light1_s", (0, 400), 64), ("light1_s", (13, 70), 512),
          ("one", (13, 70), 64), ("one", (37, 5), 64), ("rated", (13, 70), 64), ("rated", (0, 400), 260)]
CASES += [("cols2", (17, 2080), 64), ("cols2", (17, 2080), 260),
          ("cols2_light", (17, 2080), 64), ("cols2_light", (17, 2080), 512), ("cols2_light", (17, 2080), 600)]
CASES += [("windows", (5, 4100), 64), ("windows", (5, 4100), 260), ("windows", (5, 4100), 600),
          ("windows_light", (5, 4100), 64)]
CASES += [("wg", (17, 2080), 64), ("wg", (17, 2080), 512), ("wg", (17, 2080), 600)]

ROUTES = [("cols1", False), ("cols1", True), ("cols2", False), ("cols2", True), ("windows", None), ("wg", False)]


def _route_key(name, win, h):
  route, HV, light = eu.bwd_route(_design(name), win[0], win[1], h)
  return (route, None if route == "windows" else light), HV


def test_the_cases_reach_every_route_at_every_vector_width():
  """Host only: the six launch routes, each at HV = 1 and at some HV > 1, HV = 4 on at least three of them, and on
  every route one block whose item count is no multiple of 4 (dead waves in the last workgroup, Q = ceil(n_b / 4))."""
  seen, odd = {}, set()
  for name, win, h in CASES:
    key, HV = _route_key(name, win, h)
    seen.setdefault(key, set()).add(HV)
    if _design(name).n_b % 4:
      odd.add(key)
  assert sorted(seen, key=str) == sorted(ROUTES, key=str), sorted(seen, key=str)
  for key in ROUTES:
    assert 1 in seen[key] and seen[key] & {2, 4}, (key, seen[key])
  assert sum(4 in v for v in seen.values()) >= 3, seen
  assert odd == set(ROUTES), sorted(set(ROUTES) - odd, key=str)
  assert any(_design(name).n_b == 1 for name, _, _ in CASES)
  print("routes reached:", {k: sorted(v) for k, v in seen.items()})


@pytest.mark.parametrize("name", ["small", "light1", "cols2", "cols2_light", "windows", "windows_light"])
def test_the_column_populations_of_the_wave_per_column_blocks(name):
  """Host only: counted inside the design window, the block holds a column of every population at which the body
  takes another branch."""
  d = _design(name)
  off, B = d.win
  pop = {tag: int(np.sum((d.col_rows.get(item, np.zeros(0)) >= off) & (d.col_rows.get(item, np.zeros(0)) < off + B)))
         for tag, item in d.special.items()}
  assert pop["none"] == 0 and pop["every"] == B and pop["dropped"] == 20
  assert [pop["p%d" % p] for p in POPS] == list(POPS)
  assert -(-301 // 4) % 64 != 0                      # a wave's quarter of the 301 entries is no multiple of 64
  if name.startswith("windows"):
    rows = lambda tag: d.col_rows[d.special[tag]]
    cut = off + eu.BWD_WINDOW
    assert rows("first").max() < cut <= rows("second").min() and rows("both").min() < cut <= rows("both").max()


# ------------------------------------------------------------------ data and launches
def _data(c, h, kind, seed):
  """svals (written into the block) and dZ of one case: (s, dZ, prefill scale)."""
  d = c.d
  rng = np.random.RandomState(seed)
  if kind == "exact":
    s = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), size=c.nnz)
    live = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=c.nnz)
  else:
    s = (rng.rand(c.nnz) * (rng.rand(c.nnz) < 0.5)).astype(np.float32)
    live = (0.05 + 0.95 * rng.rand(c.nnz)).astype(np.float32)
  for tag in ("p8", "p9", "p65"):                    # exactly 8 / 9 / 65 LIVE entries: whole passes plus one
    if c.col_of.get(tag, -1) >= 0:
      m = c.cols == c.col_of[tag]
      s[m] = live[m]
  if c.col_of.get("dropped", -1) >= 0:
    s[c.cols == c.col_of["dropped"]] = 0.0
  B = d.S_cap
  if kind == "exact":
    dZ = (rng.randint(-8, 9, size=(B, h)) * 2.0 ** -6).astype(np.float32)
  else:
    dZ = (rng.randn(B, h) * 1e-2).astype(np.float32)
  return s, dZ, (2.0 ** -6 if kind == "exact" else 2.0 ** -12)


def _bwd(c, row_off, B, dZd, h, accumulate, prefill, with_gb):
  """One launch into canary-filled buffers: (G_en [n_cap, h], gb [8 h]); the floats behind G_en stay untouched."""
  lib = _lib.load()
  dev = dZd.device
  n_cap = c.blk.n_cap
  G = torch.full((n_cap * h + TAIL,), CANARY, dtype=torch.float32, device=dev)
  if accumulate:
    G[:c.n_b * h] = prefill.reshape(-1)
  gb = torch.full((8 * h,), CANARY, dtype=torch.float32, device=dev)
  check(lib.rk_ae_encode_bwd(c.blk.ref, row_off, B, ptr(dZd), h, ptr(G), accumulate, ptr(gb) if with_gb else None,
                             current_stream()), "rk_ae_encode_bwd")
  torch.cuda.synchronize()
  assert bool((G[n_cap * h:] == CANARY).all()), "the launch wrote behind row n_cap of G_en"
  return G[:n_cap * h].view(n_cap, h).cpu().numpy(), gb.cpu().numpy()


@gpu
@pytest.mark.parametrize("name,win,h", CASES, ids=["%s-%d+%d-h%d" % (n, w[0], w[1], h) for n, w, h in CASES])
def test_encoder_backward_against_float64(name, win, h):
  c = _block(name)
  d, dev = c.d, torch.device("cuda")
  row_off, B = win
  (route, light), HV = _route_key(name, win, h)
  n_win = -(-B // eu.BWD_WINDOW) if route == "windows" else 1
  worst = [0.0, 0.0]               # error / bound on the generic data, without and with the accumulate add
  for kind in ("exact", "generic"):
    s, dZ_all, pscale = _data(c, h, kind, seed=h + row_off + (0 if kind == "exact" else 1))
    dZ = np.ascontiguousarray(dZ_all[:B])
    c.blk.svals[:c.nnz].copy_(torch.from_numpy(s))
    dZd = torch.from_numpy(dZ).to(dev)
    G64, A, n, gb64, gA = eu.encode_bwd64(c.indptr, c.cols, s, dZ, row_off, B, c.n_b)
    P = (np.random.RandomState(7).randint(-64, 65, size=(c.n_b, h)) * pscale).astype(np.float32)
    Pd = torch.from_numpy(P).to(dev)
    empty = n == 0
    for accumulate in (0, 1):
      for with_gb in (True, False):
        tag = "%s rows %d+%d h = %d %s accumulate = %d gb = %d" % (name, row_off, B, h, kind, accumulate, with_gb)
        G, gb = _bwd(c, row_off, B, dZd, h, accumulate, Pd, with_gb)
        assert np.all(G[c.n_b:] == CANARY), tag + ": rows past n_b were written"
        assert np.all(gb[h:] == CANARY), tag + ": gb_en was written past h"
        if not with_gb:
          assert np.all(gb == CANARY), tag + ": gb_en == NULL, yet written"
        got = G[:c.n_b]
        want = G64 + (P.astype(np.float64) if accumulate else 0.0)
        # a column without an entry in the window: zeros, or the row as it was, bit for bit
        if accumulate:
          assert np.array_equal(got[empty].view(np.int32), P[empty].view(np.int32)), tag
        else:
          assert np.all(got[empty] == 0.0), tag
        if kind == "exact":
          bad = np.argwhere(got.astype(np.float64) != want)
          assert len(bad) == 0, "%s: %d elements differ, first (column, j) = %s, entries %d" % (
              tag, len(bad), bad[0], n[bad[0][0]])
          if with_gb:
            assert np.array_equal(gb[:h].astype(np.float64), gb64), tag
        else:
          bound = (n[:, None] + 8) * U * A + (accumulate * n_win * U) * np.abs(P)
          err = np.abs(got.astype(np.float64) - want)
          rel = err / np.maximum(bound, 1e-300) * (err > 0)
          worst[accumulate] = max(worst[accumulate], float(rel.max()))
          col = int(rel.max(1).argmax())
          assert np.all(err <= bound), "%s: worst error / bound %.3g at column %d (%d entries)" % (
              tag, rel.max(), col, n[col])
          if with_gb:
            gerr = np.abs(gb[:h].astype(np.float64) - gb64)
            gbound = (B + 8) * U * gA
            worst_gb = np.max(gerr / np.maximum(gbound, 1e-300) * (gerr > 0))
            assert np.all(gerr <= gbound), "%s: gb_en, worst error / bound %.3g" % (tag, worst_gb)
            print("ENCBWD-GB route=%s light=%s HV=%d %s ratio=%.4f" % (route, light, HV, tag, worst_gb))
  print("ENCBWD route=%s light=%s HV=%d %s rows %d+%d h=%d n_b=%d ratio=%.4f accumulating=%.4f exact=bitwise" % (
      route, light, HV, name, row_off, B, h, c.n_b, worst[0], worst[1]))


@gpu
def test_host_refusals_leave_a_message_and_the_next_call_succeeds():
  lib = _lib.load()
  c = _block("small")
  st, S = current_stream(), c.d.S_cap
  dZ = torch.zeros(S * 1028, dtype=torch.float32, device="cuda")
  G = torch.zeros(c.blk.n_cap * 1028, dtype=torch.float32, device="cuda")
  gb = torch.zeros(8 * 1028, dtype=torch.float32, device="cuda")

  def bwd(row_off=0, B=S, h=8):
    return lib.rk_ae_encode_bwd(c.blk.ref, row_off, B, ptr(dZ), h, ptr(G), 0, ptr(gb), st)
  refusals = {
    "h = 6": lambda: bwd(h=6),
    "h = 1028": lambda: bwd(h=1028),
    "row_off + B > S_cap": lambda: bwd(row_off=S - 2, B=3),
  }
  for name, call in refusals.items():
    assert call() != 0, name
    assert len(lib.rk_last_error()) > 0, name
    assert bwd() == 0, "the valid call after '%s'" % name
  torch.cuda.synchronize()


# ------------------------------------------------------------------ the dZ slab reduces with act' folded in
@gpu
@pytest.mark.parametrize("B,h,n_items", [(33, 20, 400), (130, 64, 900), (33, 20, 2000)])
def test_dz_slab_reduces_with_the_activation_gradient_against_float64(B, h, n_items):
  """rk_decode_dz_reduce, rk_fdec_dz_reduce and rk_decode_bwd_dw2_dz_reduce with Zact given:
  dZ = (sum of the LIVE slabs, ceil(n_b / 128) of the ceil(n_cap / 128)) . act'(Z), act' in float64 from the same
  fp32 Z by the formula in the output (encoder_util.act_dy64), for every activation code.  The slabs past the live
  ones hold 3e30 and must not enter the sum.  Tolerance: the slab sum by the chain bound with n_c = the live slabs;
  the act' factor at the tolerance rk_act_grad is held to in test_linear_layer_entry_points_match_torch
  (rtol 1e-4, atol 1e-6).  With exact dyadic slabs and no activation: bit for bit."""
  lib = _lib.load()
  dev = torch.device("cuda")
  st = current_stream()
  f = dict(dtype=torch.float32, device=dev)
  csr = synth_csr(max(B, 600), n_items, 14, seed=B + h + n_items)
  dcsr = DeviceCSR(csr)
  blk = Block(B, int(np.sort(dcsr.degrees)[-B:].sum()), n_items, dev, n_cap=n_items)
  blk.collate(dcsr, torch.arange(B, dtype=torch.int64, device=dev))
  n_b, nnz, ld, _ = blk.counts_host()
  assert blk.n_cap == n_items
  n_tiles, live = -(-blk.n_cap // 128), -(-n_b // 128)
  assert 1 <= live <= n_tiles
  if n_items == 2000:
    assert live < n_tiles
  rng = np.random.RandomState(B + h)
  Z = np.tanh(rng.randn(B, h)).astype(np.float32)
  Zd = torch.from_numpy(Z).to(dev)
  # the dW half of the fused launch (its operands as in test_dw_and_dz_reduce_in_one_launch_equal_the_two_launches)
  pairs = lib.rk_split_zt_ok() == 1
  g = torch.Generator(device=dev)
  g.manual_seed(B + 1)
  dO = torch.zeros(B * blk.ld_cap, **f)
  dO[:B * ld].view(B, ld)[:, :n_b] = torch.randn(B, n_b, generator=g, **f) * 1e-3
  blk.counts[8:72].zero_()
  blk.counts[8:9].copy_(dO.abs().max().reshape(1).view(torch.int32))
  ranges = torch.zeros(128, dtype=torch.int32, device=dev)
  wsz = lib.rk_dw3_workspace_bytes(B, h, blk.n_cap) // 4 + 64

  def reduces(slabs_d, zact, act):
    out = {}
    for entry in ("rk_decode_dz_reduce", "rk_fdec_dz_reduce"):
      dZ = torch.full((B * h + 64,), CANARY, **f)
      check(getattr(lib, entry)(ptr(slabs_d), B, h, blk.ref, zact, act, ptr(dZ), st), entry)
      out[entry] = dZ
    dZ = torch.full((B * h + 64,), CANARY, **f)
    ws = torch.zeros(wsz, **f)
    blk.counts[4:5].zero_()
    rc = lib.rk_decode_bwd_dw2_dz_reduce(ptr(dO), ptr(Zd), B, h, blk.ref, ptr(ws), None, ptr(ranges), ptr(slabs_d),
                                         zact, act, ptr(dZ), st)
    if pairs:
      check(rc, "rk_decode_bwd_dw2_dz_reduce")
      out["rk_decode_bwd_dw2_dz_reduce"] = dZ
    else:
      assert rc != 0          # (dW is not on fp16 pairs: the fused launch refuses)
    torch.cuda.synchronize()
    for name, dZ in out.items():
      assert bool((dZ[B * h:] == CANARY).all()), name
    return {name: dZ[:B * h].view(B, h).cpu().numpy() for name, dZ in out.items()}

  def slabs_of(values):
    slabs = np.full((n_tiles, B, h), 3.0e30, np.float32)
    slabs[:live] = values
    return slabs
  # exact dyadic slabs, no activation: with and without Zact, bit for bit
  slabs = slabs_of((rng.randint(-8, 9, size=(live, B, h)) * 2.0 ** -6).astype(np.float32))
  want = slabs[:live].astype(np.float64).sum(0)
  sd = torch.from_numpy(slabs).to(dev)
  for zact in (None, ptr(Zd)):
    for name, got in reduces(sd, zact, eu.ACT_NONE).items():
      assert np.array_equal(got.astype(np.float64), want), name
  # generic slabs, every activation
  slabs = slabs_of(rng.randn(live, B, h).astype(np.float32))
  sd = torch.from_numpy(slabs).to(dev)
  S64 = slabs[:live].astype(np.float64).sum(0)
  dS = (live + 8) * U * np.abs(slabs[:live].astype(np.float64)).sum(0)
  for act in ACTS:
    a = eu.act_dy64(Z, act)
    da = 0.0 if act == eu.ACT_NONE else 1e-4 * np.abs(a) + 1e-6
    tol = dS * (np.abs(a) + da) + np.abs(S64) * da
    for name, got in reduces(sd, ptr(Zd), act).items():
      err = np.abs(got.astype(np.float64) - S64 * a)
      assert np.all(err <= tol), "%s act = %d: worst error / tolerance %.3g" % (name, act, np.max(err / np.maximum(tol, 1e-300)))
      assert np.all(np.isfinite(got)), name
    if act == eu.ACT_RELU:
      assert (a == 0).any() and (a == 1).any()
