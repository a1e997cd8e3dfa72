"""GPU: the three kernels behind Recoder.recommend against their numpy restatements (tests/recommend_util.py), through
the C ABI, at their edges.  Every comparison is exact (ids, counts, value bits); the one tolerance is the 6e-7 of
tests/test_gemm_precision.py for the split-fp16 contraction against float64.

* rk_topk_masked: (n, k) from 5 columns to k = n = 1024, padded / offset / strided layouts, the three kinds of seen
  block, rows of every data family (ties across chunk and wave boundaries, fewer than k unseen items, specials).
* rk_topk_pairs: capacities 1 .. rk_topk_pairs_max_cap(), cnt == k / cap / cap + 1 / k - 1, the status bits.
* rk_decode_filter_planes: its scores are the stored scores of rk_decode_loss_planes BIT FOR BIT, whichever image
  (full, strided sample, strip), column position and tile shape computed them -- the invariant the fused recommend
  path compares its thresholds under -- and its epilogue keeps exactly the restatement's survivors.
* Recoder.recommend end to end at a catalogue that takes the 128-row filter tile by its size.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import recommend_util as ru

pytestmark = pytest.mark.gpu

IDX_SENT, VAL_SENT = -77, 12345.0
POISON_VAL, POISON_IDX = 0x7fc00abc, -7


@pytest.fixture(scope="module")
def lib():
  from recoder_amd import _lib
  return _lib.load()


def _dev():
  return torch.device("cuda")


def _seen_block(seen, kind):
  """A scipy CSR of seen items as the collated input block of all its rows."""
  from recoder_amd.device import Block, DeviceCSR
  if seen is None:
    return None
  dcsr = DeviceCSR(seen)
  assert dcsr.implicit == (kind == "implicit")
  blk = Block(seen.shape[0], max(1, int(dcsr.nnz)), seen.shape[1], _dev(), negative_sampling=False, need_bits_cr=False)
  blk.collate(dcsr, torch.arange(seen.shape[0], dtype=torch.int64, device=_dev()), negative_sampling=False)
  blk.dcsr = dcsr
  return blk


def _ref(blk):
  return None if blk is None else blk.ref


# ----------------------------------------------------------------------------------------- rk_topk_masked
@pytest.mark.parametrize("layout", list(ru.LAYOUTS))
@pytest.mark.parametrize("seen_kind", [None, "implicit", "explicit"])
@pytest.mark.parametrize("n,k", ru.NK)
def test_topk_masked_equals_the_restatement(lib, n, k, seen_kind, layout):
  """Ids equal and values bitwise equal to masked_topk: the order is (key descending, item id ascending), the zeros
  tie, the canonical NaN ranks on top, seen items (stored value > 0 only) fill the tail lowest id first.  The NaN
  padding of the rows and the sentinel columns of the outputs are not touched; a second run gives the same bits."""
  from recoder_amd._lib import check
  from recoder_amd.device import current_stream
  col_off, col_stride, row_off = ru.LAYOUTS[layout]
  sc, seen = ru.topk_case(n, k, seen_kind, col_off, col_stride, row_off)
  B = sc.shape[0]
  assert k <= lib.rk_topk_max_k()
  ld = n if layout == "tight" else -(-n // 32) * 32 + 32
  sd = torch.full((B, ld), float("nan"), device=_dev())
  sd[:, :n] = torch.from_numpy(sc).to(_dev())
  blk = _seen_block(seen, seen_kind)
  out_ld = k + 3

  def run():
    idx = torch.full((B, out_ld), IDX_SENT, dtype=torch.int64, device=_dev())
    val = torch.full((B, out_ld), VAL_SENT, dtype=torch.float32, device=_dev())
    check(lib.rk_topk_masked(sd.data_ptr(), B, n, ld, _ref(blk), row_off, k, col_off, col_stride, idx.data_ptr(),
                             val.data_ptr(), out_ld, current_stream()), "rk_topk_masked")
    return idx.cpu().numpy(), val.cpu().numpy()
  idx, val = run()
  idx2, val2 = run()
  want_idx, want_val = ru.masked_topk(sc, k, None if seen is None else seen[row_off:row_off + B], col_off, col_stride)
  for r in range(B):
    assert np.array_equal(idx[r, :k], want_idx[r]), (ru.FAMILIES[r], idx[r, :k][:12], want_idx[r][:12])
    assert np.array_equal(ru.bits(val[r, :k]), ru.bits(want_val[r])), ru.FAMILIES[r]
  assert (idx[:, k:] == IDX_SENT).all() and (val[:, k:] == VAL_SENT).all()
  assert np.array_equal(idx, idx2) and np.array_equal(ru.bits(val), ru.bits(val2))
  # ids only (out_val == NULL): the same ids
  only = torch.full((B, out_ld), IDX_SENT, dtype=torch.int64, device=_dev())
  check(lib.rk_topk_masked(sd.data_ptr(), B, n, ld, _ref(blk), row_off, k, col_off, col_stride, only.data_ptr(),
                           None, out_ld, current_stream()), "rk_topk_masked")
  assert np.array_equal(only.cpu().numpy(), idx)


# ----------------------------------------------------------------------------------------- rk_topk_pairs
@pytest.mark.parametrize("kind", ["good", "over", "under", "both"])
@pytest.mark.parametrize("cap", [1, 2, 64, 4096, "max"])
def test_topk_pairs_equals_the_restatement(lib, cap, kind):
  """k = 1, a middle value and cap at every capacity up to the advertised maximum: the written rows hold pairs_topk's ids
  (equal scores: lower id first; nothing at or past cnt matters), rows with cnt > cap / cnt < k keep their sentinels
  and set status bit 1 / 2.  Written rows also equal rk_topk_masked over the dense scatter of the same pairs, for the
  k that kernel takes."""
  from recoder_amd._lib import check
  from recoder_amd.device import current_stream
  cap = lib.rk_topk_pairs_max_cap() if cap == "max" else cap
  assert cap <= lib.rk_topk_pairs_max_cap() == 8192
  for k in sorted({1, max(1, cap // 3), cap}):
    val, idx, cnt, n_ids = ru.pairs_case(cap, k, kind)
    B = len(cnt)
    want, written, want_status = ru.pairs_topk(val, idx, cnt, cap, k)
    assert want_status == {"good": 0, "over": 1, "under": 2, "both": 3}[kind]
    out_ld = k + 3
    dv, di, dc = (torch.from_numpy(a).to(_dev()) for a in (val, idx, cnt))
    out = torch.full((B, out_ld), IDX_SENT, dtype=torch.int64, device=_dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    check(lib.rk_topk_pairs(dv.data_ptr(), di.data_ptr(), dc.data_ptr(), B, cap, k, out.data_ptr(), out_ld,
                            status.data_ptr(), current_stream()), "rk_topk_pairs")
    got = out.cpu().numpy()
    assert int(status.item()) == want_status, (cap, k)
    assert np.array_equal(got[written, :k], want[written]), (cap, k)
    assert (got[~written] == IDX_SENT).all() and (got[:, k:] == IDX_SENT).all()
    if k <= lib.rk_topk_max_k():
      dense = np.full((B, n_ids), -np.inf, dtype=np.float32)
      for r in range(B):
        c = min(int(cnt[r]), cap)
        dense[r, idx[r, :c]] = val[r, :c]
      dd = torch.from_numpy(dense).to(_dev())
      mi = torch.empty(B, k, dtype=torch.int64, device=_dev())
      check(lib.rk_topk_masked(dd.data_ptr(), B, n_ids, n_ids, None, 0, k, 0, 1, mi.data_ptr(), None, k,
                               current_stream()), "rk_topk_masked")
      assert np.array_equal(mi.cpu().numpy()[written], got[written, :k]), (cap, k)


# ----------------------------------------------------------------------------------------- the filter
class _Images:
  """Plane images of Z (slot 0) and W (slot 1) made by rk_split_image as FusedEngine._eval_images / recommend_fused
  make them, and the stored scores rk_decode_loss_planes(LOSS_NONE) computes from them over an item-set block."""

  def __init__(self, lib, Z, W, b):
    self.lib, self.dev = lib, _dev()
    self.B, self.h = Z.shape
    self.n = W.shape[0]
    self.KT = -(-self.h // 32)
    self.Z, self.W, self.b = (torch.from_numpy(a).to(self.dev) for a in (Z, W, b))
    self.scales = torch.zeros(64, dtype=torch.float32, device=self.dev)
    self.zimg = self.split(self.Z, self.B, self.h, 32.0, 0)
    self.wimg = self.split(self.W, self.n, self.h, 128.0, 1)

  def split(self, X, rows, ld, dflt, slot):
    from recoder_amd._lib import check
    from recoder_amd.device import current_stream
    img = torch.full((rows * self.KT * 32,), float("nan"), dtype=torch.float32, device=self.dev)
    check(self.lib.rk_split_image(X.data_ptr(), rows, self.h, ld, None, dflt, img.data_ptr(), self.scales.data_ptr(),
                                  slot, current_stream()), "rk_split_image")
    return img

  def strip_ptr(self, col_off):
    return self.wimg.data_ptr() + col_off * self.KT * 128            # the same image, advanced by col_off rows

  def scores(self, w_ptr, items, tile, bias=True):
    """[B, len(items)] stored scores (numpy) and their device matrix [B, ld]; `w_ptr` holds the image rows of `items`."""
    from recoder_amd._lib import LOSS_NONE, RkPlanes, check
    from recoder_amd.device import Block, current_stream
    lib, B, m = self.lib, self.B, len(items)
    sblk = Block(1, 1, self.n, self.dev, negative_sampling=True, need_bits_cr=False, n_cap=m)
    sblk.set_items(torch.from_numpy(np.asarray(items, dtype=np.int32)).to(self.dev), m, 1)
    sblk.c.S_cap = max(sblk.c.S_cap, B)                               # (an item set without rows: any B)
    ld = -(-m // 32) * 32
    pl = RkPlanes()
    pl.scales, pl.z, pl.w, pl.wt = self.scales.data_ptr(), self.zimg.data_ptr(), w_ptr, None
    pl.h, pl.B_cap, pl.n_cap, pl.n_ld = self.h, B, m, ld
    out = torch.full((B, ld), float("nan"), dtype=torch.float32, device=self.dev)
    lib.rk_planes_tile(tile)
    try:
      check(lib.rk_decode_loss_planes(ctypes.byref(pl), B, sblk.ref, 0, self.b.data_ptr() if bias else None, LOSS_NONE,
                                      0.0, 1.0, out.data_ptr(), ld, None, None, current_stream()),
            "rk_decode_loss_planes")
      torch.cuda.synchronize()
    finally:
      lib.rk_planes_tile(0)
    return out[:, :m].cpu().numpy(), out

  def filter(self, tile, col_off, thr, cap, bias, blk, row_off):
    """rk_decode_filter_planes over items [col_off, n) -> cand_cnt [B], cand_idx [B, cap], cand_val bits [B, cap]."""
    from recoder_amd._lib import check
    from recoder_amd.device import current_stream
    lib, B, n = self.lib, self.B, self.n - col_off
    cv = torch.full((B, cap), POISON_VAL, dtype=torch.int32, device=self.dev)
    ci = torch.full((B, cap), POISON_IDX, dtype=torch.int32, device=self.dev)
    cc = torch.zeros(B, dtype=torch.int32, device=self.dev)
    n_dev = torch.tensor([n], dtype=torch.int32, device=self.dev)
    lib.rk_planes_tile(tile)
    try:
      check(lib.rk_decode_filter_planes(self.zimg.data_ptr(), self.strip_ptr(col_off), self.scales.data_ptr(), self.h, B,
                                        n, col_off, self.b.data_ptr() if bias else None, _ref(blk), row_off,
                                        thr.data_ptr(), cv.data_ptr(), ci.data_ptr(), cc.data_ptr(), cap,
                                        n_dev.data_ptr(), current_stream()), "rk_decode_filter_planes")
      torch.cuda.synchronize()
    finally:
      lib.rk_planes_tile(0)
    return cc, ci, cv


def _images(lib, B, h, n):
  if lib.rk_gemm_plain_bf16():
    pytest.skip("RK_GEMM_PREC=bf16: plain bf16 images; the fp16-pair filter is never launched there")
  return _Images(lib, *ru.filter_operands(B, h, n))


@pytest.mark.parametrize("B,h,n", ru.FILTER_SHAPES)
def test_filter_scores_are_pinned_and_position_independent(lib, B, h, n):
  """The stored scores against Z @ W.T + b in float64 (error / (|Z| @ |W|.T + |b|) < 6e-7), and THE SAME BITS from
  the 64-row and the 128-row tile, from the strided-sample image (columns 0, stride, 2 stride ... of the full image's
  scores) and from a strip of the full image (its columns col_off ...)."""
  im = _images(lib, B, h, n)
  Z, W, b = (a.cpu().numpy().astype(np.float64) for a in (im.Z, im.W, im.b))
  full = np.arange(n)
  S64, _ = im.scores(im.wimg.data_ptr(), full, 64)
  S128, _ = im.scores(im.wimg.data_ptr(), full, 128)
  assert np.isfinite(S128).all()
  err = (np.abs(S128 - (Z @ W.T + b)) / (np.abs(Z) @ np.abs(W).T + np.abs(b))).max()
  print("B %d h %d n %d: split-fp16 error %.2e of the sum of magnitudes" % (B, h, n, err))
  assert err < 6e-7
  assert np.array_equal(ru.bits(S64), ru.bits(S128))
  for stride in (3, 8):
    m = -(-n // stride)
    simg = im.split(im.W, m, h * stride, 128.0, 1)
    Ss, _ = im.scores(simg.data_ptr(), full[::stride], 64)
    assert Ss.shape == (B, m) and np.array_equal(ru.bits(Ss), ru.bits(S128[:, ::stride])), stride
  for col_off in (128, 333):
    if col_off >= n:
      continue                                                         # (n = 97: no such strip)
    for tile in (64, 128):
      St, _ = im.scores(im.strip_ptr(col_off), full[col_off:], tile)
      assert np.array_equal(ru.bits(St), ru.bits(S128[:, col_off:])), (col_off, tile)


# cand_cap, bias, seen block, row_off, col_off (0: the whole catalogue; a strip where n allows it)
FILTER_CONFIGS = [(64, True, None, 0, 0), (4096, True, "implicit", 5, 0), (64, False, "explicit", 5, 128),
                  (4096, False, None, 0, 333), (64, True, "implicit", 0, 333), (4096, True, "explicit", 0, 128)]


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("B,h,n", ru.FILTER_SHAPES)
def test_filter_keeps_exactly_the_restatements_survivors(lib, B, h, n, tile):
  """cand_cnt is the restatement's count (also past the capacity), the stored pairs ARE its (item id, score bits) set
  (rows past the capacity: cap distinct members of it), slots at and past min(cnt, cap) keep their poison, nothing seen
  appears, the +inf and NaN thresholds keep nothing."""
  im = _images(lib, B, h, n)
  stored, blocks = {}, {}
  for cap, bias, seen_kind, row_off, col_off in FILTER_CONFIGS:
    if col_off >= n:
      col_off = 0
    if (bias, col_off) not in stored:
      stored[(bias, col_off)] = im.scores(im.strip_ptr(col_off), np.arange(col_off, n), tile, bias)[0]
    S = stored[(bias, col_off)]
    if (seen_kind, row_off) not in blocks:
      seen = ru.seen_matrix(row_off + B + 2, n, seen_kind, seed=h)
      blocks[(seen_kind, row_off)] = (seen, _seen_block(seen, seen_kind))
    seen, blk = blocks[(seen_kind, row_off)]
    for rot in range(4 if B == 1 else 1):
      thr = ru.filter_thresholds(S, rot)
      want = ru.filter_survivors(S, thr, seen, col_off, row_off)
      cc, ci, cv = (t.cpu().numpy() for t in
                    im.filter(tile, col_off, torch.from_numpy(thr).to(_dev()), cap, bias, blk, row_off))
      what = dict(cap=cap, bias=bias, seen=seen_kind, row_off=row_off, col_off=col_off, rot=rot)
      over = 0
      for r in range(B):
        assert cc[r] == len(want[r]), (what, r, cc[r], len(want[r]))
        c = min(int(cc[r]), cap)
        got = set(zip(ci[r, :c].tolist(), cv[r, :c].view(np.uint32).tolist()))
        assert len(got) == c, (what, r)
        assert got == want[r] if cc[r] <= cap else got < want[r], (what, r)
        assert (ci[r, c:] == POISON_IDX).all() and (cv[r, c:] == POISON_VAL).all(), (what, r)
        if seen is not None and c:
          assert not ru.seen_mask(seen[row_off + r], ci[r, :c])[0].any(), (what, r)
        kind = r + rot
        if kind in (1, 2):
          assert cc[r] == 0
        elif kind == 0:
          assert cc[r] == n - col_off - (0 if seen is None else int(ru.seen_mask(seen[row_off + r],
                                                                                 np.arange(col_off, n)).sum()))
        over += cc[r] > cap
      if cap == 64 and n - col_off > 200 and rot == 0:                  # (row 0 at -inf: every unseen item)
        assert over >= 1, what                                          # (the capacity really was exceeded)


@pytest.mark.parametrize("B,h,n", ru.FILTER_SHAPES)
def test_filter_chain_equals_masked_topk_of_the_full_scores(lib, B, h, n):
  """recommend_fused's three steps on the kernels themselves: the row threshold is the k-th value rk_topk_masked finds
  in the strided sample's scores (64-row tile), the filter runs over the full image (128-row tile), rk_topk_pairs
  sorts the survivors: the ids are masked_topk's of the full stored scores wherever the row was written."""
  from recoder_amd._lib import check
  from recoder_amd.device import current_stream
  im = _images(lib, B, h, n)
  k, stride = 5, 3
  seen = ru.seen_matrix(B + 2, n, "explicit", seed=h + 1)
  blk = _seen_block(seen, "explicit")
  S_full, _ = im.scores(im.wimg.data_ptr(), np.arange(n), 128)
  m = -(-n // stride)
  simg = im.split(im.W, m, h * stride, 128.0, 1)
  _, sample = im.scores(simg.data_ptr(), np.arange(0, n, stride), 64)
  s_idx = torch.empty(B, k, dtype=torch.int64, device=_dev())
  s_val = torch.empty(B, k, dtype=torch.float32, device=_dev())
  check(lib.rk_topk_masked(sample.data_ptr(), B, m, sample.shape[1], blk.ref, 0, k, 0, stride, s_idx.data_ptr(),
                           s_val.data_ptr(), k, current_stream()), "rk_topk_masked")
  thr = s_val[:, k - 1].contiguous()
  want, _ = ru.masked_topk(S_full, k, seen[:B])
  compared = 0
  for cap in (4096, 64):
    cc, ci, cv = im.filter(128, 0, thr, cap, True, blk, 0)
    out = torch.full((B, k), IDX_SENT, dtype=torch.int64, device=_dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    check(lib.rk_topk_pairs(cv.data_ptr(), ci.data_ptr(), cc.data_ptr(), B, cap, k, out.data_ptr(), k,
                            status.data_ptr(), current_stream()), "rk_topk_pairs")
    cnt = cc.cpu().numpy()
    assert (cnt >= k).all()                                             # the bound is a lower bound: no row starves
    ok = cnt <= cap
    assert int(status.item()) == (0 if ok.all() else 1)
    got = out.cpu().numpy()
    assert np.array_equal(got[ok], want[ok]), cap
    assert (got[~ok] == IDX_SENT).all()
    compared += int(ok.sum())
    if cap == 4096:
      assert ok.all()
  assert compared >= B


# ----------------------------------------------------------------------------------------- end to end
def test_recommend_fused_at_a_catalogue_that_takes_the_128_row_tile(lib, monkeypatch):
  """Recoder.recommend with n_items = 33000: the filter launch runs decode_planes_kernel<2, 2, EPI_FILTER> by the
  catalogue's size (>= 32768 columns) while the sample (516 items) is scored on the 64-row tile; a run of 40 tied
  items straddles the boundary of two 8192-item strips.  The fused ids are the strip path's, nothing seen returns."""
  from recoder_amd.data import RecommendationDataset, UsersInteractions
  from recoder_amd.engine import FusedEngine
  from recoder_amd.model import Recoder
  from recoder_amd.nn import DynamicAutoencoder
  from tests.test_hip_parity import synth_csr
  n_items, n_users, B, k = 33000, 150, 3, 5
  csr = synth_csr(n_users, n_items, 12, seed=733)
  torch.manual_seed(61)
  rec = Recoder(model=DynamicAutoencoder([8], activation_type="tanh", sparse=False), use_cuda=True,
                optimizer_type="adam", loss="mse")
  rec.train(RecommendationDataset(csr), batch_size=50, lr=1e-2, weight_decay=0.0, num_epochs=1, negative_sampling=True)
  W, b = rec._engine()._decoder_params()
  with torch.no_grad():
    W[8172:8212] = W[8172:8173]
    b[8172:8212] = b[8172]
  monkeypatch.setattr(FusedEngine, "EVAL_CAND_CAP", 4096)
  monkeypatch.setattr(FusedEngine, "EVAL_SAMPLE_MIN", 512)
  monkeypatch.setattr(type(rec), "eval_strip_items", 8192, raising=False)
  users = np.random.RandomState(5).permutation(n_users)[:B]
  ui = UsersInteractions(users=users, interactions_matrix=csr[users])
  rec.eval_fused_batches = 0
  got = rec.recommend_array(ui, k)
  fused = rec.eval_fused_batches
  monkeypatch.setenv("RK_EVAL_FUSED", "0")
  want = rec.recommend_array(ui, k)
  assert rec.eval_fused_batches == fused
  assert got.shape == (B, k) and np.array_equal(got, want)
  if not lib.rk_gemm_plain_bf16():
    assert fused == 1                                                   # (the filter really ran)
    assert rec._engine()._eval_img["m"] < 32768 <= n_items              # sample on the 64-row tile, filter on the 128-row
  seen = csr[users].toarray() > 0
  assert not np.take_along_axis(seen, got, axis=1).any()
