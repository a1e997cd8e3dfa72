"""rk_adam_multi (csrc/optim.hip) against tests/adam_util.adam64 -- a float64 restatement of adam1 with a counted
rounding bound -- in every form a job takes: scalar and float4 elements, rows through pos, owned rows, partial
gradients (unrolled and remainder, device-resident stride and count), SparseAdam jobs (against sadam64), the big
tables' UTab records, the job lookup with and without the loss block, the running |p| maximum, the per-step
constants of a replay, 25 steps fed back into the kernel, and rk_adam_lazy_flush at and behind an epoch's first step.

Every launch gets p, m, v and the summed gradient exactly (tests/adam_util.sum_parts32 is the kernel's own order of
adds), so each of p, m, v is asserted with |got - ref.v| <= ref.e: tests/test_adam_multi_host.py shows on the CPU
that this bound stays below the project's parameter tolerance and that adam64 is torch.optim.Adam.  Every array
lies between canaries, checked after every launch; rows and elements a job does not own keep their bits.

Largest |got - ref.v| / ref.e per group, measured on an MI355X (1.0 would be the bound; a single correctly rounded
operation, as m's fma, reaches it just above a power of two):
  a. one job      dense 0.990   through pos 0.997   SparseAdam 0.984
  b. parts        general path 0.923   SparseAdam 0.885   UTab 0.987
  c. owned rows   0.932
  d. edge values  0.960
  e. ten jobs     0.992 (bit-equal with and without the loss block)
  g. replay       0.996
  h. 25 steps     0.340 (of the carried bound)
  i. flush        0.916
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import adam_util as au

pytestmark = pytest.mark.gpu

F32 = np.float32
B1, B2, EPS = 0.9, 0.999, 1e-8
GUARD = 256
CANARY = {np.dtype(np.float32): 12345.0, np.dtype(np.int32): 0x5A5A5A5A, np.dtype(np.int64): 0x5A5A5A5A5A5A}


def _lib():
  from recoder_amd import _lib as L
  return L.load()


def _stream():
  from recoder_amd.device import current_stream
  return current_stream()


class Buf:
  """A host array on the device with GUARD canary elements in front of it and behind it, in one allocation."""

  def __init__(self, a):
    a = np.ascontiguousarray(a)
    self.shape, self.n, self.dtype = a.shape, a.size, a.dtype
    self.canary = CANARY[a.dtype]
    whole = np.full(GUARD + a.size + GUARD, self.canary, a.dtype)
    whole[GUARD:GUARD + a.size] = a.ravel()
    self.t = torch.from_numpy(whole).to("cuda")
    self.ptr = self.t.data_ptr() + GUARD * a.dtype.itemsize
    assert self.ptr % 16 == 0

  def get(self):
    return self.t.cpu().numpy()[GUARD:GUARD + self.n].reshape(self.shape).copy()

  def guards_ok(self):
    w = self.t.cpu().numpy()
    return bool(np.all(w[:GUARD] == self.canary) and np.all(w[GUARD + self.n:] == self.canary))


class Arena:
  def __init__(self):
    self.bufs = []

  def add(self, a):
    self.bufs.append(Buf(a))
    return self.bufs[-1]

  def check(self):
    for k, b in enumerate(self.bufs):
      assert b.guards_ok(), "canary of buffer %d (%s %r) overwritten" % (k, b.dtype, b.shape)


def _bits(a):
  return np.ascontiguousarray(a).view(np.int32)


def _ratio(got, ref):
  """max |got - ref.v| / ref.e, asserting finiteness and the bound (a zero bound demands the exact value)."""
  assert np.all(np.isfinite(got))
  err = np.abs(got.astype(np.float64) - ref.v)
  e = np.broadcast_to(ref.e, err.shape)
  assert np.all(err <= e), "worst excess %.3e at %r" % (float((err - e).max()), np.unravel_index((err - e).argmax(), err.shape))
  pos = e > 0
  return float((err[pos] / e[pos]).max()) if pos.any() else 0.0


class Job:
  """One rk_adam_job_t with its host data and its float64 reference.  form: "dense" (a plain tensor, pos NULL),
  "pos" (a table whose rows find their compact gradient row through pos; about a third have one, the table's last
  row among them, in scrambled order) or "sparse" (SparseAdam on rows[0 .. n_dev), n_dev < n_cap, the table's last
  row listed first).  The gradient is the sum of `parts` arrays `stride` floats apart; the padding between them and
  the parts past a device-resident count hold 1e30."""

  def __init__(self, seed, n_rows, h, form="dense", step=1, wd=0.0, lr=1e-3, parts=1, parts_dev=None, stride_dev=False,
               row0=0, row_step=0, amax=None, edit=None, par=None):
    rng = np.random.RandomState(seed)
    self.n, self.h, self.form, self.step, self.wd, self.lr = n_rows, h, form, step, wd, lr
    self.parts, self.parts_dev, self.stride_dev, self.row0, self.row_step = parts, parts_dev, stride_dev, row0, row_step
    self.amax, self.par = amax, par or {}
    n = n_rows
    self.p = (0.3 * rng.randn(n, h)).astype(F32)
    if step == 1:                          # fresh moments
      self.m, self.v = np.zeros((n, h), F32), np.zeros((n, h), F32)
    else:
      self.m, self.v = (0.01 * rng.randn(n, h)).astype(F32), (1e-4 * rng.rand(n, h)).astype(F32)
    self.pos = self.rows = None
    self.n_dev = self.n_cap = 0
    n_g = n
    if form == "pos" and n > 0:
      n_g = max(1, n // 3)
      chosen = rng.permutation(np.concatenate([rng.permutation(n - 1)[:n_g - 1], [n - 1]]))
      self.pos = np.full(n, -1, np.int32)
      self.pos[chosen] = np.arange(n_g, dtype=np.int32)
    elif form == "sparse":
      if n == 1:                           # (one row: listed twice, live once)
        self.rows, self.n_cap, self.n_dev = np.zeros(2, np.int32), 2, 1
      else:
        self.n_cap = min(n, n // 3 + 2)
        self.rows = np.concatenate([[n - 1], rng.permutation(n - 1)[:self.n_cap - 1]]).astype(np.int32)
        self.n_dev = max(1, self.n_cap - 2)
      n_g = self.n_cap
    self.n_g, self.elems = n_g, n_g * h
    self.stride = max(4, self.elems + (8 if parts > 1 or stride_dev else 0))
    self.live = parts if parts_dev is None else min(parts_dev, parts)
    self.G = np.full((parts, self.stride), 1e30, F32)
    self.G[:self.live, :self.elems] = (0.1 * rng.randn(self.live, self.elems)).astype(F32)
    if edit:
      edit(self)

  def grad0(self):
    """part 0 as [gradient rows, h] (a view: the edge cases write into it)"""
    return self.G[0, :self.elems].reshape(self.n_g, self.h)

  def upload(self, arena):
    from recoder_amd._lib import RkAdamJob
    self.bp, self.bm, self.bv, self.bg = arena.add(self.p), arena.add(self.m), arena.add(self.v), arena.add(self.G)
    j = RkAdamJob()
    a = j.par
    a.p, a.m, a.v = self.bp.ptr, self.bm.ptr, self.bv.ptr
    a.lr, a.beta1, a.beta2, a.eps = self.par.get("lr", self.lr), B1, B2, EPS
    a.weight_decay, a.step, a.sparse = self.par.get("wd", self.wd), self.par.get("step", self.step), int(self.form == "sparse")
    j.n_rows, j.h, j.g, j.g_parts = self.n, self.h, self.bg.ptr, self.parts
    # (with a device-resident stride the host's is WRONG, one float short: the device value must win)
    j.g_stride = self.stride - 1 if self.stride_dev else self.stride
    if self.stride_dev:
      j.gstride_dev = arena.add(np.array([self.stride], np.int32)).ptr
    if self.parts_dev is not None:
      j.gparts_dev = arena.add(np.array([self.parts_dev], np.int32)).ptr
    if self.pos is not None:
      j.pos = arena.add(self.pos).ptr
    if self.form == "sparse":
      j.rows, j.n_dev, j.n_cap = arena.add(self.rows).ptr, arena.add(np.array([self.n_dev], np.int32)).ptr, self.n_cap
    j.row0, j.row_step = self.row0, self.row_step
    if self.amax is not None:
      self.bamax = arena.add(self.amax)
      j.amax_out = self.bamax.ptr
    self.c = j
    return j

  def reference(self):
    """(owned table rows, (p, m, v) as E over those rows)"""
    n, h = self.n, self.h
    gsum = au.sum_parts32([self.G[t, :self.elems] for t in range(self.live)]).reshape(self.n_g, h)
    if self.form == "sparse":
      own = self.rows[:self.n_dev].astype(np.int64)
      return own, au.sadam64(self.p[own], self.m[own], self.v[own], gsum[:self.n_dev], self.lr, B1, B2, EPS, self.step)
    own = np.arange(self.row0, n, max(self.row_step, 1), dtype=np.int64) if self.row0 < n else np.zeros(0, np.int64)
    g = np.zeros((n, h), F32)
    if self.pos is not None:
      g[self.pos >= 0] = gsum[self.pos[self.pos >= 0]]
    else:
      g = gsum
    return own, au.adam64(self.p[own], self.m[own], self.v[own], g[own], self.lr, B1, B2, EPS, self.wd, self.step)

  def verify(self):
    """Rows the job does not own keep their bits, the others lie within the bound: the largest err / bound."""
    own, ref = self.reference()
    rest = np.setdiff1d(np.arange(self.n), own)
    self.got = [b.get() for b in (self.bp, self.bm, self.bv)]
    worst = 0.0
    for name, got, host, r in zip("pmv", self.got, (self.p, self.m, self.v), ref):
      assert np.array_equal(_bits(got[rest]), _bits(host[rest])), "%s: a row outside the job changed" % name
      if len(own):
        worst = max(worst, _ratio(got[own], r))
    self.own = own
    if self.amax is not None:
      self.verify_amax()
    return worst

  def verify_amax(self):
    """max(slots) as fp32 == max(seed, max |p_new|) bit for bit; no slot ever falls"""
    slots, seed = self.bamax.get().view(np.uint32), self.amax.view(np.uint32)
    new = np.abs(self.got[0][self.own]).max() if len(self.own) else F32(0)
    want = max(int(seed.max()), int(np.asarray(new, F32).view(np.uint32)))
    assert int(slots.max()) == want
    assert np.all(slots >= seed)


def launch(jobs, arena, loss=None, replay=None):
  """One rk_adam_multi call over the uploaded jobs; loss = (Buf partials, n_part, denom, Buf out)."""
  from recoder_amd._lib import RkAdamJob, check
  lib = _lib()
  arr = (RkAdamJob * max(1, len(jobs)))(*[j.c for j in jobs])
  lp, n_part, denom, lo = (loss[0].ptr, loss[1], loss[2], loss[3].ptr) if loss else (None, 0, 1.0, None)
  if replay is not None:
    lib.rk_replay_set(ctypes.byref(replay))
  try:
    check(lib.rk_adam_multi(arr, len(jobs), lp, n_part, denom, lo, _stream()), "rk_adam_multi")
  finally:
    if replay is not None:
      lib.rk_replay_set(None)
  torch.cuda.synchronize()
  arena.check()


def run_jobs(jobs, **kw):
  arena = Arena()
  for j in jobs:
    j.upload(arena)
  launch(jobs, arena, **kw)
  return max([j.verify() for j in jobs] + [0.0])


# ------------------------------------------------------------------ a. one job, every form
@pytest.mark.parametrize("form", ["dense", "pos", "sparse"])
@pytest.mark.parametrize("n_rows,h", [(1, 1), (7, 3), (5, 4), (33, 200), (1023, 64), (1024, 64)])
def test_one_job_every_form(n_rows, h, form):
  """(1023, 64) and (1024, 64) straddle the 65 536 floats from which a table through pos becomes a UTab record."""
  worst = 0.0
  for step in (1, 1000):
    for wd in (0.0, 2e-5):
      job = Job(n_rows * 31 + h + step, n_rows, h, form, step=step, wd=wd)
      worst = max(worst, run_jobs([job]))
      if form == "pos" and wd:           # a row without a gradient still moves under weight decay
        r = int(np.nonzero(job.pos < 0)[0][0]) if (job.pos < 0).any() else None
        assert r is None or not np.array_equal(job.got[0][r], job.p[r])
      if form == "sparse" and n_rows > 1:   # rows listed past n_dev kept their bits (verify: they are not owned)
        assert not set(job.rows[job.n_dev:]) & set(job.own)
  print("rk_adam_multi one job %dx%d %s: largest err / bound %.3f" % (n_rows, h, form, worst))


# ------------------------------------------------------------------ b. gradient parts
PART_CASES = (
    [("vec%d" % k, dict(n_rows=7, h=8, parts=k)) for k in (2, 4, 5, 6)] +              # float4: groups of 4 from part 1
    [("vec%d_pos" % k, dict(n_rows=7, h=8, parts=k, form="pos")) for k in (5,)] +
    [("scalar%d" % k, dict(n_rows=7, h=3, parts=k)) for k in (2, 8, 9, 10, 17)] +      # scalar: groups of 8
    [("scalar%d_pos" % k, dict(n_rows=7, h=3, parts=k, form="pos")) for k in (10,)] +
    [("stride_dev", dict(n_rows=7, h=3, parts=3, stride_dev=True)),                      # the device's stride wins
     ("parts_dev_below", dict(n_rows=7, h=3, parts=10, parts_dev=9)),                    # parts past the count: 1e30
     ("parts_dev_below_vec", dict(n_rows=7, h=8, parts=6, parts_dev=5)),
     ("parts_dev_one", dict(n_rows=7, h=3, parts=4, parts_dev=1)),
     ("parts_dev_above", dict(n_rows=7, h=3, parts=3, parts_dev=9)),                     # g_parts caps it
     ("parts_dev_above_vec", dict(n_rows=7, h=8, parts=5, parts_dev=64)),
     ("sparse3", dict(n_rows=40, h=3, parts=3, form="sparse")),
     ("sparse3_vec", dict(n_rows=40, h=8, parts=3, form="sparse")),
     # the big tables' own gradient sum (pairs from part 1): the K slabs of dW with their device-resident count
     ("utab2", dict(n_rows=1024, h=64, parts=2, form="pos")),
     ("utab5", dict(n_rows=1024, h=64, parts=5, form="pos")),
     ("utab_parts_dev", dict(n_rows=1024, h=64, parts=4, parts_dev=3, form="pos"))])


@pytest.mark.parametrize("name,kw", PART_CASES, ids=[c[0] for c in PART_CASES])
def test_gradient_parts(name, kw):
  worst = 0.0
  for step, wd in ((1, 2e-5), (1000, 0.0)):
    job = Job(len(name) * 101 + step, step=step, wd=wd, **kw)
    assert job.live == min(kw["parts"], kw.get("parts_dev", kw["parts"]))
    worst = max(worst, run_jobs([job]))
  print("rk_adam_multi parts %s: largest err / bound %.3f" % (name, worst))


# ------------------------------------------------------------------ c. owned rows
@pytest.mark.parametrize("row0,row_step", [(0, 1), (1, 2), (2, 3), (5, 8)])
def test_owned_rows(row0, row_step):
  """21 rows: (n_rows - row0) is no multiple of any of the steps."""
  worst = 0.0
  for form in ("dense", "pos"):
    for h in (4, 6):
      for step, wd in ((1, 2e-5), (1000, 0.0)):
        job = Job(row0 * 17 + row_step + h, 21, h, form, step=step, wd=wd, row0=row0, row_step=row_step)
        worst = max(worst, run_jobs([job]))
        assert list(job.own) == list(range(row0, 21, row_step))
  print("rk_adam_multi owned rows (%d, %d): largest err / bound %.3f" % (row0, row_step, worst))


@pytest.mark.parametrize("h", [4, 6])
def test_a_job_that_owns_no_row_changes_nothing(h):
  """row0 >= n_rows: the job takes no workgroup, and its neighbours in the launch are the jobs they were."""
  jobs = [Job(1, 21, h, "pos", step=3, wd=2e-5), Job(2, 21, h, "dense", step=3, wd=2e-5, row0=21, row_step=2),
          Job(3, 21, h, "pos", step=3, wd=2e-5, row0=30), Job(4, 9, 3, "dense", step=3, wd=2e-5)]
  worst = run_jobs(jobs)
  assert len(jobs[1].own) == 0 and len(jobs[2].own) == 0
  print("rk_adam_multi beside jobs without rows, h %d: largest err / bound %.3f" % (h, worst))


# ------------------------------------------------------------------ d. edge values
def _edges(job):
  p, m, v, g = job.p, job.m, job.v, job.grad0()
  v[0] = 0; m[0] = 0; g[0] = 0                     # nothing at all: p moves with weight decay only
  v[1] = 0; m[1] = 1e-6; g[1] = 0                  # the denominator is eps alone
  v[2] = 1e-40; g[2] = 0                           # v in the subnormals
  v[3] = 1e-44; g[3] = 0
  v[4] = 1e-40; g[4] = 1e-20
  v[5] = 1e-44; g[5] = 1e-20
  m[6] = 1e-40; m[7] = -1e-44                      # m in the subnormals
  m[8] = 1e-40; g[8] = 0; v[8] = 0
  g[9] = 1e15; g[10] = -1e15
  g[11] = 1e-30
  p[12] = 0
  p[13] = 1e4; p[14] = -1e4
  p[15] = 1e4; g[15] = -1e15
  p[16] = 0; m[16] = 0; v[16] = 0; g[16] = 0
  v[17, :4] = 0; m[17, :4] = 0; g[17, :4] = 1e-30  # (1 - b2) g g underflows to nothing


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("wd", [0.0, 2e-5])
def test_edge_values(step, wd):
  job = Job(5, 64, 8, "dense", step=2 if step == 1 else step, wd=wd, edit=_edges)   # (step 2's generator: moments)
  job.step = step
  assert 0 < job.v[2, 0] < 2.0 ** -126 and 0 < job.m[6, 0] < 2.0 ** -126 and job.v[3, 0] > 0
  worst = run_jobs([job])
  gp = job.got[0]
  if wd:
    assert np.all(gp[0] != job.p[0])
  else:
    assert np.array_equal(_bits(gp[0]), _bits(job.p[0]))
  assert np.array_equal(_bits(gp[16]), _bits(job.p[16]))        # p = 0 with nothing to move it
  if not wd:
    assert np.all(gp[1] < job.p[1])                               # m / eps: a step of 90 lr / bc1 down, whatever p
  print("rk_adam_multi edge values step %d wd %g: largest err / bound %.3f" % (step, wd, worst))


# ------------------------------------------------------------------ e. many jobs in one launch, with and without the loss
def _ten_jobs(wd=2e-5):
  return [Job(11, 1, 1, "dense", step=7, wd=wd),                        # a 1 x 1 bias
          Job(12, 1, 200, "dense", step=7, wd=wd, parts=9),             # a bias summed from 9 row-tile partials
          Job(13, 33, 200, "pos", step=7, wd=wd),
          Job(14, 0, 4, "dense", step=7, wd=wd),                        # no rows: takes no record
          Job(15, 40, 8, "sparse", step=7, parts=2),
          Job(16, 21, 6, "dense", step=7, wd=wd, row0=1, row_step=2),
          Job(17, 1024, 64, "pos", step=7, wd=wd),                      # UTab 0
          Job(18, 1024, 64, "pos", step=1, wd=0.0, parts=3),            # UTab 1
          Job(19, 1024, 64, "pos", step=7, wd=wd),                      # a third big table: the general path
          Job(20, 7, 3, "pos", step=1000, wd=wd)]


def _partials(n_part):
  rng = np.random.RandomState(n_part)
  x = (10.0 ** rng.uniform(-8, 4, size=n_part + 5) * np.where(rng.rand(n_part + 5) < 0.3, -1.0, 1.0)).astype(F32)
  exact = math.fsum(float(a) for a in x[:n_part])
  # (the double sum's own error, n 2^-53 sum |x|, lies far below an fp32 ulp of the result)
  assert n_part * 2.0 ** -53 * float(np.abs(x[:n_part].astype(np.float64)).sum()) <= 2.0 ** -30 * abs(exact)
  return x, exact


def _check_loss(x, exact, n_part, denom, part, out, slot=0):
  want = F32(exact) / F32(denom)
  got = out.get()
  assert abs(float(got[slot]) - float(want)) <= float(np.spacing(np.abs(want))), (got[slot], want)
  assert np.all(np.delete(got, slot) == out.canary)
  p = part.get()
  assert np.all(p[:n_part] == 0) and np.array_equal(_bits(p[n_part:]), _bits(x[n_part:]))


@pytest.fixture(scope="module")
def ten_without_loss():
  jobs = _ten_jobs()
  worst = run_jobs(jobs)
  print("rk_adam_multi ten jobs, no loss block: largest err / bound %.3f" % worst)
  return [j.got for j in jobs]


def test_ten_jobs_in_one_launch(ten_without_loss):
  assert len(ten_without_loss) == 10


@pytest.mark.parametrize("n_part", [1, 255, 2048, 2049, 5000])
def test_ten_jobs_behind_the_loss_block(ten_without_loss, n_part):
  """Workgroup 0 reduces the loss and every job starts one workgroup later: the same bits in every table."""
  jobs = _ten_jobs()
  arena = Arena()
  for j in jobs:
    j.upload(arena)
  x, exact = _partials(n_part)
  part, out = arena.add(x), arena.add(np.full(4, 12345.0, F32))
  launch(jobs, arena, loss=(part, n_part, 37.0, out))
  worst = max(j.verify() for j in jobs)
  for k, (j, base) in enumerate(zip(jobs, ten_without_loss)):
    for a, b in zip(j.got, base):
      assert np.array_equal(_bits(a), _bits(b)), "job %d differs behind the loss block" % k
  _check_loss(x, exact, n_part, 37.0, part, out)
  print("rk_adam_multi ten jobs, n_part %d: largest err / bound %.3f" % (n_part, worst))


# ------------------------------------------------------------------ f. amax_out
@pytest.mark.parametrize("n_rows,h,form", [(33, 200, "pos"), (1024, 64, "pos"), (9, 3, "dense"), (40, 8, "sparse")])
def test_amax_out_is_the_running_maximum(n_rows, h, form):
  zero = np.zeros(64, np.int32)
  seeded = zero.copy()
  seeded[37] = np.asarray(50.0, F32).view(np.int32)                 # above every |p|
  low = np.full(64, np.asarray(1e-3, F32).view(np.int32), np.int32)  # below the maximum: the slots that see more rise
  for amax in (zero, seeded, low):
    job = Job(n_rows + h, n_rows, h, form, step=4, wd=2e-5, amax=amax)
    run_jobs([job])
    slots = job.bamax.get()
    assert np.abs(job.got[0]).max() < 50.0
    if amax is seeded:
      assert slots[37] == seeded[37] and slots.max() == seeded[37]
    else:
      assert int(slots.max()) == int(np.abs(job.got[0][job.own]).max().view(np.int32))


# ------------------------------------------------------------------ g. replay constants
R_BASE, R_FIRST, R_STEPS, R_STRIDE, R_LOCAL = 1000, 5, 6, 2, 4
R_WD = (2e-5, 0.0)                                                  # per slot


def _r_lr(i):
  return 1e-3 if i < 3 else 1e-4


def _replay_table():
  """[R_STEPS][R_STRIDE] entries of 8 floats, from the restatement (test_adam_multi_host pins rk_adam_consts to it)"""
  t = np.zeros((R_STEPS, R_STRIDE, 8), F32)
  for i in range(R_STEPS):
    for s in range(R_STRIDE):
      t[i, s] = np.array(au.consts32(_r_lr(i), B1, B2, EPS, R_WD[s], R_FIRST + i), np.float64).astype(F32)
  return t


@pytest.mark.parametrize("with_loss", [False, True])
def test_replay_takes_each_jobs_constants_from_its_slot_and_step(with_loss):
  from recoder_amd._lib import RkReplay
  # the jobs' own hyper-parameters are NOT the table's: par.step is slot + 1, lr and wd are decoys
  mk = lambda seed, n, h, slot: Job(seed, n, h, "pos", step=R_FIRST + R_LOCAL, wd=R_WD[slot], lr=_r_lr(R_LOCAL),
                                    par=dict(step=slot + 1, lr=0.5, wd=0.25))
  jobs = [mk(31, 33, 200, 1), mk(32, 1024, 64, 0), mk(33, 7, 3, 0)]
  arena = Arena()
  for j in jobs:
    j.upload(arena)
  table = arena.add(_replay_table())
  cursor = arena.add(np.array([R_BASE + R_LOCAL - 1, R_BASE], np.int64))      # + off 1: local step 4
  nxt = arena.add(np.array([-1, -1], np.int64))
  ctx = RkReplay()
  ctx.cursor, ctx.off, ctx.B, ctx.users_base = cursor.ptr, 1, 1, cursor.ptr
  ctx.adam_table, ctx.tab_stride = table.ptr, R_STRIDE
  ctx.cursor_next, ctx.advance = nxt.ptr, 3
  loss = None
  if with_loss:
    x, exact = _partials(300)
    part, out = arena.add(x), arena.add(np.full(R_STEPS, 12345.0, F32))
    loss = (part, 300, 37.0, out)
  launch(jobs, arena, loss=loss, replay=ctx)
  worst = max(j.verify() for j in jobs)
  assert np.array_equal(cursor.get(), [R_BASE + R_LOCAL - 1, R_BASE])
  if with_loss:
    _check_loss(x, exact, 300, 37.0, part, out, slot=R_LOCAL)
    assert np.array_equal(nxt.get(), [R_BASE + R_LOCAL - 1 + 3, R_BASE])
  else:
    assert np.array_equal(nxt.get(), [-1, -1])               # the next cursor is the loss block's to write
  print("rk_adam_multi replay, loss block %s: largest err / bound %.3f" % (with_loss, worst))


# ------------------------------------------------------------------ h. twenty-five steps
@pytest.mark.parametrize("wd", [0.0, 2e-5])
@pytest.mark.parametrize("scale", au.TRAJ_SCALES)
def test_twenty_five_steps_fed_back(scale, wd):
  """The host test's trajectory through the kernel, its own output its next input: the final p, m, v within the
  bound adam64 carried over the 25 steps (shown on the CPU to be below 2e-7 + 1e-5 |p| everywhere)."""
  from recoder_amd._lib import RkAdamJob, check
  lib = _lib()
  p0, steps = au.trajectory_inputs(scale)
  n, h = p0.shape
  arena = Arena()
  bp, bm, bv = arena.add(p0), arena.add(np.zeros_like(p0)), arena.add(np.zeros_like(p0))
  for t, (rows, g) in enumerate(steps):
    pos = np.full(n, -1, np.int32)
    pos[rows] = np.arange(len(rows), dtype=np.int32)
    bpos, bg = arena.add(pos), arena.add(g)
    j = RkAdamJob()
    a = j.par
    a.p, a.m, a.v = bp.ptr, bm.ptr, bv.ptr
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step, a.sparse = au.TRAJ_HYPER["lr"], B1, B2, EPS, wd, t + 1, 0
    j.n_rows, j.h, j.g, j.g_parts, j.pos = n, h, bg.ptr, 1, bpos.ptr
    check(lib.rk_adam_multi(ctypes.byref(j), 1, None, 0, 1.0, None, _stream()), "rk_adam_multi")
    torch.cuda.synchronize()
    for b in (bp, bm, bv, bpos, bg):
      assert b.guards_ok(), t
  arena.check()
  ref = au.trajectory64(scale, wd)
  worst = max(_ratio(b.get(), r) for b, r in zip((bp, bm, bv), ref))
  assert np.abs(bp.get() - p0).max() > 1e-3
  print("rk_adam_multi 25 steps, scale %g wd %g: largest err / bound %.3f" % (scale, wd, worst))


# ------------------------------------------------------------------ i. rk_adam_lazy_flush at the epoch's first steps
def _flush_setup(stamps, n=40, h=8):
  rng = np.random.RandomState(9)
  host = [(0.3 * rng.randn(n, h)).astype(F32), (0.01 * rng.randn(n, h)).astype(F32), (1e-4 * rng.rand(n, h)).astype(F32)]
  arena = Arena()
  bufs = [arena.add(x) for x in host]
  stamp = arena.add(np.asarray(stamps, np.int32))
  # the constants table one entry into its buffer, NaN in front of it: no load leaves the allocation
  lead = np.full((1, R_STRIDE, 8), np.nan, F32)
  whole = arena.add(np.concatenate([lead, _replay_table()]))
  return arena, host, bufs, stamp, whole.ptr + R_STRIDE * 8 * 4


def _flush(bufs, stamp, table_ptr, slot, next_step, n=40, h=8):
  from recoder_amd._lib import RkAdamJob, check
  j = RkAdamJob()
  j.par.p, j.par.m, j.par.v = (b.ptr for b in bufs)
  j.n_rows, j.h, j.lazy_stamp, j.lazy_period = n, h, stamp.ptr, 1
  sl = (ctypes.c_int32 * 1)(slot)
  check(_lib().rk_adam_lazy_flush(ctypes.byref(j), 1, table_ptr, R_STRIDE, sl, next_step, R_BASE, _stream()),
        "rk_adam_lazy_flush")
  torch.cuda.synchronize()


def test_flush_at_the_epochs_first_step_touches_nothing():
  stamps = np.full(40, R_BASE, np.int32)
  arena, host, bufs, stamp, table_ptr = _flush_setup(stamps)
  _flush(bufs, stamp, table_ptr, 0, R_BASE)
  arena.check()
  for b, x in zip(bufs, host):
    assert np.array_equal(_bits(b.get()), _bits(x))
  assert np.array_equal(stamp.get(), stamps)


@pytest.mark.parametrize("slot", [0, 1])
def test_flush_replays_the_missed_steps_with_their_own_constants(slot):
  """Two steps into the epoch: rows stamped base replay local steps 0 and 1, rows stamped base + 1 step 1, rows
  stamped base + 2 nothing -- each step adam64 with g = 0 and the table entry of (step, slot)."""
  stamps = (R_BASE + np.arange(40) % 3).astype(np.int32)
  arena, host, bufs, stamp, table_ptr = _flush_setup(stamps)
  _flush(bufs, stamp, table_ptr, slot, R_BASE + 2)
  arena.check()
  assert np.all(stamp.get() == R_BASE + 2)
  got = [b.get() for b in bufs]
  worst = 0.0
  for lag in (0, 1, 2):
    rows = np.nonzero(stamps == R_BASE + 2 - lag)[0]
    ref = [x[rows] for x in host]
    if lag == 0:
      for g_, x in zip(got, ref):
        assert np.array_equal(_bits(g_[rows]), _bits(x))
      continue
    for i in range(2 - lag, 2):
      ref = au.adam64(ref[0], ref[1], ref[2], np.zeros_like(host[0][rows]), _r_lr(i), B1, B2, EPS, R_WD[slot], R_FIRST + i)
    worst = max([worst] + [_ratio(g_[rows], r) for g_, r in zip(got, ref)])
  print("rk_adam_lazy_flush two steps in, slot %d: largest err / bound %.3f" % (slot, worst))
