"""GPU: three one-call training steps (rk_ae_train_step through FusedEngine._c_train_step) leave the parameters, the
Adam moments and the losses with the bits recorded in tests/golden/step_bits.json (SHA-256 digests written by
tests/golden/make_step_bits.py at commit 660bd50: its docstring lists the cases).  The parity tests compare the step
with the oracle within bounds; this one pins which kernels a step launches, with which arguments and in which order,
so that a change to the step's sequencing which is meant to leave all of that alone can show that it did.

Coverage is a condition: the cases must reach every value of every field of the route word (include/recoder_hip.h,
rk_ae_step_uses_pg) that FusedEngine can reach.  Two values it cannot: dW in line behind dZ (the engine lends every
step that leaves K slabs a side stream) and the encoder forward writing Z^T planes without the operand split (the
engine offers the operand planes whenever the 16-bit contractions are on); tests/test_step_route.py reaches both on
synthetic step structs."""
import json

import pytest

from tests.golden import make_step_bits as msb

pytestmark = pytest.mark.gpu

with open(msb.OUT) as f:
  WANT = json.load(f)

# field -> (shift, mask, the values the cases must reach)
FIELDS = {
  "mode": (0, 15, {0, 1, 3}),
  "bias in the dW tiles' column h": (4, 1, {0, 1}),
  "decode family": (5, 7, {0, 1, 2, 3, 4}),
  "decoder-side rows": (8, 3, {0, 1, 2, 3}),
  "decoder bias gradient": (10, 3, {0, 1, 2}),
  "encoder-side segments": (12, 15, {0, 1, 3}),          # none; one (B <= 512); cdiv(1056, 512)
  "dW kernel": (16, 7, {0, 1, 2, 3, 4, 5}),
  "dW placement": (19, 3, {0, 1, 2}),                    # (3, in line: see above)
  "encoder forward": (21, 7, {0, 2, 3, 4}),              # (1, Z^T planes without the split: see above)
}


@pytest.fixture(scope="module")
def got():
  out = {}
  for prec in msb.PRECS:
    out.update(msb.digests("") if prec == "" else msb.child_digests(prec))
  return out


def test_every_recorded_case_is_computed(got):
  assert sorted(got) == sorted(WANT) == sorted(msb.CASES)


@pytest.mark.parametrize("name", sorted(WANT))
def test_bits(got, name):
  assert got[name]["sha256"] == WANT[name]["sha256"]
  if WANT[name]["mode"] is not None:       # (whole single-process steps: what the engine read of the word before)
    assert got[name]["mode"] == WANT[name]["mode"] == got[name]["route"] & 31


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_the_cases_reach_every_value_of_the_route(got, field):
  shift, mask, want = FIELDS[field]
  seen = {(v["route"] >> shift) & mask for v in got.values()}
  assert want <= seen, (field, sorted(want - seen))
