"""Host only: the route of the one-call step (csrc/step.hip step_route, reported by rk_ae_step_uses_pg) on a few
hundred synthetic step structs -- the shapes, activations, losses and tied / untied tables of
tests/golden/make_step_bits.py crossed with the resources a caller may leave out (dummy non-null pointers: the call
reads host state only).

 (a) A step's calls see ONE route.  rk_ae_train_step is called once with RK_STEP_ALL (a whole step), or two or three
     times with parts of the mask (a phased, data-parallel step: FWD_DW, DZ_ENC, UPDATE, or FWD_DW | DZ_ENC with tied
     tables), or three times with the RK_STEP_IP_* segments.  Whatever a later call reads of the route must be what
     the earlier one acted on, so the whole word is compared: equal over every proper part of RK_STEP_ALL, equal over
     every part of RK_STEP_IP_ALL, and phase 0 equal to RK_STEP_ALL.  (A whole step is a different row of the table
     than a phased one -- its dW leaves K slabs for the Adam sweep where the phased step sends a dense G_de off early --
     so RK_STEP_ALL is not compared with its parts.)
 (b) Bits 0-4 are what rk_ae_step_uses_pg returned before the route existed: tests/golden/step_modes.json, recorded
     by make_step_bits.py --modes at commit 660bd50.
RK_GEMM_PREC is read once per process: f32 and bf16 run in a child process each."""
import json

import pytest

from tests.golden import make_step_bits as msb

with open(msb.MODES_OUT) as f:
  WANT = json.load(f)

PHASED = [msb.ROUTE_PHASES.index(p) for p in (1, 2, 4, 3, 5, 6)]
ITEMS = [msb.ROUTE_PHASES.index(p) for p in (8, 16, 32, 24, 40, 48, 56)]
WHOLE = [msb.ROUTE_PHASES.index(p) for p in (7, 0)]


@pytest.fixture(scope="module", params=msb.PRECS, ids=lambda p: p or "split")
def words(request):
  prec = request.param
  return prec or "split", (msb.words() if prec == "" else msb.child_words(prec))


def test_the_configurations_are_the_recorded_ones(words):
  prec, got = words
  assert sorted(got) == sorted(WANT[prec]) and len(got) >= 300


def test_phased_calls_see_one_route(words):
  prec, got = words
  for group in (PHASED, ITEMS, WHOLE):
    bad = [k for k, row in got.items() if len({row[i] for i in group}) != 1]
    assert bad == [], (prec, bad[:5])


def test_bits_0_to_4_are_the_recorded_modes(words):
  prec, got = words
  have = msb.modes(got)
  bad = [(k, have[k], WANT[prec][k]) for k in WANT[prec] if have[k] != WANT[prec][k]]
  assert bad == [], (prec, bad[:5])


def test_the_word_decodes_into_the_engines_enums(words):
  """every reported word names a member of engine.Rows / engine.Bias, and bit 4 is Bias.SLABS"""
  from recoder_amd.engine import Bias, StepRoute
  prec, got = words
  for row in got.values():
    for w in row:
      r = StepRoute.of(w)
      assert (r.bias is Bias.SLABS) == bool(w & 16)
      assert r.mode in (0, 1, 3) and 0 <= r.en_segs <= 8
