"""GPU: every output buffer of every rk_als_* entry point that launches a kernel has the bits recorded in
tests/golden/als_bits.json (SHA-256 digests, written by tests/golden/make_als_bits.py: its docstring lists the
cases).  The other ALS tests compare against float64 restatements within bounds; this one pins the order of
operations itself, so that a change which is meant to leave the kernels' arithmetic alone can show that it did."""
import json
import os

import pytest

from tests.golden import make_als_bits

pytestmark = pytest.mark.gpu

with open(make_als_bits.OUT) as f:
  WANT = json.load(f)
FAMILIES = sorted({k.split(".")[-2].rstrip("0123456789_") for k in WANT})


@pytest.fixture(scope="module")
def got():
  return make_als_bits.digests()


def test_every_recorded_buffer_is_computed(got):
  assert sorted(got) == sorted(WANT)
  assert {int(k[1:].split(".")[0]) for k in WANT if k[0] == "h"} == set(make_als_bits.HS)


@pytest.mark.parametrize("family", FAMILIES)
def test_bits(got, family):
  keys = [k for k in WANT if k.split(".")[-2].rstrip("0123456789_") == family]
  assert keys
  assert [k for k in keys if got.get(k) != WANT[k]] == []
