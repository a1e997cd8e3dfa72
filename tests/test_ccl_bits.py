"""GPU: every output buffer of rk_als_ccl_grad and rk_als_ccl_scatter has the bits recorded in
tests/golden/ccl_bits.json (SHA-256 digests, written by tests/golden/make_ccl_bits.py: its docstring lists the cases
and names the commit the fixture was written at).  tests/test_ccl.py compares against float64 restatements within
bounds; this one pins the order of operations itself, as tests/test_als_bits.py does for the families before CCL."""
import json

import pytest

from tests.golden import make_als_bits, make_ccl_bits

pytestmark = pytest.mark.gpu

with open(make_ccl_bits.OUT) as f:
  WANT = json.load(f)
FAMILIES = sorted({k.split(".")[-2].rstrip("0123456789_") for k in WANT})


@pytest.fixture(scope="module")
def got():
  return make_ccl_bits.digests()


def test_every_recorded_buffer_is_computed(got):
  assert sorted(got) == sorted(WANT)
  assert FAMILIES == ["ccl_grad", "ccl_scatter"]
  assert {int(k[1:].split(".")[0]) for k in WANT} == set(make_als_bits.HS)
  outputs = {"cand", "key", "coef", "self", "DU", "valid", "loss", "live"}
  for h in make_als_bits.HS:
    for R in make_ccl_bits.RS:
      assert {k.split(".")[-1] for k in WANT if k.startswith("h%d.ccl_grad%d." % (h, R))} == outputs
    assert {k.split(".")[-1] for k in WANT if k.startswith("h%d.ccl_scatter." % h)} == {"G", "count"}


@pytest.mark.parametrize("family", ["ccl_grad", "ccl_scatter"])
def test_bits(got, family):
  keys = [k for k in WANT if k.split(".")[-2].rstrip("0123456789_") == family]
  assert keys
  assert [k for k in keys if got.get(k) != WANT[k]] == []
