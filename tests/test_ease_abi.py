"""CPU: librecoder_ease.so is built beside the other four libraries and exports exactly what
include/recoder_ease.h declares (each bound in _ease_lib.SIGNATURES); the other libraries' exports are
unchanged."""
import os

from tests.abi_util import built, declared  # noqa: F401  (built: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EASE_HEADER = os.path.join(ROOT, "include", "recoder_ease.h")


def test_build_produces_the_ease_library(built):
  assert os.path.basename(built.EASE_LIB) == "librecoder_ease.so"
  assert os.path.exists(built.EASE_LIB)


def test_ease_library_exports_exactly_its_header(built):
  from recoder_amd import _ease_lib
  lib = _ease_lib.load()
  # the workspace query is host arithmetic: no device needed; the driver restates it for its memory check
  from recoder_amd import ease
  for n in (1, 64, 129, 7915, 20108, 41140):
    assert lib.rk_ease_spd_inverse_workspace_bytes(n) == ease.inverse_workspace_bytes(n) > 0
  assert lib.rk_ease_spd_inverse_workspace_bytes(0) < 0
