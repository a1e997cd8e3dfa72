"""CPU: every row of recoder_amd.build.LIBRARIES is built; each side library exports exactly what its public
header declares, each name bound in its binding's SIGNATURES and carrying the library's prefix; the training
library exports exactly its two headers; no library exports a name that belongs to another.  What is
particular to one library (constants, workspace arithmetic, argument checks) is in its own test_<x>_abi.py."""
import importlib
import os

import pytest

from recoder_amd.build import LIBRARIES, lib_path
from tests.abi_util import INC, built, declared, exports  # noqa: F401  (built: a fixture)

SIDE = LIBRARIES[1:]


def _headers(row):
  return [os.path.join(INC, h) for h in row[2]]


def test_the_table_lists_the_training_library_and_seven_side_libraries():
  assert [row[0] for row in LIBRARIES] == ["hip", "index", "als", "vae", "ease", "svd", "rp3", "slim"]
  assert [row[0] for row in LIBRARIES if row[3]] == ["hip", "vae", "svd"]       # (these include csrc/common.h)
  prefixes = [row[4] for row in SIDE]
  assert len(set(prefixes)) == len(SIDE) and all(p.startswith("rk_") and p.endswith("_") for p in prefixes)


@pytest.mark.parametrize("row", SIDE, ids=[row[0] for row in SIDE])
def test_side_library_exports_exactly_its_header(built, row):
  stem, sources, _, _, prefix = row
  path = lib_path(stem)
  assert os.path.basename(path) == "librecoder_%s.so" % stem and os.path.exists(path)
  assert sources == [stem + ".hip"]
  binding = importlib.import_module("recoder_amd._%s_lib" % stem)
  assert binding.LIB_PATH == path
  want = declared(_headers(row))
  assert want and all(s.startswith(prefix) for s in want)
  assert exports(path) == want
  assert sorted(binding.SIGNATURES) == want
  lib = binding.load()
  assert lib is binding.load()
  assert getattr(lib, prefix + "version")() >= 100
  assert isinstance(getattr(lib, prefix + "last_error")(), bytes)


def test_training_library_exports_exactly_its_two_headers(built):
  exported = exports(built.LIB)
  assert exported == declared(_headers(LIBRARIES[0]))
  assert len(exported) == 80


def test_no_library_exports_a_name_with_another_librarys_prefix(built):
  for stem, _, _, _, prefix in SIDE:
    for other in LIBRARIES:
      if other[0] != stem:
        assert not any(s.startswith(prefix) for s in exports(lib_path(other[0]))), (prefix, other[0])


def test_a_missing_library_or_symbol_fails_loudly(tmp_path, built):
  from ctypes import c_int32
  from recoder_amd import _lib
  with pytest.raises(_lib.RecoderHipError, match="librecoder_none.so not found at .* build it with "
                                                 "`python -m recoder_amd.build`"):
    _lib.loader(str(tmp_path / "librecoder_none.so"), {})()
  with pytest.raises(AttributeError):
    _lib.loader(built.SLIM_LIB, {"rk_slim_no_such_symbol": (c_int32, [])})()
