"""What the ABI tests share: the names a public header declares, the names a built library exports, and the
build itself, done once per test run.  ``built`` is a fixture: a test module imports it by name."""
import functools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def declared(paths):
  """The sorted rk_* functions that the headers ``paths`` declare (comments stripped)."""
  src = "".join(open(p).read() for p in paths)
  src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
  return sorted(set(re.findall(r"\b(rk_[a-z0-9_]+)\s*\(", src)))


def exports(path):
  """The sorted names of the functions a shared library exports."""
  out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
  return sorted(l.split()[-1] for l in out.splitlines() if " T " in l)


@functools.lru_cache(maxsize=None)
def build_once():
  """recoder_amd.build with every library built (anything stale is rebuilt on the first call only)."""
  from recoder_amd import build
  build.build_library(verbose=False)
  return build


@pytest.fixture(scope="module")
def built():
  return build_once()
