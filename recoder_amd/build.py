"""Build the six HIP libraries of the training, index, ALS, VAE, EASE and SVD paths and a seventh for
RP3beta and an eighth for SLIM (hand-written kernels + C ABI) for gfx950.

    python -m recoder_amd.build [--force]

librecoder_hip.so  the training and recommend path (include/recoder_hip.h)
librecoder_index.so  exact item similarity (include/recoder_index.h), a library of its
                   own so that the training library's exported symbol set stays as it is
librecoder_als.so  implicit-feedback ALS for MatrixFactorization (include/recoder_als.h),
                   likewise a library of its own
librecoder_vae.so  the stochastic bottleneck of VariationalAutoencoder (include/recoder_vae.h),
                   likewise a library of its own
librecoder_ease.so  the closed-form EASE fit and its scores for ShallowAutoencoder
                   (include/recoder_ease.h), likewise a library of its own
librecoder_svd.so  the randomized truncated SVD behind PureSVD for MatrixFactorization
                   (include/recoder_svd.h), likewise a library of its own
librecoder_rp3.so  the RP3beta item-graph fit and its scores for RandomWalkItemModel
                   (include/recoder_rp3.h), likewise a library of its own
librecoder_slim.so  the SLIM coordinate-descent fit and its scores for SparseLinearModel
                   (include/recoder_slim.h), likewise a library of its own

hipcc cross-compiles without a GPU; the built libraries stay in-tree
(recoder_amd/csrc/*.so, git-ignored) so that they travel with the repository
snapshot to the GPU box.
"""
import os
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "librecoder_hip.so")
INDEX_LIB = os.path.join(CSRC, "librecoder_index.so")
ALS_LIB = os.path.join(CSRC, "librecoder_als.so")
VAE_LIB = os.path.join(CSRC, "librecoder_vae.so")
EASE_LIB = os.path.join(CSRC, "librecoder_ease.so")
SVD_LIB = os.path.join(CSRC, "librecoder_svd.so")
RP3_LIB = os.path.join(CSRC, "librecoder_rp3.so")
SLIM_LIB = os.path.join(CSRC, "librecoder_slim.so")
SOURCES = ["capi.hip", "collate.hip", "encoder.hip", "gemm.hip", "decode16.hip", "linear.hip", "dw3.hip", "pgemm.hip", "fdecode.hip", "optim.hip", "topk.hip", "step.hip", "comm.hip"]
INDEX_SOURCES = ["index.hip"]
ALS_SOURCES = ["als.hip"]
VAE_SOURCES = ["vae.hip"]
EASE_SOURCES = ["ease.hip"]
SVD_SOURCES = ["svd.hip"]
RP3_SOURCES = ["rp3.hip"]
SLIM_SOURCES = ["slim.hip"]
# -amdgpu-mfma-vgpr-form: keep MFMA accumulators in VGPRs (gfx950 has a unified register
# file); without it hipcc copied all accumulators AGPR<->VGPR around every k-tile
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
         "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-mllvm", "-amdgpu-mfma-vgpr-form",
         "-fvisibility=hidden",       # (exports: what include/recoder_hip.h declares, nothing else)
         "--offload-compress"]        # (the gfx950 code objects zstd-compressed in the bundle: 3.6 -> ~1 MB)


def _stale(target, deps):
  if not os.path.exists(target):
    return True
  t = os.path.getmtime(target)
  return any(os.path.getmtime(d) > t for d in deps)


def _build_one(lib, sources, headers, force, verbose):
  hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
  objs = []
  procs = []
  for src in sources:
    s = os.path.join(CSRC, src)
    o = os.path.join(CSRC, src.replace(".hip", ".o"))
    objs.append(o)
    if force or _stale(o, [s] + headers):
      cmd = [hipcc] + FLAGS + ["-c", s, "-o", o]
      if verbose:
        print(" ".join(cmd), flush=True)
      procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
  failed = False
  for src, p in procs:
    out, _ = p.communicate()
    if out and verbose:
      sys.stdout.write(out.decode(errors="replace"))
    if p.returncode != 0:
      failed = True
      print("FAILED:", src)
  if failed:
    raise RuntimeError("hipcc failed")
  if force or procs or _stale(lib, objs):
    # (-z defs: an internal helper that is declared but defined nowhere must fail HERE, not at dlopen on the GPU box)
    cmd = [hipcc, "--offload-arch=gfx950", "--offload-compress", "-shared", "-fPIC", "-Wl,-z,defs", "-o", lib] + objs + ["-ldl"]
    if verbose:
      print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
  return lib


def build_library(force=False, verbose=True):
  """Build the libraries (each only if one of its sources or headers is newer); returns the training library's path."""
  include = os.path.join(os.path.dirname(CSRC), "..", "include")
  headers = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + \
      [os.path.join(include, "recoder_hip.h"), os.path.join(include, "recoder_hip_probe.h")]
  _build_one(LIB, SOURCES, headers, force, verbose)
  _build_one(INDEX_LIB, INDEX_SOURCES, [os.path.join(include, "recoder_index.h")], force, verbose)
  _build_one(ALS_LIB, ALS_SOURCES, [os.path.join(include, "recoder_als.h")], force, verbose)
  # (vae.hip includes csrc/common.h for the counter RNG and the step cursor: the training headers too)
  _build_one(VAE_LIB, VAE_SOURCES, headers + [os.path.join(include, "recoder_vae.h")], force, verbose)
  _build_one(EASE_LIB, EASE_SOURCES, [os.path.join(include, "recoder_ease.h")], force, verbose)
  # (svd.hip includes csrc/common.h for the counter RNG, as vae.hip does)
  _build_one(SVD_LIB, SVD_SOURCES, headers + [os.path.join(include, "recoder_svd.h")], force, verbose)
  _build_one(RP3_LIB, RP3_SOURCES, [os.path.join(include, "recoder_rp3.h")], force, verbose)
  _build_one(SLIM_LIB, SLIM_SOURCES, [os.path.join(include, "recoder_slim.h")], force, verbose)
  return LIB


if __name__ == "__main__":
  build_library(force="--force" in sys.argv)
  print("built", LIB, INDEX_LIB, ALS_LIB, VAE_LIB, EASE_LIB, SVD_LIB, RP3_LIB, SLIM_LIB)
