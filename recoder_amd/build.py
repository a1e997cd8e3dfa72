"""Build the HIP libraries (hand-written kernels + C ABI) for gfx950, one row of LIBRARIES each: the
six HIP libraries of the training, index, ALS, VAE, EASE and SVD paths, a seventh for RP3beta and an
eighth for SLIM.

    python -m recoder_amd.build [--force]

librecoder_hip.so  the training and recommend path (include/recoder_hip.h)
librecoder_index.so  exact item similarity (include/recoder_index.h), a library of its
                   own so that the training library's exported symbol set stays as it is
librecoder_als.so  implicit-feedback ALS for MatrixFactorization (include/recoder_als.h),
                   likewise a library of its own.  It also holds the BPR pairwise-ranking step of the
                   same model (rk_als_bpr_*: sample, grad, apply), the model-aware sampler of WARP and dynamic
                   negative sampling with WARP's gradient (rk_als_rank_sample, rk_als_warp_grad) and the LightGCN kernels
                   (rk_als_lgcn_*: propagate, scatter, adam) that train it over the user-item graph
                   and SimGCL's on top of them (rk_als_gcl_*: the propagation with noise in its epilogue,
                   the contrast between two views) and DirectAU's (rk_als_dau_workspace_bytes,
                   rk_als_dau_grad: the alignment and uniformity loss with its gradient rows, on the contrast's
                   tile code) and the sampled softmax's (rk_als_ssm_workspace_bytes, rk_als_ssm_grad: the
                   softmax over in-batch and shared uniform negatives with its gradient rows, on the f32 MFMA)
                   and UltraGCN's (rk_als_ugcn_workspace_bytes, rk_als_ugcn_grad, rk_als_ugcn_scatter: the
                   constraint loss over a slot's private negatives and the positive's neighbours, and the
                   item-side sum that gathers its user rows) and the cosine contrastive loss' (rk_als_ccl_workspace_bytes,
                   rk_als_ccl_grad, rk_als_ccl_scatter: the hinge on the cosine over a slot's private negatives, and
                   the item-side sum over the live entries only) and the ranking metrics of device-resident top-k lists
                   (rk_als_rank_metrics: Recall / NDCG / AveragePrecision for validation during a fit) and NeuMF's step,
                   dense Adam, item half and scores for NeuralMatrixFactorization (rk_als_ncf_*: a per-pair MLP on
                   16 x 16 f32-MFMA tiles against weights in LDS, csrc/als/ncf.h) and the constrained-serving kernels
                   of Recoder.recommend_filtered (rk_als_serve_mask, rk_als_pair_scores, rk_als_pairs_topk: the per-row
                   deny bitmap, the scores of ragged candidate lists and their ragged top-k, csrc/als/serve.h)
librecoder_vae.so  the stochastic bottleneck of VariationalAutoencoder (include/recoder_vae.h),
                   likewise a library of its own
librecoder_ease.so  the closed-form EASE fit and its scores for ShallowAutoencoder
                   (include/recoder_ease.h), likewise a library of its own.  It also holds the dense
                   rank-k update of GraphFilterModel's GF-CF fit (rk_ease_lowrank_add), which shares the
                   inverse's MFMA tile, and the general dense f32 product and the element-wise pass of
                   AdmmSlimModel's ADMM-SLIM fit (rk_ease_gemm, rk_ease_admm_update) on the same tile, and the row
                   passes of LowRankShallowAutoencoder's ELSA fit and serving (rk_ease_elsa_*, rk_ease_csr_sub), which
                   live in the private header csrc/ease/elsa.h that ease.hip includes
librecoder_svd.so  the randomized truncated SVD behind PureSVD for MatrixFactorization
                   (include/recoder_svd.h), likewise a library of its own
librecoder_rp3.so  the RP3beta item-graph fit and its scores for RandomWalkItemModel
                   (include/recoder_rp3.h), likewise a library of its own.  It also holds the
                   user-neighbourhood kernels of UserNeighbourhoodModel (rk_rp3_user_*): they share
                   the fit's row hand-out and selection, which live in this translation unit, and so
                   does the item-neighbourhood fit of ItemNeighbourhoodModel (rk_rp3_item_*), whose
                   scores are rk_slim_scores
librecoder_slim.so  the SLIM coordinate-descent fit and its scores for SparseLinearModel
                   (include/recoder_slim.h), likewise a library of its own

The seven side libraries share csrc/side_error.h (the last-error buffer and the argument / launch
checks); each stays one translation unit, so each has its own buffer.  csrc/side_explain.h is shared likewise:
the device code of the explanation kernels (rk_ease_explain, rk_slim_explain, rk_als_explain: the order of the
candidates, a wave's selection, the one-wave kernel of the item-item models), which recoder_amd/explain.py calls.  A library's source may be laid out
over private headers in csrc/<stem>/ (als.hip is: csrc/als/*.h, one file a family; ease.hip has csrc/ease/elsa.h); they are that library's
dependencies and nobody else's.

hipcc cross-compiles without a GPU; the built libraries stay in-tree
(recoder_amd/csrc/*.so, git-ignored) so that they travel with the repository
snapshot to the GPU box.
"""
import os
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
INCLUDE = os.path.join(os.path.dirname(CSRC), "..", "include")
# one row per library, in build order: (stem, sources, public headers, whether it depends on the training
# path's headers (every csrc/*.h and include/recoder_hip*.h), the prefix of its exported names).  A side
# library depends on its own header, csrc/side_error.h, csrc/side_explain.h and the headers in csrc/<stem>/; vae.hip and svd.hip also include csrc/common.h
# (the counter RNG, the step cursor), so they follow the training headers too.
LIBRARIES = (
    ("hip", ["capi.hip", "collate.hip", "encoder.hip", "gemm.hip", "decode16.hip", "linear.hip", "dw3.hip",
             "pgemm.hip", "fdecode.hip", "optim.hip", "topk.hip", "step.hip", "comm.hip"],
     ["recoder_hip.h", "recoder_hip_probe.h"], True, "rk_"),
    ("index", ["index.hip"], ["recoder_index.h"], False, "rk_ix_"),
    ("als", ["als.hip"], ["recoder_als.h"], False, "rk_als_"),
    ("vae", ["vae.hip"], ["recoder_vae.h"], True, "rk_vae_"),
    ("ease", ["ease.hip"], ["recoder_ease.h"], False, "rk_ease_"),
    ("svd", ["svd.hip"], ["recoder_svd.h"], True, "rk_svd_"),
    ("rp3", ["rp3.hip"], ["recoder_rp3.h"], False, "rk_rp3_"),
    ("slim", ["slim.hip"], ["recoder_slim.h"], False, "rk_slim_"),
)


def lib_path(stem):
  return os.path.join(CSRC, "librecoder_%s.so" % stem)


# (the names the bindings, the tests and the tools import)
LIB, INDEX_LIB, ALS_LIB, VAE_LIB, EASE_LIB, SVD_LIB, RP3_LIB, SLIM_LIB = (lib_path(row[0]) for row in LIBRARIES)
SOURCES, INDEX_SOURCES, ALS_SOURCES, VAE_SOURCES, EASE_SOURCES, SVD_SOURCES, RP3_SOURCES, SLIM_SOURCES = \
    (row[1] for row in LIBRARIES)
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


def headers_of(stem):
  """The headers whose change rebuilds library `stem` (a row of LIBRARIES)."""
  _, _, public, needs_training, _ = next(row for row in LIBRARIES if row[0] == stem)
  training = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + \
      [os.path.join(INCLUDE, h) for h in LIBRARIES[0][2]]
  own = [os.path.join(INCLUDE, h) for h in public]
  headers = training + [h for h in own if h not in training] if needs_training else \
      own + [os.path.join(CSRC, "side_error.h"), os.path.join(CSRC, "side_explain.h")]
  private = os.path.join(CSRC, stem)                 # csrc/<stem>/*.h: the library's own private headers
  if os.path.isdir(private):
    headers = headers + sorted(os.path.join(private, f) for f in os.listdir(private) if f.endswith(".h"))
  return headers


def build_library(force=False, verbose=True):
  """Build the libraries (each only if one of its sources or headers is newer); returns the training library's path."""
  for stem, sources, _, _, _ in LIBRARIES:
    _build_one(lib_path(stem), sources, headers_of(stem), force, verbose)
  return LIB


if __name__ == "__main__":
  build_library(force="--force" in sys.argv)
  print("built", *(lib_path(row[0]) for row in LIBRARIES))
