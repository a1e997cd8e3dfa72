// rk_ae_train_step: one C-ABI call = one optimisation step of the
// DynamicAutoencoder hot path (reference model.py:383-404 for the common
// hidden_layers=[h] case): encode -> decode + loss -> {dW chain || dZ chain} ->
// Adam / SparseAdam.  It only sequences the kernels of this library on the two
// caller-provided HIP streams; keeping the sequencing in C removes ~35
// Python->ctypes transitions per step (the host enqueue time was approaching the
// GPU time of the step).
#include <stdlib.h>

#include "common.h"
#include "planes.h"

extern "C" void *rk_event_create(int32_t timing) {
  // timing == 0: ordering-only events between streams of ONE device -- no timing, and no
  // system-scope fence (host / peer visibility is not needed for them)
  hipEvent_t e = nullptr;
  const hipError_t rc = timing ? hipEventCreate(&e)
                               : hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence);
  if (rc != hipSuccess) {
    rk_set_error("hipEventCreate failed");
    return nullptr;
  }
  return (void *)e;
}

extern "C" void rk_event_destroy(void *e) {
  if (e) (void)hipEventDestroy((hipEvent_t)e);
}

extern "C" float rk_event_elapsed_ms(void *e0, void *e1) {
  float ms = -1.f;
  if (hipEventSynchronize((hipEvent_t)e1) != hipSuccess) return -1.f;
  if (hipEventElapsedTime(&ms, (hipEvent_t)e0, (hipEvent_t)e1) != hipSuccess) {
    (void)hipGetLastError();      // (an entry this step never launched: do not leave the error behind)
    return -1.f;
  }
  return ms;
}

extern "C" int rk_event_record(void *event, void *stream) {
  if (hipEventRecord((hipEvent_t)event, (hipStream_t)stream) != hipSuccess) {
    rk_set_error("hipEventRecord failed");
    return -1;
  }
  return 0;
}

extern "C" int rk_stream_wait_event(void *stream, void *event) {
  if (hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0) != hipSuccess) {
    rk_set_error("hipStreamWaitEvent failed");
    return -1;
  }
  return 0;
}

extern "C" int rk_graph_begin(void *stream) {
  // relaxed mode: other threads (torch's allocator, a second virtual rank) may call into HIP
  const hipError_t e = hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed);
  if (e != hipSuccess) {
    rk_set_error("hipStreamBeginCapture: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

extern "C" void *rk_graph_end(void *stream) {
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamEndCapture((hipStream_t)stream, &graph);
  if (e != hipSuccess || graph == nullptr) {
    rk_set_error("hipStreamEndCapture: %s", hipGetErrorString(e));
    return nullptr;
  }
  hipGraphExec_t exec = nullptr;
  e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) {
    rk_set_error("hipGraphInstantiate: %s", hipGetErrorString(e));
    return nullptr;
  }
  // move the executable graph to the device now, not inside its first (timed) launch
  (void)hipGraphUpload(exec, (hipStream_t)stream);
  (void)hipGetLastError();
  return (void *)exec;
}

// Can a timing event be recorded as an event-record NODE of a stream capture
// (hipEventRecordWithFlags(..., hipEventRecordExternal))?  Works on the ROCm 7.2 runtime
// (tools/probes/graph_event_probe.hip), returns "invalid argument" on the 7.0 runtime PyTorch
// bundles: probed once on a scratch stream, so that callers can fall back to eager brackets.
static int timing_route();
extern "C" int32_t rk_graph_timing_supported(void) { return timing_route() != 0 ? 1 : 0; }

// 1: hipEventRecordExternal inside a capture; 2: explicit event-record nodes (capture_record_node,
// below); 0: neither -- probed once
static int external_flag_ok() {
  static const int ok = [] {
    hipStream_t s = nullptr;
    hipEvent_t e = nullptr;
    hipGraph_t g = nullptr;
    int good = 0;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&e) == hipSuccess &&
        hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess) {
      good = hipEventRecordWithFlags(e, s, hipEventRecordExternal) == hipSuccess;
      (void)hipStreamEndCapture(s, &g);
    }
    if (g) (void)hipGraphDestroy(g);
    if (e) (void)hipEventDestroy(e);
    if (s) (void)hipStreamDestroy(s);
    (void)hipGetLastError();
    return good;
  }();
  return ok;
}

extern "C" float rk_graph_event_node_probe(void);
static int timing_route() {
  if (external_flag_ok()) return 1;
  if (rk_tune_get(RK_TUNE_GRAPH_EVENT_NODES) != 1) return 0;
  static const int route = [] {
    // (opt-in, rk_tune(RK_TUNE_GRAPH_EVENT_NODES, 1): measured on the 7.0 runtime the bracketed group costs the same
    // replayed with event nodes as enqueued eagerly -- 0.1385-0.1403 vs 0.1367-0.1385 ms per step of a
    // 20-step run -- and its intervals read 1.5-5 us longer than rocprofv3's kernel durations, where
    // the eager brackets agree with them)
    return rk_graph_event_node_probe() > 0.f ? 2 : 0;
  }();
  return route;
}

// Add an event-record node for `e` at the current point of the capture on `s` through the explicit
// graph API (capture info -> hipGraphAddEventRecordNode on the capturing graph -> the node becomes
// the stream's capture dependency): the route that does not need hipEventRecordExternal.
static hipError_t capture_record_node(hipEvent_t e, hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  hipGraph_t g = nullptr;
  const hipGraphNode_t *deps = nullptr;
  size_t n_deps = 0;
  hipError_t rc = hipStreamGetCaptureInfo_v2(s, &st, &id, &g, &deps, &n_deps);
  if (rc != hipSuccess) return rc;
  if (st != hipStreamCaptureStatusActive || g == nullptr) return hipErrorInvalidValue;
  hipGraphNode_t node = nullptr;
  rc = hipGraphAddEventRecordNode(&node, g, deps, n_deps, e);
  if (rc != hipSuccess) return rc;
  return hipStreamUpdateCaptureDependencies(s, &node, 1, hipStreamSetCaptureDependencies);
}

// Probe of that route in THIS process (its HIP runtime): two event-record nodes around a 64 MB
// memset inside a captured graph, replayed twice; returns the interval in ms read from the events
// (> 0: usable), or -(step that failed) - 0.001 * hip error code.
extern "C" float rk_graph_event_node_probe(void) {
  hipStream_t s = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipGraph_t g = nullptr;
  hipGraphExec_t ex = nullptr;
  void *buf = nullptr;
  float out = 0.f;
  hipError_t rc = hipSuccess;
  int step = 0;
#define PSTEP(call) do { ++step; rc = (call); if (rc != hipSuccess) goto done; } while (0)
  PSTEP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  PSTEP(hipEventCreate(&e0));
  PSTEP(hipEventCreate(&e1));
  PSTEP(hipMalloc(&buf, 64 << 20));
  PSTEP(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
  PSTEP(hipMemsetAsync(buf, 0, 4096, s));
  PSTEP(capture_record_node(e0, s));
  PSTEP(hipMemsetAsync(buf, 1, 64 << 20, s));
  PSTEP(capture_record_node(e1, s));
  PSTEP(hipMemsetAsync(buf, 2, 4096, s));
  PSTEP(hipStreamEndCapture(s, &g));
  PSTEP(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
  PSTEP(hipGraphLaunch(ex, s));
  PSTEP(hipGraphLaunch(ex, s));
  PSTEP(hipStreamSynchronize(s));
  PSTEP(hipEventElapsedTime(&out, e0, e1));
#undef PSTEP
done:
  if (rc != hipSuccess) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (s && hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive) {
      hipGraph_t junk = nullptr;
      (void)hipStreamEndCapture(s, &junk);
      if (junk) (void)hipGraphDestroy(junk);
    }
    out = -(float)step - 0.001f * (float)rc;
  }
  if (ex) (void)hipGraphExecDestroy(ex);
  if (g) (void)hipGraphDestroy(g);
  if (buf) (void)hipFree(buf);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (s) (void)hipStreamDestroy(s);
  (void)hipGetLastError();
  return out;
}

extern "C" int rk_graph_launch(void *graph_exec, void *stream) {
  const hipError_t e = hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream);
  if (e != hipSuccess) {
    rk_set_error("hipGraphLaunch: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

extern "C" void rk_graph_destroy(void *graph_exec) {
  if (graph_exec) (void)hipGraphExecDestroy((hipGraphExec_t)graph_exec);
}

namespace {

// A timing event recorded while its stream is being CAPTURED becomes an event-record NODE of the
// graph (hipEventRecordExternal): every replay re-records it, and hipEventElapsedTime between two
// of them reads the interval inside the replayed graph (tools/probes/graph_event_probe.hip) -- so a
// bracketed group of steps can be a graph replay like every other one.
inline void timer_record(hipEvent_t e, hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  hipError_t rc;
  if (hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive)
    // (the HIP 7.0 runtime PyTorch bundles refuses the external flag but runs event-record nodes
    // added through the graph API: rk_graph_event_node_probe)
    rc = timing_route() == 2 ? capture_record_node(e, s) : hipEventRecordWithFlags(e, s, hipEventRecordExternal);
  else
    rc = hipEventRecord(e, s);
  (void)rc;
}

struct Timer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t s;
  Timer(const rk_ae_step_t *a, int id, void *stream) : s((hipStream_t)stream) {
    if (a->time_entry == id && a->time_ev0 && a->time_ev1) {
      e0 = (hipEvent_t)a->time_ev0; e1 = (hipEvent_t)a->time_ev1;
    } else if (a->time_entry == RK_ENTRY_ALL && a->time_all) {
      e0 = (hipEvent_t)a->time_all[2 * id]; e1 = (hipEvent_t)a->time_all[2 * id + 1];
    }
    if (e0) timer_record(e0, s);
  }
  ~Timer() {
    if (e1) timer_record(e1, s);
  }
};

// |act(x)| <= 1: the static split scale of Z is always in range
inline bool act_bounded(int act) { return act == RK_ACT_TANH || act == RK_ACT_SIGMOID; }

// one rk_adam_multi job for a [n_rows, h] table (dense Adam through pos, or SparseAdam
// on the block's item rows) or a flat tensor (pos == items == null)
rk_adam_job_t table_job(const rk_adam_param_t &par, const rk_block_t *blk, int n_rows, int h,
                        const float *G, bool table) {
  rk_adam_job_t j = {};
  j.par = par;
  j.n_rows = n_rows; j.h = h; j.g = G; j.g_parts = 1;
  if (table && par.sparse) {
    j.rows = blk->items; j.n_dev = blk->counts; j.n_cap = blk->n_cap;
  } else {
    j.par.sparse = 0;
    if (table) j.pos = blk->pos;
  }
  return j;
}

// ---- The ROUTE of a step: which kernels it launches and where they leave the gradients, as one value that
// step_route() computes from the step's configuration, shape and the resources on offer.  The phase bodies below, the
// Adam jobs and rk_ae_step_uses_pg read it and decide nothing themselves (DESIGN.md section 4 has the table).
// A step's phased calls see ONE route: the phase mask enters through `kind` alone.
enum { KIND_WHOLE, KIND_PHASED, KIND_ITEMS };      // phase 0 / RK_STEP_ALL; any other mask of RK_STEP_*; RK_STEP_IP_*
// decode family (engine.Decode); the dZ kernel follows it: rk_decode_bwd_dz, rk_decode_bwd_dz_planes,
// rk_decode_dz_reduce, rk_pg_dz, rk_fdec_dz_reduce
enum { DEC_PLAIN, DEC_PLANES, DEC_DZ_PLANES, DEC_PG, DEC_FDEC };
// encoder forward: rk_ae_encode_fwd; .._planes (with the Z^T planes); .._at (at the cursor); .._at with the operand
// split riding on it; .._partial (item parallel)
enum { ENC_PLAIN, ENC_ZT, ENC_CURSOR, ENC_SPLIT, ENC_PARTIAL };
// dW kernel: fp32 tiles; fp16 pairs / bf16 triples (dw3.hip); rk_pg_dw at 64 x 32 or 32 x 64; rk_pg_dw_dense.  Merged
// with the encoder backward they are rk_decode_bwd_dw_encode_bwd, rk_decode_bwd_dw2_encode_bwd and
// rk_pg_dw_encode_bwd (_ones: BIAS_SLABS)
enum { DWK_F32, DWK_PAIRS, DWK_BF16X3, DWK_PG_64x32, DWK_PG_32x64, DWK_PG_DENSE };
// dW placement: on its own and dense into G_de, in front of the encoder backward (FWD_DW: tied tables accumulate onto
// its rows, MNLL adds the column sums of dO, phased steps send G_de off early); one launch with the encoder backward;
// on the side stream next to dZ -> encoder backward; in line behind dZ
enum { DWP_EARLY, DWP_MERGED, DWP_BRANCH, DWP_INLINE };
// decoder-side rows (engine.Rows): G_de; K slabs at rk_dw3_slabs(dw_ws); K slabs at dw_ws, counts[4] of them;
// row_parts K slabs of the fp32 tiles at dw_ws
enum { ROWS_DENSE, ROWS_DW3, ROWS_PG, ROWS_SPLITK };
// decoder bias gradient (engine.Bias): gb_de; the decode's row-tile partials in gb_part; one partial per K slab of dW
// in gb_part (output column h of the dW tiles against a ones column of the Z image: csrc/internal.h)
enum { BIAS_DENSE, BIAS_TILES, BIAS_SLABS };

struct step_route_t {
  int kind, decode, enc, dw_kernel, dw_place, rows, bias;
  int row_parts;        // capacity of the rows' K slabs
  int en_segs;          // > 0: G_en and gb_en as that many row-segment partials (the fused fp32 dW || encoder backward)
  bool zt;              // the encoder forward writes the Z^T planes, dW reads them
  bool dw_fork;         // dw_fork is recorded behind the decode (the caller may queue work of its own behind it)
  bool bias_colsum;     // phased steps: the row-tile partials are summed into gb_de for the exchange
  float *dw_ws;         // dW's workspace
};

// the merged dW || encoder-backward launch of csrc/pgemm.hip covers this row window (rk_dw_encode_bwd_fused_ok also asks for
// the fp16-pair dW of dw3.hip, which plain bf16 operands -- RK_GEMM_PREC=bf16 -- do not have: the pgemm tiles do not care)
bool pg_merged_ok(int row_off, int B) {
  if (rk_dw_encode_bwd_fused_ok(row_off, B)) return true;
  return rk_gemm_plain_bf16() && rk_tune_get(RK_TUNE_DW_ENC_FUSED) == 1 &&
         (((row_off + B + 31) >> 5) - (row_off >> 5) <= 64);
}
// the decoder bias gradient as output column h of the dW tiles (a ones column in the Z image's padding, written
// by this call's encoder forward; csrc/internal.h): whole steps on the fused decode with the merged dW || encoder
// backward launch, h % 32 != 0, and room for one bias slab per K slab in gb_part (the fused decode leaves it unused)
bool dw_ones_ok(const rk_ae_step_t *a) {
  const int B = a->B, h = a->h, n_cap = a->blk->n_cap;
  if (!act_bounded(a->act) || a->gb_part == nullptr || !pg_merged_ok(a->row_off, B)) return false;
  const int row_tiles = rk_cdiv(B, rk_decode_row_tile());
  return rk_tune_get(RK_TUNE_DW_ONES) != 0 && rk_pg_dw_ones_ok(B, h, n_cap) != 0 &&
         (int64_t)row_tiles * (rk_cdiv(n_cap, 32) * 32) >= (int64_t)rk_pg_dw_splits(B, h, n_cap) * n_cap;
}
// Do the contractions run on the pipelined pair-plane kernels (csrc/pgemm.h)?  Untied MSE / BCE steps with operand
// planes and a scale table.  0: no; 1: all three, outside the fused decode + dZ launch's domain (h > 256 or >= 1024
// rows); 3: the register-resident fused decode (csrc/fdecode.hip) with its image, dW on the pgemm tiles
int pg_mode(const rk_ae_step_t *a, bool whole) {
  const int B = a->B, h = a->h, n_cap = a->blk->n_cap;
  if (a->tied || a->loss_kind == RK_LOSS_MNLL) return 0;
  if (!rk_gemm_split16() || a->ws == nullptr || a->planes == nullptr) return 0;
  if (a->do_scales == nullptr || !rk_pg_enabled()) return 0;
  const bool fdec_ok = a->ws_dw != nullptr && rk_fdec_ok(B, h, n_cap, a->loss_kind);
  const bool dz_fused_ok = rk_decode_dz_fused_ok(B, h, n_cap, a->loss_kind) != 0;
  // RK_GEMM_PREC=bf16 on the current family: whole steps in the fused decode's domain whose decoder bias gradient comes
  // out of the dW tiles (the image's column-sum range reads fp16 pairs) -- fdec_kernel<.., PLAIN> +
  // dw_encbwd_kernel<64, 128, .., PLAIN>; everything else keeps the plain kernels of dw3.hip / decode16.hip
  if (rk_gemm_plain_bf16())
    return whole && B < 1024 && fdec_ok && rkp::kp_of(h) <= 256 && dw_ones_ok(a) ? 3 : 0;
  // phased (data-parallel) steps: the fused decode in FWD_DW, dW dense + the bias gradient from its image
  // (rk_pg_dw_dense), the slab reduce + encoder backward in DZ_ENC
  if (!whole) return fdec_ok && dz_fused_ok ? 3 : 0;
  if (!dz_fused_ok) return 1;
  // rk_pg_dw || encoder backward || image column sums -- when that launch can be the merged one (a->ws_dw, the row
  // window).  (A third form -- the LDS-staged fused decode of decode16.hip writing the image as well -- was measured
  // and dropped: at C2 the image pass cost that launch 6 us and rk_pg_dw gained 0.8: 0.1222 vs 0.1188 ms)
  return fdec_ok && rk_dw_encode_bwd_fused_ok(a->row_off, B) ? 3 : 0;
}

step_route_t step_route(const rk_ae_step_t *a) {
  step_route_t r = {};
  const int B = a->B, h = a->h, n_cap = a->blk->n_cap;
  const bool mnll = a->loss_kind == RK_LOSS_MNLL, early = a->tied || mnll;
  const bool split16 = rk_gemm_split16() != 0;
  // fp16 pairs (three products) by default, bf16 triples otherwise -- with a workspace; else the fp32-MFMA tiles
  auto split_kernel = [&](const float *ws) { return !(split16 && ws) ? DWK_F32 : rk_dw_pairs() ? DWK_PAIRS : DWK_BF16X3; };
  r.row_parts = 1;
  if (a->phase & RK_STEP_IP_ALL) {
    // (the partial encoder sums are not Z yet: no planes, no images)
    r.kind = KIND_ITEMS; r.enc = ENC_PARTIAL; r.decode = DEC_PLAIN;
    r.dw_ws = a->ws;
    r.dw_place = early ? DWP_EARLY : DWP_MERGED;
    r.dw_kernel = early ? split_kernel(a->ws) : DWK_F32;
    // large global batches: dW comes out as K slabs; rk_adam_multi sums them in slab order while it reads the
    // gradient (g_parts), so the separate summing launch is skipped
    if (!early && a->ws != nullptr && rk_dw_splits(B) > 1) { r.rows = ROWS_SPLITK; r.row_parts = rk_dw_splits(B); }
    r.bias = mnll ? BIAS_DENSE : BIAS_TILES;
    r.en_segs = early ? 0 : rk_encode_bwd_segments(B);
    return r;
  }
  const bool whole = a->phase == 0 || a->phase == RK_STEP_ALL;
  r.kind = whole ? KIND_WHOLE : KIND_PHASED;
  // pre-split operand planes (decode16.hip): W_de[items] is split by extra workgroups of the encoder-forward launch,
  // Z by that kernel's epilogue; decode and dZ copy the images into LDS
  const bool pl = a->planes != nullptr && split16;
  // whole untied MSE / BCE steps on the 16-bit pipe: dW leaves its K slabs in a workspace for the Adam sweep
  const bool slabs = whole && !early && split16 && a->ws != nullptr;
  const int mode = pg_mode(a, whole);
  // dZ fused into the decode launch: the untied MSE / BCE step whose dZ slabs stay alone in `ws` until they are reduced.
  // Phased steps: they must survive from the FWD_DW call to the DZ_ENC call, so dW needs the workspace of its own.
  const bool dz_fused = pl && !early && a->ws != nullptr && (whole || a->ws_dw != nullptr) &&
                        (mode == 3 || rk_decode_dz_fused_ok(B, h, n_cap, a->loss_kind) != 0);
  r.decode = !pl ? DEC_PLAIN : mode == 3 ? DEC_FDEC : dz_fused ? DEC_DZ_PLANES : mode == 1 ? DEC_PG : DEC_PLANES;
  // the Z^T planes of the dw3.hip kernels (the pair split needs a static scale: bounded activations)
  r.zt = mode == 0 && split16 && a->ws != nullptr && a->zt_planes != nullptr && (!rk_dw_pairs() || act_bounded(a->act));
  r.enc = pl ? ENC_SPLIT : a->cursor ? ENC_CURSOR : r.zt ? ENC_ZT : ENC_PLAIN;
  r.dw_fork = slabs && a->dw_stream != nullptr;
  if (early || !whole) {
    r.dw_place = DWP_EARLY;
    r.dw_ws = dz_fused ? a->ws_dw : a->ws;     // (the fused decode's dZ slabs sit in a->ws until the DZ_ENC call)
    r.dw_kernel = mode == 3 ? DWK_PG_DENSE : split_kernel(r.dw_ws);
  } else if (!slabs) {
    r.dw_place = DWP_MERGED; r.dw_kernel = DWK_F32; r.dw_ws = a->ws;
    r.en_segs = rk_encode_bwd_segments(B);
  } else {
    // dW and the encoder backward as ONE launch on the chain in the small-shape domain of the fused decodes only: at
    // C5's sizes -- dW 100+ us -- the side-stream branch next to dZ -> encoder backward is worth more than its two
    // edges (0.75 vs 0.83 ms per step)
    const bool merged = dz_fused && (mode == 3 ? pg_merged_ok(a->row_off, B) : rk_dw_encode_bwd_fused_ok(a->row_off, B) != 0);
    r.dw_ws = r.dw_fork ? a->ws_dw : a->ws;
    r.dw_place = merged ? DWP_MERGED : r.dw_fork ? DWP_BRANCH : DWP_INLINE;
    r.dw_kernel = mode == 1 ? DWK_PG_64x32 : mode == 3 ? DWK_PG_32x64 : split_kernel(r.dw_ws);
    r.rows = mode ? ROWS_PG : ROWS_DW3;
    r.row_parts = mode ? rk_pg_dw_splits(B, h, n_cap) : rk_dw3_max_splits();
  }
  const bool ones = whole && mode == 3 && dw_ones_ok(a);
  r.bias = ones ? BIAS_SLABS : (whole && !mnll && mode != 3) ? BIAS_TILES : BIAS_DENSE;
  r.bias_colsum = !whole && !mnll && mode != 3;
  return r;
}

// dW = dO^T . Z on its own: dense into G_de (DWP_EARLY; + the column sums of dO for MNLL), else as K slabs in r.dw_ws
int dw_launch(const rk_ae_step_t *a, const step_route_t &r, void *stream) {
  const bool early = r.dw_place == DWP_EARLY;
  float *G_de = early ? a->G_de : nullptr;
  float *gb_de = early && a->loss_kind == RK_LOSS_MNLL ? a->gb_de : nullptr;
  // (the Z^T planes come from the encoder forward when it could write them, else the kernel makes them from Z with
  // the bound rk_amax left in ranges)
  void *zt = r.zt ? a->zt_planes : nullptr;
  switch (r.dw_kernel) {
    case DWK_PAIRS:
      return rk_decode_bwd_dw2(a->dO, a->Z0, a->B, a->h, a->blk, G_de, gb_de, r.dw_ws, zt, a->ranges, stream);
    case DWK_BF16X3:
      return rk_decode_bwd_dw3(a->dO, a->Z0, a->B, a->h, a->blk, G_de, gb_de, r.dw_ws, zt, stream);
    case DWK_PG_64x32:
      return rk_pg_dw(a->dO, a->do_scales, 64, 32, a->B, a->planes, a->blk, r.dw_ws, nullptr, stream);
    case DWK_PG_32x64:
      return rk_pg_dw(a->dO, a->do_scales, 32, 64, a->B, a->planes, a->blk, r.dw_ws, a->gb_de, stream);
    case DWK_PG_DENSE:   // (on the fused decode's image: G_de dense, gb_de from the image's columns)
      return rk_pg_dw_dense(a->dO, a->do_scales, 32, 64, a->B, a->planes, a->blk, a->G_de, a->gb_de, stream);
    default:
      return rk_decode_bwd_dw(a->dO, a->Z0, a->B, a->h, a->blk, G_de, gb_de, stream);
  }
}

// The rk_adam_multi jobs of a step, reading the gradients where the route left them: W_en, W_de (untied), b_de, b_en,
// their parameter slots beside them; returns their number
int route_jobs(const rk_ae_step_t *a, const step_route_t &r, rk_adam_job_t *jobs, int32_t *slots) {
  const rk_block_t *blk = a->blk;
  const int B = a->B, h = a->h, n_items = blk->n_items;
  int n = 0;
  slots[n] = RK_PAR_W_EN;
  jobs[n] = table_job(a->par[RK_PAR_W_EN], blk, n_items, h, a->tied ? a->G_de : a->G_en, true);
  if (r.en_segs) { jobs[n].g_parts = r.en_segs; jobs[n].g_stride = blk->n_cap * h; }
  if (a->tied && a->ranges) jobs[n].amax_out = a->ranges + 64;     // the decoder reads this table
  ++n;
  if (!a->tied) {
    slots[n] = RK_PAR_W_DE;
    jobs[n] = table_job(a->par[RK_PAR_W_DE], blk, n_items, h, a->G_de, true);
    if (a->ranges) jobs[n].amax_out = a->ranges + 64;
    if (r.rows != ROWS_DENSE) {
      jobs[n].g = r.rows == ROWS_DW3 ? rk_dw3_slabs(r.dw_ws, B, h) : r.dw_ws;
      jobs[n].g_parts = r.row_parts; jobs[n].g_stride = blk->n_cap * h;
      if (r.rows != ROWS_SPLITK) jobs[n].gparts_dev = blk->counts + 4;
    }
    ++n;
  }
  slots[n] = RK_PAR_B_DE;
  jobs[n] = table_job(a->par[RK_PAR_B_DE], blk, n_items, 1, a->gb_de, true);
  jobs[n].par.sparse = 0; jobs[n].rows = nullptr; jobs[n].n_dev = nullptr; jobs[n].pos = blk->pos;
  if (r.bias == BIAS_TILES) {
    jobs[n].g = a->gb_part; jobs[n].g_parts = rk_cdiv(B, rk_decode_row_tile()); jobs[n].gstride_dev = blk->counts + 2;
  } else if (r.bias == BIAS_SLABS) {
    jobs[n].g = a->gb_part; jobs[n].g_parts = rk_pg_dw_splits(B, h, blk->n_cap); jobs[n].g_stride = blk->n_cap;
    jobs[n].gparts_dev = blk->counts + 4;
  }
  ++n;
  slots[n] = RK_PAR_B_EN;
  jobs[n] = table_job(a->par[RK_PAR_B_EN], blk, 1, h, a->gb_en, false);
  if (r.en_segs) { jobs[n].g_parts = r.en_segs; jobs[n].g_stride = h; }
  return n + 1;
}

}  // namespace

#define RK_TRY(call)          \
  do {                        \
    int rc__ = (call);        \
    if (rc__ != 0) return rc__; \
  } while (0)

/* the route as one word: include/recoder_hip.h */
extern "C" int32_t rk_ae_step_uses_pg(const rk_ae_step_t *a) {
  if (!(a && a->blk)) return 0;
  const step_route_t r = step_route(a);
  const int mode = r.decode == DEC_PG ? 1 : r.decode == DEC_FDEC ? 3 : 0;
  return mode | (r.bias == BIAS_SLABS ? 16 : 0) | r.decode << 5 | r.rows << 8 | r.bias << 10 | r.en_segs << 12 |
         r.dw_kernel << 16 | r.dw_place << 19 | r.enc << 21;
}

// Item-parallel step (rk_ae_step_t.own_world ranks, item i owned by rank i % own_world).
// The block holds the rows of ALL users of the global batch restricted to this rank's
// items; three segments with an all-reduce (SUM) of a [B, h] matrix between them:
//   IP_ENC : Z0 = partial encoder sums over the local items (whole-row norms)
//   -- all-reduce Z0 --
//   IP_MID : Z0 = act(Z0 + b_en) ; decode + loss over the local items ;
//            dZ0 = (dO . W_de) * act'(Z0)   (this rank's share of the pre-activation gradient)
//   -- all-reduce dZ0 --
//   IP_TAIL: dW || encoder backward ; Adam on the OWNED rows (+ b_en, which is
//            replicated: every rank computes the identical update) ; local loss partial
static int step_item_parallel(const rk_ae_step_t *a, const step_route_t &r) {
  const rk_block_t *blk = a->blk;
  hipStream_t sm = (hipStream_t)a->stream;
  const int B = a->B, h = a->h, phase = a->phase;
  const float *W_de = a->tied ? a->par[RK_PAR_W_EN].p : a->par[RK_PAR_W_DE].p;
  float *G_en = a->tied ? a->G_de : a->G_en;
  RK_REQUIRE(a->own_world >= 1 && a->own_rank >= 0 && a->own_rank < a->own_world, "bad ownership");
  // the softmax of the multinomial loss spans every target item of a row, i.e. all ranks
  RK_REQUIRE(a->loss_kind != RK_LOSS_MNLL, "item-parallel training supports the mse / logistic losses");
  if (phase & RK_STEP_IP_ENC) {
    Timer t(a, RK_ENTRY_ENCODE_FWD, sm);
    RK_TRY(rk_ae_encode_fwd_partial(blk, a->row_off, B, a->par[RK_PAR_W_EN].p, h, a->keep, a->noise_p,
                                    a->seed, a->rng_step, a->users, a->user_norm, a->Z0, sm));
  }
  if (phase & RK_STEP_IP_MID) {
    RK_TRY(rk_bias_act(a->Z0, a->par[RK_PAR_B_EN].p, B, h, a->act, sm));
    {
      Timer t(a, RK_ENTRY_DECODE_LOSS, sm);
      if (a->ranges && !act_bounded(a->act)) RK_TRY(rk_amax(a->Z0, (int64_t)B * h, a->ranges, sm));
      RK_TRY(rk_decode_loss(a->Z0, B, h, blk, a->row_off, W_de, a->par[RK_PAR_B_DE].p, a->loss_kind,
                            a->confidence, a->inv_B, a->dO, 0, a->loss_part, a->gb_part, a->ranges, sm));
    }
    // act'(Z0) is applied to this rank's PARTIAL dZ0 here, inside the split-K reduce: Z0 is the
    // same on every rank, so sum_ranks(dZ0_r) * act'(Z0) = sum_ranks(dZ0_r * act'(Z0)) and the
    // element-wise launch after the all-reduce disappears
    Timer t(a, RK_ENTRY_DECODE_BWD_DZ, sm);
    RK_TRY(rk_decode_bwd_dz(a->dO, B, h, blk, W_de, a->Z0, a->act, a->dZ0, a->ws, a->ranges, sm));
  }
  if (phase & RK_STEP_IP_TAIL) {
    if (r.dw_place == DWP_EARLY) {
      RK_TRY(dw_launch(a, r, sm));
      RK_TRY(rk_ae_encode_bwd(blk, a->row_off, B, a->dZ0, h, G_en, a->tied ? 1 : 0, a->gb_en, sm));
    } else {
      Timer t(a, RK_ENTRY_DECODE_BWD_DW, sm);
      RK_TRY(rk_decode_bwd_dw_encode_bwd(a->dO, a->Z0, B, h, blk, r.rows == ROWS_SPLITK ? nullptr : a->G_de,
                                         a->row_off, a->dZ0, G_en, a->gb_en, a->ws, sm));
    }
    rk_adam_job_t jobs[4];
    int32_t slots[4];
    const int n = route_jobs(a, r, jobs, slots);
    for (int j = 0; j < n - 1; ++j)      // (b_en is replicated: every rank computes the identical update)
      if (!jobs[j].par.sparse) { jobs[j].row0 = a->own_rank; jobs[j].row_step = a->own_world; }
    Timer t(a, RK_ENTRY_ADAM_MULTI, sm);
    RK_TRY(rk_adam_multi(jobs, n, a->loss_part, rk_loss_partials(B, blk->n_cap), a->denom, a->loss_out, sm));
  }
  return 0;
}

// The whole step is a serial chain on ONE stream:
//   encode_fwd ; decode+loss ; dW ; dZ split-K ; reduce ; encode_bwd (+gb_en) ; update
// (an earlier version ran the dW chain on a second stream: each cross-stream event
// costs 10-20 us of dependency latency on this stack -- tools/sync_cost2.py -- which
// ate the overlap; the small kernels it needed are folded into the big ones instead).
extern "C" int rk_ae_train_step(const rk_ae_step_t *a) {
  RK_REQUIRE(a && a->blk, "null step / block");
  RK_REQUIRE(a->phase >= 0 && a->phase <= 63, "phase is a mask of RK_STEP_*");
  RK_REQUIRE(a->time_entry >= RK_ENTRY_ALL && a->time_entry < RK_ENTRY_COUNT, "time_entry");
  const step_route_t r = step_route(a);
  if (r.kind == KIND_ITEMS) {
    RK_REQUIRE((a->phase & RK_STEP_ALL) == 0, "item-parallel and data-parallel phases do not mix");
    return step_item_parallel(a, r);
  }
  const int phase = a->phase == 0 ? RK_STEP_ALL : a->phase;
  const bool whole = r.kind == KIND_WHOLE;
  const rk_block_t *blk = a->blk;
  hipStream_t sm = (hipStream_t)a->stream;
  const int B = a->B, h = a->h, n_items = blk->n_items;
  const bool mnll = a->loss_kind == RK_LOSS_MNLL;
  const bool bounded = act_bounded(a->act);
  const float *W_de = a->tied ? a->par[RK_PAR_W_EN].p : a->par[RK_PAR_W_DE].p;
  float *G_en = a->tied ? a->G_de : a->G_en;
  const int n_part = mnll ? B : rk_loss_partials(B, blk->n_cap);   // unused slots hold 0
  void *zt = r.zt ? a->zt_planes : nullptr;
  RK_REQUIRE(!r.dw_fork || (a->ws_dw && a->dw_fork && a->dw_join), "dw_stream needs ws_dw, dw_fork, dw_join");

  if (phase & RK_STEP_FWD_DW) {
    {
      Timer t(a, RK_ENTRY_ENCODE_FWD, sm);
      switch (r.enc) {
        case ENC_SPLIT: {
          rk_enc_split_t es = {};
          es.sw = rk_split_w_args(W_de, blk, a->ranges, a->planes);
          // (dZ reads the W image along its rows: no W^T image)
          if (r.decode == DEC_PG || r.decode == DEC_FDEC) es.sw.wtp = nullptr;
          es.n_split = rk_cdiv(blk->n_cap, 32);
          es.zimg = bounded ? (char *)a->planes->z : nullptr;
          es.z_kt = rkp::kp_of(h) / 32;
          es.z_ones = r.bias == BIAS_SLABS ? 1 : 0;
          RK_REQUIRE(a->planes->h == h && B <= a->planes->B_cap && blk->n_cap <= a->planes->n_cap,
                     "planes were laid out for another shape");
          RK_TRY(rk_ae_encode_fwd_at(blk, a->row_off, B, a->par[RK_PAR_W_EN].p, a->par[RK_PAR_B_EN].p, h,
                                     a->keep, a->noise_p, a->seed, a->cursor, a->cursor_off, a->users,
                                     a->act, a->Z0, zt, sm, &es, a->rng_step));
          break;
        }
        case ENC_CURSOR:
          RK_TRY(rk_ae_encode_fwd_at(blk, a->row_off, B, a->par[RK_PAR_W_EN].p, a->par[RK_PAR_B_EN].p, h,
                                     a->keep, a->noise_p, a->seed, a->cursor, a->cursor_off, a->users,
                                     a->act, a->Z0, zt, sm, nullptr, 0));
          break;
        case ENC_ZT:
          RK_TRY(rk_ae_encode_fwd_planes(blk, a->row_off, B, a->par[RK_PAR_W_EN].p, a->par[RK_PAR_B_EN].p,
                                         h, a->keep, a->noise_p, a->seed, a->rng_step, a->users, a->act,
                                         a->Z0, a->zt_planes, sm));
          break;
        default:
          RK_TRY(rk_ae_encode_fwd(blk, a->row_off, B, a->par[RK_PAR_W_EN].p, a->par[RK_PAR_B_EN].p, h,
                                  a->keep, a->noise_p, a->seed, a->rng_step, a->users, a->act, a->Z0, sm));
      }
    }
    {
      Timer t(a, RK_ENTRY_DECODE_LOSS, sm);
      if (a->ranges && !bounded) RK_TRY(rk_amax(a->Z0, (int64_t)B * h, a->ranges, sm));
      // (unbounded activations: the split scale of Z needs its maximum first)
      if (r.decode != DEC_PLAIN && !bounded) RK_TRY(rk_split_z(a->Z0, B, h, a->ranges, a->planes, sm));
      switch (r.decode) {
        case DEC_FDEC:
          RK_TRY(rk_fdec_loss_dz(a->planes, B, blk, a->row_off, a->par[RK_PAR_B_DE].p, a->loss_kind, a->confidence,
                                 a->inv_B, a->dO, a->do_rows, a->do_scales, a->loss_part, a->ws, sm));
          break;
        case DEC_DZ_PLANES:
          RK_TRY(rk_decode_loss_dz_planes(a->planes, B, blk, a->row_off, a->par[RK_PAR_B_DE].p, a->loss_kind,
                                          a->confidence, a->inv_B, a->dO, a->loss_part, a->gb_part, a->ws, sm));
          break;
        case DEC_PG:
          RK_TRY(rk_pg_decode_loss(a->planes, B, blk, a->row_off, a->par[RK_PAR_B_DE].p, a->loss_kind,
                                   a->confidence, a->inv_B, a->dO, a->do_rows, a->do_scales, nullptr,
                                   a->loss_part, a->gb_part, sm));
          break;
        case DEC_PLANES:
          RK_TRY(rk_decode_loss_planes(a->planes, B, blk, a->row_off, a->par[RK_PAR_B_DE].p, a->loss_kind,
                                       a->confidence, a->inv_B, a->dO, 0, a->loss_part, a->gb_part, sm));
          break;
        default:
          RK_TRY(rk_decode_loss(a->Z0, B, h, blk, a->row_off, W_de, a->par[RK_PAR_B_DE].p, a->loss_kind,
                                a->confidence, a->inv_B, a->dO, 0, a->loss_part, a->gb_part, a->ranges, sm));
      }
      if (mnll) RK_TRY(rk_mnll_finish(a->dO, B, blk, a->row_off, a->inv_B, nullptr, nullptr, nullptr, a->loss_part, sm));
    }
    // dO and the Z^T planes are ready: the dW branch starts here -- and so does whatever else the
    // caller queues behind this event (graph.GraphStepper: the look-ahead collation, which must not
    // run next to the decode: its workgroups do not fit into the LDS the fused decode leaves)
    if (r.dw_fork) RK_TRY(rk_event_record(a->dw_fork, sm));
    if (r.dw_place == DWP_EARLY) {
      Timer t(a, RK_ENTRY_DECODE_BWD_DW, sm);
      RK_TRY(dw_launch(a, r, sm));
    }
    if (!whole) {
      // the data-parallel exchange needs gb_de and the loss scalar as arrays of their own
      if (r.bias_colsum)
        RK_TRY(rk_colsum(a->gb_part, rk_cdiv(B, rk_decode_row_tile()), blk->n_cap, 0, blk->counts, a->gb_de, sm));
      RK_TRY(rk_loss_reduce(a->loss_part, n_part, a->denom, a->loss_out, sm));
    }
  }
  if (phase & RK_STEP_DZ_ENC) {
    {
      Timer t(a, RK_ENTRY_DECODE_BWD_DZ, sm);
      switch (r.decode) {
        case DEC_FDEC:        // (the fused decode left one slab per group of column tiles in the workspace)
          RK_TRY(rk_fdec_dz_reduce(a->ws, B, h, blk, a->Z0, a->act, a->dZ0, sm));
          break;
        case DEC_DZ_PLANES:   // (the decode launch left the column tiles' partials in the workspace)
          RK_TRY(rk_decode_dz_reduce(a->ws, B, h, blk, a->Z0, a->act, a->dZ0, sm));
          break;
        case DEC_PG:
          RK_TRY(rk_pg_dz(a->dO, a->do_scales, 64, 32, B, a->planes, blk, a->Z0, a->act, a->dZ0, a->ws, sm));
          break;
        case DEC_PLANES:
          RK_TRY(rk_decode_bwd_dz_planes(a->dO, B, a->planes, blk, a->Z0, a->act, a->dZ0, a->ws, sm));
          break;
        default:
          RK_TRY(rk_decode_bwd_dz(a->dO, B, h, blk, W_de, a->Z0, a->act, a->dZ0, a->ws, a->ranges, sm));
      }
    }
    switch (r.dw_place) {
      case DWP_EARLY: {
        Timer t(a, RK_ENTRY_ENCODE_BWD, sm);
        RK_TRY(rk_ae_encode_bwd(blk, a->row_off, B, a->dZ0, h, G_en, a->tied ? 1 : 0, a->gb_en, sm));
        break;
      }
      case DWP_MERGED: {     // dW || encoder backward in ONE launch on the chain: no side stream
        Timer t(a, RK_ENTRY_DECODE_BWD_DW, sm);
        if (r.dw_kernel == DWK_PG_32x64 && r.bias == BIAS_SLABS)   // (no column-sum range)
          RK_TRY(rk_pg_dw_encode_bwd_ones(a->dO, a->do_scales, 32, 64, B, a->planes, blk, r.dw_ws,
                                          a->row_off, a->dZ0, G_en, a->gb_en, a->gb_part, sm));
        else if (r.dw_kernel == DWK_PG_32x64)
          RK_TRY(rk_pg_dw_encode_bwd(a->dO, a->do_scales, 32, 64, B, a->planes, blk, r.dw_ws,
                                     a->row_off, a->dZ0, G_en, a->gb_en, a->gb_de, sm));
        else if (r.dw_kernel == DWK_PAIRS)
          RK_TRY(rk_decode_bwd_dw2_encode_bwd(a->dO, a->Z0, B, h, blk, r.dw_ws, zt, a->ranges, a->row_off, a->dZ0,
                                              G_en, a->gb_en, sm));
        else
          RK_TRY(rk_decode_bwd_dw_encode_bwd(a->dO, a->Z0, B, h, blk, a->G_de, a->row_off, a->dZ0, G_en,
                                             a->gb_en, a->ws, sm));
        break;
      }
      case DWP_BRANCH: {
        {
          Timer t(a, RK_ENTRY_ENCODE_BWD, sm);
          RK_TRY(rk_ae_encode_bwd(blk, a->row_off, B, a->dZ0, h, G_en, 0, a->gb_en, sm));
        }
        // (enqueued behind the chain: see rk_ae_step_t.dw_stream)
        RK_TRY(rk_stream_wait_event(a->dw_stream, a->dw_fork));
        {
          Timer t(a, RK_ENTRY_DECODE_BWD_DW, a->dw_stream);
          RK_TRY(dw_launch(a, r, a->dw_stream));
        }
        RK_TRY(rk_event_record(a->dw_join, a->dw_stream));
        RK_TRY(rk_stream_wait_event(sm, a->dw_join));
        break;
      }
      default: {
        // the dZ slabs in the workspace are consumed: dW takes it over (its own K slabs, which rk_adam_multi
        // sums while it reads the gradient)
        {
          Timer t(a, RK_ENTRY_DECODE_BWD_DW, sm);
          RK_TRY(dw_launch(a, r, sm));
        }
        Timer t(a, RK_ENTRY_ENCODE_BWD, sm);
        RK_TRY(rk_ae_encode_bwd(blk, a->row_off, B, a->dZ0, h, G_en, 0, a->gb_en, sm));
      }
    }
  }
  if (phase & RK_STEP_UPDATE) {
    rk_adam_job_t jobs[4];
    int32_t slots[4];
    const int n = route_jobs(a, r, jobs, slots);
    const int n_tab = n - 2;           // the embedding tables; the two bias jobs follow them
    // sharded dense Adam (rk_ae_step_t.zero_lo): the table jobs cover this rank's rows only and read the
    // reduce-scattered dense gradient shard -- row r of the table at zero_g + (r - zero_lo) * h
    if (a->zero_hi > 0) {
      RK_REQUIRE(!whole && a->zero_lo >= 0 && a->zero_lo <= a->zero_hi && a->zero_hi <= n_items && a->zero_g_en,
                 "zero_lo / zero_hi: a row range of the tables, phased steps, with the gradient shards");
      for (int k = 0; k < n_tab; ++k) {
        if (jobs[k].par.sparse) continue;
        const float *shard = slots[k] == RK_PAR_W_DE ? a->zero_g_de : a->zero_g_en;
        RK_REQUIRE(shard != nullptr, "zero_g_de");
        jobs[k].pos = nullptr; jobs[k].g_parts = 1; jobs[k].gparts_dev = nullptr;
        jobs[k].g = shard - (int64_t)a->zero_lo * h;
        jobs[k].row0 = a->zero_lo; jobs[k].row_step = 1; jobs[k].n_rows = a->zero_hi;
      }
    }
    // lazy dense Adam of the embedding tables (rk_adam_job_t.lazy_stamp): rows without a gradient that the next
    // step does not read are caught up later
    if (a->lazy_stamp_en) {
      // (whole steps, or the UPDATE call of a phased data-parallel step with the replicated update: every rank sweeps
      // the same rows of identical tables)
      RK_REQUIRE((whole || phase == RK_STEP_UPDATE) && a->cursor != nullptr && a->zero_hi == 0 && a->zero_gb_de == nullptr &&
                 a->lazy_period >= 1 && (a->tied || a->lazy_stamp_de),
                 "lazy Adam: replayed steps with the replicated update, both stamp arrays, lazy_period >= 1");
      for (int k = 0; k < n_tab; ++k) {
        if (jobs[k].par.sparse) continue;
        jobs[k].lazy_stamp = slots[k] == RK_PAR_W_DE ? a->lazy_stamp_de : a->lazy_stamp_en;
        jobs[k].lazy_pos_next = a->lazy_pos_next;
        jobs[k].lazy_period = a->lazy_period;
        jobs[k].lazy_need_list = a->lazy_pos_next ? a->lazy_need_list : nullptr;
        jobs[k].lazy_need_count = a->lazy_pos_next ? a->lazy_need_count : nullptr;
      }
    }
    if (a->zero_gb_de) {           // (per-rank item sets: the summed gradient arrives laid out by item id)
      RK_REQUIRE(!whole, "zero_gb_de: phased steps");
      jobs[n_tab].g = a->zero_gb_de; jobs[n_tab].pos = nullptr;
    }
    RK_REQUIRE(a->cursor == nullptr || a->adam_table != nullptr,
               "graph replay needs the Adam constants table");
    // replayed PHASED steps (data parallel): the caller's exchange has left the global loss in a
    // scalar of its own; the update phase gets it as loss_part[0] (denom 1) and this launch's loss
    // block files it under the step's slot of loss_out and publishes the next cursor
    const bool with_loss = whole || a->cursor != nullptr;
    // the two bias jobs go FIRST in the grid (the launch dispatches its workgroups in order): a few
    // dozen workgroups with a long chain of dependent loads (pos -> 8 partial gradient rows), which
    // as the LAST ones dispatched were the tail of the whole sweep (43 vs 37 us in isolation)
    rk_adam_job_t j2[4];
    int32_t s2[4];
    for (int k = 0; k < n; ++k) { j2[k] = jobs[(k + n_tab) % n]; s2[k] = slots[(k + n_tab) % n]; }
    Timer t(a, RK_ENTRY_ADAM_MULTI, sm);
    RK_TRY(rk_adam_multi_at(j2, n, with_loss ? a->loss_part : nullptr, whole ? n_part : 1,
                            whole ? a->denom : 1.0f, with_loss ? a->loss_out : nullptr, a->cursor,
                            a->cursor_off, a->adam_table,
                            RK_PAR_COUNT, s2, a->cursor_next, a->cursor_advance, sm));
  }
  return 0;
}
