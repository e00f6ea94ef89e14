// gop_session.hip — the GOP session of include/av1mi.h: closed-GOP orchestration, the encoder's filter-parameter policy and
// the PCIe plumbing around the block pipeline, in ONE place (round 1 had two hand-kept copies, pipeline.py and
// host/backend.cpp, that disagreed on the P-frame deblocking level).  What stands in for the encode the reference delegates
// to its FFmpeg child (internal/ffmpeg/transcode.go:120,194); the caller it serves is internal/daemon/daemon.go:101.
//
// Streams.  The context's stream runs the kernels; the session adds an upload stream and a download stream.  A batch is the stages
// of submit_batch, in this order on every stream:
//   feed_source       (a batch from the frame store, av1mi_gop_submit_stored: main: wait store.filled -> k_frames_gather into the fed buffers
//                     -> store.read_done, in place of the upload; the input stages follow as below.  A session that deinterlaces
//                     (av1mi_gop_config.deinterlace) launches k_deint_gather in its place: same events, and the store is only read)
//                     up:   wait slot.filters_done (the kernels that last read this slot's source) -> H2D of the fed buffers -> uploaded
//                     main: wait uploaded -> [k_input_convert] -> [k_chroma_convert] -> [k_scale | k_crop_copy] -> [k_tone_map] -> [k_depth_reduce]
//   code_blocks       main: k_intra_pipe | [k_me_down + k_me_coarse] + k_me_int + k_inter_pipe -> kernel_done
//   download_symbols  down: wait kernel_done -> D2H of the symbols into pinned memory
//   loop_filters      main: deblock_search ([lf_search]: levels and a map per frame), deblock_cdef (one kernel; at a padded size or with [cdef_search]
//                     the two on their own, the search between them), restore ([lr_search], k_lr_yuv (the sampled tiles of the three planes) ->
//                     k_lr_decide -> k_lr_yuv (the rest where restoration stays on) -> reference) -> filters_done;  down: download_search_results
//                     (the searches' mirrors -> search_down), (symbols for the host) the decision -> downloaded
//   measure_quality   main: (quality_stats) k_quality_tiles + k_quality_sum, the records written into the slot's pinned memory -> quality_done
//   start_coder       side: (GPU entropy coding) wait filters_done -> two memsets, k_av1_info / tokens / chains;  back: k_av1_code -> k_av1_gather,
//                     which stores payloads, tile sizes, total + status and the decision into the slot's pinned buffers -> ent_done (no copies)
// Source and symbol buffers exist kSlots = 3 times (slot = batch % 3): batch t + 2 uploads while batch t + 1 is in the block
// pipeline and the coder works on batch t, whose predecessor the host is still reading.  Four streams, one hardware queue each
// (a fifth would share a queue with one of these and serialise behind it).
//
// The source path: ONE layout, ONE chain.  av1mi_gop_source_layout (include/av1mi.h) says what a batch is FED: the buffers' luma size
// (the coded size, or with scaling the source size rounded up to 8), the true size inside them, the depth, and per plane its size and
// the bytes of one frame.  The session keeps that layout; every number of the fed side — buffers, store, gathers, analysis, the stages'
// launches, av1mi_gop_download_fed, the planes av1mi_gop_submit_device expects — is read from it.  A fed batch crosses PCIe from the
// slot's pinned h_in into d_in, is gathered there from a store, or is the caller's.  The CHAIN, built once by setup(), holds the 0-2
// input stages that turn it into the planar 4:2:0 planes at the coded size (d_src) which the block pipeline and the restoration
// decision read, one launch each on the main stream:
//   convert  input_format not PLANAR: k_input_convert (input_kernels.hip), wire format -> planar, at the fed size;  or
//   chroma   a source that is not 4:2:0 at bit_depth (planar only): k_chroma_convert, fed layout -> planar 4:2:0 at the fed size.
//            Where the depths are equal it passes the luma plane THROUGH: the plane stays in the buffer it is in;  then
//   scale    source_width given: the resampler (scale_kernels.hip), fed size -> coded size.
// The crop window (av1mi_gop_config.crop_*) is NOT a stage of its own and adds no plane: it is handed to the last stage as an origin
// and the fed planes' stride.  Where the window is resampled that stage is `scale`, whose plan then reads from the window's origin and
// clamps at the window's edges; where the window's size is the target, `crop` (k_crop_copy, crop_kernels.hip) takes scale's place and
// copies the window, replicating its last column / row into the coded planes' padding.  Either way the chain stays at most two stages
// (convert | chroma, then scale | crop) with d_pre between them, and a session without a window builds exactly the chain it always did.
// slot_buffers() walks the chain once per slot and plane: the last stage that writes a plane writes d_src, a stage before it a plane
// between (d_pre), and a plane that no stage writes IS d_src from the start (all planes with ZERO stages, the luma plane behind chroma
// alone): the upload lands where the kernels read.  feed_source() walks it once per batch.
//
// The coded depth.  cfg.bit_depth is the depth of the INPUT side: the fed layout, the chain, the tone map.  What everything from
// code_blocks on works at — planes, policy, pipelines, filters, searches, coder, quality records — is coded_depth(cfg), kept as g->bd, and
// nothing behind the chain reads cfg.bit_depth.  Where the two differ (cfg.coded_bit_depth 8 in a 10-bit session) the chain ends in d_work,
// the slot's planar planes at bit_depth and the coded size, instead of d_src, and ONE more launch at the end of feed_source (k_depth_reduce,
// depth_kernels.hip) writes the 8-bit d_src from wherever the planes are then: d_work, or in a device batch the caller's planes, which it
// only reads.  A session without the option has no d_work and launches what it always did.
//
// The frame store (av1mi_gop_config.store_frames; nothing of it exists at 0).  Two stores of store_frames fed frames, a plane per
// buffer, frames in file order.  The upload stream carries everything that fills and reads a store for the analysis: the puts (pinned
// buffer -> store), then the three launches of the scene analysis, whose last one writes the records into pinned memory; scene_done is
// what av1mi_gop_store_analyse waits for, so the batches of the OTHER store that are in flight on the main stream are not waited for.
// The main stream reads a store only in a batch's gather: it waits for store.filled (recorded behind the last put) and records
// store.read_done behind the gather, which the next put into that store waits for on the upload stream.  No host wait orders the two.
#include <algorithm>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "av1mi_internal.hpp"
#include "quality.hpp"

namespace {

// ---- the policy (non-normative encoder choices; mirrored nowhere else) ---------------------------------------------------
int lf_level_from_q(int ac_q, int bd, bool key) {   // libaom LPF_PICK_FROM_Q: a linear fit of the level to the AC step
  long g;
  if (bd == 8) g = key ? ((long)ac_q * 17563 - 421574 + (1 << 17)) >> 18 : ((long)ac_q * 6017 + 650707 + (1 << 17)) >> 18;
  else g = ((long)ac_q * 20723 + 4060632 + (1 << 19)) >> 20;
  return (int)(g < 0 ? 0 : g > 63 ? 63 : g);
}
void frame_params(int q, int bd, int frame_type, av1mi_frame_params *p) {
  memset(p, 0, sizeof(*p));
  const int ac_q = av1mi_ac_q(q, bd), q8 = ac_q >> (bd - 8);
  p->frame_type = frame_type; p->base_q_idx = q;
  const int lvl = lf_level_from_q(ac_q, bd, frame_type == 0);
  p->lf_level[0] = p->lf_level[1] = p->lf_level[2] = p->lf_level[3] = lvl;
  p->lf_sharpness = 0;
  // CDEF strengths from the quantiser step: libaom's CDEF_PICK_FROM_Q fit (pickcdef.c av1_pick_cdef_from_qp: quadratic fits of the
  // strengths its full search picks, separate for intra-only and inter frames; secondary codes 0..3 = strengths 0, 1, 2, 4).  At
  // mid quantisers inter frames get secondary strength 0: two thirds of k_cdef's taps drop out (cdef_kernel.hip).
  p->cdef_damping = 3 + (q >> 6);
  {
    const float x = (float)q8, x2 = x * x;
    auto fit = [&](float a, float b, float c, int hi) { const int v = (int)lroundf(x2 * a + x * b + c); return v < 0 ? 0 : v > hi ? hi : v; };
    int y1, y2, c1, c2;
    if (frame_type == 0) {
      y1 = fit(0.0000033731974f, 0.008070594f, 0.0187634f, 15); y2 = fit(0.0000029167343f, 0.0027798624f, 0.0079405f, 3);
      c1 = fit(-0.0000130790995f, 0.012892405f, -0.00748388f, 15); c2 = fit(0.0000032651783f, 0.00035520183f, 0.00228092f, 3);
    } else {
      y1 = fit(-0.0000023593946f, 0.0068615186f, 0.02709886f, 15); y2 = fit(-0.00000057629734f, 0.0013993345f, 0.03831067f, 3);
      c1 = fit(-0.0000007095069f, 0.0034628846f, 0.00887099f, 15); c2 = fit(0.00000023874085f, 0.00028223585f, 0.05576307f, 3);
    }
    p->cdef_y = (uint8_t)(y1 << 2 | y2); p->cdef_uv = (uint8_t)(c1 << 2 | c2);
  }
  p->lr_unit_size = 64;
  static const int8_t wy[8] = { 1, 3, -7, 15, 3, -7, 15, 0 }, wc[8] = { 1, 0, -7, 15, 0, -7, 15, 0 };   // Wiener, libaom's mid-range taps
  memcpy(p->lr_unit_y, wy, 8); memcpy(p->lr_unit_uv, wc, 8);
}

enum { kSlots = 3, kFallbacksToHostMode = 3, kMaxStages = 2 };      // batches in flight: one uploading / in the block pipeline, one in the coder, one being read by the host

// plane p of the session's 4:2:0 frames: subsampling shift, coded and true (visible) size of one frame, samples and bytes of a batch
struct Plane { int ss = 0, w = 0, h = 0, vw = 0, vh = 0; size_t n = 0, bytes = 0; };

struct Slot {
  // the source as fed (the session's format, at the fed size): pinned + device, [2] unused by the semi-planar formats
  void *h_in[3] = { nullptr, nullptr, nullptr }, *d_in[3] = { nullptr, nullptr, nullptr };
  void *d_pre[3] = { nullptr, nullptr, nullptr };       // two stages: the planar planes at the fed size that the first one writes
  void *stage_out[kMaxStages][3] = {};                  // where stage k writes plane p, resolved at open; null = the plane passes through
  void *d_src[3] = { nullptr, nullptr, nullptr };       // planar, coded size, coded depth: what the block pipeline and the restoration decision read
  void *d_work[3] = { nullptr, nullptr, nullptr };      // depth reduction: planar, coded size, at bit_depth: where the chain ends; the stage writes d_src
  // symbols: device + pinned host mirror
  void *d_lev[3] = { nullptr, nullptr, nullptr }, *h_lev[3] = { nullptr, nullptr, nullptr };
  void *d_modes[2] = { nullptr, nullptr }, *h_modes[2] = { nullptr, nullptr };
  void *d_mv = nullptr, *h_mv = nullptr, *d_skip = nullptr, *h_skip = nullptr;
  hipEvent_t uploaded = nullptr, kernel_done = nullptr, filters_done = nullptr, downloaded = nullptr;
  bool upload_pending = false, kernel_pending = false;
  // restoration on / off per (segment, plane), decided by the GPU against the source (k_lr + k_lr_decide): device + pinned mirror
  void *d_lr_on = nullptr, *h_lr_on = nullptr;
  // lr_search: the batch's chosen unit records per plane, the cost table and the index bytes — per SLOT: the tokenizer of batch t reads
  // the records while the filters of batch t + 1 run — and their pinned mirrors
  void *d_lr_units[3] = {}, *h_lr_units[3] = {}, *d_lr_cost = nullptr, *d_lr_choice = nullptr, *h_lr_choice = nullptr;
  // cdef_search: the batch's cost table, the chosen strength records and index bytes — per SLOT for the same reason — the indices' mirror
  void *d_cdef_cost = nullptr, *d_cdef_rec = nullptr, *d_cdef_idx = nullptr, *h_cdef_idx = nullptr;
  // lf_search: the batch's header levels [segment][4] and chosen candidates [segment][2] — per SLOT: the host reads them while later
  // batches search — and their pinned mirrors
  void *d_lf_levels = nullptr, *h_lf_levels = nullptr, *d_lf_choice = nullptr, *h_lf_choice = nullptr;
  // the searches' results path: what the enabled searches send to the host with every batch, in the order slot_buffers() allocated it (lr
  // units x 3, lr choice, cdef idx, lf levels, lf choice), copied behind the filters on the download stream in front of search_down
  struct Mirror { const void *device; void *pinned; size_t bytes; } mirror[7] = {}; int mirrors = 0;
  hipEvent_t search_down = nullptr;
  int frame_type = 0;
  int q = 0;                          // the batch's quantiser (av1mi_gop_set_base_q_idx) and what the policy derives from it for its frame type
  av1mi_frame_params params{};
  // GPU entropy coding (gpu_entropy != 0): coded tile payloads (pinned host memory, written by the GPU) + sizes (device + pinned mirror)
  void *h_ent_out = nullptr, *d_tile_size = nullptr, *h_tile_size = nullptr, *d_total = nullptr, *h_total = nullptr;
  hipEvent_t ent_done = nullptr;      // coder + download of sizes / total finished (side stream)
  bool ent_pending = false;
  bool symbols_down = false;          // this batch's symbols were sent to the host at submit time
  int ent_ticket = -1;                // >= 0: the range coder of this batch is still to be launched (coder_streams 3: av1_entropy_back)
  // quality_stats: the batch's records [segment * 3 + plane], pinned and written by the GPU (k_quality_sum); quality_done follows
  void *h_quality = nullptr;
  hipEvent_t quality_done = nullptr;
  // store_frames: the gather's table of this slot's batch, [segment * 3 + plane] source pointers: pinned, and the device copy the kernel reads
  void *h_table = nullptr, *d_table = nullptr;
  // denoise: the batch's grain records [segment * 3 + plane], pinned and written by the GPU (k_grain_sum); grain_done follows
  void *h_grain = nullptr;
  void *h_grain_cov = nullptr;        // grain_cov: the batch's covariance records beside them (k_grain_cov_sum), in front of the same event
  hipEvent_t grain_done = nullptr;
  bool has_grain = false;             // this batch went through the denoising gather (a batch of av1mi_gop_submit_device does not)
};

// one frame store: a buffer per plane, store_frames frames of layout.plane[p].frame_bytes each
struct Store {
  void *d[3] = { nullptr, nullptr, nullptr };
  hipEvent_t filled = nullptr, read_done = nullptr;      // behind the last put (upload stream) / behind the last gather (main stream)
  bool has_fill = false, has_reader = false;
  int run = 0;                                           // frames 0 .. run - 1 were put since position 0 was last put: the deinterlacer's run
};

}  // namespace

struct av1mi_gop {
  av1mi_ctx *ctx = nullptr;
  av1mi_gop_config cfg{};
  Plane plane[3];                              // the coded planes
  int bd = 8;                                  // the CODED depth (coded_depth(cfg)): what everything behind the input chain works at
  size_t nb = 0, bps = 1;                      // blocks of a BATCH (segments stacked), bytes per sample of the coded planes
  av1mi_source_layout layout{};                // what the session is fed (av1mi_gop_source_layout(cfg)): the fed side's only geometry
  int stages = 0, chain[kMaxStages] = {};      // the input stages in launch order (Stage)
  uintptr_t fed_align = 8;                     // of the planes av1mi_gop_submit_device is given: 16 where convert or chroma reads them (16-byte loads)
  av1mi::ScalePlan *scale = nullptr;           // scaling sessions: the resampler's tables
  bool cropping = false;                       // cfg.crop_*: the window, handed to the scale stage's plan or to the crop stage
  av1mi::CropWindow window{};
  hipStream_t up = nullptr, down = nullptr;     // with the context's main and side streams: four, one hardware queue each
  Slot slot[kSlots];
  void *d_rec[3] = {}, *d_dbl[3] = {}, *d_cdef[3] = {}, *d_ref[3] = {};
  void *d_mi[3][2] = {};                       // [key / inter / key in 32x32 blocks][luma / chroma] deblocking mode-info maps (one frame, shared by the batch)
  // lf_search: a map per frame of a batch [luma / chroma] (k_mi_levels_frames writes them from d_mi in front of the batch's deblocking),
  // the search's scratch table and its sums — once per session: the batches are serial on the main stream
  void *d_mi_frames[2] = {}, *d_lf_table = nullptr, *d_lf_sse = nullptr;
  int key32 = 0, key_rows32 = 0;               // key frames in 32x32 blocks over the first key_rows32 luma rows (the complete superblock rows)
  int key_modes_band = 0, key_modes_stride = 0;  // mode bytes per segment: the 32x32 blocks, then (from key_modes_band) the 8x8 blocks of the last rows
  void *d_cdef_sb[2] = {}, *d_lr[2] = {}, *d_zero_skip = nullptr;
  void *d_lr_scratch = nullptr;                // the restoration decision's partial sums (three planes)
  int lr_units[3] = {};                        // lr_search: units per frame of Y, U, V
  void *d_me = nullptr;                        // coarse_range: the coarse search's quarter planes and centres of one batch (single: the chain is serial in t)
  void *d_denoise_vectors = nullptr;           // denoise_range: the blocks' vectors of one batch (the main stream orders its users)
  void *d_grain_scratch = nullptr;             // denoise: the workgroups' partial records of one batch (the main stream orders its users)
  void *d_grain_cov_scratch = nullptr;         // grain_cov: the workgroups' partial sums of one batch (likewise)
  void *d_tone_tables = nullptr;               // tone_map: the tables (av1mi_tone_tables), uploaded at open
  void *d_quality_scratch = nullptr;           // quality_stats: the tiles' partial sums of one batch (the main stream orders its users)
  int vw = 0, vh = 0;                          // the true frame size (== the coded size unless cfg.visible_* say otherwise)
  int last = 0;                                // slot of the most recent batch (its d_lr_on selects the next batch's references)
  av1mi_frame_params params[2];                // key, inter: at the session's own quantiser (cfg.base_q_idx), what side_information builds from
  int next_q = 0;                              // the quantiser of the batches to come (av1mi_gop_set_base_q_idx; cfg.base_q_idx until then)
  int mi_q[3] = {}, cdef_q[2] = {};            // the quantiser whose levels d_mi[t] / whose strengths d_cdef_sb[t] hold now (follow_q rewrites them)
  size_t ent_cap = 0; int tiles = 0;           // GPU entropy coding: payload capacity of a batch, tiles per frame
  long submitted = 0, collected = 0;           // batches
  long fallbacks = 0;                          // batches the GPU coder could not hold (handed out as symbols instead)
  bool symbols_always = false;                 // after kFallbacksToHostMode of them: the symbols go down with every batch, beside the filters
  int gop_pos = 0;
  bool acquired = false;
  int coder_streams = 0;                       // 0 = tokenizer + chains on the side stream, range coder on the back stream (default)
  int intra_open_loop = 0;                     // key frames: open-loop mode decision (k_intra_modes) instead of the closed-loop search
  Store store[2];                              // the frame store (cfg.store_frames != 0)
  void *d_scene = nullptr, *h_records = nullptr;      // the analysis' scratch area (one store's) and its records, pinned
  hipEvent_t scene_done = nullptr;
  void *d_telecine = nullptr, *h_telecine = nullptr;  // telecine: the field-match records' partials (one store's) and the records, pinned
  hipEvent_t telecine_done = nullptr;                 // ... and the event behind them: its own, so the scene analysis and this never wait for each other's records
  long puts = 0;                               // av1mi_gop_store_put calls: the pinned buffers of slot puts % kSlots are handed out next
  hipEvent_t put_done[kSlots] = {};            // the copy that last read those pinned buffers
  bool put_pending[kSlots] = {};
  std::vector<void *> dev_allocs, host_allocs;
};

namespace {

#define G_HIP(expr)                                                                                          \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return av1mi::ctx_fail(g->ctx, AV1MI_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define G_TRY(expr)                              \
  do {                                           \
    int rc_ = (expr);                            \
    if (rc_ != AV1MI_OK) return rc_;             \
  } while (0)

int dev_alloc(av1mi_gop *g, void **p, size_t bytes) {
  G_HIP(hipMalloc(p, bytes ? bytes : 8));
  g->dev_allocs.push_back(*p);
  return AV1MI_OK;
}
int host_alloc(av1mi_gop *g, void **p, size_t bytes) {
  G_HIP(hipHostMalloc(p, bytes ? bytes : 8, hipHostMallocDefault));
  g->host_allocs.push_back(*p);
  return AV1MI_OK;
}

// THE place that says what depth is coded: the input side's, unless the config asks for the reduction
int coded_depth(const av1mi_gop_config &c) { return c.coded_bit_depth ? c.coded_bit_depth : c.bit_depth; }
bool reducing(const av1mi_gop *g) { return g->bd != g->cfg.bit_depth; }
// the frames a store holds: store_frames, and in a session that weaves room for one context frame in front of a group and one behind it
int store_capacity(const av1mi_gop_config &c) { return c.store_frames + (c.telecine ? 2 : 0); }

enum Stage { kConvert, kChroma, kScale, kCrop };      // the input stages (the chain of "The source path"); kCrop stands where kScale would
// Does stage k write plane p?  All do but chroma at equal depths, which passes the luma plane through
bool stage_writes(const av1mi_gop *g, int k, int p) { return !(g->chain[k] == kChroma && p == 0 && g->layout.bit_depth == g->cfg.bit_depth); }
size_t fed_bytes(const av1mi_gop *g, int p) { return g->layout.plane[p].frame_bytes * (size_t)g->cfg.segments; }      // plane p of a batch as fed

// the fed planes at their true sizes, for the filtering gathers: chroma subsampled where the layout's plane is smaller than the luma
// buffer.  s: the slot whose table is read and whose fed buffers are written, or null where only the sizes are asked for
void fed_geometry(const av1mi_gop *g, const Slot *s, av1mi::GatherPlanes &L) {
  const av1mi_source_layout &Y = g->layout;
  L.bd = Y.bit_depth; L.segments = g->cfg.segments; L.table = s ? (const void *const *)s->d_table : nullptr;
  for (int p = 0; p < 3; p++) {
    const int sx = Y.plane[p].width < Y.width, sy = Y.plane[p].height < Y.height;
    L.plane_w[p] = Y.plane[p].width; L.plane_h[p] = Y.plane[p].height; L.dst[p] = s ? s->d_in[p] : nullptr;
    L.true_w[p] = (Y.true_width + sx) >> sx; L.true_h[p] = (Y.true_height + sy) >> sy;
  }
}

int slot_buffers(av1mi_gop *g, Slot &s) {
  const av1mi_gop_config &c = g->cfg;
  const int S = c.segments;
  for (int p = 0; p < 3; p++) {
    const Plane &P = g->plane[p];
    // the source: pinned + device as fed, then the chain's planes (a plane that no stage writes is fed straight into d_src)
    if (fed_bytes(g, p)) G_TRY(host_alloc(g, &s.h_in[p], fed_bytes(g, p)));
    G_TRY(dev_alloc(g, &s.d_src[p], P.bytes));
    void *end = s.d_src[p];      // where the chain leaves the plane: d_src, or in front of the depth reduction d_work
    if (reducing(g)) { G_TRY(dev_alloc(g, &s.d_work[p], P.n * 2)); end = s.d_work[p]; }
    int last = -1;
    for (int k = 0; k < g->stages; k++) if (stage_writes(g, k, p)) last = k;
    if (last < 0) s.d_in[p] = end;
    else if (fed_bytes(g, p)) G_TRY(dev_alloc(g, &s.d_in[p], fed_bytes(g, p)));
    for (int k = 0; k <= last; k++) {
      if (!stage_writes(g, k, p)) continue;
      if (k < last) G_TRY(dev_alloc(g, &s.d_pre[p], av1mi_input_plane_bytes(AV1MI_INPUT_PLANAR, c.bit_depth, p, g->layout.width, g->layout.height * S)));
      s.stage_out[k][p] = k < last ? s.d_pre[p] : end;
    }
    // the pinned mirror of the levels (as large as the source) is needed when the symbols go to the host; with the GPU coder
    // only a batch the coder gives back needs it, and it is allocated then (pinning memory is a good part of the start-up time)
    if (c.gpu_entropy != 1) G_TRY(host_alloc(g, &s.h_lev[p], P.n * 2));
    G_TRY(dev_alloc(g, &s.d_lev[p], P.n * 2));
  }
  for (int k = 0; k < 2; k++) { G_TRY(host_alloc(g, &s.h_modes[k], g->nb)); G_TRY(dev_alloc(g, &s.d_modes[k], g->nb)); }
  G_TRY(host_alloc(g, &s.h_mv, g->nb * 4)); G_TRY(dev_alloc(g, &s.d_mv, g->nb * 4));
  G_TRY(host_alloc(g, &s.h_skip, g->nb)); G_TRY(dev_alloc(g, &s.d_skip, g->nb));
  for (hipEvent_t *e : { &s.uploaded, &s.kernel_done, &s.filters_done, &s.downloaded }) G_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  G_TRY(dev_alloc(g, &s.d_lr_on, (size_t)S * 3 + 4)); G_TRY(host_alloc(g, &s.h_lr_on, (size_t)S * 3));      // (+ 4: the kernels read the flags as aligned dwords)
  if (c.gpu_entropy) {
    G_TRY(host_alloc(g, &s.h_ent_out, g->ent_cap));        // pinned and device-visible: the gather kernel writes it over PCIe
    G_TRY(dev_alloc(g, &s.d_tile_size, (size_t)g->tiles * S * 4)); G_TRY(host_alloc(g, &s.h_tile_size, (size_t)g->tiles * S * 4));
    G_TRY(dev_alloc(g, &s.d_total, 16)); G_TRY(host_alloc(g, &s.h_total, 16));
    G_HIP(hipEventCreateWithFlags(&s.ent_done, hipEventDisableTiming));
  }
  if (c.store_frames) {
    // (a session that deinterlaces or denoises keeps three pointers per segment and plane: the frames before, at and after the position)
    // (a session that weaves two: the top and the bottom source)
    const size_t entries = (size_t)S * 3 * (c.deinterlace || c.denoise ? 3 : c.telecine ? 2 : 1);
    // (at field rate a phase byte per segment rides behind the pointers, in the same copy)
    const size_t phases = c.deinterlace_fields ? (size_t)S : 0;
    G_TRY(host_alloc(g, &s.h_table, entries * sizeof(void *) + phases));
    G_TRY(dev_alloc(g, &s.d_table, entries * sizeof(void *) + phases));
  }
  if (c.denoise) {
    G_TRY(host_alloc(g, &s.h_grain, (size_t)S * 3 * sizeof(av1mi_grain_record)));
    G_HIP(hipEventCreateWithFlags(&s.grain_done, hipEventDisableTiming));
    if (c.grain_cov) G_TRY(host_alloc(g, &s.h_grain_cov, (size_t)S * 3 * sizeof(av1mi_grain_cov_record)));
  }
  auto mirrored = [&](void **d, void **h, size_t bytes) {      // a search's result the host gets: device array + pinned mirror, entered into the slot's table
    G_TRY(dev_alloc(g, d, bytes)); G_TRY(host_alloc(g, h, bytes));
    s.mirror[s.mirrors++] = { *d, *h, bytes }; return (int)AV1MI_OK;
  };
  if (c.lr_search) {
    for (int p = 0; p < 3; p++) G_TRY(mirrored(&s.d_lr_units[p], &s.h_lr_units[p], (size_t)S * g->lr_units[p] * 8));
    G_TRY(dev_alloc(g, &s.d_lr_cost, av1mi_lr_search_scratch_bytes(c.width, c.height, 64, S)));
    G_TRY(mirrored(&s.d_lr_choice, &s.h_lr_choice, (size_t)S * (g->lr_units[0] + g->lr_units[1] + g->lr_units[2])));
  }
  if (c.cdef_search) {
    const size_t nsb = (size_t)S * av1mi::sb_count(c.width, c.height);
    G_TRY(dev_alloc(g, &s.d_cdef_cost, av1mi_cdef_search_table_bytes(c.width, c.height, S)));
    G_TRY(dev_alloc(g, &s.d_cdef_rec, nsb * 4)); G_TRY(mirrored(&s.d_cdef_idx, &s.h_cdef_idx, nsb));
  }
  if (c.lf_search) { G_TRY(mirrored(&s.d_lf_levels, &s.h_lf_levels, (size_t)S * 4)); G_TRY(mirrored(&s.d_lf_choice, &s.h_lf_choice, (size_t)S * 2)); }
  if (s.mirrors) G_HIP(hipEventCreateWithFlags(&s.search_down, hipEventDisableTiming));
  if (c.quality_stats) {
    G_TRY(host_alloc(g, &s.h_quality, (size_t)S * 3 * sizeof(av1mi_quality)));
    G_HIP(hipEventCreateWithFlags(&s.quality_done, hipEventDisableTiming));
  }
  return AV1MI_OK;
}

// constant side information: one map per frame type, shared by every frame of a batch (frame stride 0)
int side_information(av1mi_gop *g) {
  const av1mi_gop_config &c = g->cfg;
  const int w = c.width, h = c.height;
  const size_t fy = (size_t)w * h, fc = fy / 4;
  const int nsb = av1mi::sb_count(w, h);
  auto units = [](int n) { const int u = (n + 32) / 64; return u > 1 ? u : 1; };
  const size_t uy = (size_t)units(h) * units(w), uc = (size_t)units(h / 2) * units(w / 2);
  if (c.key_block_size == 32) {
    g->key32 = 1; g->key_rows32 = (h / 64) * 64;
    // mode bytes of a frame: the 32x32 blocks from entry 0, the 8x8 blocks of the last rows where the 8x8 grid has them anyway
    g->key_modes_band = (g->key_rows32 / 8) * (w / 8);
    g->key_modes_stride = (h / 8) * (w / 8);
  }
  for (int t = 0; t < 2 + g->key32; t++) {
    if (t < 2) frame_params(c.base_q_idx, g->bd, t, &g->params[t]);
    const av1mi_frame_params &P = g->params[t == 2 ? 0 : t];
    // deblocking mode-info words (av1mi_deblock_plane): 8x8 luma / 4x4 chroma transforms, every block edge a prediction edge
    std::vector<uint32_t> mi(fy / 16, 3u | (3u << 4) | ((uint32_t)P.lf_level[0] << 8) | ((uint32_t)P.lf_level[1] << 16) | (3u << 25));
    std::vector<uint32_t> mic(fc / 16, 2u | (2u << 4) | ((uint32_t)P.lf_level[2] << 8) | ((uint32_t)P.lf_level[2] << 16) | (3u << 25));
    // units that start at or beyond the true size (spec 7.14.2 onScreen; a chroma unit is two luma units wide) are never filtered:
    // "skipped inter block, no block edge"
    for (int r = 0; r < h / 4; r++) for (int cc = 0; cc < w / 4; cc++) if (4 * r >= g->vh || 4 * cc >= g->vw) mi[(size_t)r * (w / 4) + cc] = 3u | (3u << 4) | (1u << 24);
    for (int r = 0; r < h / 8; r++) for (int cc = 0; cc < w / 8; cc++) if (8 * r >= g->vh || 8 * cc >= g->vw) mic[(size_t)r * (w / 8) + cc] = 2u | (2u << 4) | (1u << 24);
    if (t == 2) {      // key frames in 32x32 blocks: 32x32 luma / 16x16 chroma transforms over the complete superblock rows (always on screen)
      for (int r = 0; r < g->key_rows32 / 4; r++) for (int cc = 0; cc < w / 4; cc++) mi[(size_t)r * (w / 4) + cc] = (mi[(size_t)r * (w / 4) + cc] & ~0xFFu) | 5u | (5u << 4);
      for (int r = 0; r < g->key_rows32 / 8; r++) for (int cc = 0; cc < w / 8; cc++) mic[(size_t)r * (w / 8) + cc] = (mic[(size_t)r * (w / 8) + cc] & ~0xFFu) | 4u | (4u << 4);
    }
    G_TRY(dev_alloc(g, &g->d_mi[t][0], mi.size() * 4)); G_TRY(av1mi_upload(g->ctx, g->d_mi[t][0], mi.data(), mi.size() * 4));
    G_TRY(dev_alloc(g, &g->d_mi[t][1], mic.size() * 4)); G_TRY(av1mi_upload(g->ctx, g->d_mi[t][1], mic.data(), mic.size() * 4));
    g->mi_q[t] = c.base_q_idx;
  }
  for (int t = 0; t < 2; t++) {      // CDEF strengths: one set per frame type
    const av1mi_frame_params &P = g->params[t];
    std::vector<uint8_t> sb((size_t)nsb * 4);
    for (int i = 0; i < nsb; i++) { sb[4 * i] = P.cdef_y >> 2; sb[4 * i + 1] = P.cdef_y & 3; sb[4 * i + 2] = P.cdef_uv >> 2; sb[4 * i + 3] = P.cdef_uv & 3; }
    G_TRY(dev_alloc(g, &g->d_cdef_sb[t], sb.size())); G_TRY(av1mi_upload(g->ctx, g->d_cdef_sb[t], sb.data(), sb.size()));
    g->cdef_q[t] = c.base_q_idx;
  }
  {
    const av1mi_frame_params &P = g->params[0];     // the restoration units do not depend on the frame type
    std::vector<int8_t> lr((uy > uc ? uy : uc) * 8);
    for (size_t i = 0; i < uy; i++) memcpy(&lr[i * 8], P.lr_unit_y, 8);
    G_TRY(dev_alloc(g, &g->d_lr[0], uy * 8)); G_TRY(av1mi_upload(g->ctx, g->d_lr[0], lr.data(), uy * 8));
    for (size_t i = 0; i < uc; i++) memcpy(&lr[i * 8], P.lr_unit_uv, 8);
    G_TRY(dev_alloc(g, &g->d_lr[1], uc * 8)); G_TRY(av1mi_upload(g->ctx, g->d_lr[1], lr.data(), uc * 8));
  }
  if (c.lf_search) {      // a map per frame of a batch, the scratch table [segment][superblock][2][8] and the sums [segment][2][8]
    G_TRY(dev_alloc(g, &g->d_mi_frames[0], (size_t)c.segments * (fy / 16) * 4)); G_TRY(dev_alloc(g, &g->d_mi_frames[1], (size_t)c.segments * (fc / 16) * 4));
    G_TRY(dev_alloc(g, &g->d_lf_table, av1mi_lf_search_scratch_bytes(w, h, c.segments)));
    G_TRY(dev_alloc(g, &g->d_lf_sse, (size_t)c.segments * 2 * AV1MI_LF_SEARCH_CANDIDATES * sizeof(uint64_t)));
  }
  return AV1MI_OK;
}

// av1mi_gop_open's argument rules: null = fine, else the reason (written into buf)
const char *config_error(const av1mi_gop_config *c, char (&buf)[512]) {
#define WHY(...) (snprintf(buf, sizeof(buf), __VA_ARGS__), buf)
  if (!c) return WHY("null config");
  if (c->width <= 0 || c->height <= 0 || (c->width & 7) || (c->height & 7) || c->width > 16384 || c->height > 16384)
    return WHY("frame %dx%d must be a multiple of 8", c->width, c->height);
  if (c->visible_width < 0 || c->visible_height < 0 || (c->visible_width && (c->visible_width > c->width || c->width - c->visible_width >= 8)) ||
      (c->visible_height && (c->visible_height > c->height || c->height - c->visible_height >= 8)))
    return WHY("visible size %dx%d must lie within 7 samples below the coded size %dx%d", c->visible_width, c->visible_height, c->width, c->height);
  if (c->bit_depth != 8 && c->bit_depth != 10) return WHY("bit depth %d not supported (8 or 10)", c->bit_depth);
  if (c->base_q_idx < 1 || c->base_q_idx > 255 || c->gop_length < 1 || c->segments < 1 || c->segments > 4096 || c->search_range < 0 ||
      c->search_range > 15 || c->gpu_entropy < 0 || c->gpu_entropy > 2 || c->coder_streams < 0 || c->coder_streams > 3)
    return WHY("bad base_q_idx / gop_length / segments / search_range / gpu_entropy");
  if (c->input_format < AV1MI_INPUT_PLANAR || c->input_format > AV1MI_INPUT_NV12)
    return WHY("input_format %d unknown (0 planar, 1 packed 10-bit, 2 P010, 3 NV12)", c->input_format);
  if ((c->input_format == AV1MI_INPUT_PACKED10 || c->input_format == AV1MI_INPUT_P010) && c->bit_depth != 10)
    return WHY("input_format %d (%s) needs bit_depth 10, not %d", c->input_format, c->input_format == AV1MI_INPUT_P010 ? "P010" : "packed 10-bit", c->bit_depth);
  if (c->input_format == AV1MI_INPUT_NV12 && c->bit_depth != 8) return WHY("input_format 3 (NV12) needs bit_depth 8, not %d", c->bit_depth);
  if (c->source_chroma < AV1MI_CHROMA_420 || c->source_chroma > AV1MI_CHROMA_400)
    return WHY("source_chroma %d unknown (0 4:2:0, 1 4:2:2, 2 4:4:4, 3 grey)", c->source_chroma);
  if (c->source_bit_depth != 0 && c->source_bit_depth != 8 && c->source_bit_depth != 10 && c->source_bit_depth != 12)
    return WHY("source_bit_depth %d not supported (8, 10 or 12; 0 = bit_depth)", c->source_bit_depth);
  if (const char *why = av1mi::chroma_format_error(c->source_chroma, c->source_bit_depth ? c->source_bit_depth : c->bit_depth, c->bit_depth))
    return WHY("source_bit_depth %d with bit_depth %d: %s", c->source_bit_depth, c->bit_depth, why);
  if ((c->source_chroma != AV1MI_CHROMA_420 || (c->source_bit_depth && c->source_bit_depth != c->bit_depth)) && c->input_format != AV1MI_INPUT_PLANAR)
    return WHY("a source that is not 4:2:0 at bit_depth (source_chroma %d, source_bit_depth %d) needs input_format 0 (planar), not %d", c->source_chroma,
               c->source_bit_depth, c->input_format);
  if ((c->source_width != 0) != (c->source_height != 0) || c->source_width < 0 || c->source_height < 0)
    return WHY("source size %dx%d: give both source_width and source_height, or neither", c->source_width, c->source_height);
  const bool crop = c->crop_x || c->crop_y || c->crop_width || c->crop_height;
  if (crop) {
    const int x = c->crop_x, y = c->crop_y, cw = c->crop_width, ch = c->crop_height;
    if (!c->source_width) return WHY("crop window %dx%d+%d+%d: a session with a window is fed whole frames, give their true size as source_width x source_height", cw, ch, x, y);
    if (c->source_width < 16 || c->source_height < 16 || c->source_width > 16384 || c->source_height > 16384)
      return WHY("crop window: source size %dx%d out of range (16 .. 16384)", c->source_width, c->source_height);
    if (x < 0 || y < 0 || cw < 0 || ch < 0 || ((x | y | cw | ch) & 1)) return WHY("crop window %dx%d+%d+%d: the four numbers must be even and not negative", cw, ch, x, y);
    if (cw < 16 || ch < 16) return WHY("crop window %dx%d+%d+%d: smaller than 16x16", cw, ch, x, y);
    if (x > c->source_width - cw || y > c->source_height - ch)
      return WHY("crop window %dx%d+%d+%d lies outside the source's true size %dx%d", cw, ch, x, y, c->source_width, c->source_height);
  }
  if (c->source_width) {      // what is resampled: the window, or the whole fed frame; a window of the target's size is copied
    const int tw = c->visible_width ? c->visible_width : c->width, th = c->visible_height ? c->visible_height : c->height;
    const int sw = crop ? c->crop_width : c->source_width, sh = crop ? c->crop_height : c->source_height;
    if (!(crop && sw == tw && sh == th))
      if (const char *why = av1mi::scale_geometry_error(sw, sh, tw, th))
        return WHY("%s %dx%d -> %dx%d: %s", crop ? "crop window" : "source size", sw, sh, tw, th, why);
  }
  if (c->key_block_size != 0 && c->key_block_size != 8 && c->key_block_size != 32) return WHY("key_block_size %d not supported (8 or 32)", c->key_block_size);
  if (c->key_block_size == 32 && (c->width & 31))
    return WHY("key_block_size 32 needs a width that is a multiple of 32");
  if (c->gpu_entropy && (c->width > 4096 || c->height > 4096)) return WHY("the AV1 tile coder takes frames up to 4096x4096");
  if ((size_t)c->height * c->segments > 65535u * 8u) return WHY("segments x height too large for one launch");
  if (c->coarse_range < 0 || c->coarse_range > 64 || (c->coarse_range & 3))
    return WHY("coarse_range %d must be 0 (off) or a multiple of 4 up to 64", c->coarse_range);
  if (c->quality_stats && ((c->visible_width ? c->visible_width : c->width) < 16 || (c->visible_height ? c->visible_height : c->height) < 16))
    return WHY("quality_stats needs a true luma size of at least 16x16");
  if (c->store_frames < 0 || c->store_frames > 65535) return WHY("store_frames %d out of range (0 = none, up to 65535)", c->store_frames);
  if (c->telecine != 0 && c->telecine != 1) return WHY("telecine %d unknown (0 none, 1 inverse telecine: fields woven, duplicates dropped by the caller's plan)", c->telecine);
  if (c->telecine && c->input_format != AV1MI_INPUT_PLANAR) return WHY("telecine %d needs input_format 0 (planar), not %d: the fields are woven from planar frames in the store", c->telecine, c->input_format);
  if (c->store_frames && c->input_format != AV1MI_INPUT_PLANAR) return WHY("a frame store (store_frames %d) needs input_format 0 (planar), not %d", c->store_frames, c->input_format);
  if (c->deinterlace < 0 || c->deinterlace > 2) return WHY("deinterlace %d unknown (0 none, 1 top field first, 2 bottom field first)", c->deinterlace);
  if (c->deinterlace && !c->store_frames) return WHY("deinterlace %d needs a frame store (store_frames > 0): the filter reads the frames before and after each frame", c->deinterlace);
  if (c->deinterlace_fields != 0 && c->deinterlace_fields != 1) return WHY("deinterlace_fields %d unknown (0 one frame per frame, 1 one frame per field)", c->deinterlace_fields);
  if (c->deinterlace_fields && !c->deinterlace) return WHY("deinterlace_fields %d needs deinterlace (1 top field first, 2 bottom field first): it is that filter's output rate", c->deinterlace_fields);
  if (c->denoise < 0 || c->denoise > 16) return WHY("denoise %d out of range (0 none, 1 .. 16 the strength)", c->denoise);
  if (c->denoise && !c->store_frames) return WHY("denoise %d needs a frame store (store_frames > 0): the filter reads the frames before and after each frame", c->denoise);
  if (c->denoise && c->deinterlace) return WHY("denoise %d together with deinterlace %d is not built: the chain of the two needs a third copy of a group", c->denoise, c->deinterlace);
  if (c->telecine && !c->store_frames) return WHY("telecine %d needs a frame store (store_frames > 0): a frame is woven from the fields of two stored frames", c->telecine);
  if (c->telecine && c->deinterlace) return WHY("telecine %d together with deinterlace %d is not built: a source is woven back to film or deinterlaced, not both", c->telecine, c->deinterlace);
  if (c->telecine && c->denoise) return WHY("telecine %d together with denoise %d is not built: the denoiser's neighbours would be video frames, not the woven film frames", c->telecine, c->denoise);
  if (c->denoise && c->source_bit_depth == 12) return WHY("denoise %d takes fed samples of 8 or 10 bits, not source_bit_depth 12", c->denoise);
  if (c->denoise_range != 0 && c->denoise_range != 4 && c->denoise_range != 8) return WHY("denoise_range %d unknown (0 none, 4 or 8 the block search's range)", c->denoise_range);
  if (c->denoise_range && !c->denoise) return WHY("denoise_range %d needs denoise (1 .. 16): it is the range of the denoiser's block search", c->denoise_range);
  if (c->grain_cov != 0 && c->grain_cov != 1) return WHY("grain_cov %d unknown (0 none, 1 the covariance of what the denoiser removed)", c->grain_cov);
  if (c->grain_cov && !c->denoise) return WHY("grain_cov %d needs denoise (1 .. 16): it measures what the denoiser removed", c->grain_cov);
  if (c->lr_search != 0 && c->lr_search != 1) return WHY("lr_search %d unknown (0 the policy's record in every unit, 1 a record chosen per unit)", c->lr_search);
  if (c->lr_search) {      // the filters' units tile the coded size, the syntax's the true size: the search needs the two grids to be one
    const int vw = c->visible_width ? c->visible_width : c->width, vh = c->visible_height ? c->visible_height : c->height;
    auto units = [](int n) { const int u = (n + 32) / 64; return u > 1 ? u : 1; };
    if (units(vw) != units(c->width) || units(vh) != units(c->height) || units((vw + 1) / 2) != units(c->width / 2) || units((vh + 1) / 2) != units(c->height / 2))
      return WHY("lr_search at a true size %dx%d whose restoration units differ from those of the coded size %dx%d is not built", vw, vh, c->width, c->height);
  }
  if (c->cdef_search < 0 || c->cdef_search > 3) return WHY("cdef_search %d unknown (0 the policy's strength set in every superblock, 1 .. 3 = cdef_bits: one of 2, 4, 8 sets chosen per superblock)", c->cdef_search);
  if (c->lf_search != 0 && c->lf_search != 1) return WHY("lf_search %d unknown (0 the policy's deblocking levels in every frame, 1 levels chosen per frame against the source)", c->lf_search);
  if (c->tone_map != 0 && c->tone_map != 1) return WHY("tone_map %d unknown (0 none, 1 BT.2390)", c->tone_map);
  if (c->tone_map_peak && !c->tone_map) return WHY("tone_map_peak %d needs tone_map", c->tone_map_peak);
  if (c->tone_map && c->bit_depth != 10) return WHY("tone_map needs bit_depth 10, not %d: an HDR10 source has 10 bits", c->bit_depth);
  if (c->tone_map && c->tone_map_peak && (c->tone_map_peak < 100 || c->tone_map_peak > 10000)) return WHY("tone_map_peak %d out of range (100 .. 10000 cd/m2; 0 = 1000)", c->tone_map_peak);
  if (c->tone_map && c->denoise) return WHY("tone_map together with denoise %d is not built: the grain records would be measured in the source's light, the grain synthesised in the output's", c->denoise);
  if (c->coded_bit_depth != 0 && c->coded_bit_depth != 8 && c->coded_bit_depth != c->bit_depth)
    return WHY("coded_bit_depth %d not supported with bit_depth %d (0 = bit_depth; 8: a 10-bit session coded at 8 bits)", c->coded_bit_depth, c->bit_depth);
  if (c->coded_bit_depth == 8 && c->bit_depth == 8) return WHY("coded_bit_depth 8 with bit_depth 8: there is nothing to reduce, leave it 0");
  if (c->depth_dither < 0 || c->depth_dither > 1) return WHY("depth_dither %d unknown (0 round, 1 ordered)", c->depth_dither);
  if (c->depth_dither && c->coded_bit_depth != 8) return WHY("depth_dither %d needs coded_bit_depth 8: it is the dither of the depth reduction", c->depth_dither);
  if (c->coded_bit_depth && c->coded_bit_depth != c->bit_depth && c->denoise)
    return WHY("coded_bit_depth %d together with denoise %d is not built: the grain records are measured in %d-bit codes and the grain would be synthesised into an 8-bit stream",
               c->coded_bit_depth, c->denoise, c->bit_depth);
  return nullptr;
#undef WHY
}

int setup(av1mi_gop *g) {
  const av1mi_gop_config &c = g->cfg;
  const int w = c.width, h = c.height, S = c.segments;
  g->bd = coded_depth(c);
  g->bps = g->bd == 8 ? 1 : 2;
  g->vw = c.visible_width ? c.visible_width : w; g->vh = c.visible_height ? c.visible_height : h;
  for (int p = 0; p < 3; p++) {
    Plane &P = g->plane[p];
    P.ss = p > 0;
    P.w = w >> P.ss; P.h = h >> P.ss; P.vw = (g->vw + P.ss) >> P.ss; P.vh = (g->vh + P.ss) >> P.ss;
    P.n = (size_t)P.w * P.h * S; P.bytes = P.n * g->bps;
  }
  g->nb = g->plane[0].n / 64;
  for (int p = 0; p < 3; p++) { const av1mi::LrGeom lg(g->plane[p].w, g->plane[p].h, p ? 1 : 0, 64, 1); g->lr_units[p] = lg.unit_rows * lg.unit_cols; }
  g->next_q = c.base_q_idx;
  G_TRY(av1mi_gop_source_layout(&c, &g->layout));
  // the chain (config_error: never convert AND chroma)
  if (c.input_format != AV1MI_INPUT_PLANAR) { g->chain[g->stages++] = kConvert; g->fed_align = 16; }
  if (c.source_chroma != AV1MI_CHROMA_420 || g->layout.bit_depth != c.bit_depth) { g->chain[g->stages++] = kChroma; g->fed_align = 16; }
  g->cropping = c.crop_width != 0;
  if (g->cropping) g->window = { c.crop_x, c.crop_y, c.crop_width, c.crop_height, c.source_width, c.source_height };
  const bool copy = g->cropping && c.crop_width == g->vw && c.crop_height == g->vh;      // a window of the target's size: nothing to resample
  if (c.source_width) g->chain[g->stages++] = copy ? kCrop : kScale;
  if (c.gpu_entropy) {
    g->tiles = av1mi::sb_count(w, h);
    // the size of the batch's frames as packed 4:2:0 samples: a frame codes to several times less at any sane quantiser, and to about
    // that at the finest one (one byte per luma sample, the capacity before, gave an 8-bit key frame at base_q_idx 1 back to the host)
    g->ent_cap = (size_t)w * h * S * 3 * g->bd / 16;
  }
  G_HIP(hipSetDevice(av1mi::ctx_device(g->ctx)));
  if (c.source_width && !copy)
    G_HIP(g->cropping ? av1mi::scale_plan_create(c.bit_depth, c.crop_width, c.crop_height, g->vw, g->vh, &g->scale, &g->window)
                      : av1mi::scale_plan_create(c.bit_depth, c.source_width, c.source_height, g->vw, g->vh, &g->scale));
  G_HIP(hipStreamCreateWithFlags(&g->up, hipStreamNonBlocking));
  // (created in every mode, used only where symbols go to the host at submit time or a batch falls back.  HIP deals its four
  // default hardware queues to streams in creation order: main, up, down, side — and the coder's back stream, the fifth, shares
  // the main stream's queue, i.e. the range coder of batch t and the block pipeline of batch t + 1 run one after the other.
  // Measured A/B on one box: that is the FASTEST arrangement, 1 800 frames/s end to end at 4K against 1 500-1 600 with a queue
  // per stream (without this stream, or with GPU_MAX_HW_QUEUES=8) and 1 500 with the coder on the main stream itself: the
  // range coder is one long wave per CU, and beside it every kernel of the block pipeline runs at a fraction of its speed.)
  G_HIP(hipStreamCreateWithFlags(&g->down, hipStreamNonBlocking));
  for (Slot &s : g->slot) G_TRY(slot_buffers(g, s));
  for (int p = 0; p < 3; p++)      // reconstruction, deblocked, CDEF and reference planes: single (the chain is serial in t)
    for (void **d : { &g->d_rec[p], &g->d_dbl[p], &g->d_cdef[p], &g->d_ref[p] }) G_TRY(dev_alloc(g, d, g->plane[p].bytes));
  G_TRY(dev_alloc(g, &g->d_lr_scratch, av1mi_lr_yuv_decide_scratch_bytes(h, S)));
  // the decision's sums, zeroed ONCE: every batch's decision leaves them zero behind it (capi.hip lr_yuv_decide_with: the rule)
  G_HIP(hipMemset(g->d_lr_scratch, 0, av1mi_lr_yuv_decide_scratch_bytes(h, S)));
  if (c.coarse_range) G_TRY(dev_alloc(g, &g->d_me, av1mi::me_layout(w, h, S).bytes));
  if (c.quality_stats) G_TRY(dev_alloc(g, &g->d_quality_scratch, av1mi::quality_scratch_bytes(g->bd, g->vw, g->vh, S)));
  if (c.denoise) {
    av1mi::DenoiseMcLaunch L{};
    fed_geometry(g, nullptr, L);
    L.strength = c.denoise; L.range = c.denoise_range;
    const size_t bytes = c.denoise_range ? av1mi::denoise_mc_scratch_bytes(L) : av1mi::grain_scratch_bytes(L);
    if (!bytes) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "denoise %d: the fed layout %dx%d (true %dx%d) is not one the denoising gather takes", c.denoise, g->layout.width,
                                      g->layout.height, g->layout.true_width, g->layout.true_height);
    G_TRY(dev_alloc(g, &g->d_grain_scratch, bytes));
    if (c.denoise_range) G_TRY(dev_alloc(g, &g->d_denoise_vectors, av1mi::denoise_mc_vector_bytes(L)));
    if (c.grain_cov) G_TRY(dev_alloc(g, &g->d_grain_cov_scratch, av1mi::grain_cov_scratch_bytes(L)));      // (the gather's geometry: not 0 here)
  }
  if (c.store_frames) {
    for (Store &st : g->store) {
      for (int p = 0; p < 3; p++)
        if (g->layout.plane[p].frame_bytes) G_TRY(dev_alloc(g, &st.d[p], g->layout.plane[p].frame_bytes * (size_t)store_capacity(c)));
      G_HIP(hipEventCreateWithFlags(&st.filled, hipEventDisableTiming));
      G_HIP(hipEventCreateWithFlags(&st.read_done, hipEventDisableTiming));
    }
    G_TRY(dev_alloc(g, &g->d_scene, av1mi::scene_layout(g->layout.width, g->layout.height, c.store_frames).bytes));
    G_TRY(host_alloc(g, &g->h_records, (size_t)c.store_frames * sizeof(av1mi_scene_record)));
    G_HIP(hipEventCreateWithFlags(&g->scene_done, hipEventDisableTiming));
    for (hipEvent_t &e : g->put_done) G_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (c.telecine) {
      G_TRY(dev_alloc(g, &g->d_telecine, av1mi::telecine_layout(g->layout.bit_depth, g->layout.true_width, g->layout.true_height, store_capacity(c)).bytes));
      G_TRY(host_alloc(g, &g->h_telecine, (size_t)store_capacity(c) * sizeof(av1mi_telecine_record)));
      G_HIP(hipEventCreateWithFlags(&g->telecine_done, hipEventDisableTiming));
    }
  }
  if (c.tone_map) {
    av1mi_tone_tables tables;
    if (av1mi_tone_map_tables(c.tone_map_peak ? c.tone_map_peak : 1000, &tables) != AV1MI_OK) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "tone_map_peak %d: no tables", c.tone_map_peak);
    G_TRY(dev_alloc(g, &g->d_tone_tables, sizeof(tables)));
    G_TRY(av1mi_upload(g->ctx, g->d_tone_tables, &tables, sizeof(tables)));
  }
  G_TRY(dev_alloc(g, &g->d_zero_skip, g->nb));
  G_TRY(av1mi_memset(g->ctx, g->d_zero_skip, 0, g->nb));
  G_TRY(side_information(g));
  return av1mi_sync(g->ctx);
}

}  // namespace

extern "C" {

int av1mi_policy_frame_params(int base_q_idx, int bit_depth, int frame_type, av1mi_frame_params *out) {
  if (!out || base_q_idx < 0 || base_q_idx > 255 || (bit_depth != 8 && bit_depth != 10) || frame_type < 0 || frame_type > 1) return AV1MI_E_INVAL;
  frame_params(base_q_idx, bit_depth, frame_type, out);
  return AV1MI_OK;
}

int av1mi_gop_source_layout(const av1mi_gop_config *c, av1mi_source_layout *out) {
  char why[512];
  if (!out || config_error(c, why)) return AV1MI_E_INVAL;
  av1mi_source_layout L = {};
  const bool scaling = c->source_width != 0;      // the ONE place that says: scaling ? the source's size : the coded / visible size
  L.width = scaling ? (c->source_width + 7) & ~7 : c->width; L.height = scaling ? (c->source_height + 7) & ~7 : c->height;
  L.true_width = scaling ? c->source_width : c->visible_width ? c->visible_width : c->width;
  L.true_height = scaling ? c->source_height : c->visible_height ? c->visible_height : c->height;
  L.bit_depth = c->source_bit_depth ? c->source_bit_depth : c->bit_depth;
  // a wire format (4:2:0 at bit_depth: config_error) or a planar source in its chroma layout; 4:2:0 planar is both
  const int fmt = c->input_format, sx = c->source_chroma != AV1MI_CHROMA_444, sy = c->source_chroma == AV1MI_CHROMA_420;
  const int pairs = fmt == AV1MI_INPUT_P010 || fmt == AV1MI_INPUT_NV12;      // the second plane interleaves U and V
  for (int p = 0; p < 3; p++) {
    L.plane[p].frame_bytes = fmt != AV1MI_INPUT_PLANAR ? av1mi_input_plane_bytes(fmt, L.bit_depth, p, L.width, L.height)
                                                        : av1mi_source_plane_bytes(c->source_chroma, L.bit_depth, p, L.width, L.height);
    if (!L.plane[p].frame_bytes) continue;
    L.plane[p].width = p ? (L.width >> sx) << pairs : L.width; L.plane[p].height = p ? L.height >> sy : L.height;
  }
  *out = L;
  return AV1MI_OK;
}

int av1mi_gop_open(av1mi_ctx *ctx, const av1mi_gop_config *cfg, av1mi_gop **out) {
  if (!ctx || !out) return AV1MI_E_INVAL;
  *out = nullptr;
  char why[512];
  if (config_error(cfg, why)) return av1mi::ctx_fail(ctx, AV1MI_E_INVAL, "%s", why);
  av1mi_gop *g = new (std::nothrow) av1mi_gop();
  if (!g) return AV1MI_E_NOMEM;
  g->ctx = ctx; g->cfg = *cfg;
  g->coder_streams = cfg->coder_streams;
  if (const char *e = getenv("AV1MI_INTRA_OPEN_LOOP")) g->intra_open_loop = atoi(e) ? 1 : 0;
  if (const char *e = getenv("AV1MI_CODER_STREAMS")) g->coder_streams = !strcmp(e, "side") ? 1 : !strcmp(e, "main") ? 2 : !strcmp(e, "defer") ? 3 : 0;
  const int rc = setup(g);
  if (rc != AV1MI_OK) { av1mi_gop_close(g); return rc; }
  *out = g;
  return AV1MI_OK;
}

void av1mi_gop_close(av1mi_gop *g) {
  if (!g) return;
  (void)hipSetDevice(av1mi::ctx_device(g->ctx));
  (void)av1mi_sync(g->ctx);
  if (g->up) { (void)hipStreamSynchronize(g->up); (void)hipStreamDestroy(g->up); }
  if (g->down) { (void)hipStreamSynchronize(g->down); (void)hipStreamDestroy(g->down); }
  for (Slot &s : g->slot)
    for (hipEvent_t e : { s.uploaded, s.kernel_done, s.filters_done, s.downloaded, s.ent_done, s.quality_done, s.grain_done, s.search_down })
      if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : { g->store[0].filled, g->store[0].read_done, g->store[1].filled, g->store[1].read_done, g->scene_done, g->telecine_done, g->put_done[0], g->put_done[1], g->put_done[2] })
    if (e) (void)hipEventDestroy(e);
  for (void *p : g->dev_allocs) (void)hipFree(p);
  for (void *p : g->host_allocs) (void)hipHostFree(p);
  av1mi::scale_plan_destroy(g->scale);
  delete g;
}

int av1mi_gop_max_in_flight(void) { return kSlots; }

}  // extern "C"

// ---- a batch: the stages of submit_batch, each named for what it enqueues ---------------------------------------------------------

// The source as fed -> src: the three planar planes at the coded size that the rest of the batch reads.  dev_src: the fed planes in
// device memory (av1mi_gop_submit_device), or null = upload the slot's pinned buffers first.  Two hazards:
//  - d_src (and d_pre, the planes between conversion and scaling) is read by the slot's previous batch up to its restoration
//    decision.  That ran on the main stream too, so the launches here are ordered behind it by the stream itself; no event.
//  - d_in, the device buffer of the source as fed (with zero stages: d_src itself), is read by the input stages / the kernels of the
//    slot's previous batch.  The upload into it waits for that batch's filters_done, which was recorded on the main stream AFTER those
//    launches (the restoration decision is the last reader), and with quality_stats for its quality_done (measure_quality reads the
//    source after the filters).
// `uploaded` keeps its two meanings: the main stream waits for it before the first launch, and av1mi_gop_acquire_input waits for
// it before the host may overwrite the pinned buffers.
// A batch from the frame store (index != null: the store position per segment, -1 = a flat slot) is gathered into d_in on the main
// stream instead of being uploaded: the stream itself orders the gather behind the slot's previous readers, store.filled orders it
// behind the puts, and store.read_done lets the next put into that store wait for it.
// A woven batch (bottom != null, av1mi_gop_submit_woven): index[] holds the top source's position, bottom[] the bottom source's; the table
// holds the two pointers and k_telecine_gather stands where k_frames_gather stands.  Same events.
static int feed_source(av1mi_gop *g, Slot &s, const void *const *dev_src, const void *src[3], int store = 0, const int32_t *index = nullptr,
                       const int32_t *bottom = nullptr) {
  hipStream_t main = av1mi::ctx_stream(g->ctx);
  const av1mi_gop_config &c = g->cfg;
  const av1mi_source_layout &Y = g->layout;
  const int S = c.segments, dei = c.deinterlace, three = dei || c.denoise;      // three: the table holds P, C, N
  const int fields = c.deinterlace_fields;      // index[] holds OUTPUT positions: source frame o >> 1, phase o & 1
  for (int p = 0; p < 3; p++) src[p] = dev_src ? dev_src[p] : s.d_in[p];
  s.has_grain = index && c.denoise;
  if (index) {
    Store &st = g->store[store];
    const void **table = (const void **)s.h_table;
    const size_t frame_bytes[3] = { Y.plane[0].frame_bytes, Y.plane[1].frame_bytes, Y.plane[2].frame_bytes };
    auto frame = [&](int p, int pos) { return (const void *)((const char *)st.d[p] + frame_bytes[p] * (size_t)pos); };
    const size_t table_bytes = (size_t)S * 3 * (three ? 3 : bottom ? 2 : 1) * sizeof(void *);
    uint8_t *phase = (uint8_t *)s.h_table + table_bytes;      // (field rate only: the slot's table was allocated with S bytes more)
    for (int sg = 0; sg < S; sg++) {
      const int pos = fields && index[sg] >= 0 ? index[sg] >> 1 : index[sg];
      if (fields) phase[sg] = index[sg] >= 0 ? (uint8_t)(index[sg] & 1) : 0;
      for (int p = 0; p < 3; p++) {
        const bool flat = pos < 0 || !frame_bytes[p];
        if (bottom) {
          table[(sg * 3 + p) * 2] = flat ? nullptr : frame(p, pos);
          table[(sg * 3 + p) * 2 + 1] = flat ? nullptr : frame(p, bottom[sg]);
        } else if (!three) table[sg * 3 + p] = flat ? nullptr : frame(p, pos);
        else {      // P, C, N follow the POSITION in the store's run, clamped at its ends
          const void **e = table + (sg * 3 + p) * 3;
          e[0] = flat ? nullptr : frame(p, pos > 0 ? pos - 1 : 0);
          e[1] = flat ? nullptr : frame(p, pos);
          e[2] = flat ? nullptr : frame(p, pos + 1 < st.run ? pos + 1 : st.run - 1);
        }
      }
    }
    G_HIP(hipMemcpyAsync(s.d_table, s.h_table, table_bytes + (fields ? (size_t)S : 0), hipMemcpyHostToDevice, main));
    G_HIP(hipStreamWaitEvent(main, st.filled, 0));
    {
      av1mi::ProfScope ps(g->ctx, AV1MI_K_SCENE, main);
      if (fields) {
        av1mi::DeintFieldsLaunch L;
        fed_geometry(g, &s, L);
        L.parity = dei - 1; L.phase = (const uint8_t *)s.d_table + table_bytes;
        G_HIP(av1mi::launch_deint_gather_fields(L, main));
      } else if (dei) {
        av1mi::DeintLaunch L;
        fed_geometry(g, &s, L);
        L.parity = dei - 1;
        G_HIP(av1mi::launch_deint_gather(L, main));
      } else if (c.denoise_range) {      // the block search, the filter on displaced neighbours, the records as below
        av1mi::DenoiseMcLaunch L;
        fed_geometry(g, &s, L);
        L.strength = c.denoise; L.range = c.denoise_range; L.scratch = g->d_grain_scratch; L.records = (av1mi_grain_record *)s.h_grain;
        L.vectors = (av1mi_denoise_vec *)g->d_denoise_vectors;
        G_HIP(av1mi::launch_denoise_mc_gather(L, main));
      } else if (c.denoise) {      // ... and the records of what it removed, straight into the slot's pinned memory
        av1mi::DenoiseLaunch L;
        fed_geometry(g, &s, L);
        L.strength = c.denoise; L.scratch = g->d_grain_scratch; L.records = (av1mi_grain_record *)s.h_grain;
        G_HIP(av1mi::launch_denoise_gather(L, main));
      } else if (bottom) {
        av1mi::GatherPlanes L;
        fed_geometry(g, &s, L);
        G_HIP(av1mi::launch_telecine_gather(L, main));
      } else G_HIP(av1mi::launch_frames_gather(frame_bytes, S, (const void *const *)s.d_table, s.d_in, main));
      if (c.grain_cov) {           // one more launch behind either denoising gather: C from the table, out from the fed buffers
        av1mi::GrainCovLaunch L;
        fed_geometry(g, &s, L);
        L.scratch = g->d_grain_cov_scratch; L.cov = (av1mi_grain_cov_record *)s.h_grain_cov;
        G_HIP(av1mi::launch_grain_cov(L, main));
      }
    }
    if (c.denoise) G_HIP(hipEventRecord(s.grain_done, main));
    G_HIP(hipEventRecord(st.read_done, main));
    st.has_reader = true;
  } else if (!dev_src) {
    if (s.kernel_pending) G_HIP(hipStreamWaitEvent(g->up, s.filters_done, 0));
    if (s.kernel_pending && c.quality_stats) G_HIP(hipStreamWaitEvent(g->up, s.quality_done, 0));
    for (int p = 0; p < 3; p++)
      if (fed_bytes(g, p)) G_HIP(hipMemcpyAsync(s.d_in[p], s.h_in[p], fed_bytes(g, p), hipMemcpyHostToDevice, g->up));
    G_HIP(hipEventRecord(s.uploaded, g->up));
    s.upload_pending = true;
    G_HIP(hipStreamWaitEvent(main, s.uploaded, 0));
  }
  // the chain: a stage reads the planes where they are now and moves those it writes to its outputs (resolved by slot_buffers)
  for (int k = 0; k < g->stages; k++) {
    void *const *out = s.stage_out[k];
    av1mi::ProfScope ps(g->ctx, AV1MI_K_INPUT, main);
    if (g->chain[k] == kConvert) {
      av1mi::InputLaunch L{};
      for (int p = 0; p < 3; p++) { L.in[p] = src[p]; L.out[p] = out[p]; }
      L.ny = (size_t)Y.width * Y.height * S; L.nc = L.ny / 4;
      G_HIP(av1mi::launch_input_convert(c.input_format, L, main));
    } else if (g->chain[k] == kChroma) {      // at the fed frames' TRUE size
      av1mi::ChromaLaunch L;
      for (int p = 0; p < 3; p++) { L.in[p] = src[p]; L.out[p] = out[p]; }
      L.chroma = c.source_chroma; L.src_bd = Y.bit_depth; L.bd = c.bit_depth; L.frames = S; L.w = Y.true_width; L.h = Y.true_height;
      G_HIP(av1mi::launch_chroma_convert(L, main));
    } else if (g->chain[k] == kCrop) {
      G_HIP(av1mi::launch_crop_copy(g->window, c.bit_depth, c.width, c.height, S, src, out, main));
    } else G_HIP(av1mi::launch_scale(g->scale, S, src, out, main));
    for (int p = 0; p < 3; p++) if (out[p]) src[p] = out[p];      // (a plane that passes through stays where it was fed: the caller's, in a device batch)
  }
  if (c.tone_map) {      // behind the last stage, in place: the planes are the slot's own (av1mi_gop_submit_device is refused)
    av1mi::ProfScope ps(g->ctx, AV1MI_K_INPUT, main);
    void *const planes[3] = { const_cast<void *>(src[0]), const_cast<void *>(src[1]), const_cast<void *>(src[2]) };
    G_HIP(av1mi::launch_tone_map(c.width, c.height, S, planes, g->d_tone_tables, main));
  }
  if (reducing(g)) {      // the last word of the input side: the planes at bit_depth, wherever they are now (read only) -> the slot's coded planes
    av1mi::ProfScope ps(g->ctx, AV1MI_K_INPUT, main);
    G_HIP(av1mi::launch_depth_reduce(c.depth_dither, c.width, c.height, S, src, s.d_src, main));
    for (int p = 0; p < 3; p++) src[p] = s.d_src[p];
  }
  return AV1MI_OK;
}

// the block pipeline: key (8x8 blocks | two bands, 32x32 + 8x8) or inter; then kernel_done.  (The symbols of this slot were downloaded
// before the slot was collected, so they may be overwritten.)
static int code_blocks(av1mi_gop *g, Slot &s, int frame_type, const void *const src[3]) {
  const av1mi_gop_config &c = g->cfg;
  const int w = c.width, h = c.height;
  if (frame_type == 0) {
    av1mi_intra_job j;
    memset(&j, 0, sizeof(j));
    j.width = w; j.height = h; j.bit_depth = g->bd; j.nframes = c.segments; j.qindex = s.q; j.block_size = 8; j.stride_y = g->plane[0].w; j.stride_uv = g->plane[1].w;
    j.d_src_y = src[0]; j.d_src_u = src[1]; j.d_src_v = src[2];
    j.d_rec_y = g->d_rec[0]; j.d_rec_u = g->d_rec[1]; j.d_rec_v = g->d_rec[2];
    j.d_lev_y = (int16_t *)s.d_lev[0]; j.d_lev_u = (int16_t *)s.d_lev[1]; j.d_lev_v = (int16_t *)s.d_lev[2];
    j.d_modes_y = (uint8_t *)s.d_modes[0]; j.d_modes_uv = (uint8_t *)s.d_modes[1];
    j.open_loop = g->intra_open_loop;
    if (!g->key32) {
      G_TRY(av1mi_intra_encode(g->ctx, &j));
    } else {
      // two bands of every frame: the complete superblock rows in 32x32 blocks, a last partial row (if any) in 8x8 blocks.  Tiles are
      // single superblocks, so the bands share nothing.
      const int hA = g->key_rows32, hB = h - hA;
      j.open_loop = 0; j.frame_rows = h; j.modes_frame_stride = g->key_modes_stride;
      if (hA) { j.height = hA; j.block_size = 32; G_TRY(av1mi_intra_encode(g->ctx, &j)); }
      if (hB) {
        size_t o[3];      // samples of a plane above the second band
        for (int p = 0; p < 3; p++) o[p] = (size_t)(hA >> g->plane[p].ss) * g->plane[p].w;
        j.height = hB; j.block_size = 8;
        j.d_src_y = (const char *)src[0] + o[0] * g->bps; j.d_src_u = (const char *)src[1] + o[1] * g->bps; j.d_src_v = (const char *)src[2] + o[2] * g->bps;
        j.d_rec_y = (char *)g->d_rec[0] + o[0] * g->bps; j.d_rec_u = (char *)g->d_rec[1] + o[1] * g->bps; j.d_rec_v = (char *)g->d_rec[2] + o[2] * g->bps;
        j.d_lev_y = (int16_t *)s.d_lev[0] + o[0]; j.d_lev_u = (int16_t *)s.d_lev[1] + o[1]; j.d_lev_v = (int16_t *)s.d_lev[2] + o[2];
        j.d_modes_y = (uint8_t *)s.d_modes[0] + g->key_modes_band; j.d_modes_uv = (uint8_t *)s.d_modes[1] + g->key_modes_band;
        G_TRY(av1mi_intra_encode(g->ctx, &j));
      }
    }
  } else {
    av1mi_inter_job j;
    memset(&j, 0, sizeof(j));
    j.width = w; j.height = h; j.bit_depth = g->bd; j.nframes = c.segments; j.qindex = s.q; j.search_range = c.search_range; j.stride_y = g->plane[0].w; j.stride_uv = g->plane[1].w;
    j.d_src_y = src[0]; j.d_src_u = src[1]; j.d_src_v = src[2];
    j.d_ref_y = g->d_ref[0]; j.d_ref_u = g->d_ref[1]; j.d_ref_v = g->d_ref[2];
    j.d_rec_y = g->d_rec[0]; j.d_rec_u = g->d_rec[1]; j.d_rec_v = g->d_rec[2];
    j.d_lev_y = (int16_t *)s.d_lev[0]; j.d_lev_u = (int16_t *)s.d_lev[1]; j.d_lev_v = (int16_t *)s.d_lev[2];
    j.d_mvs = (int16_t *)s.d_mv; j.d_skip = (uint8_t *)s.d_skip;
    // per segment and plane: the restored plane of the previous frame, or its CDEF output where restoration was switched off
    j.d_ref_alt_y = g->d_cdef[0]; j.d_ref_alt_u = g->d_cdef[1]; j.d_ref_alt_v = g->d_cdef[2];
    j.d_ref_sel = (const uint8_t *)g->slot[g->last].d_lr_on;
    // coarse_range: k_me_down + k_me_coarse at the head of the batch, in the session's own scratch area (the previous batch's k_me_int,
    // its last reader, ran on this stream)
    j.coarse_range = c.coarse_range;
    G_TRY(av1mi::inter_encode_with(g->ctx, &j, g->d_me));
  }
  G_HIP(hipEventRecord(s.kernel_done, av1mi::ctx_stream(g->ctx)));
  s.kernel_pending = true;
  s.frame_type = frame_type;
  return AV1MI_OK;
}

// the symbols of a slot -> its pinned host mirrors, on the download stream: the levels, then the modes (key frames) or the vectors +
// skip flags (inter frames)
static int download_symbols(av1mi_gop *g, Slot &s) {
  for (int p = 0; p < 3; p++) G_HIP(hipMemcpyAsync(s.h_lev[p], s.d_lev[p], g->plane[p].n * 2, hipMemcpyDeviceToHost, g->down));
  if (s.frame_type == 0) {
    for (int k = 0; k < 2; k++) G_HIP(hipMemcpyAsync(s.h_modes[k], s.d_modes[k], g->nb, hipMemcpyDeviceToHost, g->down));
  } else {
    G_HIP(hipMemcpyAsync(s.h_mv, s.d_mv, g->nb * 4, hipMemcpyDeviceToHost, g->down));
    G_HIP(hipMemcpyAsync(s.h_skip, s.d_skip, g->nb, hipMemcpyDeviceToHost, g->down));
  }
  return AV1MI_OK;
}

static int extend_plane(av1mi_gop *g, const Plane &P, void *d) {
  return av1mi_extend_frames(g->ctx, d, P.w, P.w, P.h, P.vw, P.vh, g->bd, g->cfg.segments);
}

// The device state derived from the quantiser follows the batch: the deblocking map pair this batch's filters read (key / inter / key in
// 32x32 blocks) and the CDEF strength records of its frame type.  They exist once (the batches are serial on the main stream), so
// where they hold the levels of another quantiser than the batch's, ONE launch of k_mi_levels (levels_kernels.hip) on the main stream
// patches the level fields in place: behind the previous batch's filters, their last readers, and in front of this batch's.  The
// geometry the host wrote at open stays.  No host copy, no synchronisation; and no launch while the quantiser stays what the arrays hold,
// so a session on which av1mi_gop_set_base_q_idx is never called launches what it always did.
static int follow_q(av1mi_gop *g, const Slot &s) {
  const int t = s.frame_type, m = t == 0 && g->key32 ? 2 : t;
  const av1mi_frame_params &P = s.params;
  av1mi::LevelsLaunch L;
  memset(&L, 0, sizeof(L));
  if (g->mi_q[m] != s.q) {
    const size_t fy = (size_t)g->cfg.width * g->cfg.height;
    const uint32_t keep = ~0x00FFFF00u, hold = 1u << 24;      // the two level bytes; off-screen words ("skipped inter block") keep level 0
    L.a[L.arrays++] = { (uint32_t *)g->d_mi[m][0], fy / 16, keep, (uint32_t)P.lf_level[0] << 8 | (uint32_t)P.lf_level[1] << 16, hold };
    L.a[L.arrays++] = { (uint32_t *)g->d_mi[m][1], fy / 64, keep, (uint32_t)P.lf_level[2] << 8 | (uint32_t)P.lf_level[2] << 16, hold };
    g->mi_q[m] = s.q;
  }
  if (g->cdef_q[t] != s.q) {      // one dword per superblock: primary / secondary strength of luma, then of chroma
    const size_t nsb = (size_t)av1mi::sb_count(g->cfg.width, g->cfg.height);
    L.a[L.arrays++] = { (uint32_t *)g->d_cdef_sb[t], nsb, 0u,
                        (uint32_t)(P.cdef_y >> 2) | (uint32_t)(P.cdef_y & 3) << 8 | (uint32_t)(P.cdef_uv >> 2) << 16 | (uint32_t)(P.cdef_uv & 3) << 24, 0u };
    g->cdef_q[t] = s.q;
  }
  if (!L.arrays) return AV1MI_OK;
  hipStream_t main = av1mi::ctx_stream(g->ctx);
  av1mi::ProfScope ps(g->ctx, AV1MI_K_MISC, main);
  G_HIP(av1mi::launch_mi_levels(L, main));
  return AV1MI_OK;
}

// The stages of loop_filters.  A job's _y / _u / _v fields from a triple of planes
template <typename T, typename P> static void yuv(T &y, T &u, T &v, const P &planes) { y = planes[0]; u = planes[1]; v = planes[2]; }
// a true size that is not a multiple of 8: the decoder's restoration clamps at the true last column / row, so the planes it reads are
// extended from the true size (CDEF reads the planes as they are: it works on the coded size in a decoder too)
static bool padded(const av1mi_gop *g) { return g->vw != g->cfg.width || g->vh != g->cfg.height; }
// the deblocking maps a batch's launches read [luma / chroma], and the units between the frames' maps (0 = the one shared map)
struct LfMaps { void *const *mi; size_t frame_stride[2]; };

// The batch's deblocking maps: the frame type's shared pair at the policy's levels, or (lf_search) the levels of every frame chosen
// against the source and a map per frame with them
static int deblock_search(av1mi_gop *g, Slot &s, const void *const src[3], LfMaps &M) {
  const av1mi_gop_config &c = g->cfg;
  const int w = c.width, h = c.height;
  M = { g->d_mi[s.frame_type == 0 && g->key32 ? 2 : s.frame_type], { 0, 0 } };
  if (!c.lf_search) return AV1MI_OK;
  av1mi_lf_search_job sj;
  memset(&sj, 0, sizeof(sj));
  sj.width = w; sj.height = h; sj.bit_depth = g->bd; sj.nframes = c.segments; sj.stride_y = g->plane[0].w; sj.stride_uv = g->plane[1].w;
  yuv(sj.d_rec_y, sj.d_rec_u, sj.d_rec_v, g->d_rec); yuv(sj.d_orig_y, sj.d_orig_u, sj.d_orig_v, src);
  sj.true_width = g->vw; sj.true_height = g->vh; sj.params = &s.params; sj.d_mi_y_out = (uint32_t *)g->d_mi_frames[0]; sj.d_mi_uv_out = (uint32_t *)g->d_mi_frames[1];
  sj.d_mi_y = (const uint32_t *)M.mi[0]; sj.d_mi_uv = (const uint32_t *)M.mi[1]; sj.mi_stride_y = g->plane[0].w / 4; sj.mi_stride_uv = g->plane[1].w / 4;
  sj.d_scratch = g->d_lf_table; sj.d_sse = (uint64_t *)g->d_lf_sse; sj.d_choice = (uint8_t *)s.d_lf_choice; sj.d_levels = (uint8_t *)s.d_lf_levels;
  G_TRY(av1mi_lf_search(g->ctx, &sj));
  M = { g->d_mi_frames, { (size_t)(w / 4) * (h / 4), (size_t)(w / 8) * (h / 8) } };
  return AV1MI_OK;
}

// reconstruction -> deblocked planes (d_dbl) -> CDEF output (d_cdef), with the maps of deblock_search
static int deblock_cdef(av1mi_gop *g, Slot &s, const void *const src[3], const LfMaps &M) {
  const av1mi_gop_config &c = g->cfg;
  const int w = c.width, h = c.height, S = c.segments, bd = g->bd, key = s.frame_type == 0;
  const av1mi_frame_params &P = s.params;
  // key frames are coded with skip = 0 everywhere (no block is exempt from CDEF); P frames: the kernel's skip flags, per frame
  // (the slot's next inter kernel is kSlots batches away and ordered behind this CDEF on the main stream, nothing else writes them)
  const uint8_t *skip8 = (const uint8_t *)(key ? g->d_zero_skip : s.d_skip);
  const size_t skip_frame_stride = key ? 0 : (size_t)(w / 8) * (h / 8);
  // cdef_search: the search reads WHOLE deblocked planes, so every size takes the kernels one by one
  if (!padded(g) && !c.cdef_search) {
    // deblocking and CDEF in one kernel: the deblocked samples stay in LDS, and d_dbl receives only the rows restoration reads
    av1mi_deblock_cdef_job fj;
    memset(&fj, 0, sizeof(fj));
    fj.width = w; fj.height = h; fj.bit_depth = bd; fj.nframes = S; fj.damping = P.cdef_damping; fj.sharpness = P.lf_sharpness;
    fj.rec_stride_y = fj.dbl_stride_y = fj.dst_stride_y = g->plane[0].w; fj.rec_stride_uv = fj.dbl_stride_uv = fj.dst_stride_uv = g->plane[1].w;
    yuv(fj.d_rec_y, fj.d_rec_u, fj.d_rec_v, g->d_rec); yuv(fj.d_dbl_y, fj.d_dbl_u, fj.d_dbl_v, g->d_dbl); yuv(fj.d_dst_y, fj.d_dst_u, fj.d_dst_v, g->d_cdef);
    fj.d_mi_y = (const uint32_t *)M.mi[0]; fj.d_mi_uv = (const uint32_t *)M.mi[1]; fj.mi_stride_y = g->plane[0].w / 4; fj.mi_stride_uv = g->plane[1].w / 4;
    fj.mi_frame_stride_y = M.frame_stride[0]; fj.mi_frame_stride_uv = M.frame_stride[1];
    fj.d_sb_strength = (const uint8_t *)g->d_cdef_sb[s.frame_type]; fj.sb_frame_stride = 0; fj.d_skip8 = skip8; fj.skip_frame_stride = skip_frame_stride;
    G_TRY(av1mi_deblock_cdef_frames(g->ctx, &fj));
  } else {
    // the two kernels on their own: extend_plane below replicates row vh - 1 and column vw - 1 of the WHOLE deblocked planes
    // (restoration's boundary rows are clamped at the true size), and the fused kernel writes only four rows in 64 of them
    for (int p = 0; p < 3; p++) {
      const Plane &L = g->plane[p];
      G_TRY(av1mi_deblock_frames(g->ctx, g->d_rec[p], L.w, g->d_dbl[p], L.w, L.w, L.h, bd, L.ss, (const uint32_t *)M.mi[L.ss], L.w / 4, M.frame_stride[L.ss], P.lf_sharpness, S));
    }
    av1mi_cdef_job cj;
    memset(&cj, 0, sizeof(cj));
    cj.width = w; cj.height = h; cj.bit_depth = bd; cj.nframes = S; cj.damping = P.cdef_damping; cj.stride_y = g->plane[0].w; cj.stride_uv = g->plane[1].w;
    yuv(cj.d_src_y, cj.d_src_u, cj.d_src_v, g->d_dbl); yuv(cj.d_dst_y, cj.d_dst_u, cj.d_dst_v, g->d_cdef);
    cj.d_sb_strength = (const uint8_t *)g->d_cdef_sb[s.frame_type]; cj.sb_frame_stride = 0; cj.d_skip8 = skip8; cj.skip_frame_stride = skip_frame_stride;
    if (c.cdef_search) {      // a strength set per superblock and frame against the source; CDEF then runs with the chosen records
      av1mi_cdef_search_job sj;
      memset(&sj, 0, sizeof(sj));
      sj.width = w; sj.height = h; sj.bit_depth = bd; sj.nframes = S; sj.stride_y = cj.stride_y; sj.stride_uv = cj.stride_uv;
      yuv(sj.d_src_y, sj.d_src_u, sj.d_src_v, g->d_dbl); yuv(sj.d_orig_y, sj.d_orig_u, sj.d_orig_v, src);
      sj.d_skip8 = skip8; sj.skip_frame_stride = skip_frame_stride; sj.true_width = g->vw; sj.true_height = g->vh; sj.bits = c.cdef_search; sj.params = &P;
      sj.d_sse = (uint64_t *)s.d_cdef_cost; sj.d_strength = (uint8_t *)s.d_cdef_rec; sj.d_idx = (uint8_t *)s.d_cdef_idx;
      G_TRY(av1mi_cdef_search(g->ctx, &sj));
      cj.d_sb_strength = sj.d_strength; cj.sb_frame_stride = (size_t)av1mi::sb_count(w, h);
    }
    G_TRY(av1mi_cdef_frames(g->ctx, &cj));
  }
  if (padded(g))
    for (int p = 0; p < 3; p++) { G_TRY(extend_plane(g, g->plane[p], g->d_dbl[p])); G_TRY(extend_plane(g, g->plane[p], g->d_cdef[p])); }
  return AV1MI_OK;
}

// loop restoration of every frame, and the decision per segment and plane whether it stays ON (it must lower the squared error
// against the source): d_ref always receives the restored planes, the next batch's kernels choose between d_ref and d_cdef
static int restore(av1mi_gop *g, Slot &s, const void *const src[3]) {
  const av1mi_gop_config &c = g->cfg;
  const int w = c.width, h = c.height, S = c.segments, bd = g->bd;
  const av1mi_frame_params &P = s.params;
  av1mi_lr_decide_job lj;
  memset(&lj, 0, sizeof(lj));
  lj.width = w; lj.height = h; lj.bit_depth = bd; lj.nframes = S; lj.unit_size = P.lr_unit_size; lj.stride_y = g->plane[0].w; lj.stride_uv = g->plane[1].w;
  yuv(lj.d_cdef_y, lj.d_cdef_u, lj.d_cdef_v, g->d_cdef); yuv(lj.d_dbl_y, lj.d_dbl_u, lj.d_dbl_v, g->d_dbl);
  yuv(lj.d_out_y, lj.d_out_u, lj.d_out_v, g->d_ref); yuv(lj.d_orig_y, lj.d_orig_u, lj.d_orig_v, src);
  lj.d_units_y = (const int8_t *)g->d_lr[0]; lj.d_units_uv = (const int8_t *)g->d_lr[1];
  lj.d_scratch = g->d_lr_scratch; lj.d_on = (uint8_t *)s.d_lr_on;
  if (c.lr_search) {      // zero the cost table, search, pick; then the restoration and its decision with the batch's own units
    av1mi_lr_search_job sj;
    memset(&sj, 0, sizeof(sj));
    sj.width = w; sj.height = h; sj.bit_depth = bd; sj.nframes = S; sj.unit_size = 64; sj.qindex = s.q; sj.stride_y = lj.stride_y; sj.stride_uv = lj.stride_uv;
    yuv(sj.d_cdef_y, sj.d_cdef_u, sj.d_cdef_v, g->d_cdef); yuv(sj.d_dbl_y, sj.d_dbl_u, sj.d_dbl_v, g->d_dbl); yuv(sj.d_orig_y, sj.d_orig_u, sj.d_orig_v, src);
    sj.d_scratch = s.d_lr_cost; sj.d_units_y = (int8_t *)s.d_lr_units[0]; sj.d_units_u = (int8_t *)s.d_lr_units[1]; sj.d_units_v = (int8_t *)s.d_lr_units[2];
    sj.d_choice = (uint8_t *)s.d_lr_choice;
    G_TRY(av1mi_lr_search(g->ctx, &sj));
    lj.d_units_y = sj.d_units_y; lj.d_units_uv = sj.d_units_u; lj.d_units_v = sj.d_units_v;
    lj.unit_frame_stride_y = g->lr_units[0]; lj.unit_frame_stride_uv = g->lr_units[1]; lj.unit_frame_stride_v = g->lr_units[2];
  }
  lj.no_self_guided_units = P.lr_unit_y[0] != 2 && P.lr_unit_uv[0] != 2;
  G_TRY(av1mi::lr_yuv_decide_with(g->ctx, &lj, true));
  if (padded(g))      // the next batch's motion compensation reads this frame beyond the true size
    for (int p = 0; p < 3; p++) G_TRY(extend_plane(g, g->plane[p], g->d_ref[p]));
  return AV1MI_OK;
}

// The searches' results to the host with every batch (a few KB, for the host writer, the frame header and the statistics): the slot's
// mirrors in table order on the download stream behind filters_done, then search_down, which av1mi_gop_collect waits for
static int download_search_results(av1mi_gop *g, Slot &s) {
  if (!s.mirrors) return AV1MI_OK;
  G_HIP(hipStreamWaitEvent(g->down, s.filters_done, 0));
  for (int i = 0; i < s.mirrors; i++) G_HIP(hipMemcpyAsync(s.mirror[i].pinned, s.mirror[i].device, s.mirror[i].bytes, hipMemcpyDeviceToHost, g->down));
  G_HIP(hipEventRecord(s.search_down, g->down));
  return AV1MI_OK;
}

// in-loop filters: reconstruction -> what the next frame predicts from; then filters_done and (symbols_down) the decision -> downloaded
static int loop_filters(av1mi_gop *g, Slot &s, const void *const src[3]) {
  LfMaps maps;
  G_TRY(follow_q(g, s));
  G_TRY(deblock_search(g, s, src, maps));
  G_TRY(deblock_cdef(g, s, src, maps));
  G_TRY(restore(g, s, src));
  G_HIP(hipEventRecord(s.filters_done, av1mi::ctx_stream(g->ctx)));
  G_TRY(download_search_results(g, s));
  if (s.symbols_down) {
    G_HIP(hipStreamWaitEvent(g->down, s.filters_done, 0));
    G_HIP(hipMemcpyAsync(s.h_lr_on, s.d_lr_on, (size_t)g->cfg.segments * 3, hipMemcpyDeviceToHost, g->down));
    G_HIP(hipEventRecord(s.downloaded, g->down));
  }
  return AV1MI_OK;
}

// quality_stats: the batch's records.  The planar source at the coded size against what a decoder outputs — per segment and plane the
// restored plane (d_ref) or, where the decision just made switched restoration off, the CDEF plane (d_cdef) — over the TRUE frame size.
// On the main stream behind the filters: the next batch's filters overwrite d_ref / d_cdef later on the same stream, and this slot's
// d_lr_on is next written kSlots batches on, so stream order is the guard.  The summing launch writes the records straight into the
// slot's pinned memory; quality_done is what av1mi_gop_collect waits for (this batch's own event, not the stream), and what the
// slot's next upload waits for before it overwrites the source.
static int measure_quality(av1mi_gop *g, Slot &s, const void *const src[3]) {
  hipStream_t main = av1mi::ctx_stream(g->ctx);
  av1mi::QualityLaunch Q;
  Q.bd = g->bd; Q.w = g->vw; Q.h = g->vh; Q.frames = g->cfg.segments;
  Q.src = src; Q.dec0 = g->d_ref; Q.dec1 = g->d_cdef; Q.sel = (const uint8_t *)s.d_lr_on;
  Q.scratch = g->d_quality_scratch; Q.out = (av1mi_quality *)s.h_quality;
  {
    av1mi::ProfScope ps(g->ctx, AV1MI_K_QUALITY, main);
    G_HIP(av1mi::launch_quality(Q, main));
  }
  G_HIP(hipEventRecord(s.quality_done, main));
  return AV1MI_OK;
}

// The coder's results of a slot reach its pinned mirrors — tile sizes, total + status, the restoration flags — the way the payloads
// do: the gather stores them (av1mi::Av1EntMirrors), and ent_done, recorded on the stream the range coder ran on, is what the host
// waits for before it reads any of them.  No copies.
static av1mi::Av1EntMirrors entropy_mirrors(av1mi_gop *g, Slot &s) {
  return { (uint32_t *)s.h_tile_size, (uint64_t *)s.h_total, (uint8_t *)s.h_lr_on, (uint32_t)g->cfg.segments * 3u };
}
static int entropy_results(av1mi_gop *g, Slot &s, hipStream_t st) {
  G_HIP(hipEventRecord(s.ent_done, st));
  return AV1MI_OK;
}
// the deferred back half of a slot's entropy job (coder_streams 3)
static int finish_entropy(av1mi_gop *g, Slot &s, hipStream_t st) {
  const av1mi::Av1EntMirrors m = entropy_mirrors(g, s);
  G_TRY(av1mi::av1_entropy_back(g->ctx, s.ent_ticket, st, &m));
  s.ent_ticket = -1;
  return entropy_results(g, s, st);
}

// the AV1 tile entropy coder beside the next batch's block pipeline: tokenizer + chains on the context's side stream (after
// the filters: the restoration units a tile codes depend on the decision), the serial range coder on its back stream (so the
// next batch's tokenizer does not wait for it)
static int start_coder(av1mi_gop *g, Slot &s) {
  const av1mi_gop_config &c = g->cfg;
  const av1mi_frame_params &P = s.params;
  hipStream_t main = av1mi::ctx_stream(g->ctx), side = av1mi::ctx_side_stream(g->ctx), back = av1mi::ctx_back_stream(g->ctx);
  if (!side || !back) return av1mi::ctx_fail(g->ctx, AV1MI_E_DEVICE, "no side stream");
  if (g->coder_streams == 1) back = side;                 // diagnostic arrangements (AV1MI_CODER_STREAMS): the whole coder on the side stream
  else if (g->coder_streams == 2) side = back = main;     // ... or on the main stream, serialised behind the filters
  if (side != main) G_HIP(hipStreamWaitEvent(side, s.filters_done, 0));
  av1mi_av1_entropy_job ej;
  memset(&ej, 0, sizeof(ej));
  ej.width = c.width; ej.height = c.height; ej.nframes = c.segments; ej.key = s.frame_type == 0; ej.base_q_idx = s.q;
  ej.d_lev_y = (const int16_t *)s.d_lev[0]; ej.d_lev_u = (const int16_t *)s.d_lev[1]; ej.d_lev_v = (const int16_t *)s.d_lev[2];
  ej.d_modes_y = (const uint8_t *)s.d_modes[0]; ej.d_modes_uv = (const uint8_t *)s.d_modes[1];
  ej.d_mvs = (const int16_t *)s.d_mv; ej.d_skip = (const uint8_t *)s.d_skip;
  ej.lr_on[0] = P.lr_unit_y[0] == 1; ej.lr_on[1] = ej.lr_on[2] = P.lr_unit_uv[0] == 1;
  ej.d_lr_on = (const uint8_t *)s.d_lr_on;
  av1mi_av1_entropy_units eu;
  if (c.lr_search) for (int p = 0; p < 3; p++) { eu.d_units[p] = (const int8_t *)s.d_lr_units[p]; eu.frame_stride[p] = (size_t)g->lr_units[p]; }
  const av1mi_av1_entropy_cdef ec = { c.cdef_search, (const uint8_t *)s.d_cdef_idx, (size_t)av1mi::sb_count(c.width, c.height) };
  ej.visible_width = g->vw; ej.visible_height = g->vh;
  ej.key_rows32 = s.frame_type == 0 && g->key32 ? g->key_rows32 : 0;
  memcpy(ej.lr_unit_y, P.lr_unit_y, 8); memcpy(ej.lr_unit_uv, P.lr_unit_uv, 8);
  ej.d_out = (uint8_t *)s.h_ent_out; ej.out_cap = g->ent_cap; ej.d_tile_size = (uint32_t *)s.d_tile_size; ej.d_total = (uint64_t *)s.d_total;
  if (g->coder_streams == 3) {
    // tokenizer + chains of THIS batch on the side stream; the range coder of the PREVIOUS batch on the main stream, behind this
    // batch's filters: two queues that are both busy all the time ((pipeline + filters + coder) beside (tokenizer + chains)) instead of
    // a short one and a long one
    G_TRY(av1mi::av1_entropy_front(g->ctx, &ej, side, &s.ent_ticket, c.lr_search ? &eu : nullptr, c.cdef_search ? &ec : nullptr));
    Slot &prev = g->slot[(g->submitted + kSlots - 1) % kSlots];
    if (g->submitted > 0 && prev.ent_ticket >= 0) G_TRY(finish_entropy(g, prev, main));
  } else {
    const av1mi::Av1EntMirrors m = entropy_mirrors(g, s);
    G_TRY(av1mi::av1_entropy_submit(g->ctx, &ej, side, back, &m, c.lr_search ? &eu : nullptr, c.cdef_search ? &ec : nullptr));
    G_TRY(entropy_results(g, s, back));
  }
  s.ent_pending = true;
  return AV1MI_OK;
}

// one batch through the stages above; dev_src as for feed_source
static int submit_batch(av1mi_gop *g, int frame_type, const void *const *dev_src, int store = 0, const int32_t *index = nullptr, const int32_t *bottom = nullptr) {
  if (g->submitted - g->collected >= kSlots) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "%d batches in flight: collect first", (int)kSlots);
  if (frame_type < -1 || frame_type > 1) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "frame_type %d", frame_type);
  if (frame_type < 0) frame_type = g->gop_pos == 0 ? 0 : 1;
  if (frame_type == 1 && g->submitted == 0) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "the first frame of a session must be a key frame");
  G_HIP(hipSetDevice(av1mi::ctx_device(g->ctx)));
  Slot &s = g->slot[g->submitted % kSlots];
  // the batch's quantiser: fixed here, whatever av1mi_gop_set_base_q_idx is told while the batch is in flight
  s.q = g->next_q;
  if (s.q == g->cfg.base_q_idx) s.params = g->params[frame_type];
  else frame_params(s.q, g->bd, frame_type, &s.params);
  const void *src[3];
  G_TRY(feed_source(g, s, dev_src, src, store, index, bottom));
  if (s.ent_pending) G_HIP(hipStreamWaitEvent(av1mi::ctx_stream(g->ctx), s.ent_done, 0));      // the GPU coder of the slot's previous batch still reads its symbols
  G_TRY(code_blocks(g, s, frame_type, src));
  // symbols -> pinned host memory, beside the filters.  Not when the GPU codes the tiles (gpu_entropy == 1): the host then needs
  // the payloads only (and a fifth busy stream would share a hardware queue with one of the other four)
  s.symbols_down = g->cfg.gpu_entropy != 1 || g->symbols_always;
  if (s.symbols_down) {
    G_HIP(hipStreamWaitEvent(g->down, s.kernel_done, 0));
    G_TRY(download_symbols(g, s));
  }
  G_TRY(loop_filters(g, s, src));
  if (g->cfg.quality_stats) G_TRY(measure_quality(g, s, src));
  if (g->cfg.gpu_entropy) G_TRY(start_coder(g, s));
  g->last = (int)(g->submitted % kSlots);
  g->submitted++;
  g->gop_pos = frame_type == 0 ? 1 % g->cfg.gop_length : (g->gop_pos + 1) % g->cfg.gop_length;
  if (!index) g->acquired = false;      // (a batch from the store leaves the pinned buffers, which feed the next put, alone)
  return AV1MI_OK;
}

extern "C" {

int av1mi_gop_set_base_q_idx(av1mi_gop *g, int base_q_idx) {
  if (!g) return AV1MI_E_INVAL;
  if (base_q_idx < 1 || base_q_idx > 255) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "base_q_idx %d must lie in 1..255", base_q_idx);
  g->next_q = base_q_idx;
  return AV1MI_OK;
}

int av1mi_gop_pending(av1mi_gop *g) { return g ? (int)(g->submitted - g->collected) : 0; }
long av1mi_gop_entropy_fallbacks(av1mi_gop *g) { return g ? g->fallbacks : 0; }

int av1mi_gop_acquire_input(av1mi_gop *g, void **y, void **u, void **v) {
  if (!g || !y || !u || !v) return AV1MI_E_INVAL;
  G_HIP(hipSetDevice(av1mi::ctx_device(g->ctx)));
  if (g->cfg.store_frames) {      // the pinned buffers feed the store, not a batch: a ring of their own, whatever is in flight
    const int k = (int)(g->puts % kSlots);
    if (g->put_pending[k]) { G_HIP(hipEventSynchronize(g->put_done[k])); g->put_pending[k] = false; }
    *y = g->slot[k].h_in[0]; *u = g->slot[k].h_in[1]; *v = g->slot[k].h_in[2];
    g->acquired = true;
    return AV1MI_OK;
  }
  if (g->submitted - g->collected >= kSlots) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "%d batches in flight: collect before acquiring the next input", (int)kSlots);
  Slot &s = g->slot[g->submitted % kSlots];
  if (s.upload_pending) { G_HIP(hipEventSynchronize(s.uploaded)); s.upload_pending = false; }   // the copy engine still reads these buffers
  *y = s.h_in[0]; *u = s.h_in[1]; *v = s.h_in[2];      // in the session's format; no third plane in the semi-planar ones, no chroma for a grey source
  g->acquired = true;
  return AV1MI_OK;
}

int av1mi_gop_submit(av1mi_gop *g, int frame_type) {
  if (!g) return AV1MI_E_INVAL;
  if (g->cfg.store_frames) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "a session with a frame store is fed through av1mi_gop_store_put / av1mi_gop_submit_stored");
  if (!g->acquired) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "submit without av1mi_gop_acquire_input");
  return submit_batch(g, frame_type, nullptr);
}

int av1mi_gop_store_put(av1mi_gop *g, int store, int first, int count) {
  if (!g) return AV1MI_E_INVAL;
  const int N = store_capacity(g->cfg);
  if (!g->cfg.store_frames) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "the session has no frame store (store_frames 0)");
  if (store < 0 || store > 1 || count < 1 || count > g->cfg.segments || first < 0 || first > N - count)
    return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "store_put: store %d, frames %d .. %d + %d of %d (at most %d at a time)", store, first, first, count, N, g->cfg.segments);
  if (!g->acquired) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "store_put without av1mi_gop_acquire_input");
  G_HIP(hipSetDevice(av1mi::ctx_device(g->ctx)));
  Store &st = g->store[store];
  const int k = (int)(g->puts % kSlots);
  if (st.has_reader) G_HIP(hipStreamWaitEvent(g->up, st.read_done, 0));      // the batches that gather from this store
  for (int p = 0; p < 3; p++)
    if (const size_t fb = g->layout.plane[p].frame_bytes)
      G_HIP(hipMemcpyAsync((char *)st.d[p] + fb * (size_t)first, g->slot[k].h_in[p], fb * (size_t)count, hipMemcpyHostToDevice, g->up));
  G_HIP(hipEventRecord(g->put_done[k], g->up));
  g->put_pending[k] = true;
  G_HIP(hipEventRecord(st.filled, g->up));
  st.has_fill = true;
  st.run = first == 0 ? count : std::max(st.run, first + count);
  g->puts++;
  g->acquired = false;
  return AV1MI_OK;
}

int av1mi_gop_store_analyse(av1mi_gop *g, int store, int frames, av1mi_scene_record *out) {
  if (!g) return AV1MI_E_INVAL;
  if (!g->cfg.store_frames) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "the session has no frame store (store_frames 0)");
  if (store < 0 || store > 1 || frames < 1 || frames > g->cfg.store_frames || !out)
    return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "store_analyse: store %d, %d frames of %d", store, frames, g->cfg.store_frames);
  G_HIP(hipSetDevice(av1mi::ctx_device(g->ctx)));
  av1mi::SceneLaunch L;
  L.bd = g->layout.bit_depth; L.w = g->layout.width; L.h = g->layout.height; L.frames = frames;
  L.luma = g->store[store].d[0]; L.scratch = g->d_scene; L.out = (av1mi_scene_record *)g->h_records;
  // on the upload stream, behind the puts; the summing launch writes the records into pinned memory
  G_HIP(av1mi::launch_scene(L, g->up));
  G_HIP(hipEventRecord(g->scene_done, g->up));
  G_HIP(hipEventSynchronize(g->scene_done));
  memcpy(out, g->h_records, (size_t)frames * sizeof(av1mi_scene_record));
  return AV1MI_OK;
}

int av1mi_gop_submit_stored(av1mi_gop *g, int store, const int32_t *index, int frame_type) {
  if (!g) return AV1MI_E_INVAL;
  if (!g->cfg.store_frames) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "the session has no frame store (store_frames 0)");
  if (store < 0 || store > 1 || !index || !g->store[store].has_fill) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "submit_stored: store %d holds nothing, or no index", store);
  if (frame_type != 0 && frame_type != 1) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "submit_stored: frame_type %d (0 key or 1 inter: the layout is the caller's)", frame_type);
  const int per = g->cfg.deinterlace_fields ? 2 : 1;      // output positions per source frame
  for (int s = 0; s < g->cfg.segments; s++)
    if (index[s] < -1 || index[s] >= per * store_capacity(g->cfg))      // (a session that weaves: its context positions included)
      return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "submit_stored: index[%d] = %d outside the store of %d frames%s", s, (int)index[s], store_capacity(g->cfg), per == 2 ? " (two output positions each)" : "");
  for (int s = 0; (g->cfg.deinterlace || g->cfg.denoise) && s < g->cfg.segments; s++)
    if (index[s] >= per * g->store[store].run)
      return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "submit_stored: index[%d] = %d beyond the store's run of %d frames%s (the filter reads the neighbours inside it)", s, (int)index[s], g->store[store].run, per == 2 ? " (two output positions each)" : "");
  return submit_batch(g, frame_type, nullptr, store, index);
}

int av1mi_gop_store_telecine(av1mi_gop *g, int store, int frames, av1mi_telecine_record *out) {
  if (!g) return AV1MI_E_INVAL;
  if (!g->cfg.telecine) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "the session does not weave (telecine 0)");
  if (store < 0 || store > 1 || frames < 1 || frames > store_capacity(g->cfg) || frames > g->store[store].run || !out)
    return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "store_telecine: store %d, %d frames of a run of %d (the store holds %d)", store, frames, store >= 0 && store <= 1 ? g->store[store].run : 0, store_capacity(g->cfg));
  G_HIP(hipSetDevice(av1mi::ctx_device(g->ctx)));
  av1mi::TelecineLaunch L;
  L.bd = g->layout.bit_depth; L.stride = g->layout.width; L.rows = g->layout.height; L.w = g->layout.true_width; L.h = g->layout.true_height; L.frames = frames;
  L.luma = g->store[store].d[0]; L.scratch = g->d_telecine; L.out = (av1mi_telecine_record *)g->h_telecine;
  // on the upload stream, behind the puts; the summing launch writes the records into pinned memory
  G_HIP(av1mi::launch_telecine_analyse(L, g->up));
  G_HIP(hipEventRecord(g->telecine_done, g->up));
  G_HIP(hipEventSynchronize(g->telecine_done));
  memcpy(out, g->h_telecine, (size_t)frames * sizeof(av1mi_telecine_record));
  return AV1MI_OK;
}

int av1mi_gop_submit_woven(av1mi_gop *g, int store, const int32_t *top, const int32_t *bottom, int frame_type) {
  if (!g) return AV1MI_E_INVAL;
  if (!g->cfg.telecine) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "the session does not weave (telecine 0)");
  if (store < 0 || store > 1 || !top || !bottom || !g->store[store].has_fill) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "submit_woven: store %d holds nothing, or no positions", store);
  if (frame_type != 0 && frame_type != 1) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "submit_woven: frame_type %d (0 key or 1 inter: the layout is the caller's)", frame_type);
  for (int s = 0; s < g->cfg.segments; s++) {
    if (top[s] == -1) continue;      // a flat slot: bottom[s] is not read
    if (top[s] < 0 || bottom[s] < 0 || top[s] >= g->store[store].run || bottom[s] >= g->store[store].run)
      return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "submit_woven: segment %d weaves positions %d / %d, outside the store's run of %d frames", s, (int)top[s], (int)bottom[s], g->store[store].run);
  }
  return submit_batch(g, frame_type, nullptr, store, top, bottom);
}

int av1mi_gop_submit_device(av1mi_gop *g, const void *d_y, const void *d_u, const void *d_v, int frame_type) {
  if (!g) return AV1MI_E_INVAL;
  if (g->cfg.tone_map) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "av1mi_gop_submit_device in a tone_map session is not built: the map runs in place and would overwrite the caller's planes");
  if (!g->layout.plane[2].frame_bytes) d_v = d_u;            // planes the layout does not have (semi-planar: the third; grey: both chroma
  if (!g->layout.plane[1].frame_bytes) d_u = d_v = d_y;      // planes) are not read
  if (!d_y || !d_u || !d_v || (((uintptr_t)d_y | (uintptr_t)d_u | (uintptr_t)d_v) & (g->fed_align - 1)))
    return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "null or misaligned device source plane");
  const void *src[3] = { d_y, d_u, d_v };
  return submit_batch(g, frame_type, src);
}

int av1mi_gop_collect(av1mi_gop *g, av1mi_gop_frame *out) {
  if (!g || !out) return AV1MI_E_INVAL;
  if (g->submitted == g->collected) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "nothing in flight");
  G_HIP(hipSetDevice(av1mi::ctx_device(g->ctx)));
  Slot &s = g->slot[g->collected % kSlots];
  if (s.symbols_down) G_HIP(hipEventSynchronize(s.downloaded));
  memset(out, 0, sizeof(*out));
  out->params = s.params;
  out->lr_on = (const uint8_t *)s.h_lr_on;
  if (s.mirrors) G_HIP(hipEventSynchronize(s.search_down));      // the searches' results, all of them (download_search_results)
  if (g->cfg.lr_search) {
    for (int p = 0; p < 3; p++) { out->lr_units[p] = (const int8_t *)s.h_lr_units[p]; out->lr_units_per_frame[p] = g->lr_units[p]; }
    out->lr_choice = (const uint8_t *)s.h_lr_choice;
  }
  if (g->cfg.cdef_search) {
    out->cdef_bits = g->cfg.cdef_search; out->cdef_idx = (const uint8_t *)s.h_cdef_idx;
    av1mi_cdef_search_sets(&s.params, out->cdef_bits, out->cdef_y, out->cdef_uv);
  }
  if (g->cfg.lf_search) { out->lf_levels = (const uint8_t *)s.h_lf_levels; out->lf_choice = (const uint8_t *)s.h_lf_choice; }
  if (g->cfg.quality_stats) { G_HIP(hipEventSynchronize(s.quality_done)); out->quality = (const av1mi_quality *)s.h_quality; }
  if (g->cfg.denoise && s.has_grain) { G_HIP(hipEventSynchronize(s.grain_done)); out->grain = (const av1mi_grain_record *)s.h_grain; out->grain_cov = (const av1mi_grain_cov_record *)s.h_grain_cov; }
  out->segments = g->cfg.segments;
  out->bit_depth = g->bd;
  out->blocks_per_frame = g->nb / (size_t)g->cfg.segments;
  out->key_block_size = s.frame_type == 0 && g->key32 ? 32 : 8;
  out->key_modes_stride = g->key_modes_stride; out->key_modes_band = g->key_modes_band;
  auto symbols = [&](bool levels) {
    if (s.frame_type == 0) { out->y_mode = (const uint8_t *)s.h_modes[0]; out->uv_mode = (const uint8_t *)s.h_modes[1]; }
    else { out->mv = (const int16_t *)s.h_mv; out->skip = (const uint8_t *)s.h_skip; }
    if (levels) { out->lev_y = (const int16_t *)s.h_lev[0]; out->lev_u = (const int16_t *)s.h_lev[1]; out->lev_v = (const int16_t *)s.h_lev[2]; }
  };
  if (s.symbols_down) symbols(true);
  if (g->cfg.gpu_entropy) {
    if (s.ent_ticket >= 0) G_TRY(finish_entropy(g, s, av1mi::ctx_stream(g->ctx)));      // no later batch came to carry it (coder_streams 3)
    G_HIP(hipEventSynchronize(s.ent_done));
    const uint64_t total = ((const uint64_t *)s.h_total)[0], status = ((const uint64_t *)s.h_total)[1];
    // the payloads are already here: k_av1_gather wrote them into the slot's pinned buffer (a copy enqueued NOW would queue
    // behind the next batches' work, which is already submitted)
    if (status || total > g->ent_cap) {
      if (getenv("AV1MI_DEBUG"))
        fprintf(stderr, "[av1mi] batch %ld (frame type %d) falls back to the host coder: status %llx (1 list / records, 2 payload slot, 4 output), %llu bytes of %zu\n",
                (long)g->collected, s.frame_type, (unsigned long long)status, (unsigned long long)total, g->ent_cap);
      // A tile exceeded the coder's list / record / payload capacity (very fine quantisers on dense content).  The batch is not
      // lost: its symbols are still in the slot's device buffers (the next kernel that overwrites them is kSlots submits away),
      // so they are downloaded now and handed out like in host mode: tile_size stays NULL, the caller entropy-codes this batch.
      if (!s.symbols_down) {
        // the pinned mirrors of the levels exist only once a batch has needed them: all slots' at the first fallback (pinning memory
        // stalls the device), not one slot at a time in the middle of later batches
        for (Slot &o : g->slot)
          for (int p = 0; p < 3; p++)
            if (!o.h_lev[p]) G_TRY(host_alloc(g, &o.h_lev[p], g->plane[p].n * 2));
        G_TRY(download_symbols(g, s));
        G_HIP(hipStreamSynchronize(g->down));
        symbols(true);
      }
      // content the GPU coder cannot hold tends to stay that way: from the third such batch on the symbols are sent down with every
      // batch, beside the filters (as in host mode), instead of after the coder has given the batch back
      if (g->fallbacks + 1 >= kFallbacksToHostMode) g->symbols_always = true;
      g->fallbacks++;
    } else {
      out->tiles_per_frame = g->tiles; out->tile_size = (const uint32_t *)s.h_tile_size; out->tile_payload = (const uint8_t *)s.h_ent_out; out->payload_bytes = total;
    }
  }
  g->collected++;
  return AV1MI_OK;
}

int av1mi_gop_download_fed(av1mi_gop *g, void *y, void *u, void *v) {
  if (!g || !y) return AV1MI_E_INVAL;
  if (!g->submitted) return av1mi::ctx_fail(g->ctx, AV1MI_E_INVAL, "download_fed: nothing was submitted");
  G_TRY(av1mi_sync(g->ctx));
  G_HIP(hipStreamSynchronize(g->up));
  void *dst[3] = { y, u, v };
  for (int p = 0; p < 3; p++)
    if (fed_bytes(g, p) && dst[p]) G_TRY(av1mi_download(g->ctx, dst[p], g->slot[g->last].d_in[p], fed_bytes(g, p)));
  return AV1MI_OK;
}

int av1mi_gop_download_reference(av1mi_gop *g, void *y, void *u, void *v) {
  if (!g || !y || !u || !v) return AV1MI_E_INVAL;
  G_TRY(av1mi_sync(g->ctx));
  // per segment and plane the restored plane or, where restoration was switched off, the CDEF output: what the decoder outputs
  const int S = g->cfg.segments;
  std::vector<uint8_t> on((size_t)S * 3, 1);
  if (g->submitted) G_TRY(av1mi_download(g->ctx, on.data(), g->slot[g->last].d_lr_on, on.size()));
  void *dst[3] = { y, u, v };
  for (int p = 0; p < 3; p++) {
    const size_t per = g->plane[p].bytes / (size_t)S;
    for (int sg = 0; sg < S; sg++)
      G_TRY(av1mi_download(g->ctx, (char *)dst[p] + per * sg, (const char *)(on[(size_t)sg * 3 + p] ? g->d_ref[p] : g->d_cdef[p]) + per * sg, per));
  }
  return AV1MI_OK;
}

}  // extern "C"
