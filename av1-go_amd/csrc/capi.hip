// capi.hip — the C ABI of libav1mi.so (include/av1mi.h).  Thin: argument checks, device selection,
// error text, and launches onto the context's stream.  No CPU fallback exists: without a usable HIP
// device av1mi_open() fails with AV1MI_E_NODEV and every other entry point needs a context.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "av1mi_internal.hpp"
#include "qtables.hpp"
#include "quality.hpp"

struct av1mi_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;             // AV1 coder of a GOP session: tokenizer + chains beside the main stream's next launches
  hipStream_t back = nullptr;             // AV1 coder of a GOP session: the serial range coder, beside the next batch's tokenizer on `side`
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  char err[801] = { 0 };  // transcode.go:295-297 caps the reason text at 800 chars
  char name[256] = { 0 };
  void *scratch = nullptr;  // staging for the host-pointer single-block forms
  size_t scratch_bytes = 0;
  av1mi_av1ent_state *av1ent = nullptr;   // the AV1-syntax tile coder's scratch (av1_entropy_kernels.hip)
  av1mi::ScalePlan *scale_plan = nullptr; // av1mi_scale_planes: the tables of the geometry it was last called with
  void *quality_scratch = nullptr;        // av1mi_quality_planes: the tiles' partial sums (grown on demand)
  size_t quality_scratch_bytes = 0;
  void *me_scratch = nullptr;             // av1mi_inter_encode / av1mi_me_search with a coarse_range: quarter planes + centres (grown on demand)
  size_t me_scratch_bytes = 0;
  void *scene_scratch = nullptr;          // av1mi_scene_analyse: quarter planes + block results (grown on demand)
  size_t scene_scratch_bytes = 0;
  void *crop_scratch = nullptr;           // av1mi_crop_analyse: the partial row / column sums (grown on demand)
  size_t crop_scratch_bytes = 0;
  void *noise_scratch = nullptr;          // av1mi_noise_analyse: the workgroups' partial histograms (grown on demand)
  size_t noise_scratch_bytes = 0;
  void *peak_scratch = nullptr;           // av1mi_peak_analyse: the workgroups' partial histograms (grown on demand)
  size_t peak_scratch_bytes = 0;
  void *telecine_scratch = nullptr;       // av1mi_telecine_analyse: the waves' partial sums (grown on demand)
  size_t telecine_scratch_bytes = 0;
  void *grain_scratch = nullptr;          // av1mi_denoise_gather: the workgroups' partial records (grown on demand)
  size_t grain_scratch_bytes = 0;
  void *denoise_vectors = nullptr;        // av1mi_denoise_mc_gather without d_vectors: the blocks' vectors (grown on demand)
  void *grain_cov_scratch = nullptr;      // av1mi_grain_cov: the workgroups' partial sums (grown on demand)
  size_t grain_cov_scratch_bytes = 0;
  size_t denoise_vectors_bytes = 0;
  // per-kernel profile: one event pair per launch while enabled
  bool prof_on = false;
  struct ProfRec { int kind; hipEvent_t e0, e1; };
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> prof_pool;
  int prof_calls[AV1MI_K_KINDS] = { 0 };
  double prof_ms[AV1MI_K_KINDS] = { 0 };
};

namespace {

constexpr auto &fail = av1mi::ctx_fail;      // the one failure formatter, under the name the checks below use
#define HIP_TRY(ctx, expr)                                                                     \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(ctx, AV1MI_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define BIND(ctx)                                                   \
  do {                                                              \
    if (!(ctx)) return AV1MI_E_INVAL;                               \
    HIP_TRY(ctx, hipSetDevice((ctx)->device));                      \
  } while (0)

hipEvent_t prof_event(av1mi_ctx *ctx) {
  if (!ctx->prof_pool.empty()) { hipEvent_t e = ctx->prof_pool.back(); ctx->prof_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
using av1mi::ProfScope;
void prof_drain(av1mi_ctx *ctx) {
  if (ctx->prof_recs.empty()) return;
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->side) (void)hipStreamSynchronize(ctx->side);
  if (ctx->back) (void)hipStreamSynchronize(ctx->back);
  for (auto &r : ctx->prof_recs) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { ctx->prof_calls[r.kind]++; ctx->prof_ms[r.kind] += ms; }
    ctx->prof_pool.push_back(r.e0); ctx->prof_pool.push_back(r.e1);
  }
  ctx->prof_recs.clear();
}

bool tx_valid(int tx_size, int tx_type) {
  if (tx_type == AV1MI_WHT_WHT) return tx_size == AV1MI_TX_4X4;
  if (tx_size < 0 || tx_size >= AV1MI_TX_SIZES_ALL || tx_type < 0 || tx_type >= AV1MI_TX_TYPES) return false;
  const int w = av1mi::tx_width(tx_size), h = av1mi::tx_height(tx_size);
  static const int colk[16] = { 0, 1, 0, 1, 2, 0, 2, 1, 2, 3, 0, 3, 1, 3, 2, 3 };
  static const int rowk[16] = { 0, 0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 3, 1, 3, 2 };
  const int r = rowk[tx_type], c = colk[tx_type];
  if ((r == 1 || r == 2) && w > 16) return false;
  if ((c == 1 || c == 2) && h > 16) return false;
  if (r == 3 && w > 32) return false;
  if (c == 3 && h > 32) return false;
  return true;
}
// one of the context's scratch areas, grown on demand to hold `need` bytes (hipFree waits for the launches that still read the old one)
int grow(av1mi_ctx *ctx, void **buf, size_t *bytes, size_t need) {
  if (*bytes >= need) return AV1MI_OK;
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr; *bytes = 0;
  HIP_TRY(ctx, hipMalloc(buf, need));
  *bytes = need;
  return AV1MI_OK;
}
// the argument rules that every entry point states in the same words
int check_bd(av1mi_ctx *ctx, int bd) { return bd != 8 && bd != 10 ? fail(ctx, AV1MI_E_INVAL, "bit depth %d not supported (8 or 10)", bd) : AV1MI_OK; }
int check_nframes(av1mi_ctx *ctx, int nframes) { return nframes < 0 || nframes > 65535 ? fail(ctx, AV1MI_E_INVAL, "nframes %d out of range", nframes) : AV1MI_OK; }
// ... of a 4:2:0 filter job (CDEF, its search, the deblocking search, deblock + CDEF): the frame and one pair of strides; cap: up to 16384 x 16384 only
int check_frame420(av1mi_ctx *ctx, int w, int h, int stride_y, int stride_uv, bool cap) {
  if (w <= 0 || h <= 0 || (w & 7) || (h & 7) || (cap && (w > 16384 || h > 16384))) return fail(ctx, AV1MI_E_INVAL, "frame %dx%d must be a multiple of 8", w, h);
  if (stride_y < w || stride_uv < w / 2 || (stride_y & 3) || (stride_uv & 3)) return fail(ctx, AV1MI_E_INVAL, "bad strides");
  return AV1MI_OK;
}
// the true size a job's sums run over: 0 = the coded size, else within 7 samples below it
int check_true_size(av1mi_ctx *ctx, int w, int h, int true_w, int true_h, int *tw, int *th) {
  *tw = true_w ? true_w : w; *th = true_h ? true_h : h;
  return *tw > w || *th > h || *tw <= w - 8 || *th <= h - 8 ? fail(ctx, AV1MI_E_INVAL, "true size %dx%d does not round up to %dx%d", *tw, *th, w, h) : AV1MI_OK;
}
// every pointer of a list there and aligned to `align` bytes (a power of two); what: "device", "map"
template <size_t N> int check_pointers(av1mi_ctx *ctx, const char *what, uintptr_t align, const void *const (&ptrs)[N]) {
  for (const void *p : ptrs) if (!p || ((uintptr_t)p & (align - 1))) return fail(ctx, AV1MI_E_INVAL, "null or misaligned %s pointer", what);
  return AV1MI_OK;
}
// a job's _y / _u / _v fields as a launch's planes
template <typename T, typename U> void planes3(T (&dst)[3], U y, U u, U v) { dst[0] = y; dst[1] = u; dst[2] = v; }
int check_lr_unit(av1mi_ctx *ctx, int unit_size, int subsampled) {      // 32 is a chroma unit size only
  if (unit_size == 64 || unit_size == 128 || unit_size == 256 || (unit_size == 32 && subsampled)) return AV1MI_OK;
  return fail(ctx, AV1MI_E_INVAL, "restoration unit size %d not allowed", unit_size);
}
int check_lr_plane(av1mi_ctx *ctx, const av1mi::LrLaunch &L) {      // ... of one plane's restoration (av1mi_lr_frames, av1mi_lr_frames_decide)
  if (!L.cdef || !L.dbl || !L.out || !L.units || L.out == L.cdef || L.out == L.dbl) return fail(ctx, AV1MI_E_INVAL, "null or aliased device pointer");
  if (int rc = check_bd(ctx, L.bd)) return rc;
  if (L.w <= 0 || L.h <= 0 || L.stride < L.w) return fail(ctx, AV1MI_E_INVAL, "bad plane geometry %dx%d stride %d", L.w, L.h, L.stride);
  return check_lr_unit(ctx, L.unit_size, L.ss);
}
int check_tx_launch(av1mi_ctx *ctx, int tx_size, const void *coef, const void *plane, int stride, int nblocks) {
  if (tx_size < 0 || tx_size >= AV1MI_TX_SIZES_ALL) return fail(ctx, AV1MI_E_INVAL, "tx_size %d out of range", tx_size);
  if (!coef || !plane) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  if (nblocks < 0) return fail(ctx, AV1MI_E_INVAL, "nblocks %d < 0", nblocks);
  if (stride <= 0 || (stride & 3)) return fail(ctx, AV1MI_E_INVAL, "stride %d must be a positive multiple of 4", stride);
  if (((uintptr_t)coef & 15) || ((uintptr_t)plane & 7)) return fail(ctx, AV1MI_E_INVAL, "misaligned device pointer");
  return AV1MI_OK;
}
// the fed planes of a filtering gather (av1mi_deinterlace_gather, av1mi_denoise_gather, av1mi_denoise_mc_gather: `name`), checked and
// written into L: bit depth 8 .. max_bd, the segments, per plane the sizes, the destination and, under cell_rule, that the last 16-byte
// cell of a row starts inside the true width
int check_gather_planes(av1mi_ctx *ctx, const char *name, int max_bd, bool cell_rule, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3],
                        const int true_h[3], int segments, const void *const *d_table, void *const d_dst[3], av1mi::GatherPlanes &L) {
  if (bit_depth != 8 && bit_depth != 10 && (bit_depth != 12 || max_bd < 12)) return fail(ctx, AV1MI_E_INVAL, "%s: bit depth %d not supported (%s)", name, bit_depth, max_bd < 12 ? "8 or 10" : "8, 10 or 12");
  if (segments < 1 || segments > 4096) return fail(ctx, AV1MI_E_INVAL, "%s: segments %d out of range (1 .. 4096)", name, segments);
  L.bd = bit_depth; L.segments = segments; L.table = d_table;
  const int bps = bit_depth == 8 ? 1 : 2;
  for (int p = 0; p < 3; p++) {
    const bool have = plane_w[p] > 0 && plane_h[p] > 0;
    if (plane_w[p] < 0 || plane_h[p] < 0 || plane_w[p] > 16384 || plane_h[p] > 16384 || ((size_t)plane_w[p] * bps & 3))
      return fail(ctx, AV1MI_E_INVAL, "%s: plane %d of %dx%d samples (rows of whole dwords, up to 16384x16384)", name, p, plane_w[p], plane_h[p]);
    if (have && (true_w[p] < 1 || true_h[p] < 1 || true_w[p] > plane_w[p] || true_h[p] > plane_h[p] || plane_w[p] - true_w[p] >= 8 || plane_h[p] - true_h[p] >= 8))
      return fail(ctx, AV1MI_E_INVAL, "%s: plane %d: the true size %dx%d must lie within 7 samples below the buffer's %dx%d", name, p, true_w[p], true_h[p], plane_w[p], plane_h[p]);
    if (cell_rule && have && (plane_w[p] * bps - 1) / 16 * (16 / bps) > true_w[p] - 1)
      return fail(ctx, AV1MI_E_INVAL, "%s: plane %d: the last 16-byte cell of a row of %d samples starts beyond the true width %d", name, p, plane_w[p], true_w[p]);
    if (have && (!d_dst[p] || ((uintptr_t)d_dst[p] & 15))) return fail(ctx, AV1MI_E_INVAL, "%s: null or misaligned destination (plane %d)", name, p);
    L.plane_w[p] = have ? plane_w[p] : 0; L.plane_h[p] = have ? plane_h[p] : 0; L.true_w[p] = true_w[p]; L.true_h[p] = true_h[p]; L.dst[p] = d_dst[p];
  }
  return AV1MI_OK;
}

}  // namespace

namespace av1mi {
hipStream_t ctx_stream(av1mi_ctx *ctx) { return ctx->stream; }
int ctx_device(av1mi_ctx *ctx) { return ctx->device; }
av1mi_av1ent_state *ctx_av1ent(av1mi_ctx *ctx) {
  if (!ctx->av1ent) ctx->av1ent = av1ent_new();
  return ctx->av1ent;
}
static hipStream_t lazy_stream(hipStream_t *st) {
  if (!*st && hipStreamCreateWithFlags(st, hipStreamNonBlocking) != hipSuccess) return nullptr;
  return *st;
}
hipStream_t ctx_side_stream(av1mi_ctx *ctx) { return lazy_stream(&ctx->side); }
hipStream_t ctx_back_stream(av1mi_ctx *ctx) { return lazy_stream(&ctx->back); }
ProfToken ctx_prof_begin(av1mi_ctx *ctx, int kind, hipStream_t st) {
  ProfToken t;
  t.kind = kind;
  if (ctx->prof_on) { t.e0 = prof_event(ctx); (void)hipEventRecord(t.e0, st); }
  return t;
}
void ctx_prof_end(av1mi_ctx *ctx, const ProfToken &t, hipStream_t st) {
  if (!t.e0) return;
  hipEvent_t e1 = prof_event(ctx);
  (void)hipEventRecord(e1, st);
  ctx->prof_recs.push_back({ t.kind, t.e0, e1 });
}
int ctx_fail(av1mi_ctx *ctx, int code, const char *fmt, ...) {
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
    va_end(ap);
  }
  return code;
}
}  // namespace av1mi

extern "C" {

const char *av1mi_version(void) { return "av1mi 0.1.0 (gfx950)"; }

int av1mi_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int av1mi_open(int device, av1mi_ctx **out) {
  if (!out) return AV1MI_E_INVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return AV1MI_E_NODEV;
  av1mi_ctx *ctx = new (std::nothrow) av1mi_ctx();
  if (!ctx) return AV1MI_E_NOMEM;
  ctx->device = device;
  hipDeviceProp_t prop;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
    delete ctx;
    return AV1MI_E_NODEV;
  }
  snprintf(ctx->name, sizeof(ctx->name), "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  *out = ctx;
  return AV1MI_OK;
}

void av1mi_close(av1mi_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->side) { (void)hipStreamSynchronize(ctx->side); (void)hipStreamDestroy(ctx->side); }
  if (ctx->back) { (void)hipStreamSynchronize(ctx->back); (void)hipStreamDestroy(ctx->back); }
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->quality_scratch) (void)hipFree(ctx->quality_scratch);
  if (ctx->me_scratch) (void)hipFree(ctx->me_scratch);
  if (ctx->scene_scratch) (void)hipFree(ctx->scene_scratch);
  if (ctx->crop_scratch) (void)hipFree(ctx->crop_scratch);
  if (ctx->noise_scratch) (void)hipFree(ctx->noise_scratch);
  if (ctx->peak_scratch) (void)hipFree(ctx->peak_scratch);
  if (ctx->telecine_scratch) (void)hipFree(ctx->telecine_scratch);
  if (ctx->grain_scratch) (void)hipFree(ctx->grain_scratch);
  if (ctx->denoise_vectors) (void)hipFree(ctx->denoise_vectors);
  if (ctx->grain_cov_scratch) (void)hipFree(ctx->grain_cov_scratch);
  if (ctx->av1ent) av1mi::av1ent_free(ctx->av1ent);
  av1mi::scale_plan_destroy(ctx->scale_plan);
  for (auto &r : ctx->prof_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  for (auto e : ctx->prof_pool) (void)hipEventDestroy(e);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char *av1mi_last_error(av1mi_ctx *ctx) { return ctx ? ctx->err : "null context"; }
const char *av1mi_device_name(av1mi_ctx *ctx) { return ctx ? ctx->name : ""; }

int av1mi_malloc(av1mi_ctx *ctx, void **d_ptr, size_t bytes) {
  BIND(ctx);
  if (!d_ptr) return fail(ctx, AV1MI_E_INVAL, "null out pointer");
  *d_ptr = nullptr;
  hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 16);
  if (e == hipErrorOutOfMemory) return fail(ctx, AV1MI_E_NOMEM, "hipMalloc(%zu): out of memory", bytes);
  HIP_TRY(ctx, e);
  return AV1MI_OK;
}
int av1mi_free(av1mi_ctx *ctx, void *d_ptr) {
  BIND(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipFree(d_ptr));
  return AV1MI_OK;
}
int av1mi_upload(av1mi_ctx *ctx, void *d_dst, const void *src, size_t bytes) {
  BIND(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return AV1MI_OK;
}
int av1mi_download(av1mi_ctx *ctx, void *dst, const void *d_src, size_t bytes) {
  BIND(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return AV1MI_OK;
}
int av1mi_memset(av1mi_ctx *ctx, void *d_dst, int value, size_t bytes) {
  BIND(ctx);
  HIP_TRY(ctx, hipMemsetAsync(d_dst, value, bytes, ctx->stream));
  return AV1MI_OK;
}
int av1mi_copy(av1mi_ctx *ctx, void *d_dst, const void *d_src, size_t bytes) {
  BIND(ctx);
  if (!d_dst || !d_src) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  HIP_TRY(ctx, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return AV1MI_OK;
}
int av1mi_sync(av1mi_ctx *ctx) {
  BIND(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->side) HIP_TRY(ctx, hipStreamSynchronize(ctx->side));
  if (ctx->back) HIP_TRY(ctx, hipStreamSynchronize(ctx->back));
  return AV1MI_OK;
}
int av1mi_timer_begin(av1mi_ctx *ctx) {
  BIND(ctx);
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return AV1MI_OK;
}
int av1mi_timer_end(av1mi_ctx *ctx, float *elapsed_ms) {
  BIND(ctx);
  if (!elapsed_ms) return fail(ctx, AV1MI_E_INVAL, "null out pointer");
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
  HIP_TRY(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
  return AV1MI_OK;
}

int av1mi_prof_enable(av1mi_ctx *ctx, int on) {
  BIND(ctx);
  if (!on) prof_drain(ctx);
  ctx->prof_on = on != 0;
  return AV1MI_OK;
}
int av1mi_prof_reset(av1mi_ctx *ctx) {
  BIND(ctx);
  prof_drain(ctx);
  for (int k = 0; k < AV1MI_K_KINDS; k++) { ctx->prof_calls[k] = 0; ctx->prof_ms[k] = 0; }
  return AV1MI_OK;
}
int av1mi_prof_get(av1mi_ctx *ctx, int kind, int *launches, double *total_ms) {
  BIND(ctx);
  if (kind < 0 || kind >= AV1MI_K_KINDS || !launches || !total_ms) return fail(ctx, AV1MI_E_INVAL, "bad profile query");
  prof_drain(ctx);
  *launches = ctx->prof_calls[kind];
  *total_ms = ctx->prof_ms[kind];
  return AV1MI_OK;
}
const char *av1mi_kernel_kind_name(int kind) {
  static const char *n[AV1MI_K_KINDS] = { "fwd_txfm", "inv_txfm", "quantize", "dequantize", "intra_pred", "mc", "deblock",
                                          "cdef", "loop_restoration", "intra_pipeline", "inter_pipeline", "misc", "entropy_code", "entropy_pack", "entropy_tokens", "me_integer", "entropy_chains", "input_convert", "quality", "me_coarse", "scene" };
  return kind < 0 || kind >= AV1MI_K_KINDS ? "?" : n[kind];
}

int av1mi_txfm_valid(int tx_size, int tx_type) { return tx_valid(tx_size, tx_type) ? 1 : 0; }
int av1mi_tx_width(int tx_size) { return tx_size < 0 || tx_size >= AV1MI_TX_SIZES_ALL ? 0 : av1mi::tx_width(tx_size); }
int av1mi_tx_height(int tx_size) { return tx_size < 0 || tx_size >= AV1MI_TX_SIZES_ALL ? 0 : av1mi::tx_height(tx_size); }

int av1mi_inv_txfm_add_grid(av1mi_ctx *ctx, int tx_size, const int32_t *d_coef, void *d_plane, int stride, int bd,
                            int blocks_per_row, int nblocks, const uint8_t *d_tx_types, int uniform_type) {
  BIND(ctx);
  if (int rc = check_tx_launch(ctx, tx_size, d_coef, d_plane, stride, nblocks)) return rc;
  if (int rc = check_bd(ctx, bd)) return rc;
  if (blocks_per_row <= 0) return fail(ctx, AV1MI_E_INVAL, "blocks_per_row %d <= 0", blocks_per_row);
  if (!d_tx_types && !tx_valid(tx_size, uniform_type))
    return fail(ctx, AV1MI_E_INVAL, "tx_type %d is not defined for tx_size %d", uniform_type, tx_size);
  av1mi::TxLaunch L = { const_cast<int32_t *>(d_coef), d_plane, stride, nblocks, nullptr, d_tx_types, uniform_type, blocks_per_row };
  { ProfScope ps(ctx, AV1MI_K_INV_TXFM); HIP_TRY(ctx, av1mi::launch_inv_txfm(tx_size, L, bd, ctx->stream)); }
  return AV1MI_OK;
}
int av1mi_inv_txfm_add_list(av1mi_ctx *ctx, int tx_size, const int32_t *d_coef, void *d_plane, int stride, int bd,
                            const av1mi_txb *d_list, int nblocks) {
  BIND(ctx);
  if (int rc = check_tx_launch(ctx, tx_size, d_coef, d_plane, stride, nblocks)) return rc;
  if (int rc = check_bd(ctx, bd)) return rc;
  if (!d_list) return fail(ctx, AV1MI_E_INVAL, "null block list");
  av1mi::TxLaunch L = { const_cast<int32_t *>(d_coef), d_plane, stride, nblocks, d_list, nullptr, 0, 1 };
  { ProfScope ps(ctx, AV1MI_K_INV_TXFM); HIP_TRY(ctx, av1mi::launch_inv_txfm(tx_size, L, bd, ctx->stream)); }
  return AV1MI_OK;
}
int av1mi_fwd_txfm_grid(av1mi_ctx *ctx, int tx_size, const int16_t *d_resid, int stride, int32_t *d_coef,
                        int blocks_per_row, int nblocks, const uint8_t *d_tx_types, int uniform_type) {
  BIND(ctx);
  if (int rc = check_tx_launch(ctx, tx_size, d_coef, d_resid, stride, nblocks)) return rc;
  if (blocks_per_row <= 0) return fail(ctx, AV1MI_E_INVAL, "blocks_per_row %d <= 0", blocks_per_row);
  if (!d_tx_types && !tx_valid(tx_size, uniform_type))
    return fail(ctx, AV1MI_E_INVAL, "tx_type %d is not defined for tx_size %d", uniform_type, tx_size);
  av1mi::TxLaunch L = { d_coef, const_cast<int16_t *>(d_resid), stride, nblocks, nullptr, d_tx_types, uniform_type, blocks_per_row };
  { ProfScope ps(ctx, AV1MI_K_FWD_TXFM); HIP_TRY(ctx, av1mi::launch_fwd_txfm(tx_size, L, ctx->stream)); }
  return AV1MI_OK;
}
int av1mi_fwd_txfm_list(av1mi_ctx *ctx, int tx_size, const int16_t *d_resid, int stride, int32_t *d_coef,
                        const av1mi_txb *d_list, int nblocks) {
  BIND(ctx);
  if (int rc = check_tx_launch(ctx, tx_size, d_coef, d_resid, stride, nblocks)) return rc;
  if (!d_list) return fail(ctx, AV1MI_E_INVAL, "null block list");
  av1mi::TxLaunch L = { d_coef, const_cast<int16_t *>(d_resid), stride, nblocks, d_list, nullptr, 0, 1 };
  { ProfScope ps(ctx, AV1MI_K_FWD_TXFM); HIP_TRY(ctx, av1mi::launch_fwd_txfm(tx_size, L, ctx->stream)); }
  return AV1MI_OK;
}

int av1mi_intra_pred_list(av1mi_ctx *ctx, int tx_size, const void *d_ref, int ref_stride, void *d_dst, int dst_stride,
                          int bd, const av1mi_intra_blk *d_list, int nblocks) {
  BIND(ctx);
  if (tx_size < 0 || tx_size >= AV1MI_TX_SIZES_ALL) return fail(ctx, AV1MI_E_INVAL, "tx_size %d out of range", tx_size);
  if (!d_ref || !d_dst || !d_list) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  if (int rc = check_bd(ctx, bd)) return rc;
  if (nblocks < 0 || ref_stride <= 0 || dst_stride <= 0 || (dst_stride & 3))
    return fail(ctx, AV1MI_E_INVAL, "bad geometry (nblocks %d, strides %d/%d)", nblocks, ref_stride, dst_stride);
  if ((uintptr_t)d_dst & 7) return fail(ctx, AV1MI_E_INVAL, "misaligned device pointer");
  av1mi::IntraLaunch L = { d_ref, d_dst, ref_stride, dst_stride, bd, nblocks, d_list };
  { ProfScope ps(ctx, AV1MI_K_INTRA_PRED); HIP_TRY(ctx, av1mi::launch_intra_pred(tx_size, L, ctx->stream)); }
  return AV1MI_OK;
}

int av1mi_cfl_pred_list(av1mi_ctx *ctx, int tx_size, const void *d_luma, int luma_stride, void *d_dst, int dst_stride, int bd,
                        const av1mi_cfl_blk *d_list, int nblocks) {
  BIND(ctx);
  if (int rc = check_bd(ctx, bd)) return rc;
  if (tx_size < 0 || tx_size >= AV1MI_TX_SIZES_ALL || av1mi::tx_width(tx_size) > 32 || av1mi::tx_height(tx_size) > 32)
    return fail(ctx, AV1MI_E_INVAL, "chroma-from-luma is defined for blocks up to 32x32 (tx_size %d)", tx_size);
  if (nblocks < 0) return fail(ctx, AV1MI_E_INVAL, "nblocks %d < 0", nblocks);
  if (nblocks == 0) return AV1MI_OK;
  if (!d_luma || !d_dst || !d_list) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  if (luma_stride <= 0 || dst_stride <= 0 || (dst_stride & 3)) return fail(ctx, AV1MI_E_INVAL, "bad strides %d/%d", luma_stride, dst_stride);
  av1mi::CflLaunch L;
  L.luma = d_luma; L.dst = d_dst; L.luma_stride = luma_stride; L.dst_stride = dst_stride; L.bd = bd; L.nblocks = nblocks; L.blocks = d_list;
  { ProfScope ps(ctx, AV1MI_K_INTRA_PRED); HIP_TRY(ctx, av1mi::launch_cfl_pred(tx_size, L, ctx->stream)); }
  return AV1MI_OK;
}

int av1mi_mc_list(av1mi_ctx *ctx, int size_id, const void *d_ref, int ref_stride, int plane_w, int plane_h, void *d_dst,
                  int dst_stride, int bd, const av1mi_mc_blk *d_list, int nblocks) {
  BIND(ctx);
  if (size_id < 0 || size_id >= AV1MI_TX_SIZES_ALL) return fail(ctx, AV1MI_E_INVAL, "size_id %d out of range", size_id);
  if (!d_ref || !d_dst || !d_list || d_ref == d_dst) return fail(ctx, AV1MI_E_INVAL, "null or aliased device pointer");
  if (int rc = check_bd(ctx, bd)) return rc;
  if (nblocks < 0 || plane_w <= 0 || plane_h <= 0 || ref_stride < plane_w || dst_stride <= 0 || (dst_stride & 3))
    return fail(ctx, AV1MI_E_INVAL, "bad geometry");
  if ((uintptr_t)d_dst & 7) return fail(ctx, AV1MI_E_INVAL, "misaligned device pointer");
  av1mi::McLaunch L = { d_ref, d_dst, ref_stride, dst_stride, plane_w, plane_h, bd, nblocks, d_list };
  { ProfScope ps(ctx, AV1MI_K_MC); HIP_TRY(ctx, av1mi::launch_mc(size_id, L, ctx->stream)); }
  return AV1MI_OK;
}

int av1mi_deblock_frames(av1mi_ctx *ctx, const void *d_src, int src_stride, void *d_dst, int dst_stride, int w, int h,
                         int bd, int is_chroma, const uint32_t *d_mi, int mi_stride, size_t mi_frame_stride, int sharpness,
                         int nframes) {
  BIND(ctx);
  if (!d_src || !d_dst || !d_mi || d_src == d_dst) return fail(ctx, AV1MI_E_INVAL, "null or aliased device pointer");
  if (int rc = check_bd(ctx, bd)) return rc;
  if (w <= 0 || h <= 0 || (w & 3) || (h & 3) || src_stride < w || dst_stride < w || (src_stride & 3) || (dst_stride & 3) ||
      mi_stride < w / 4)
    return fail(ctx, AV1MI_E_INVAL, "bad plane geometry %dx%d strides %d/%d/%d", w, h, src_stride, dst_stride, mi_stride);
  if (sharpness < 0 || sharpness > 7) return fail(ctx, AV1MI_E_INVAL, "sharpness %d out of range", sharpness);
  if (int rc = check_nframes(ctx, nframes)) return rc;
  if (((uintptr_t)d_src & 7) || ((uintptr_t)d_dst & 7)) return fail(ctx, AV1MI_E_INVAL, "misaligned device pointer");
  if (nframes == 0) return AV1MI_OK;
  av1mi::DeblockLaunch L = { d_src, d_dst, src_stride, dst_stride, w, h, bd, is_chroma ? 1 : 0, d_mi, mi_stride, sharpness,
                             nframes, mi_frame_stride };
  { ProfScope ps(ctx, AV1MI_K_DEBLOCK); HIP_TRY(ctx, av1mi::launch_deblock(L, ctx->stream)); }
  return AV1MI_OK;
}
int av1mi_deblock_plane(av1mi_ctx *ctx, const void *d_src, int src_stride, void *d_dst, int dst_stride, int w, int h,
                        int bd, int is_chroma, const uint32_t *d_mi, int mi_stride, int sharpness) {
  return av1mi_deblock_frames(ctx, d_src, src_stride, d_dst, dst_stride, w, h, bd, is_chroma, d_mi, mi_stride, 0, sharpness, 1);
}

int av1mi_cdef_frames(av1mi_ctx *ctx, const av1mi_cdef_job *j) {
  BIND(ctx);
  if (!j) return fail(ctx, AV1MI_E_INVAL, "null job");
  if (int rc = check_bd(ctx, j->bit_depth)) return rc;
  if (int rc = check_frame420(ctx, j->width, j->height, j->stride_y, j->stride_uv, false)) return rc;
  if (j->damping < 3 || j->damping > 6 || j->nframes < 0 || j->nframes > 65535) return fail(ctx, AV1MI_E_INVAL, "bad damping/nframes");
  if (int rc = check_pointers(ctx, "device", 8, { j->d_src_y, j->d_src_u, j->d_src_v, j->d_dst_y, j->d_dst_u, j->d_dst_v })) return rc;
  if (int rc = check_pointers(ctx, "map", 1, { j->d_sb_strength, j->d_skip8 })) return rc;
  if (j->d_src_y == j->d_dst_y || j->d_src_u == j->d_dst_u || j->d_src_v == j->d_dst_v) return fail(ctx, AV1MI_E_INVAL, "CDEF cannot run in place");
  if (j->nframes == 0) return AV1MI_OK;
  av1mi::CdefLaunch L;
  planes3(L.src, j->d_src_y, j->d_src_u, j->d_src_v); planes3(L.dst, j->d_dst_y, j->d_dst_u, j->d_dst_v);
  L.w = j->width; L.h = j->height; L.stride_y = j->stride_y; L.stride_uv = j->stride_uv; L.bd = j->bit_depth; L.damping = j->damping;
  L.nframes = j->nframes; L.sb_strength = j->d_sb_strength; L.sb_frame_stride = j->sb_frame_stride;
  L.skip8 = j->d_skip8; L.skip_frame_stride = j->skip_frame_stride;
  { ProfScope ps(ctx, AV1MI_K_CDEF); HIP_TRY(ctx, av1mi::launch_cdef(L, ctx->stream)); }
  return AV1MI_OK;
}

// ---- CDEF search
int av1mi_cdef_search_sets(const av1mi_frame_params *p, int bits, uint8_t y[8], uint8_t uv[8]) {
  if (!p || !y || !uv || bits < 1 || bits > 3) return AV1MI_E_INVAL;
  auto dbl = [](int x) { return std::min(15, std::max(1, 2 * x)); };
  auto up = [](int x) { return std::min(3, x + 1); };
  auto sets = [&](int v, uint8_t out[8]) {
    const int P = v >> 2, S = v & 3;
    const int pri[8] = { P, 0, P >> 1, dbl(P), P, P, dbl(P), dbl(dbl(P)) }, sec[8] = { S, 0, S, S, up(S), 0, up(S), up(S) };
    for (int c = 0; c < 8; c++) out[c] = c < (1 << bits) ? (uint8_t)((pri[c] << 2) | sec[c]) : (uint8_t)0;
  };
  sets(p->cdef_y, y); sets(p->cdef_uv, uv);
  return AV1MI_OK;
}
size_t av1mi_cdef_search_table_bytes(int width, int height, int nframes) {
  if (width <= 0 || height <= 0 || nframes <= 0) return 0;
  return (size_t)nframes * av1mi::sb_count(width, height) * 8 * sizeof(uint64_t);
}
int av1mi_cdef_search(av1mi_ctx *ctx, const av1mi_cdef_search_job *j) {
  BIND(ctx);
  if (!j) return fail(ctx, AV1MI_E_INVAL, "null job");
  if (int rc = check_bd(ctx, j->bit_depth)) return rc;
  if (int rc = check_frame420(ctx, j->width, j->height, j->stride_y, j->stride_uv, true)) return rc;
  if (int rc = check_nframes(ctx, j->nframes)) return rc;
  int tw, th;
  if (int rc = check_true_size(ctx, j->width, j->height, j->true_width, j->true_height, &tw, &th)) return rc;
  if (!j->params || j->bits < 1 || j->bits > 3) return fail(ctx, AV1MI_E_INVAL, "CDEF search: bits %d outside 1 .. 3, or no frame parameters", j->bits);
  if (j->params->cdef_damping < 3 || j->params->cdef_damping > 6) return fail(ctx, AV1MI_E_INVAL, "bad damping/nframes");
  if (int rc = check_pointers(ctx, "device", 8, { j->d_src_y, j->d_src_u, j->d_src_v, j->d_orig_y, j->d_orig_u, j->d_orig_v, j->d_sse })) return rc;
  if (int rc = check_pointers(ctx, "map", 1, { j->d_skip8, j->d_idx })) return rc;
  if (int rc = check_pointers(ctx, "map", 4, { j->d_strength })) return rc;
  if (j->nframes == 0) return AV1MI_OK;
  av1mi::CdefSearchLaunch L;
  memset(&L, 0, sizeof(L));
  planes3(L.src, j->d_src_y, j->d_src_u, j->d_src_v); planes3(L.orig, j->d_orig_y, j->d_orig_u, j->d_orig_v);
  L.w = j->width; L.h = j->height; L.tw = tw; L.th = th; L.stride_y = j->stride_y; L.stride_uv = j->stride_uv; L.bd = j->bit_depth;
  L.damping = j->params->cdef_damping; L.nframes = j->nframes; L.ncand = 1 << j->bits;
  L.skip8 = j->d_skip8; L.skip_frame_stride = j->skip_frame_stride;
  uint8_t y[8], uv[8];
  av1mi_cdef_search_sets(j->params, j->bits, y, uv);
  for (int c = 0; c < 8; c++) L.sets[c] = (uint32_t)(y[c] >> 2) | (uint32_t)(y[c] & 3) << 8 | (uint32_t)(uv[c] >> 2) << 16 | (uint32_t)(uv[c] & 3) << 24;
  L.sse = (unsigned long long *)j->d_sse; L.strength = j->d_strength; L.idx = j->d_idx;
  { ProfScope ps(ctx, AV1MI_K_CDEF); HIP_TRY(ctx, av1mi::launch_cdef_search(L, ctx->stream)); }
  return AV1MI_OK;
}

// ---- deblocking search
// null = fine, else why the policy levels P cannot be searched
static const char *lf_search_error(const av1mi_frame_params *p) {
  if (!p) return "no frame parameters";
  for (int i = 0; i < 4; i++) if (p->lf_level[i] < 0 || p->lf_level[i] > 63) return "a policy level outside 0 .. 63";
  if (p->lf_level[2] != p->lf_level[3]) return "the policy's U and V levels differ (the search gives both chroma planes one level)";
  if (p->lf_level[0] == 0 && p->lf_level[1] == 0 && p->lf_level[2] != 0) return "policy luma levels 0 with a chroma level: the frame header could not carry the chroma level";
  return nullptr;
}
int av1mi_lf_search_levels(const av1mi_frame_params *p, int c, int out[4]) {
  if (!out || c < 0 || c >= AV1MI_LF_SEARCH_CANDIDATES || lf_search_error(p)) return AV1MI_E_INVAL;
  static const int m[AV1MI_LF_SEARCH_CANDIDATES] = { 4, 0, 2, 3, 5, 6, 8, 12 };
  for (int i = 0; i < 4; i++) {
    const int L = p->lf_level[i], lo = i < 2 ? 1 : 0;
    out[i] = c == 0 ? L : std::min(63, std::max(lo, (L * m[c] + 2) >> 2));
  }
  return AV1MI_OK;
}
size_t av1mi_lf_search_scratch_bytes(int width, int height, int nframes) {
  if (width <= 0 || height <= 0 || nframes <= 0) return 0;
  return (size_t)nframes * av1mi::sb_count(width, height) * 2 * AV1MI_LF_SEARCH_CANDIDATES * sizeof(uint64_t);
}
int av1mi_lf_search(av1mi_ctx *ctx, const av1mi_lf_search_job *j) {
  BIND(ctx);
  if (!j) return fail(ctx, AV1MI_E_INVAL, "null job");
  if (int rc = check_bd(ctx, j->bit_depth)) return rc;
  if (int rc = check_frame420(ctx, j->width, j->height, j->stride_y, j->stride_uv, true)) return rc;
  if (int rc = check_nframes(ctx, j->nframes)) return rc;
  if (j->mi_stride_y < j->width / 4 || j->mi_stride_uv < j->width / 8)
    return fail(ctx, AV1MI_E_INVAL, "bad plane geometry %dx%d strides %d/%d/%d", j->width, j->height, j->stride_y, j->mi_stride_y, j->mi_stride_uv);
  int tw, th;
  if (int rc = check_true_size(ctx, j->width, j->height, j->true_width, j->true_height, &tw, &th)) return rc;
  if (const char *why = lf_search_error(j->params)) return fail(ctx, AV1MI_E_INVAL, "deblocking search: %s", why);
  if (j->params->lf_sharpness < 0 || j->params->lf_sharpness > 7) return fail(ctx, AV1MI_E_INVAL, "sharpness %d out of range", j->params->lf_sharpness);
  if (int rc = check_pointers(ctx, "device", 8, { j->d_rec_y, j->d_rec_u, j->d_rec_v, j->d_orig_y, j->d_orig_u, j->d_orig_v, j->d_scratch, j->d_sse })) return rc;
  if (int rc = check_pointers(ctx, "map", 1, { j->d_mi_y, j->d_mi_uv, j->d_choice })) return rc;
  if (int rc = check_pointers(ctx, "map", 4, { j->d_levels })) return rc;
  if (!j->d_mi_y_out != !j->d_mi_uv_out) return fail(ctx, AV1MI_E_INVAL, "deblocking search: give both output maps or neither");
  if (j->d_mi_y_out == j->d_mi_y || j->d_mi_uv_out == j->d_mi_uv) return fail(ctx, AV1MI_E_INVAL, "null or aliased device pointer");
  if (j->nframes == 0) return AV1MI_OK;
  av1mi::LfSearchLaunch L;
  memset(&L, 0, sizeof(L));
  planes3(L.rec, j->d_rec_y, j->d_rec_u, j->d_rec_v); planes3(L.orig, j->d_orig_y, j->d_orig_u, j->d_orig_v);
  L.w = j->width; L.h = j->height; L.tw = tw; L.th = th; L.stride_y = j->stride_y; L.stride_uv = j->stride_uv; L.bd = j->bit_depth;
  L.sharpness = j->params->lf_sharpness; L.nframes = j->nframes;
  L.mi_y = j->d_mi_y; L.mi_uv = j->d_mi_uv; L.mi_stride_y = j->mi_stride_y; L.mi_stride_uv = j->mi_stride_uv;
  L.mi_frame_stride_y = j->mi_frame_stride_y; L.mi_frame_stride_uv = j->mi_frame_stride_uv;
  for (int c = 0; c < AV1MI_LF_SEARCH_CANDIDATES; c++) {
    int lv[4];
    av1mi_lf_search_levels(j->params, c, lv);
    for (int i = 0; i < 4; i++) L.lvl[c][i] = (uint8_t)lv[i];
    // the lowest candidate with the same levels: luma = the pair (vertical, horizontal), chroma = the one level
    for (int g = 0; g < 2; g++) {
      int first = c;
      for (int e = c - 1; e >= 0; e--) if (g == 0 ? (L.lvl[e][0] == L.lvl[c][0] && L.lvl[e][1] == L.lvl[c][1]) : L.lvl[e][2] == L.lvl[c][2]) first = e;
      L.first[g][c] = (uint8_t)first;
    }
  }
  L.table = (unsigned long long *)j->d_scratch; L.sse = (unsigned long long *)j->d_sse; L.choice = j->d_choice; L.levels = j->d_levels;
  ProfScope ps(ctx, AV1MI_K_DEBLOCK);
  HIP_TRY(ctx, av1mi::launch_lf_search(L, ctx->stream));
  HIP_TRY(ctx, av1mi::launch_lf_pick(L, ctx->stream));
  if (j->d_mi_y_out) {
    av1mi::LevelsFramesLaunch M;
    memset(&M, 0, sizeof(M));
    M.levels = j->d_levels; M.nframes = j->nframes;
    M.base[0] = j->d_mi_y; M.out[0] = j->d_mi_y_out; M.cols[0] = j->width / 4; M.rows[0] = j->height / 4; M.stride[0] = j->mi_stride_y; M.frame_stride[0] = j->mi_frame_stride_y;
    M.base[1] = j->d_mi_uv; M.out[1] = j->d_mi_uv_out; M.cols[1] = j->width / 8; M.rows[1] = j->height / 8; M.stride[1] = j->mi_stride_uv; M.frame_stride[1] = j->mi_frame_stride_uv;
    HIP_TRY(ctx, av1mi::launch_mi_levels_frames(M, ctx->stream));
  }
  return AV1MI_OK;
}

int av1mi_deblock_cdef_frames(av1mi_ctx *ctx, const av1mi_deblock_cdef_job *j) {
  BIND(ctx);
  if (!j) return fail(ctx, AV1MI_E_INVAL, "null job");
  if (int rc = check_bd(ctx, j->bit_depth)) return rc;
  if (int rc = check_frame420(ctx, j->width, j->height, j->rec_stride_y, j->rec_stride_uv, false)) return rc;
  if (int rc = check_frame420(ctx, j->width, j->height, j->dbl_stride_y, j->dbl_stride_uv, false)) return rc;
  if (int rc = check_frame420(ctx, j->width, j->height, j->dst_stride_y, j->dst_stride_uv, false)) return rc;
  if (j->damping < 3 || j->damping > 6) return fail(ctx, AV1MI_E_INVAL, "bad damping/nframes");
  if (int rc = check_nframes(ctx, j->nframes)) return rc;
  if (j->sharpness < 0 || j->sharpness > 7) return fail(ctx, AV1MI_E_INVAL, "sharpness %d out of range", j->sharpness);
  if (j->mi_stride_y < j->width / 4 || j->mi_stride_uv < j->width / 8)
    return fail(ctx, AV1MI_E_INVAL, "bad plane geometry %dx%d strides %d/%d/%d", j->width, j->height, j->rec_stride_y, j->mi_stride_y, j->mi_stride_uv);
  const void *ptrs[] = { j->d_rec_y, j->d_rec_u, j->d_rec_v, j->d_dbl_y, j->d_dbl_u, j->d_dbl_v, j->d_dst_y, j->d_dst_u, j->d_dst_v };
  if (int rc = check_pointers(ctx, "device", 8, ptrs)) return rc;
  for (int a = 0; a < 9; a++)
    for (int b = a + 1; b < 9; b++) if (ptrs[a] == ptrs[b]) return fail(ctx, AV1MI_E_INVAL, "null or aliased device pointer");
  if (int rc = check_pointers(ctx, "map", 1, { j->d_mi_y, j->d_mi_uv, j->d_sb_strength, j->d_skip8 })) return rc;
  if (j->nframes == 0) return AV1MI_OK;
  av1mi::DeblockCdefLaunch L;
  planes3(L.rec, j->d_rec_y, j->d_rec_u, j->d_rec_v); planes3(L.dbl, j->d_dbl_y, j->d_dbl_u, j->d_dbl_v); planes3(L.dst, j->d_dst_y, j->d_dst_u, j->d_dst_v);
  L.w = j->width; L.h = j->height; L.rec_stride_y = j->rec_stride_y; L.rec_stride_uv = j->rec_stride_uv; L.dbl_stride_y = j->dbl_stride_y;
  L.dbl_stride_uv = j->dbl_stride_uv; L.dst_stride_y = j->dst_stride_y; L.dst_stride_uv = j->dst_stride_uv;
  L.bd = j->bit_depth; L.damping = j->damping; L.sharpness = j->sharpness; L.nframes = j->nframes;
  L.mi_y = j->d_mi_y; L.mi_uv = j->d_mi_uv; L.mi_stride_y = j->mi_stride_y; L.mi_stride_uv = j->mi_stride_uv;
  L.mi_frame_stride_y = j->mi_frame_stride_y; L.mi_frame_stride_uv = j->mi_frame_stride_uv;
  L.sb_strength = j->d_sb_strength; L.sb_frame_stride = j->sb_frame_stride; L.skip8 = j->d_skip8; L.skip_frame_stride = j->skip_frame_stride;
  // (the CDEF kind: the launch takes that kernel's place in every table)
  { ProfScope ps(ctx, AV1MI_K_CDEF); HIP_TRY(ctx, av1mi::launch_deblock_cdef(L, ctx->stream)); }
  return AV1MI_OK;
}

int av1mi_lr_frames(av1mi_ctx *ctx, const void *d_cdef, const void *d_deblocked, void *d_out, int stride, int w, int h,
                    int bd, int subsampled, int unit_size, const int8_t *d_units, size_t unit_frame_stride, int nframes) {
  BIND(ctx);
  av1mi::LrLaunch L;      // (every member by name; the decision's and the two-pass form's stay null / 0)
  L.cdef = d_cdef; L.dbl = d_deblocked; L.out = d_out; L.stride = stride; L.w = w; L.h = h; L.bd = bd; L.ss = subsampled ? 1 : 0;
  L.unit_size = unit_size; L.units = d_units; L.unit_frame_stride = unit_frame_stride; L.nframes = nframes;
  if (int rc = check_lr_plane(ctx, L)) return rc;
  if (int rc = check_nframes(ctx, nframes)) return rc;
  if (nframes == 0) return AV1MI_OK;
  { ProfScope ps(ctx, AV1MI_K_LR); HIP_TRY(ctx, av1mi::launch_lr(L, ctx->stream)); }
  return AV1MI_OK;
}

size_t av1mi_lr_decide_scratch_bytes(int h, int subsampled, int nframes) { return (size_t)(nframes > 0 ? nframes : 0) * av1mi::LrGeom::stripes_of(h, subsampled ? 1 : 0) * 16; }
int av1mi_lr_frames_decide(av1mi_ctx *ctx, const void *d_cdef, const void *d_deblocked, void *d_out, int stride, int w, int h, int bd, int subsampled,
                           int unit_size, const int8_t *d_units, size_t unit_frame_stride, int nframes, const void *d_orig, void *d_scratch, uint8_t *d_on,
                           int on_stride) {
  BIND(ctx);
  if (!d_orig || !d_scratch || !d_on) return fail(ctx, AV1MI_E_INVAL, "null or aliased device pointer");
  av1mi::LrLaunch L;
  L.cdef = d_cdef; L.dbl = d_deblocked; L.out = d_out; L.stride = stride; L.w = w; L.h = h; L.bd = bd; L.ss = subsampled ? 1 : 0;
  L.unit_size = unit_size; L.units = d_units; L.unit_frame_stride = unit_frame_stride; L.nframes = nframes;
  if (int rc = check_lr_plane(ctx, L)) return rc;
  if (nframes < 0 || nframes > 65535 || on_stride < 1) return fail(ctx, AV1MI_E_INVAL, "nframes %d / on_stride %d out of range", nframes, on_stride);
  if (nframes == 0) return AV1MI_OK;
  HIP_TRY(ctx, hipMemsetAsync(d_scratch, 0, av1mi_lr_decide_scratch_bytes(h, subsampled, nframes), ctx->stream));
  L.orig = d_orig; L.sse = (unsigned long long *)d_scratch; L.sse_stripes = av1mi::LrGeom::stripes_of(h, L.ss);
  { ProfScope ps(ctx, AV1MI_K_LR); HIP_TRY(ctx, av1mi::launch_lr(L, ctx->stream)); }
  HIP_TRY(ctx, av1mi::launch_lr_decide(L.sse, av1mi::LrGeom(L), av1mi::LrGeom(L), 1, d_on, on_stride, false, ctx->stream));      // (not cleared: the caller keeps the sums)
  return AV1MI_OK;
}

size_t av1mi_lr_yuv_decide_scratch_bytes(int h, int nframes) { return av1mi_lr_decide_scratch_bytes(h, 0, nframes) + 2 * av1mi_lr_decide_scratch_bytes(h / 2, 1, nframes); }
int av1mi_lr_yuv_decide(av1mi_ctx *ctx, const av1mi_lr_decide_job *j) { return av1mi::lr_yuv_decide_with(ctx, j, false); }

// ---- restoration search
int av1mi_lr_search_units(int width, int height, int unit_size) {
  if (width <= 0 || height <= 0 || unit_size <= 0) return 0;
  const av1mi::LrGeom gy(width, height, 0, unit_size, 1), gc(width / 2, height / 2, 1, unit_size, 1);
  return gy.unit_rows * gy.unit_cols + 2 * gc.unit_rows * gc.unit_cols;
}
size_t av1mi_lr_search_scratch_bytes(int width, int height, int unit_size, int nframes) {
  const size_t b = (size_t)(nframes > 0 ? nframes : 0) * av1mi_lr_search_units(width, height, unit_size) * AV1MI_LR_SEARCH_CANDIDATES * 8;
  return (b + 15) & ~(size_t)15;
}
int av1mi_lr_search_candidate(int chroma, int c, int8_t record[8]) {
  if (c < 0 || c >= AV1MI_LR_SEARCH_CANDIDATES || !record) return AV1MI_E_INVAL;
  av1mi::lr_search_record(chroma, c, record);
  return AV1MI_OK;
}
int av1mi_lr_search_bits(int chroma, int c) { return c < 0 || c >= AV1MI_LR_SEARCH_CANDIDATES ? -1 : av1mi::lr_search_bits(chroma, c); }
long long av1mi_lr_search_lambda(int qindex, int bit_depth) {
  const long long q = av1mi_dc_q(qindex, bit_depth);
  return (3 * q * q) >> 7;
}
int av1mi_lr_search(av1mi_ctx *ctx, const av1mi_lr_search_job *j) {
  BIND(ctx);
  if (!j) return fail(ctx, AV1MI_E_INVAL, "null job");
  const void *cdef[3] = { j->d_cdef_y, j->d_cdef_u, j->d_cdef_v }, *dbl[3] = { j->d_dbl_y, j->d_dbl_u, j->d_dbl_v }, *orig[3] = { j->d_orig_y, j->d_orig_u, j->d_orig_v };
  int8_t *units[3] = { j->d_units_y, j->d_units_u, j->d_units_v };
  for (int p = 0; p < 3; p++) if (!cdef[p] || !dbl[p] || !orig[p] || !units[p]) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  if (!j->d_scratch || !j->d_choice) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  if (((uintptr_t)j->d_scratch & 15) || ((uintptr_t)units[0] & 7) || ((uintptr_t)units[1] & 7) || ((uintptr_t)units[2] & 7)) return fail(ctx, AV1MI_E_INVAL, "misaligned device pointer");
  if (int rc = check_bd(ctx, j->bit_depth)) return rc;
  if (j->width <= 0 || j->height <= 0 || (j->width & 1) || (j->height & 1) || j->width > 16384 || j->height > 16384 || j->stride_y < j->width || j->stride_uv < j->width / 2)
    return fail(ctx, AV1MI_E_INVAL, "bad frame geometry %dx%d strides %d/%d", j->width, j->height, j->stride_y, j->stride_uv);
  if (j->unit_size != 64) return fail(ctx, AV1MI_E_INVAL, "restoration search: unit size %d not supported (64)", j->unit_size);
  if (j->qindex < 0 || j->qindex > 255) return fail(ctx, AV1MI_E_INVAL, "qindex %d out of range", j->qindex);
  if (int rc = check_nframes(ctx, j->nframes)) return rc;
  if (j->nframes == 0) return AV1MI_OK;
  const av1mi::LrGeom gy(j->width, j->height, 0, 64, j->nframes), gc(j->width / 2, j->height / 2, 1, 64, j->nframes);
  av1mi::LrSearchLaunch S;
  memset(&S, 0, sizeof(S));
  for (int p = 0; p < 3; p++) {
    S.cdef[p] = cdef[p]; S.dbl[p] = dbl[p]; S.orig[p] = orig[p]; S.units[p] = units[p];
    S.stride[p] = p ? j->stride_uv : j->stride_y; S.w[p] = (p ? gc : gy).w; S.h[p] = (p ? gc : gy).h;
  }
  S.bd = j->bit_depth; S.unit_size = 64; S.nframes = j->nframes; S.sums = (unsigned long long *)j->d_scratch; S.choice = j->d_choice;
  const unsigned ny = (unsigned)(gy.unit_rows * gy.unit_cols), nc = (unsigned)(gc.unit_rows * gc.unit_cols);
  S.unit_first[0] = 0; S.unit_first[1] = ny; S.unit_first[2] = ny + nc; S.units_frame = ny + 2 * nc;
  S.lambda = av1mi_lr_search_lambda(j->qindex, j->bit_depth);
  av1mi::lr_search_tables(&S);
  { ProfScope ps(ctx, AV1MI_K_LR); HIP_TRY(ctx, av1mi::launch_zero16(j->d_scratch, av1mi_lr_search_scratch_bytes(j->width, j->height, 64, j->nframes), ctx->stream)); }
  { ProfScope ps(ctx, AV1MI_K_LR); HIP_TRY(ctx, av1mi::launch_lr_search(S, ctx->stream)); }
  { ProfScope ps(ctx, AV1MI_K_LR); HIP_TRY(ctx, av1mi::launch_lr_pick(S, ctx->stream)); }
  return AV1MI_OK;
}

}  // extern "C"

// THE RULE OF THE SCRATCH'S ZEROES, in this one place.  Pass 1 adds into the sums, so they must be zero when it starts; the decision
// kernel, their only reader, writes zero back over every sum it has read (k_lr_decide3), so a call leaves its scratch as clean as it
// must find it.  scratch_clean is the caller's promise that the scratch is in that state: zeroed once when it was allocated and since
// then written by calls of this function with the same height and frame count only (the GOP session).  Without the promise — the C
// entry point, whose caller may hand over any memory — the zeroing launch runs first, as it always did.
int av1mi::lr_yuv_decide_with(av1mi_ctx *ctx, const av1mi_lr_decide_job *j, bool scratch_clean) {
  BIND(ctx);
  if (!j) return fail(ctx, AV1MI_E_INVAL, "null job");
  const void *cdef[3] = { j->d_cdef_y, j->d_cdef_u, j->d_cdef_v }, *dbl[3] = { j->d_dbl_y, j->d_dbl_u, j->d_dbl_v }, *orig[3] = { j->d_orig_y, j->d_orig_u, j->d_orig_v };
  void *out[3] = { j->d_out_y, j->d_out_u, j->d_out_v };
  for (int p = 0; p < 3; p++) if (!cdef[p] || !dbl[p] || !out[p] || !orig[p]) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  if (!j->d_units_y || !j->d_units_uv || !j->d_scratch || !j->d_on) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  if ((uintptr_t)j->d_scratch & 15) return fail(ctx, AV1MI_E_INVAL, "misaligned scratch");
  if (int rc = check_bd(ctx, j->bit_depth)) return rc;
  if (j->width <= 0 || j->height <= 0 || (j->width & 1) || (j->height & 1) || j->stride_y < j->width || j->stride_uv < j->width / 2)
    return fail(ctx, AV1MI_E_INVAL, "bad frame geometry %dx%d strides %d/%d", j->width, j->height, j->stride_y, j->stride_uv);
  if (int rc = check_lr_unit(ctx, j->unit_size, 0)) return rc;
  if (int rc = check_nframes(ctx, j->nframes)) return rc;
  if (j->nframes == 0) return AV1MI_OK;
  const int n = j->nframes;
  unsigned long long *sse = (unsigned long long *)j->d_scratch;
  if (!scratch_clean) HIP_TRY(ctx, av1mi::launch_zero16(sse, av1mi_lr_yuv_decide_scratch_bytes(j->height, n), ctx->stream));
  for (int p = 0; p < 3; p++) if (out[p] == cdef[p] || out[p] == dbl[p]) return fail(ctx, AV1MI_E_INVAL, "aliased device pointer");
  const av1mi::LrGeom gy(j->width, j->height, 0, j->unit_size, n), gc(j->width / 2, j->height / 2, 1, j->unit_size, n);
  av1mi::LrYuvLaunch Y;
  for (int p = 0; p < 3; p++) {
    av1mi::LrLaunch &L = Y.plane[p];
    L.cdef = cdef[p]; L.dbl = dbl[p]; L.out = out[p]; L.orig = orig[p]; L.bd = j->bit_depth; L.ss = p ? 1 : 0; L.unit_size = j->unit_size; L.nframes = n;
    L.stride = p ? j->stride_uv : j->stride_y; L.w = (p ? gc : gy).w; L.h = (p ? gc : gy).h; L.sse_stripes = (p ? gc : gy).stripes;
    L.units = p ? j->d_units_uv : j->d_units_y; L.unit_frame_stride = p ? j->unit_frame_stride_uv : j->unit_frame_stride_y;
    if (p == 2 && j->d_units_v) { L.units = j->d_units_v; L.unit_frame_stride = j->unit_frame_stride_v; }
    L.sse = sse + 2 * av1mi::lr_first_pair(gy, gc, p); L.keep = j->d_on + p; L.keep_stride = 3; L.no_sgr = j->no_self_guided_units != 0;
  }
  // pass 1: the tiles the decision's sums run over (an eighth of a large plane); the decision; pass 2: the other tiles of the frames
  // that keep their restoration — a plane that is switched off costs an eighth of its restoration.  One launch per pass: the three
  // planes' grids end to end (launch_lr_yuv)
  for (int pass = 1; pass <= 2; pass++) {
    for (int p = 0; p < 3; p++) Y.plane[p].pass = pass;
    { ProfScope ps(ctx, AV1MI_K_LR); HIP_TRY(ctx, av1mi::launch_lr_yuv(Y, ctx->stream)); }
    if (pass == 1) HIP_TRY(ctx, av1mi::launch_lr_decide(sse, gy, gc, 3, j->d_on, 3, true, ctx->stream));
  }
  return AV1MI_OK;
}

extern "C" {

int av1mi_extend_frames(av1mi_ctx *ctx, void *d_plane, int stride, int w, int h, int visible_w, int visible_h, int bd, int nframes) {
  BIND(ctx);
  if (!d_plane) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  if (int rc = check_bd(ctx, bd)) return rc;
  if (w <= 0 || h <= 0 || stride < w || visible_w <= 0 || visible_h <= 0 || visible_w > w || visible_h > h)
    return fail(ctx, AV1MI_E_INVAL, "bad plane geometry %dx%d (visible %dx%d) stride %d", w, h, visible_w, visible_h, stride);
  if (int rc = check_nframes(ctx, nframes)) return rc;
  HIP_TRY(ctx, av1mi::launch_extend(d_plane, stride, w, h, visible_w, visible_h, bd, nframes, ctx->stream));
  return AV1MI_OK;
}

int av1mi_input_convert(av1mi_ctx *ctx, int format, int bit_depth, int width, int rows, const void *d_in0, const void *d_in1, const void *d_in2,
                        void *d_y, void *d_u, void *d_v) {
  BIND(ctx);
  if (format == AV1MI_INPUT_PLANAR || !av1mi_input_plane_bytes(format, bit_depth, 0, width, rows))
    return fail(ctx, AV1MI_E_INVAL, "input format %d with bit depth %d, %d x %d rows: nothing to convert or not a valid combination", format, bit_depth, width, rows);
  const bool semi = format != AV1MI_INPUT_PACKED10;      // P010 / NV12: two input planes
  if (semi) d_in2 = d_in1;
  const void *ptrs[] = { d_in0, d_in1, d_in2, d_y, d_u, d_v };
  for (const void *p : ptrs) if (!p || ((uintptr_t)p & 15)) return fail(ctx, AV1MI_E_INVAL, "null or misaligned device pointer (16 bytes)");
  av1mi::InputLaunch L;
  memset(&L, 0, sizeof(L));
  L.in[0] = d_in0; L.in[1] = d_in1; L.in[2] = d_in2; L.out[0] = d_y; L.out[1] = d_u; L.out[2] = d_v;
  L.ny = (size_t)width * rows; L.nc = L.ny / 4;
  ProfScope ps(ctx, AV1MI_K_INPUT);
  HIP_TRY(ctx, av1mi::launch_input_convert(format, L, ctx->stream));
  return AV1MI_OK;
}

int av1mi_chroma_convert(av1mi_ctx *ctx, int source_chroma, int source_bit_depth, int bit_depth, int width, int height, int frames,
                         const void *d_in0, const void *d_in1, const void *d_in2, void *d_y, void *d_u, void *d_v) {
  BIND(ctx);
  if (const char *why = av1mi::chroma_format_error(source_chroma, source_bit_depth, bit_depth))
    return fail(ctx, AV1MI_E_INVAL, "av1mi_chroma_convert (chroma %d, %d -> %d bits): %s", source_chroma, source_bit_depth, bit_depth, why);
  if (width < 8 || height < 8 || width > 16384 || height > 16384) return fail(ctx, AV1MI_E_INVAL, "av1mi_chroma_convert: frame %dx%d out of range (8 .. 16384)", width, height);
  if (frames < 1 || (size_t)frames * (size_t)(height + 7) > 65535u * 32u) return fail(ctx, AV1MI_E_INVAL, "frames %d out of range", frames);
  const bool luma = source_bit_depth != bit_depth, grey = source_chroma == AV1MI_CHROMA_400;
  if (!luma) { d_in0 = nullptr; d_y = nullptr; }
  if (grey) d_in1 = d_in2 = nullptr;
  const void *need[] = { luma ? d_in0 : ctx, grey ? ctx : d_in1, grey ? ctx : d_in2, luma ? d_y : ctx, d_u, d_v };
  for (const void *p : need) if (!p) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  const void *ptrs[] = { d_in0, d_in1, d_in2, d_y, d_u, d_v };
  for (const void *p : ptrs) if ((uintptr_t)p & 15) return fail(ctx, AV1MI_E_INVAL, "misaligned device pointer (16 bytes)");
  av1mi::ChromaLaunch L;
  L.in[0] = d_in0; L.in[1] = d_in1; L.in[2] = d_in2; L.out[0] = d_y; L.out[1] = d_u; L.out[2] = d_v;
  L.chroma = source_chroma; L.src_bd = source_bit_depth; L.bd = bit_depth; L.w = width; L.h = height; L.frames = frames;
  ProfScope ps(ctx, AV1MI_K_INPUT);
  HIP_TRY(ctx, av1mi::launch_chroma_convert(L, ctx->stream));
  return AV1MI_OK;
}

int av1mi_scale_planes(av1mi_ctx *ctx, int bit_depth, int src_w, int src_h, int dst_w, int dst_h, int frames, const void *const d_src[3],
                       void *const d_dst[3]) {
  BIND(ctx);
  if (int rc = check_bd(ctx, bit_depth)) return rc;
  if (const char *why = av1mi::scale_geometry_error(src_w, src_h, dst_w, dst_h)) return fail(ctx, AV1MI_E_INVAL, "%dx%d -> %dx%d: %s", src_w, src_h, dst_w, dst_h, why);
  if (frames < 1 || (size_t)frames * (size_t)((src_h > dst_h ? src_h : dst_h) + 7) > 65535u * 32u) return fail(ctx, AV1MI_E_INVAL, "frames %d out of range", frames);
  if (!d_src || !d_dst) return fail(ctx, AV1MI_E_INVAL, "null plane array");
  for (int p = 0; p < 3; p++)
    if (!d_src[p] || !d_dst[p] || (((uintptr_t)d_src[p] | (uintptr_t)d_dst[p]) & 15)) return fail(ctx, AV1MI_E_INVAL, "null or misaligned device pointer (16 bytes)");
  if (!av1mi::scale_plan_is(ctx->scale_plan, bit_depth, src_w, src_h, dst_w, dst_h)) {
    if (ctx->scale_plan) {      // a launch that still reads the old tables may be in flight
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      av1mi::scale_plan_destroy(ctx->scale_plan);
      ctx->scale_plan = nullptr;
    }
    HIP_TRY(ctx, av1mi::scale_plan_create(bit_depth, src_w, src_h, dst_w, dst_h, &ctx->scale_plan));
  }
  ProfScope ps(ctx, AV1MI_K_INPUT);
  HIP_TRY(ctx, av1mi::launch_scale(ctx->scale_plan, frames, d_src, d_dst, ctx->stream));
  return AV1MI_OK;
}

int av1mi_quality_planes(av1mi_ctx *ctx, int bit_depth, int width, int height, int frames, const void *const d_src[3], const void *const d_dec0[3],
                         const void *const d_dec1[3], const uint8_t *d_select, av1mi_quality *d_out) {
  BIND(ctx);
  if (const char *why = av1mi::quality::geometry_error(bit_depth, width, height, frames)) return fail(ctx, AV1MI_E_INVAL, "av1mi_quality_planes %dx%d: %s", width, height, why);
  if (!d_src || !d_dec0 || !d_out || (d_select && !d_dec1)) return fail(ctx, AV1MI_E_INVAL, "null pointer (d_select needs d_dec1)");
  for (int p = 0; p < 3; p++) {
    if (!d_src[p] || !d_dec0[p] || (d_dec1 && !d_dec1[p])) return fail(ctx, AV1MI_E_INVAL, "null device pointer (plane %d)", p);
    if ((((uintptr_t)d_src[p] | (uintptr_t)d_dec0[p] | (uintptr_t)(d_dec1 ? d_dec1[p] : nullptr)) & 15) || ((uintptr_t)d_out & 7))
      return fail(ctx, AV1MI_E_INVAL, "misaligned device pointer (planes 16 bytes, records 8)");
  }
  if (int rc = grow(ctx, &ctx->quality_scratch, &ctx->quality_scratch_bytes, av1mi::quality_scratch_bytes(bit_depth, width, height, frames))) return rc;
  av1mi::QualityLaunch Q;
  Q.bd = bit_depth; Q.w = width; Q.h = height; Q.frames = frames; Q.src = d_src; Q.dec0 = d_dec0; Q.dec1 = d_dec1; Q.sel = d_select;
  Q.scratch = ctx->quality_scratch; Q.out = d_out;
  ProfScope ps(ctx, AV1MI_K_QUALITY);
  HIP_TRY(ctx, av1mi::launch_quality(Q, ctx->stream));
  return AV1MI_OK;
}

int av1mi_scene_analyse(av1mi_ctx *ctx, int bit_depth, int width, int height, int frames, const void *d_luma, av1mi_scene_record *d_records) {
  BIND(ctx);
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return fail(ctx, AV1MI_E_INVAL, "av1mi_scene_analyse: bit depth %d not supported (8, 10 or 12)", bit_depth);
  if (width < 8 || height < 8 || (width & 7) || (height & 7) || width > 16384 || height > 16384)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_scene_analyse: the planes' size %dx%d must be a multiple of 8 (8 .. 16384)", width, height);
  if (frames < 1 || frames > 65535) return fail(ctx, AV1MI_E_INVAL, "av1mi_scene_analyse: frames %d out of range (1 .. 65535)", frames);
  if (!d_luma || !d_records || ((uintptr_t)d_luma & 15) || ((uintptr_t)d_records & 7)) return fail(ctx, AV1MI_E_INVAL, "av1mi_scene_analyse: null or misaligned device pointer (planes 16 bytes, records 8)");
  if (int rc = grow(ctx, &ctx->scene_scratch, &ctx->scene_scratch_bytes, av1mi::scene_layout(width, height, frames).bytes)) return rc;
  av1mi::SceneLaunch S;
  S.bd = bit_depth; S.w = width; S.h = height; S.frames = frames; S.luma = d_luma; S.scratch = ctx->scene_scratch; S.out = d_records;
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_scene(S, ctx->stream));
  return AV1MI_OK;
}

int av1mi_crop_analyse(av1mi_ctx *ctx, int bit_depth, int width, int height, int true_width, int true_height, int frames, const void *d_luma, int limit,
                       av1mi_crop_record *d_records) {
  BIND(ctx);
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return fail(ctx, AV1MI_E_INVAL, "av1mi_crop_analyse: bit depth %d not supported (8, 10 or 12)", bit_depth);
  if (width < 8 || height < 8 || (width & 7) || (height & 7) || width > 16384 || height > 16384)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_crop_analyse: the planes' size %dx%d must be a multiple of 8 (8 .. 16384)", width, height);
  if (true_width < 1 || true_width > width || width - true_width >= 8 || true_height < 1 || true_height > height || height - true_height >= 8)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_crop_analyse: the true size %dx%d must lie within 7 samples below the planes' size %dx%d", true_width, true_height, width, height);
  if (frames < 1 || frames > 65535) return fail(ctx, AV1MI_E_INVAL, "av1mi_crop_analyse: frames %d out of range (1 .. 65535)", frames);
  if (limit < 0 || limit > 255) return fail(ctx, AV1MI_E_INVAL, "av1mi_crop_analyse: limit %d out of range (0 .. 255)", limit);
  if (!d_luma || !d_records || ((uintptr_t)d_luma & 15) || ((uintptr_t)d_records & 3)) return fail(ctx, AV1MI_E_INVAL, "av1mi_crop_analyse: null or misaligned device pointer (planes 16 bytes, records 4)");
  if (int rc = grow(ctx, &ctx->crop_scratch, &ctx->crop_scratch_bytes, av1mi::crop_layout(bit_depth, true_width, true_height, frames).bytes)) return rc;
  av1mi::CropAnalyseLaunch A;
  A.bd = bit_depth; A.stride = width; A.rows = height; A.w = true_width; A.h = true_height; A.frames = frames; A.limit = limit;
  A.luma = d_luma; A.scratch = ctx->crop_scratch; A.out = d_records;
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_crop_analyse(A, ctx->stream));
  return AV1MI_OK;
}

int av1mi_noise_analyse(av1mi_ctx *ctx, int bit_depth, int width, int height, int true_width, int true_height, int pairs, const void *d_luma,
                        av1mi_noise_record *d_records) {
  BIND(ctx);
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return fail(ctx, AV1MI_E_INVAL, "av1mi_noise_analyse: bit depth %d not supported (8, 10 or 12)", bit_depth);
  if (width < 8 || height < 8 || (width & 7) || (height & 7) || width > 16384 || height > 16384)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_noise_analyse: the planes' size %dx%d must be a multiple of 8 (8 .. 16384)", width, height);
  if (true_width < 1 || true_width > width || width - true_width >= 8 || true_height < 1 || true_height > height || height - true_height >= 8)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_noise_analyse: the true size %dx%d must lie within 7 samples below the planes' size %dx%d", true_width, true_height, width, height);
  if (pairs < 1 || pairs > 32767) return fail(ctx, AV1MI_E_INVAL, "av1mi_noise_analyse: pairs %d out of range (1 .. 32767)", pairs);
  if (!d_luma || !d_records || ((uintptr_t)d_luma & 15) || ((uintptr_t)d_records & 3)) return fail(ctx, AV1MI_E_INVAL, "av1mi_noise_analyse: null or misaligned device pointer (planes 16 bytes, records 4)");
  if (int rc = grow(ctx, &ctx->noise_scratch, &ctx->noise_scratch_bytes, av1mi::noise_layout(bit_depth, true_width, true_height, pairs).bytes)) return rc;
  av1mi::NoiseAnalyseLaunch A;
  A.bd = bit_depth; A.stride = width; A.rows = height; A.w = true_width; A.h = true_height; A.pairs = pairs;
  A.luma = d_luma; A.scratch = ctx->noise_scratch; A.out = d_records;
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_noise_analyse(A, ctx->stream));
  return AV1MI_OK;
}

int av1mi_peak_analyse(av1mi_ctx *ctx, int width, int height, int true_width, int true_height, int frames, const void *d_y, const void *d_u, const void *d_v,
                       av1mi_peak_record *d_records) {
  BIND(ctx);
  if (width < 8 || height < 8 || (width & 7) || (height & 7) || width > 16384 || height > 16384)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_peak_analyse: the planes' size %dx%d must be a multiple of 8 (8 .. 16384)", width, height);
  if (true_width < 1 || true_width > width || width - true_width >= 8 || true_height < 1 || true_height > height || height - true_height >= 8)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_peak_analyse: the true size %dx%d must lie within 7 samples below the planes' size %dx%d", true_width, true_height, width, height);
  if (frames < 1 || frames > 65535) return fail(ctx, AV1MI_E_INVAL, "av1mi_peak_analyse: frames %d out of range (1 .. 65535)", frames);
  if (!d_y || !d_u || !d_v || !d_records || (((uintptr_t)d_y | (uintptr_t)d_u | (uintptr_t)d_v) & 15) || ((uintptr_t)d_records & 3))
    return fail(ctx, AV1MI_E_INVAL, "av1mi_peak_analyse: null or misaligned device pointer (planes 16 bytes, records 4)");
  if (int rc = grow(ctx, &ctx->peak_scratch, &ctx->peak_scratch_bytes, av1mi::peak_layout(true_height, frames).bytes)) return rc;
  av1mi::PeakAnalyseLaunch A;
  A.w8 = width; A.h8 = height; A.tw = true_width; A.th = true_height; A.frames = frames;
  A.y = d_y; A.u = d_u; A.v = d_v; A.scratch = ctx->peak_scratch; A.out = d_records;
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_peak_analyse(A, ctx->stream));
  return AV1MI_OK;
}

int av1mi_telecine_analyse(av1mi_ctx *ctx, int bit_depth, int width, int height, int true_width, int true_height, int frames, const void *d_luma,
                           av1mi_telecine_record *d_records) {
  BIND(ctx);
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return fail(ctx, AV1MI_E_INVAL, "av1mi_telecine_analyse: bit depth %d not supported (8, 10 or 12)", bit_depth);
  if (width < 8 || height < 8 || (width & 7) || (height & 7) || width > 16384 || height > 16384)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_telecine_analyse: the planes' size %dx%d must be a multiple of 8 (8 .. 16384)", width, height);
  if (true_width < 1 || true_width > width || width - true_width >= 8 || true_height < 1 || true_height > height || height - true_height >= 8)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_telecine_analyse: the true size %dx%d must lie within 7 samples below the planes' size %dx%d", true_width, true_height, width, height);
  if (frames < 1 || frames > 65535) return fail(ctx, AV1MI_E_INVAL, "av1mi_telecine_analyse: frames %d out of range (1 .. 65535)", frames);
  if (!d_luma || !d_records || ((uintptr_t)d_luma & 15) || ((uintptr_t)d_records & 7)) return fail(ctx, AV1MI_E_INVAL, "av1mi_telecine_analyse: null or misaligned device pointer (planes 16 bytes, records 8)");
  if (int rc = grow(ctx, &ctx->telecine_scratch, &ctx->telecine_scratch_bytes, av1mi::telecine_layout(bit_depth, true_width, true_height, frames).bytes)) return rc;
  av1mi::TelecineLaunch A;
  A.bd = bit_depth; A.stride = width; A.rows = height; A.w = true_width; A.h = true_height; A.frames = frames;
  A.luma = d_luma; A.scratch = ctx->telecine_scratch; A.out = d_records;
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_telecine_analyse(A, ctx->stream));
  return AV1MI_OK;
}

int av1mi_telecine_gather(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int segments,
                          const void *const *d_table, void *const d_dst[3]) {
  BIND(ctx);
  if (!plane_w || !plane_h || !true_w || !true_h || !d_table || !d_dst || ((uintptr_t)d_table & 7)) return fail(ctx, AV1MI_E_INVAL, "av1mi_telecine_gather: null pointer or misaligned table");
  av1mi::GatherPlanes L;
  if (int rc = check_gather_planes(ctx, "av1mi_telecine_gather", 12, false, bit_depth, plane_w, plane_h, true_w, true_h, segments, d_table, d_dst, L)) return rc;
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_telecine_gather(L, ctx->stream));
  return AV1MI_OK;
}

int av1mi_tone_map(av1mi_ctx *ctx, int width, int height, int frames, void *d_y, void *d_u, void *d_v, const av1mi_tone_tables *d_tables) {
  BIND(ctx);
  if (width < 4 || height < 2 || (width & 3) || (height & 1) || width > 16384 || height > 16384)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_tone_map: the planes' size %dx%d must be a multiple of 4 x 2 (up to 16384)", width, height);
  if (frames < 1 || frames > 65535) return fail(ctx, AV1MI_E_INVAL, "av1mi_tone_map: frames %d out of range (1 .. 65535)", frames);
  if (!d_y || !d_u || !d_v || !d_tables || (((uintptr_t)d_y | (uintptr_t)d_u | (uintptr_t)d_v | (uintptr_t)d_tables) & 15))
    return fail(ctx, AV1MI_E_INVAL, "av1mi_tone_map: null or misaligned device pointer (planes and tables 16 bytes)");
  void *const planes[3] = { d_y, d_u, d_v };
  ProfScope ps(ctx, AV1MI_K_INPUT);
  HIP_TRY(ctx, av1mi::launch_tone_map(width, height, frames, planes, d_tables, ctx->stream));
  return AV1MI_OK;
}

int av1mi_depth_reduce(av1mi_ctx *ctx, int mode, int width, int height, int frames, const void *const d_in[3], void *const d_out[3]) {
  BIND(ctx);
  if (mode != AV1MI_DEPTH_ROUND && mode != AV1MI_DEPTH_ORDERED) return fail(ctx, AV1MI_E_INVAL, "av1mi_depth_reduce: mode %d unknown (0 round, 1 ordered)", mode);
  if (width < 8 || height < 8 || (width & 7) || (height & 7) || width > 16384 || height > 16384)
    return fail(ctx, AV1MI_E_INVAL, "av1mi_depth_reduce: the planes' size %dx%d must be a multiple of 8 (8 .. 16384)", width, height);
  if (frames < 1 || (size_t)frames * (size_t)height > 65535u * 32u) return fail(ctx, AV1MI_E_INVAL, "av1mi_depth_reduce: frames %d out of range", frames);
  if (!d_in || !d_out) return fail(ctx, AV1MI_E_INVAL, "av1mi_depth_reduce: null plane array");
  for (int p = 0; p < 3; p++)
    if (!d_in[p] || !d_out[p] || (((uintptr_t)d_in[p] | (uintptr_t)d_out[p]) & 3)) return fail(ctx, AV1MI_E_INVAL, "av1mi_depth_reduce: null or misaligned device pointer (4 bytes)");
  ProfScope ps(ctx, AV1MI_K_INPUT);
  HIP_TRY(ctx, av1mi::launch_depth_reduce(mode, width, height, frames, d_in, d_out, ctx->stream));
  return AV1MI_OK;
}

int av1mi_frames_gather(av1mi_ctx *ctx, const size_t plane_bytes[3], int segments, const void *const *d_src_table, void *const d_dst[3]) {
  BIND(ctx);
  if (!plane_bytes || !d_src_table || !d_dst || ((uintptr_t)d_src_table & 7)) return fail(ctx, AV1MI_E_INVAL, "av1mi_frames_gather: null pointer or misaligned table");
  if (segments < 1 || segments > 4096) return fail(ctx, AV1MI_E_INVAL, "av1mi_frames_gather: segments %d out of range (1 .. 4096)", segments);
  for (int p = 0; p < 3; p++) {
    if ((plane_bytes[p] & 3) || plane_bytes[p] > 0x7FFFFFF0u) return fail(ctx, AV1MI_E_INVAL, "av1mi_frames_gather: plane %d of %zu bytes (a multiple of 4 below 2^31)", p, plane_bytes[p]);
    if (plane_bytes[p] && (!d_dst[p] || ((uintptr_t)d_dst[p] & 15))) return fail(ctx, AV1MI_E_INVAL, "av1mi_frames_gather: null or misaligned destination (plane %d)", p);
  }
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_frames_gather(plane_bytes, segments, d_src_table, d_dst, ctx->stream));
  return AV1MI_OK;
}

int av1mi_deinterlace_gather(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int parity,
                             int segments, const void *const *d_table, void *const d_dst[3]) {
  BIND(ctx);
  if (!plane_w || !plane_h || !true_w || !true_h || !d_table || !d_dst || ((uintptr_t)d_table & 7)) return fail(ctx, AV1MI_E_INVAL, "av1mi_deinterlace_gather: null pointer or misaligned table");
  if (parity != 0 && parity != 1) return fail(ctx, AV1MI_E_INVAL, "av1mi_deinterlace_gather: parity %d (0 = top field first, 1 = bottom field first)", parity);
  av1mi::DeintLaunch L;
  L.parity = parity;
  if (int rc = check_gather_planes(ctx, "av1mi_deinterlace_gather", 12, false, bit_depth, plane_w, plane_h, true_w, true_h, segments, d_table, d_dst, L)) return rc;
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_deint_gather(L, ctx->stream));
  return AV1MI_OK;
}

int av1mi_deinterlace_gather_fields(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int parity,
                                    int segments, const void *const *d_table, const uint8_t *d_phase, void *const d_dst[3]) {
  BIND(ctx);
  if (!plane_w || !plane_h || !true_w || !true_h || !d_table || !d_phase || !d_dst || ((uintptr_t)d_table & 7))
    return fail(ctx, AV1MI_E_INVAL, "av1mi_deinterlace_gather_fields: null pointer or misaligned table");
  if (parity != 0 && parity != 1) return fail(ctx, AV1MI_E_INVAL, "av1mi_deinterlace_gather_fields: parity %d (0 = top field first, 1 = bottom field first)", parity);
  av1mi::DeintFieldsLaunch L;
  L.parity = parity; L.phase = d_phase;
  if (int rc = check_gather_planes(ctx, "av1mi_deinterlace_gather_fields", 12, false, bit_depth, plane_w, plane_h, true_w, true_h, segments, d_table, d_dst, L)) return rc;
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_deint_gather_fields(L, ctx->stream));
  return AV1MI_OK;
}

int av1mi_denoise_gather(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int strength,
                         int segments, const void *const *d_table, void *const d_dst[3], av1mi_grain_record *d_records) {
  BIND(ctx);
  if (!plane_w || !plane_h || !true_w || !true_h || !d_table || !d_dst || ((uintptr_t)d_table & 7) || ((uintptr_t)d_records & 7))
    return fail(ctx, AV1MI_E_INVAL, "av1mi_denoise_gather: null pointer, or misaligned table or records");
  if (strength < 1 || strength > 16) return fail(ctx, AV1MI_E_INVAL, "av1mi_denoise_gather: strength %d out of range (1 .. 16)", strength);
  av1mi::DenoiseLaunch L;
  L.strength = strength; L.records = d_records; L.scratch = nullptr;
  if (int rc = check_gather_planes(ctx, "av1mi_denoise_gather", 10, true, bit_depth, plane_w, plane_h, true_w, true_h, segments, d_table, d_dst, L)) return rc;
  if (d_records) {
    if (int rc = grow(ctx, &ctx->grain_scratch, &ctx->grain_scratch_bytes, av1mi::grain_scratch_bytes(L))) return rc;
    L.scratch = ctx->grain_scratch;
    if (!L.scratch) {      // no plane at all: the records are still defined
      HIP_TRY(ctx, hipMemsetAsync(d_records, 0, (size_t)segments * 3 * sizeof(av1mi_grain_record), ctx->stream));
      return AV1MI_OK;
    }
  }
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_denoise_gather(L, ctx->stream));
  return AV1MI_OK;
}

int av1mi_denoise_mc_gather(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int strength,
                            int range, int segments, const void *const *d_table, void *const d_dst[3], av1mi_grain_record *d_records, av1mi_denoise_vec *d_vectors) {
  BIND(ctx);
  if (!plane_w || !plane_h || !true_w || !true_h || !d_table || !d_dst || ((uintptr_t)d_table & 7) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_vectors & 3))
    return fail(ctx, AV1MI_E_INVAL, "av1mi_denoise_mc_gather: null pointer, or misaligned table, records or vectors");
  if (strength < 1 || strength > 16) return fail(ctx, AV1MI_E_INVAL, "av1mi_denoise_mc_gather: strength %d out of range (1 .. 16)", strength);
  if (range != 4 && range != 8) return fail(ctx, AV1MI_E_INVAL, "av1mi_denoise_mc_gather: range %d (4 or 8)", range);
  av1mi::DenoiseMcLaunch L;
  L.strength = strength; L.range = range; L.records = d_records; L.scratch = nullptr; L.vectors = d_vectors;
  if (int rc = check_gather_planes(ctx, "av1mi_denoise_mc_gather", 10, true, bit_depth, plane_w, plane_h, true_w, true_h, segments, d_table, d_dst, L)) return rc;
  if (!L.plane_w[0]) return fail(ctx, AV1MI_E_INVAL, "av1mi_denoise_mc_gather: no luma plane (%dx%d): it is what the search reads", plane_w[0], plane_h[0]);
  for (int p = 1; p < 3; p++) {      // (an absent plane has the size 0 in L)
    const int ssx = L.plane_w[p] && L.plane_w[p] < L.plane_w[0], ssy = L.plane_w[p] && L.plane_h[p] < L.plane_h[0];
    if (L.plane_w[p] && (true_w[p] != (true_w[0] + ssx) >> ssx || true_h[p] != (true_h[0] + ssy) >> ssy))
      return fail(ctx, AV1MI_E_INVAL, "av1mi_denoise_mc_gather: plane %d: the true size %dx%d is not the luma plane's %dx%d%s", p, true_w[p], true_h[p], true_w[0], true_h[0],
                  ssx || ssy ? ", halved upwards where the plane is subsampled" : "");
  }
  if (!d_vectors) {
    const size_t need = av1mi::denoise_mc_vector_bytes(L);
    if (!need) return fail(ctx, AV1MI_E_INVAL, "av1mi_denoise_mc_gather: a geometry the launch does not take");
    if (int rc = grow(ctx, &ctx->denoise_vectors, &ctx->denoise_vectors_bytes, need)) return rc;
    L.vectors = (av1mi_denoise_vec *)ctx->denoise_vectors;
  }
  if (d_records) {
    if (int rc = grow(ctx, &ctx->grain_scratch, &ctx->grain_scratch_bytes, av1mi::denoise_mc_scratch_bytes(L))) return rc;
    L.scratch = ctx->grain_scratch;
  }
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_denoise_mc_gather(L, ctx->stream));
  return AV1MI_OK;
}

int av1mi_grain_cov(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int segments,
                    const void *const *d_table, void *const d_out[3], av1mi_grain_cov_record *d_cov) {
  BIND(ctx);
  if (!plane_w || !plane_h || !true_w || !true_h || !d_table || !d_out || !d_cov || ((uintptr_t)d_table & 7) || ((uintptr_t)d_cov & 7))
    return fail(ctx, AV1MI_E_INVAL, "av1mi_grain_cov: null pointer, or misaligned table or records");
  av1mi::GrainCovLaunch L;
  L.cov = d_cov; L.scratch = nullptr;
  if (int rc = check_gather_planes(ctx, "av1mi_grain_cov", 10, true, bit_depth, plane_w, plane_h, true_w, true_h, segments, d_table, d_out, L)) return rc;
  if (int rc = grow(ctx, &ctx->grain_cov_scratch, &ctx->grain_cov_scratch_bytes, av1mi::grain_cov_scratch_bytes(L))) return rc;
  L.scratch = ctx->grain_cov_scratch;      // (null where there is no plane at all: the launch then only clears the records)
  ProfScope ps(ctx, AV1MI_K_SCENE);
  HIP_TRY(ctx, av1mi::launch_grain_cov(L, ctx->stream));
  return AV1MI_OK;
}

int av1mi_intra_encode(av1mi_ctx *ctx, const av1mi_intra_job *j) {
  BIND(ctx);
  if (!j) return fail(ctx, AV1MI_E_INVAL, "null job");
  if (int rc = check_bd(ctx, j->bit_depth)) return rc;
  if (j->block_size != 8 && j->block_size != 16 && j->block_size != 32) return fail(ctx, AV1MI_E_INVAL, "block_size %d not supported (8, 16 or 32)", j->block_size);
  if (j->open_loop && j->block_size == 32) return fail(ctx, AV1MI_E_INVAL, "the open-loop mode decision exists for 8x8 and 16x16 blocks");
  if (j->width <= 0 || j->height <= 0 || j->width % j->block_size || j->height % j->block_size || j->width > 16384 || j->height > 16384)
    return fail(ctx, AV1MI_E_INVAL, "frame %dx%d is not a multiple of the block size %d", j->width, j->height, j->block_size);
  if (j->nframes < 0 || j->qindex < 0 || j->qindex > 255) return fail(ctx, AV1MI_E_INVAL, "bad nframes/qindex");
  if (j->stride_y < j->width || j->stride_uv < j->width / 2 || (j->stride_y & 3) || (j->stride_uv & 3))
    return fail(ctx, AV1MI_E_INVAL, "bad strides %d/%d", j->stride_y, j->stride_uv);
  const void *ptrs[] = { j->d_src_y, j->d_src_u, j->d_src_v, j->d_rec_y, j->d_rec_u, j->d_rec_v, j->d_lev_y, j->d_lev_u, j->d_lev_v,
                         j->d_modes_y, j->d_modes_uv };
  for (const void *p : ptrs) if (!p || ((uintptr_t)p & 7)) return fail(ctx, AV1MI_E_INVAL, "null or misaligned device pointer");
  av1mi::IntraPipeLaunch L;
  L.src[0] = j->d_src_y; L.src[1] = j->d_src_u; L.src[2] = j->d_src_v;
  L.rec[0] = j->d_rec_y; L.rec[1] = j->d_rec_u; L.rec[2] = j->d_rec_v;
  L.lev[0] = j->d_lev_y; L.lev[1] = j->d_lev_u; L.lev[2] = j->d_lev_v;
  L.modes_y = j->d_modes_y; L.modes_uv = j->d_modes_uv;
  L.w = j->width; L.h = j->height; L.stride_y = j->stride_y; L.stride_uv = j->stride_uv; L.bd = j->bit_depth; L.nframes = j->nframes;
  L.dc_q = av1mi_dc_q(j->qindex, j->bit_depth); L.ac_q = av1mi_ac_q(j->qindex, j->bit_depth);
  L.dc_quant = (1 << 16) / L.dc_q; L.ac_quant = (1 << 16) / L.ac_q;
  L.open_loop = j->open_loop ? 1 : 0;
  const int blocks = (j->width / j->block_size) * (j->height / j->block_size);
  if ((j->frame_rows && (j->frame_rows < j->height || (j->frame_rows & 7))) || (j->modes_frame_stride && j->modes_frame_stride < blocks))
    return fail(ctx, AV1MI_E_INVAL, "bad frame_rows %d / modes_frame_stride %d", j->frame_rows, j->modes_frame_stride);
  L.frame_rows = j->frame_rows ? j->frame_rows : j->height;
  L.modes_stride = j->modes_frame_stride ? j->modes_frame_stride : blocks;
  { ProfScope ps(ctx, AV1MI_K_INTRA_PIPE); HIP_TRY(ctx, av1mi::launch_intra_pipe(L, j->block_size, ctx->stream)); }
  return AV1MI_OK;
}

}  // extern "C"

// the argument rules of an inter job and its launch description; search_only: the job of av1mi_me_search, which reads and writes luma
// and vectors alone
static int inter_launch(av1mi_ctx *ctx, const av1mi_inter_job *j, bool search_only, av1mi::InterLaunch *out) {
  if (!j) return fail(ctx, AV1MI_E_INVAL, "null job");
  if (int rc = check_bd(ctx, j->bit_depth)) return rc;
  if (j->width <= 0 || j->height <= 0 || (j->width & 7) || (j->height & 7) || j->width > 16384 || j->height > 16384)
    return fail(ctx, AV1MI_E_INVAL, "frame %dx%d must be a multiple of 8", j->width, j->height);
  if (j->nframes < 0 || j->nframes > 65535 || j->qindex < 0 || j->qindex > 255 || j->search_range < 0 || j->search_range > 15)
    return fail(ctx, AV1MI_E_INVAL, "bad nframes/qindex/search_range");
  if (j->coarse_range < 0 || j->coarse_range > 64 || (j->coarse_range & 3))
    return fail(ctx, AV1MI_E_INVAL, "coarse_range %d must be 0 or a multiple of 4 up to 64", j->coarse_range);
  if (j->stride_y < j->width || (j->stride_y & 3) || (!search_only && (j->stride_uv < j->width / 2 || (j->stride_uv & 3))))
    return fail(ctx, AV1MI_E_INVAL, "bad strides %d/%d", j->stride_y, j->stride_uv);
  if (search_only) {
    const void *ptrs[] = { j->d_src_y, j->d_ref_y, j->d_mvs };
    for (const void *p : ptrs) if (!p || ((uintptr_t)p & 7)) return fail(ctx, AV1MI_E_INVAL, "null or misaligned device pointer");
  } else {
    const void *ptrs[] = { j->d_src_y, j->d_src_u, j->d_src_v, j->d_ref_y, j->d_ref_u, j->d_ref_v, j->d_rec_y, j->d_rec_u, j->d_rec_v,
                           j->d_lev_y, j->d_lev_u, j->d_lev_v, j->d_mvs, j->d_skip };
    for (const void *p : ptrs) if (!p || ((uintptr_t)p & 7)) return fail(ctx, AV1MI_E_INVAL, "null or misaligned device pointer");
    if (j->d_ref_y == j->d_rec_y || j->d_ref_u == j->d_rec_u || j->d_ref_v == j->d_rec_v) return fail(ctx, AV1MI_E_INVAL, "reference and reconstruction must differ");
  }
  av1mi::InterLaunch &L = *out;
  L.src[0] = j->d_src_y; L.src[1] = j->d_src_u; L.src[2] = j->d_src_v;
  L.ref[0] = j->d_ref_y; L.ref[1] = j->d_ref_u; L.ref[2] = j->d_ref_v;
  L.ref_alt[0] = j->d_ref_alt_y; L.ref_alt[1] = j->d_ref_alt_u; L.ref_alt[2] = j->d_ref_alt_v; L.ref_sel = j->d_ref_sel;
  if (L.ref_sel && (!L.ref_alt[0] || (!search_only && (!L.ref_alt[1] || !L.ref_alt[2])))) return fail(ctx, AV1MI_E_INVAL, "d_ref_sel without d_ref_alt_*");
  if (L.ref_sel && (((uintptr_t)L.ref_sel & 3) || ((uintptr_t)L.ref_alt[0] & 7))) return fail(ctx, AV1MI_E_INVAL, "misaligned d_ref_sel / d_ref_alt_y");
  L.rec[0] = j->d_rec_y; L.rec[1] = j->d_rec_u; L.rec[2] = j->d_rec_v;
  L.lev[0] = j->d_lev_y; L.lev[1] = j->d_lev_u; L.lev[2] = j->d_lev_v;
  L.mvs = j->d_mvs; L.skip = j->d_skip;
  L.w = j->width; L.h = j->height; L.stride_y = j->stride_y; L.stride_uv = j->stride_uv; L.bd = j->bit_depth; L.nframes = j->nframes;
  L.dc_q = av1mi_dc_q(j->qindex, j->bit_depth); L.ac_q = av1mi_ac_q(j->qindex, j->bit_depth); L.range = j->search_range;
  L.dc_quant = (1 << 16) / L.dc_q; L.ac_quant = (1 << 16) / L.ac_q;
  L.centres = nullptr;
  return AV1MI_OK;
}
// the context's own scratch area of the coarse search, large enough for L
static int ensure_me_scratch(av1mi_ctx *ctx, const av1mi::InterLaunch &L) {
  return grow(ctx, &ctx->me_scratch, &ctx->me_scratch_bytes, av1mi::me_layout(L.w, L.h, L.nframes).bytes);
}
// coarse search (optional) + integer search of L; with a coarse search L.centres is set to the centres in d_me
static int launch_search(av1mi_ctx *ctx, av1mi::InterLaunch &L, int coarse_range, void *d_me) {
  if (coarse_range) {
    if (!d_me || ((uintptr_t)d_me & 15)) return fail(ctx, AV1MI_E_INVAL, "coarse_range %d without a scratch area", coarse_range);
    { ProfScope ps(ctx, AV1MI_K_ME_COARSE); HIP_TRY(ctx, av1mi::launch_me_coarse(L, coarse_range, d_me, ctx->stream)); }
    L.centres = (const int16_t *)((const char *)d_me + av1mi::me_layout(L.w, L.h, L.nframes).off_centres);
  }
  // one event pair per kernel, so that either can be the bench's roofline kernel and be matched with rocprofv3's per-kernel stats
  { ProfScope ps(ctx, AV1MI_K_ME_INT); HIP_TRY(ctx, av1mi::launch_me_int(L, ctx->stream)); }
  return AV1MI_OK;
}

namespace av1mi {
int inter_encode_with(av1mi_ctx *ctx, const av1mi_inter_job *j, void *d_me) {
  BIND(ctx);
  InterLaunch L;
  if (int rc = inter_launch(ctx, j, false, &L)) return rc;
  if (int rc = launch_search(ctx, L, j->coarse_range, d_me)) return rc;
  { ProfScope ps(ctx, AV1MI_K_INTER_PIPE); HIP_TRY(ctx, launch_inter_pipe(L, ctx->stream)); }
  return AV1MI_OK;
}
}  // namespace av1mi

extern "C" {

int av1mi_inter_encode(av1mi_ctx *ctx, const av1mi_inter_job *j) {
  BIND(ctx);
  av1mi::InterLaunch L;
  if (int rc = inter_launch(ctx, j, false, &L)) return rc;
  if (j->coarse_range) if (int rc = ensure_me_scratch(ctx, L)) return rc;
  return av1mi::inter_encode_with(ctx, j, j->coarse_range ? ctx->me_scratch : nullptr);
}

int av1mi_me_search(av1mi_ctx *ctx, const av1mi_inter_job *j, uint8_t *d_q_src, uint8_t *d_q_ref, int16_t *d_centres) {
  BIND(ctx);
  av1mi::InterLaunch L;
  if (int rc = inter_launch(ctx, j, true, &L)) return rc;
  if (!d_centres || ((uintptr_t)d_centres & 3)) return fail(ctx, AV1MI_E_INVAL, "null or misaligned d_centres");
  if (L.nframes == 0) return AV1MI_OK;
  const av1mi::MeLayout M = av1mi::me_layout(L.w, L.h, L.nframes);
  if (j->coarse_range) if (int rc = ensure_me_scratch(ctx, L)) return rc;
  if (int rc = launch_search(ctx, L, j->coarse_range, ctx->me_scratch)) return rc;
  const size_t cbytes = (size_t)M.tiles * L.nframes * 4;
  if (!j->coarse_range) { HIP_TRY(ctx, hipMemsetAsync(d_centres, 0, cbytes, ctx->stream)); return AV1MI_OK; }
  const char *sc = (const char *)ctx->me_scratch;
  HIP_TRY(ctx, hipMemcpyAsync(d_centres, sc + M.off_centres, cbytes, hipMemcpyDeviceToDevice, ctx->stream));
  // the planes without the row padding of the scratch area
  uint8_t *dst[2] = { d_q_src, d_q_ref };
  for (int k = 0; k < 2; k++)
    if (dst[k]) HIP_TRY(ctx, hipMemcpy2DAsync(dst[k], (size_t)M.qw, sc + (k ? M.off_ref : 0), (size_t)M.qs, (size_t)M.qw, (size_t)M.qh * L.nframes, hipMemcpyDeviceToDevice, ctx->stream));
  return AV1MI_OK;
}


int av1mi_dc_q(int qindex, int bd) {
  const int q = qindex < 0 ? 0 : qindex > 255 ? 255 : qindex;
  return bd == 8 ? av1mi::k_dc_q8[q] : av1mi::k_dc_q10[q];
}
int av1mi_ac_q(int qindex, int bd) {
  const int q = qindex < 0 ? 0 : qindex > 255 ? 255 : qindex;
  return bd == 8 ? av1mi::k_ac_q8[q] : av1mi::k_ac_q10[q];
}
static int check_q(av1mi_ctx *ctx, const void *a, const void *b, size_t n, int coef_per_blk, int dc_q, int ac_q, int log_scale) {
  if (!a || !b) return fail(ctx, AV1MI_E_INVAL, "null device pointer");
  if (n & 3) return fail(ctx, AV1MI_E_INVAL, "coefficient count %zu must be a multiple of 4", n);
  if (coef_per_blk < 16 || (coef_per_blk & 3)) return fail(ctx, AV1MI_E_INVAL, "coef_per_blk %d invalid", coef_per_blk);
  if (dc_q < 4 || ac_q < 4 || dc_q > 32767 || ac_q > 32767) return fail(ctx, AV1MI_E_INVAL, "quantiser step out of range");
  if (log_scale < 0 || log_scale > 2) return fail(ctx, AV1MI_E_INVAL, "log_scale %d out of range", log_scale);
  return AV1MI_OK;
}
int av1mi_quantize(av1mi_ctx *ctx, const int32_t *d_coef, int16_t *d_levels, int32_t *d_dqcoef, size_t n,
                   int coef_per_blk, int dc_q, int ac_q, int log_scale) {
  BIND(ctx);
  if (int rc = check_q(ctx, d_coef, d_levels, n, coef_per_blk, dc_q, ac_q, log_scale)) return rc;
  { ProfScope ps(ctx, AV1MI_K_QUANT); HIP_TRY(ctx, av1mi::launch_quantize(d_coef, d_levels, d_dqcoef, (long long)n, coef_per_blk, dc_q, ac_q, log_scale, ctx->stream)); }
  return AV1MI_OK;
}
int av1mi_dequantize(av1mi_ctx *ctx, const int16_t *d_levels, int32_t *d_dqcoef, size_t n, int coef_per_blk,
                     int dc_q, int ac_q, int log_scale, int bd) {
  BIND(ctx);
  if (int rc = check_q(ctx, d_levels, d_dqcoef, n, coef_per_blk, dc_q, ac_q, log_scale)) return rc;
  if (int rc = check_bd(ctx, bd)) return rc;
  { ProfScope ps(ctx, AV1MI_K_DEQUANT); HIP_TRY(ctx, av1mi::launch_dequantize(d_levels, d_dqcoef, (long long)n, coef_per_blk, dc_q, ac_q, log_scale, bd, ctx->stream)); }
  return AV1MI_OK;
}

int av1mi_inv_txfm2d_add(av1mi_ctx *ctx, const int32_t *coef, void *dst, int stride, int tx_size, int tx_type, int bd) {
  BIND(ctx);
  if (!coef || !dst) return fail(ctx, AV1MI_E_INVAL, "null pointer");
  if (int rc = check_bd(ctx, bd)) return rc;
  if (!tx_valid(tx_size, tx_type)) return fail(ctx, AV1MI_E_INVAL, "tx_type %d is not defined for tx_size %d", tx_type, tx_size);
  const int w = av1mi::tx_width(tx_size), h = av1mi::tx_height(tx_size);
  if (stride < w) return fail(ctx, AV1MI_E_INVAL, "stride %d < width %d", stride, w);
  const int cw = w > 32 ? 32 : w, ch = h > 32 ? 32 : h, bps = bd == 8 ? 1 : 2;
  const size_t coef_bytes = (size_t)cw * ch * 4, pix_bytes = (size_t)w * h * bps;
  if (int rc = grow(ctx, &ctx->scratch, &ctx->scratch_bytes, coef_bytes + pix_bytes + 64)) return rc;
  char *d = (char *)ctx->scratch;
  int32_t *d_coef = (int32_t *)d;
  void *d_pix = d + coef_bytes;
  av1mi_txb *d_list = (av1mi_txb *)(d + coef_bytes + pix_bytes);
  const av1mi_txb blk = { 0, 0, 0, (uint32_t)tx_type, 0 };
  HIP_TRY(ctx, hipMemcpyAsync(d_coef, coef, coef_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpy2DAsync(d_pix, (size_t)w * bps, dst, (size_t)stride * bps, (size_t)w * bps, h, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_list, &blk, sizeof(blk), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // blk lives on this stack frame
  av1mi::TxLaunch L = { d_coef, d_pix, w, 1, d_list, nullptr, 0, 1 };
  HIP_TRY(ctx, av1mi::launch_inv_txfm(tx_size, L, bd, ctx->stream));
  HIP_TRY(ctx, hipMemcpy2DAsync(dst, (size_t)stride * bps, d_pix, (size_t)w * bps, (size_t)w * bps, h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return AV1MI_OK;
}
int av1mi_fwd_txfm2d(av1mi_ctx *ctx, const int16_t *resid, int stride, int32_t *coef, int tx_size, int tx_type) {
  BIND(ctx);
  if (!coef || !resid) return fail(ctx, AV1MI_E_INVAL, "null pointer");
  if (!tx_valid(tx_size, tx_type)) return fail(ctx, AV1MI_E_INVAL, "tx_type %d is not defined for tx_size %d", tx_type, tx_size);
  const int w = av1mi::tx_width(tx_size), h = av1mi::tx_height(tx_size);
  if (stride < w) return fail(ctx, AV1MI_E_INVAL, "stride %d < width %d", stride, w);
  const int cw = w > 32 ? 32 : w, ch = h > 32 ? 32 : h;
  const size_t coef_bytes = (size_t)cw * ch * 4, pix_bytes = (size_t)w * h * 2;
  if (int rc = grow(ctx, &ctx->scratch, &ctx->scratch_bytes, coef_bytes + pix_bytes + 64)) return rc;
  char *d = (char *)ctx->scratch;
  int32_t *d_coef = (int32_t *)d;
  int16_t *d_res = (int16_t *)(d + coef_bytes);
  av1mi_txb *d_list = (av1mi_txb *)(d + coef_bytes + pix_bytes);
  const av1mi_txb blk = { 0, 0, 0, (uint32_t)tx_type, 0 };
  HIP_TRY(ctx, hipMemcpy2DAsync(d_res, (size_t)w * 2, resid, (size_t)stride * 2, (size_t)w * 2, h, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_list, &blk, sizeof(blk), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  av1mi::TxLaunch L = { d_coef, d_res, w, 1, d_list, nullptr, 0, 1 };
  HIP_TRY(ctx, av1mi::launch_fwd_txfm(tx_size, L, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(coef, d_coef, coef_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return AV1MI_OK;
}

}  // extern "C"
