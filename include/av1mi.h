/*
 * av1mi.h — C ABI of libav1mi.so, the MI355X-native AV1 block-processing backend.
 *
 * Drop-in boundary.  The reference (IONIQ6000/av1-go) has no FFI for this path: its seam is
 * the process contract of internal/ffmpeg/transcode.go:194
 *     func RunTranscode(ffmpegPath string, args []string) (int, error)
 * fed by TranscodeArgs (transcode.go:17) and called only from daemon.ProcessJob
 * (internal/daemon/daemon.go:90,101).  All pixel work happens in the FFmpeg child
 * (transcode.go:120 "-c:v:0 av1_vaapi").  This header is what a cgo replacement of
 * RunTranscode binds instead; every entry point names the part of that
 * contract, or the SURVEY.md §8a kernel row, it stands in for.
 *
 * Conventions: plain C, no C++ types, no exceptions cross the boundary.  Return 0 = OK,
 * negative = AV1MI_E_*; av1mi_last_error(ctx) gives the text the Go wrapper turns into the
 * (int, error) pair of transcode.go:194/311.  One context per GPU; a context is not
 * thread-safe, distinct contexts are.  Every call selects the context's device first, so
 * any OS thread (goroutines migrate) may call.  No callbacks.
 * Pointers named d_* are DEVICE pointers obtained from av1mi_malloc(); others are host.
 */
#ifndef AV1MI_H
#define AV1MI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AV1MI_OK 0
#define AV1MI_E_INVAL (-1)   /* bad argument (size/type/alignment) */
#define AV1MI_E_DEVICE (-2)  /* HIP runtime error; text in av1mi_last_error */
#define AV1MI_E_NOMEM (-3)
#define AV1MI_E_NODEV (-4)   /* no gfx950 device / HIP extension unusable: the product never falls back to CPU */

/* AV1 TX_SIZE / TX_TYPE numbering (AV1 spec §6.10.19). */
enum av1mi_tx_size {
  AV1MI_TX_4X4, AV1MI_TX_8X8, AV1MI_TX_16X16, AV1MI_TX_32X32, AV1MI_TX_64X64, AV1MI_TX_4X8, AV1MI_TX_8X4,
  AV1MI_TX_8X16, AV1MI_TX_16X8, AV1MI_TX_16X32, AV1MI_TX_32X16, AV1MI_TX_32X64, AV1MI_TX_64X32, AV1MI_TX_4X16,
  AV1MI_TX_16X4, AV1MI_TX_8X32, AV1MI_TX_32X8, AV1MI_TX_16X64, AV1MI_TX_64X16, AV1MI_TX_SIZES_ALL
};
enum av1mi_tx_type {
  AV1MI_DCT_DCT, AV1MI_ADST_DCT, AV1MI_DCT_ADST, AV1MI_ADST_ADST, AV1MI_FLIPADST_DCT, AV1MI_DCT_FLIPADST,
  AV1MI_FLIPADST_FLIPADST, AV1MI_ADST_FLIPADST, AV1MI_FLIPADST_ADST, AV1MI_IDTX, AV1MI_V_DCT, AV1MI_H_DCT,
  AV1MI_V_ADST, AV1MI_H_ADST, AV1MI_V_FLIPADST, AV1MI_H_FLIPADST, AV1MI_TX_TYPES,
  AV1MI_WHT_WHT = 16   /* lossless blocks: 4x4 Walsh-Hadamard (spec 7.13.2.10), valid with AV1MI_TX_4X4 only */
};

typedef struct av1mi_ctx av1mi_ctx;

/* One transform block of a block list (16 bytes, one dwordx4 load on the device). */
typedef struct av1mi_txb {
  uint32_t coef_off; /* offset of the block's coefficients in the coefficient buffer, int32 units, multiple of 4 */
  uint16_t x, y;     /* top-left sample of the block in the plane; x multiple of 4 */
  uint32_t tx_type;  /* enum av1mi_tx_type */
  uint32_t reserved;
} av1mi_txb;

/* ---- library / context: stands in for ffmpeg provisioning + process spawn (binary.go:218, transcode.go:195) */
const char *av1mi_version(void);
int av1mi_device_count(void);                       /* number of HIP devices, 0 if none */
int av1mi_open(int device, av1mi_ctx **out);        /* AV1MI_E_NODEV when no GPU: callers must fail the job */
void av1mi_close(av1mi_ctx *ctx);
const char *av1mi_last_error(av1mi_ctx *ctx);       /* <= 800 chars, the cap of transcode.go:295-297 */
const char *av1mi_device_name(av1mi_ctx *ctx);

/* ---- device memory and stream plumbing (all on the context's own HIP stream) */
int av1mi_malloc(av1mi_ctx *ctx, void **d_ptr, size_t bytes);
int av1mi_free(av1mi_ctx *ctx, void *d_ptr);
int av1mi_upload(av1mi_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int av1mi_download(av1mi_ctx *ctx, void *dst, const void *d_src, size_t bytes);
int av1mi_memset(av1mi_ctx *ctx, void *d_dst, int value, size_t bytes);
/* device-to-device copy on the context's stream (e.g. handing a reconstructed frame to the next GOP stage; bench.py uses it to
 * measure the box's copy bandwidth, the second roofline BASELINE.md §3 asks for). */
int av1mi_copy(av1mi_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
int av1mi_sync(av1mi_ctx *ctx);
/* HIP-event stopwatch on the context's stream: begin .. end brackets whatever was enqueued between. */
int av1mi_timer_begin(av1mi_ctx *ctx);
int av1mi_timer_end(av1mi_ctx *ctx, float *elapsed_ms);

/* Per-kernel HIP-event profile (bench.py's roofline leg).  While enabled, every kernel launch made through
 * this context is bracketed by its own event pair on the context's stream; av1mi_prof_get() synchronises and
 * returns, for one kernel kind, the number of launches and the summed device time since the last reset. */
enum av1mi_kernel_kind {
  AV1MI_K_FWD_TXFM, AV1MI_K_INV_TXFM, AV1MI_K_QUANT, AV1MI_K_DEQUANT, AV1MI_K_INTRA_PRED, AV1MI_K_MC,
  AV1MI_K_DEBLOCK, AV1MI_K_CDEF, AV1MI_K_LR, AV1MI_K_INTRA_PIPE, AV1MI_K_INTER_PIPE, AV1MI_K_MISC, AV1MI_K_ENTROPY,
  AV1MI_K_ENTROPY_PACK, AV1MI_K_ENTROPY_TOKENS, AV1MI_K_ME_INT, AV1MI_K_ENTROPY_CHAINS, AV1MI_K_INPUT, AV1MI_K_QUALITY, AV1MI_K_ME_COARSE, AV1MI_K_SCENE, AV1MI_K_KINDS
};
int av1mi_prof_enable(av1mi_ctx *ctx, int on);
int av1mi_prof_reset(av1mi_ctx *ctx);
int av1mi_prof_get(av1mi_ctx *ctx, int kind, int *launches, double *total_ms);
const char *av1mi_kernel_kind_name(int kind);

/* 1 when (tx_size, tx_type) is arithmetically defined: ADST needs length 4/8/16, identity <= 32. */
int av1mi_txfm_valid(int tx_size, int tx_type);
int av1mi_tx_width(int tx_size);
int av1mi_tx_height(int tx_size);

/* ---- K2: inverse 2-D transform + add to prediction + clip.  Asynchronous.
 * d_plane holds the prediction on entry and the reconstruction afterwards; uint8 samples when
 * bd == 8, uint16 when bd == 10; stride in samples, multiple of 4.
 * Coefficients: int32, per block row-major min(w,32) x min(h,32) (64-point dimensions carry only
 * the low 32 frequencies), blocks contiguous.
 * grid form: block i covers (i % blocks_per_row, i / blocks_per_row) in units of the block size, its
 * coefficients start at i * min(w,32)*min(h,32); d_tx_types (1 byte per block) may be NULL, then
 * every block uses uniform_type. */
int av1mi_inv_txfm_add_grid(av1mi_ctx *ctx, int tx_size, const int32_t *d_coef, void *d_plane, int stride, int bd,
                            int blocks_per_row, int nblocks, const uint8_t *d_tx_types, int uniform_type);
/* list form: explicit blocks, all of size tx_size. */
int av1mi_inv_txfm_add_list(av1mi_ctx *ctx, int tx_size, const int32_t *d_coef, void *d_plane, int stride, int bd,
                            const av1mi_txb *d_list, int nblocks);

/* ---- K1: forward 2-D transform.  d_resid: int16 residual plane, stride in samples (multiple of 4). */
int av1mi_fwd_txfm_grid(av1mi_ctx *ctx, int tx_size, const int16_t *d_resid, int stride, int32_t *d_coef,
                        int blocks_per_row, int nblocks, const uint8_t *d_tx_types, int uniform_type);
int av1mi_fwd_txfm_list(av1mi_ctx *ctx, int tx_size, const int16_t *d_resid, int stride, int32_t *d_coef,
                        const av1mi_txb *d_list, int nblocks);

/* ---- K8: quantise (encoder side) / dequantise (normative).  n coefficients, multiple of 4; the first
 * coefficient of every run of coef_per_blk uses dc_q, the others ac_q.  d_dqcoef may be NULL in quantize. */
int av1mi_dc_q(int qindex, int bd);
int av1mi_ac_q(int qindex, int bd);
int av1mi_quantize(av1mi_ctx *ctx, const int32_t *d_coef, int16_t *d_levels, int32_t *d_dqcoef, size_t n,
                   int coef_per_blk, int dc_q, int ac_q, int log_scale);
int av1mi_dequantize(av1mi_ctx *ctx, const int16_t *d_levels, int32_t *d_dqcoef, size_t n, int coef_per_blk,
                     int dc_q, int ac_q, int log_scale, int bd);

/* ---- K3: intra prediction of a list of equally-sized transform blocks (AV1 spec §7.11.2).
 * d_ref is the reconstructed plane the neighbours are read from, d_dst the plane the prediction is written to
 * (may be the same allocation when no listed block is a neighbour of another).  Per block the caller passes what
 * libaom's build_intra_predictors() takes: mode (0 DC, 1 V, 2 H, 3 D45, 4 D135, 5 D113, 6 D157, 7 D203, 8 D67,
 * 9 SMOOTH, 10 SMOOTH_V, 11 SMOOTH_H, 12 PAETH), angle_delta -3..3 (directional modes), and the numbers of
 * AVAILABLE neighbour samples (top <= w, top-right <= w, left <= h, bottom-left <= h). */
typedef struct av1mi_intra_blk {
  uint16_t x, y;       /* top-left sample; x multiple of 4 */
  uint8_t mode;
  int8_t angle_delta;
  uint8_t flags;       /* bit 0: disable intra edge filter; bit 1: filter type (a neighbour is smooth-predicted) */
  uint8_t n_top, n_topright, n_left, n_bottomleft;
  uint8_t reserved[5];
} av1mi_intra_blk;
int av1mi_intra_pred_list(av1mi_ctx *ctx, int tx_size, const void *d_ref, int ref_stride, void *d_dst, int dst_stride,
                          int bd, const av1mi_intra_blk *d_list, int nblocks);

/* ---- K3, chroma-from-luma (AV1 spec §7.11.5; SURVEY.md §8f rank 4 "remaining intra modes"), 4:2:0.  For every listed
 * chroma block (tx_size up to 32x32) d_dst already holds the DC prediction; the block becomes
 *   Clip1(dc + Round2Signed(alpha_q3 * (L - avg L), 6)),  L = (2x2 sum of the reconstructed luma) << 1,
 * with luma coordinates limited to max_luma_w - 2 / max_luma_h - 2 (the spec's MaxLumaW / MaxLumaH).  alpha_q3 in -16..16. */
typedef struct av1mi_cfl_blk {
  uint16_t x, y;                 /* chroma block position in the chroma plane; x multiple of 4 */
  uint16_t max_luma_w, max_luma_h;
  int8_t alpha_q3;
  uint8_t reserved[7];
} av1mi_cfl_blk;
int av1mi_cfl_pred_list(av1mi_ctx *ctx, int tx_size, const void *d_luma, int luma_stride, void *d_dst, int dst_stride, int bd,
                        const av1mi_cfl_blk *d_list, int nblocks);

/* ---- K4: sub-pel motion compensation (AV1 spec §7.11.3.4; single reference, unscaled, no compound) of a list
 * of blocks of one size.  size_id uses the TX_SIZE numbering for w x h (0 4x4 .. 4 64x64, 5 4x8 ...).  Each block
 * at (x, y) of the plane (x multiple of 4) is predicted from d_ref displaced by (mvx, mvy) in 1/16-sample units of
 * THIS plane; reference coordinates are clamped to [0, plane_w-1] x [0, plane_h-1].  filt_x / filt_y: 0 regular,
 * 1 smooth, 2 sharp, 3 bilinear (dimensions <= 4 switch to the 4-tap variants as the spec does). */
typedef struct av1mi_mc_blk {
  uint16_t x, y;
  int16_t mvx, mvy;
  uint8_t filt_x, filt_y;
  uint8_t reserved[6];
} av1mi_mc_blk;
int av1mi_mc_list(av1mi_ctx *ctx, int size_id, const void *d_ref, int ref_stride, int plane_w, int plane_h, void *d_dst,
                  int dst_stride, int bd, const av1mi_mc_blk *d_list, int nblocks);

/* ---- K5: deblocking loop filter of one plane (AV1 spec §7.14), both passes in one launch, d_src -> d_dst
 * (different allocations; w, h multiples of 4; strides in samples, multiples of 4).
 * d_mi: (h/4) x (w/4) mode-info units of the PLANE (already subsampled for chroma), one uint32 each:
 *   bits 0-3  log2(transform width), bits 4-7 log2(transform height) of the transform block covering the unit
 *   bits 8-15 filter level used for vertical edges (pass 0), bits 16-23 for horizontal edges (pass 1), 0..63
 *   bit 24    skip && is_inter (inner transform edges are not filtered)
 *   bit 25    the unit's left edge is a prediction-block edge, bit 26 its top edge is one */
int av1mi_deblock_plane(av1mi_ctx *ctx, const void *d_src, int src_stride, void *d_dst, int dst_stride, int w, int h,
                        int bd, int is_chroma, const uint32_t *d_mi, int mi_stride, int sharpness);

/* the same over nframes frames stacked vertically in d_src / d_dst (h rows each); the mode info of frame f starts
 * at d_mi + f * mi_frame_stride (units), mi_frame_stride 0 = one shared map. */
int av1mi_deblock_frames(av1mi_ctx *ctx, const void *d_src, int src_stride, void *d_dst, int dst_stride, int w, int h,
                         int bd, int is_chroma, const uint32_t *d_mi, int mi_stride, size_t mi_frame_stride, int sharpness,
                         int nframes);

/* ---- K6: CDEF (AV1 spec §7.15) of nframes 4:2:0 frames stacked vertically; deblocked planes in, separate planes out.
 * width/height: luma size, multiples of 8.  d_sb_strength: 4 bytes per 64x64 luma block in raster order
 * {y_pri 0..15, y_sec 0..3, uv_pri, uv_sec}; y_pri = 255 switches CDEF off for that block.  d_skip8: one byte per
 * 8x8 luma block, 1 = all of its mode-info units are skipped (block left untouched).  damping 3..6.
 * sb_frame_stride (entries) / skip_frame_stride (bytes) separate the per-frame maps; 0 = one map shared by all frames. */
typedef struct av1mi_cdef_job {
  int width, height, bit_depth, nframes, damping;
  int stride_y, stride_uv;
  const void *d_src_y, *d_src_u, *d_src_v;
  void *d_dst_y, *d_dst_u, *d_dst_v;
  const uint8_t *d_sb_strength; size_t sb_frame_stride;
  const uint8_t *d_skip8; size_t skip_frame_stride;
} av1mi_cdef_job;
int av1mi_cdef_frames(av1mi_ctx *ctx, const av1mi_cdef_job *job);

/* ---- K5 + K6 in one launch: deblocking of the three planes and CDEF of nframes 4:2:0 frames stacked vertically, the deblocked
 * samples never leaving the chip.  d_rec_*: the reconstruction (what av1mi_deblock_frames takes as d_src); d_dst_*: the CDEF output,
 * bit for bit what av1mi_deblock_frames on each plane followed by av1mi_cdef_frames gives.  d_dbl_*: the deblocked planes, of which
 * ONLY the rows loop restoration reads beyond its stripe boundaries are written (luma rows 64k - 10 .. 64k - 7, chroma rows
 * 32k - 6 .. 32k - 3, for k >= 1 with 64k - 8 < height); every other sample keeps what it held.  So d_dbl_* serve av1mi_lr_frames /
 * av1mi_lr_yuv_decide as d_deblocked and nothing else.  width/height: luma size, multiples of 8.  d_mi_y / d_mi_uv: the mode-info
 * units of the luma plane and of a chroma plane (U and V share them), see av1mi_deblock_plane; mi_stride_* in units,
 * mi_frame_stride_* units between frames, 0 = one shared map.  The other fields as in av1mi_cdef_job.  All nine planes distinct. */
typedef struct av1mi_deblock_cdef_job {
  int width, height, bit_depth, nframes, damping, sharpness;
  int rec_stride_y, rec_stride_uv, dbl_stride_y, dbl_stride_uv, dst_stride_y, dst_stride_uv;
  const void *d_rec_y, *d_rec_u, *d_rec_v;
  void *d_dbl_y, *d_dbl_u, *d_dbl_v;
  void *d_dst_y, *d_dst_u, *d_dst_v;
  const uint32_t *d_mi_y, *d_mi_uv; int mi_stride_y, mi_stride_uv; size_t mi_frame_stride_y, mi_frame_stride_uv;
  const uint8_t *d_sb_strength; size_t sb_frame_stride;
  const uint8_t *d_skip8; size_t skip_frame_stride;
} av1mi_deblock_cdef_job;
int av1mi_deblock_cdef_frames(av1mi_ctx *ctx, const av1mi_deblock_cdef_job *job);

/* ---- CDEF search (policy, non-normative): one of 2, 4 or 8 CDEF strength sets chosen per 64 x 64 superblock by squared error
 * against the source.  The frame header lists the sets (cdef_bits = bits), a superblock's index is `bits` literal bits.
 *
 * The candidates.  From the frame's policy set (av1mi_frame_params.cdef_y / cdef_uv): luma (P, S), chroma (p, s); a primary strength
 * is 0 .. 15, a secondary value the 2-bit code (3 means strength 4).  With dbl(x) = min(15, max(1, 2 x)) and up(x) = min(3, x + 1):
 *     c   luma                    chroma
 *     0   (P, S)                  (p, s)                    the policy's set
 *     1   (0, 0)                  (0, 0)                    unfiltered
 *     2   (P >> 1, S)             (p >> 1, s)
 *     3   (dbl(P), S)             (dbl(p), s)
 *     4   (P, up(S))              (p, up(s))
 *     5   (P, 0)                  (p, 0)
 *     6   (dbl(P), up(S))         (dbl(p), up(s))
 *     7   (dbl(dbl(P)), up(S))    (dbl(dbl(p)), up(s))
 * bits = 1, 2, 3 takes the first 1 << bits sets.  Sets that come out equal are legal and stay where they are; they never win a tie.
 * The damping is the policy's.  av1mi_cdef_search_sets writes the sets in the (primary << 2) | secondary form of
 * av1mi_frame_params.cdef_y (entries from 1 << bits on: 0): plain host code, no device; AV1MI_E_INVAL for a null pointer or bits
 * outside 1 .. 3.
 *
 * The cost of candidate c for a superblock: SSE_c, the 64-bit sum over the three planes of the squared difference between the source
 * and the CDEF output with set c, over the superblock's samples INSIDE THE TRUE FRAME SIZE (chroma: the true size halved, rounded up).
 * Skipped 8 x 8 blocks are left unfiltered, as the filter leaves them: they count the same for every c.  The index costs the same
 * literal bits whatever its value, so there is no lambda: the lowest SSE_c wins, on a tie the lowest c.  A superblock whose blocks
 * are all skipped therefore gets 0 (the syntax codes no index for it).
 *
 * av1mi_cdef_search: geometry, d_src_* (the deblocked planes), d_skip8 and skip_frame_stride as in av1mi_cdef_job; d_orig_*: the
 * source planes, same geometry; true_width / true_height: the true frame size (0 = width / height; at most width / height, and more
 * than width - 8 / height - 8); params: the frame's policy numbers (cdef_y, cdef_uv, cdef_damping are read).  Outputs, device memory:
 *   d_sse        uint64 SSE[frame][sb][8], av1mi_cdef_search_table_bytes() bytes, 8-byte aligned; columns from 1 << bits on hold 0
 *   d_strength   the chosen set's four bytes { y_pri, y_sec, uv_pri, uv_sec } per [frame][sb], 4-byte aligned: what
 *                av1mi_cdef_job.d_sb_strength takes with sb_frame_stride = the superblocks of a frame
 *   d_idx        the chosen index, one byte per [frame][sb]
 * One launch (k_cdef_search, a workgroup per superblock: no atomics, no zeroing), asynchronous on the context's stream, under
 * AV1MI_K_CDEF in the profile. */
struct av1mi_frame_params;      /* below: the session's policy numbers for one frame */
typedef struct av1mi_cdef_search_job {
  int width, height, bit_depth, nframes;
  int stride_y, stride_uv;
  const void *d_src_y, *d_src_u, *d_src_v;
  const void *d_orig_y, *d_orig_u, *d_orig_v;
  const uint8_t *d_skip8; size_t skip_frame_stride;
  int true_width, true_height;
  int bits;
  const struct av1mi_frame_params *params;
  uint64_t *d_sse;
  uint8_t *d_strength;
  uint8_t *d_idx;
} av1mi_cdef_search_job;
int av1mi_cdef_search_sets(const struct av1mi_frame_params *params, int bits, uint8_t y[8], uint8_t uv[8]);
size_t av1mi_cdef_search_table_bytes(int width, int height, int nframes);
int av1mi_cdef_search(av1mi_ctx *ctx, const av1mi_cdef_search_job *job);

/* ---- deblocking search (policy, non-normative): the deblocking levels of a frame chosen among 8 candidates around the policy's by
 * squared error against the source, luma and chroma apart.  The levels are fixed-length bits of the frame header and nothing else.
 *
 * The candidates.  For a frame with policy levels P = av1mi_frame_params.lf_level[0..3] and m[8] = { 4, 0, 2, 3, 5, 6, 8, 12 }:
 *     level(L, 0) = L                                           the policy's level untouched
 *     level(L, c) = min(63, max(lo, (L * m[c] + 2) >> 2))       c = 1 .. 7; lo = 1 for luma, 0 for chroma
 * Luma candidate c filters vertical edges at level(P[0], c) and horizontal edges at level(P[1], c); chroma candidate c filters U and
 * V both at level(P[2], c).  A stated limit: U and V share one level, because the fused kernel (av1mi_deblock_cdef_frames) reads one
 * chroma map for both; P[2] != P[3] is refused.  So is P[0] == P[1] == 0 with P[2] != 0: the frame header carries the chroma levels
 * only behind a non-zero luma level.  Candidates that come out equal are legal and stay where they are; they never win a tie.
 * av1mi_lf_search_levels writes the four header levels of candidate c (luma's and chroma's c alike) to out: plain host code, no
 * device; AV1MI_E_INVAL for a null pointer, c outside 0 .. 7, a level outside 0 .. 63 and the two refusals.
 *
 * The cost.  SSE_y[c]: the 64-bit sum over the luma plane, over the samples INSIDE THE TRUE FRAME SIZE, of the squared difference
 * between the source and the plane deblocked WHOLE at candidate c — both passes, the policy's sharpness.  SSE_uv[c]: the same over U
 * plus V, the true size halved and rounded up.  "Deblocked at candidate c": with the frame's mode-info map in which the two level
 * bytes (bits 8 .. 23) are replaced in every word that does not carry bit 24 — k_mi_levels' hold rule, by which the session marks
 * off-screen units — and everything else of a word stays.  The levels cost the same bits whatever their value, so there is no lambda:
 * per group (luma, chroma) the lowest sum wins, on a tie the lowest c.  The groups are independent: deblocking does not cross planes.
 *
 * av1mi_lf_search: d_rec_* the reconstruction (what av1mi_deblock_frames takes as d_src) and d_orig_* the source of nframes stacked
 * 4:2:0 frames, the same geometry (width / height multiples of 8, strides in samples, multiples of 4, 8-byte aligned planes);
 * true_width / true_height as in av1mi_cdef_search_job; d_mi_y / d_mi_uv: the base maps as in av1mi_deblock_cdef_job (their level
 * bytes are not read); params: the frame's policy numbers (lf_level, lf_sharpness are read).  Device memory:
 *   d_scratch    av1mi_lf_search_scratch_bytes() bytes, 8-byte aligned: uint64 [frame][superblock][2][8], every entry written
 *   d_sse        uint64 SSE[frame][2][8] (luma, chroma), 8-byte aligned
 *   d_choice     uint8 [frame][2]: the chosen luma and chroma candidate
 *   d_levels     uint8 [frame][4], 4-byte aligned: the four header levels (luma vertical, luma horizontal, U, V)
 *   d_mi_y_out / d_mi_uv_out   one patched map per frame, dense: (height / 4) x (width / 4) words a frame (chroma: (height / 8) x
 *                (width / 8)), what av1mi_deblock_frames and av1mi_deblock_cdef_frames take with that row stride and that many units
 *                as mi_frame_stride.  Both null: no maps are wanted; one null is refused.
 * Three launches (k_lf_search: a workgroup per superblock, no atomics, no zeroing; k_lf_pick: a workgroup per frame; k_mi_levels_frames),
 * asynchronous on the context's stream, under AV1MI_K_DEBLOCK in the profile. */
typedef struct av1mi_lf_search_job {
  int width, height, bit_depth, nframes;
  int stride_y, stride_uv;
  const void *d_rec_y, *d_rec_u, *d_rec_v;
  const void *d_orig_y, *d_orig_u, *d_orig_v;
  int true_width, true_height;
  const uint32_t *d_mi_y, *d_mi_uv; int mi_stride_y, mi_stride_uv; size_t mi_frame_stride_y, mi_frame_stride_uv;
  const struct av1mi_frame_params *params;
  void *d_scratch;
  uint64_t *d_sse;
  uint8_t *d_choice;
  uint8_t *d_levels;
  uint32_t *d_mi_y_out, *d_mi_uv_out;
} av1mi_lf_search_job;
#define AV1MI_LF_SEARCH_CANDIDATES 8
int av1mi_lf_search_levels(const struct av1mi_frame_params *params, int c, int out[4]);
size_t av1mi_lf_search_scratch_bytes(int width, int height, int nframes);
int av1mi_lf_search(av1mi_ctx *ctx, const av1mi_lf_search_job *job);

/* ---- K7: loop restoration (AV1 spec §7.17) of one plane of nframes frames stacked vertically.  d_cdef: the CDEF
 * output, d_deblocked: the deblocked (pre-CDEF) plane used beyond stripe boundaries, d_out: the restored plane
 * (distinct from both).  subsampled = 1 for the chroma planes of 4:2:0 (32-row stripes offset by 4), 0 for luma.
 * unit_size: 32 (chroma only), 64, 128 or 256.  d_units: rows x cols entries of 8 bytes, rows =
 * max(1, (h + unit/2) / unit), cols likewise: {type: 0 none / 1 Wiener / 2 self-guided,
 *   Wiener: v0 v1 v2 h0 h1 h2 (int8 taps; the centre tap is 128 - 2*(sum)), pad |
 *   self-guided: set 0..15, xqd0, xqd1 (int8), pad}.  unit_frame_stride: units between frames, 0 = shared. */
int av1mi_lr_frames(av1mi_ctx *ctx, const void *d_cdef, const void *d_deblocked, void *d_out, int stride, int w, int h,
                    int bd, int subsampled, int unit_size, const int8_t *d_units, size_t unit_frame_stride, int nframes);

/* The same restoration followed by the encoder's ON / OFF decision per frame of the plane (policy, non-normative; oracle:
 * av1o_lr_keep): d_on[f * on_stride] = 1 when the restored samples are closer to the source d_orig (same geometry) than the CDEF
 * samples — sum of squared differences, strictly smaller — else 0: the plane the next frame predicts from is then d_cdef's, and
 * the frame header signals lr_type NONE for it.  d_out always receives the restored samples.  d_scratch: device memory of
 * av1mi_lr_decide_scratch_bytes(h, subsampled, nframes) bytes, 8-byte aligned. */
/* The same decision for the three planes of 4:2:0 frames in one call (what the GOP session uses), in two passes: the tiles the
 * decision's sums run over are restored first (an eighth of a large plane), the decision follows, and the other tiles are restored
 * only in the frames that keep their restoration.  So d_out_* hold the restored plane where d_on[f * 3 + plane] == 1; where it is
 * 0 — the next frame predicts from d_cdef_* there — only the sampled tiles were written.  d_scratch: 16-byte aligned,
 * av1mi_lr_yuv_decide_scratch_bytes(height, nframes) bytes.  unit_size applies to the samples of each plane (luma and chroma). */
typedef struct av1mi_lr_decide_job {
  int width, height, bit_depth, nframes, unit_size;
  int stride_y, stride_uv;
  const void *d_cdef_y, *d_cdef_u, *d_cdef_v;
  const void *d_dbl_y, *d_dbl_u, *d_dbl_v;       /* the deblocked planes (rows beside the stripes) */
  void *d_out_y, *d_out_u, *d_out_v;
  const void *d_orig_y, *d_orig_u, *d_orig_v;    /* the source */
  const int8_t *d_units_y, *d_units_uv; size_t unit_frame_stride_y, unit_frame_stride_uv;
  void *d_scratch; uint8_t *d_on;
  int no_self_guided_units;                      /* != 0: the caller promises that no unit record has type 2 (the session's policy:
                                                    Wiener or none) — the kernel then runs without the self-guided path's 18 KB of LDS, at
                                                    twice the occupancy; a type-2 unit would be left unfiltered */
  const int8_t *d_units_v; size_t unit_frame_stride_v;   /* optional: the V plane's own units (what av1mi_lr_search writes); null:
                                                    d_units_uv / unit_frame_stride_uv serve U and V */
} av1mi_lr_decide_job;
size_t av1mi_lr_yuv_decide_scratch_bytes(int height, int nframes);
int av1mi_lr_yuv_decide(av1mi_ctx *ctx, const av1mi_lr_decide_job *job);

/* In place: the column visible_w - 1 of every row replicated into columns [visible_w, w), then row visible_h - 1 into rows
 * [visible_h, h), for nframes stacked frames of one plane (see av1mi_gop_config.visible_width for when an encoder loop needs it). */
int av1mi_extend_frames(av1mi_ctx *ctx, void *d_plane, int stride, int w, int h, int visible_w, int visible_h, int bd, int nframes);
size_t av1mi_lr_decide_scratch_bytes(int h, int subsampled, int nframes);
int av1mi_lr_frames_decide(av1mi_ctx *ctx, const void *d_cdef, const void *d_deblocked, void *d_out, int stride, int w, int h, int bd, int subsampled,
                           int unit_size, const int8_t *d_units, size_t unit_frame_stride, int nframes, const void *d_orig, void *d_scratch, uint8_t *d_on,
                           int on_stride);

/* ---- restoration search (policy, non-normative): a Wiener filter chosen per 64 x 64 restoration unit, or none, by squared error
 * against the source plus the exact cost of the unit's record.
 *
 * The candidates.  Three 1-D filters per plane class, written (tap0, tap1, tap2) of the symmetric 7-tap form (layout of
 * av1mi_lr_frames; chroma filters have tap0 = 0, as the syntax demands):
 *                filter 0  I (identity)   filter 1  D (the policy's, libaom's mid-range taps)   filter 2  L (a low-pass)
 *     luma       ( 0,  0,  0)             ( 3, -7, 15)                                           ( 0,  2, 14)
 *     chroma     ( 0,  0,  0)             ( 0, -7, 15)                                           ( 0,  2, 14)
 * Candidate 0 is "none": the unit is not filtered (record type 0).  Candidate c = 1 .. 8 is the Wiener record with the VERTICAL
 * filter c / 3 and the HORIZONTAL filter c % 3:
 *     c       1      2      3      4      5      6      7      8
 *     v, h    I, D   I, L   D, I   D, D   D, L   L, I   L, D   L, L
 * The pair (I, I) is exactly the identity and is left out; candidate 4 is the record of av1mi_frame_params.
 *
 * The cost of candidate c for a unit, in 64-bit integers:  J_c = SSE_c + lambda * bits_c.  SSE_c: the squared error against the
 * source over the unit's samples of the plane after restoration with c (c = 0: of the CDEF samples).  bits_c
 * (av1mi_lr_search_bits): 1 for the use_wiener symbol plus the literal bits the tile syntax spends on the record's taps, each coded
 * against the default reference taps (3, -7, 15) — exact for this encoder's one superblock per tile, where every tile resets the
 * reference.  lambda (av1mi_lr_search_lambda) = (3 * av1mi_dc_q(qindex, bit_depth)^2) >> 7.  The lowest J wins; on a tie the
 * lowest index.
 *
 * av1mi_lr_search runs the search for the three planes of nframes 4:2:0 frames stacked vertically (geometry, d_cdef_*, d_dbl_*,
 * d_orig_* as in av1mi_lr_decide_job; unit_size must be 64).  Outputs, all device memory:
 *   d_scratch  the cost table, av1mi_lr_search_scratch_bytes() bytes, 16-byte aligned; the call zeroes it.  Afterwards it holds
 *              uint64 SSE[frame][unit][candidate], a frame's units being those of Y, then U, then V, each plane's in raster order
 *              (rows x cols as in av1mi_lr_frames): av1mi_lr_search_units(width, height, 64) of them per frame.
 *   d_units_y / d_units_u / d_units_v   the chosen 8-byte record of every unit, [frame][unit of the plane]: what av1mi_lr_frames
 *              and av1mi_lr_yuv_decide (d_units_y, d_units_uv, d_units_v) take, with the plane's unit count as the frame stride.
 *   d_choice   one byte per unit, [frame][unit] in the cost table's order: the chosen candidate's index.
 * Three launches (the zeroing one, k_lr_search, k_lr_pick), asynchronous on the context's stream; all under AV1MI_K_LR in the profile. */
#define AV1MI_LR_SEARCH_CANDIDATES 9
typedef struct av1mi_lr_search_job {
  int width, height, bit_depth, nframes, unit_size, qindex;
  int stride_y, stride_uv;
  const void *d_cdef_y, *d_cdef_u, *d_cdef_v;
  const void *d_dbl_y, *d_dbl_u, *d_dbl_v;
  const void *d_orig_y, *d_orig_u, *d_orig_v;
  void *d_scratch;
  int8_t *d_units_y, *d_units_u, *d_units_v;
  uint8_t *d_choice;
} av1mi_lr_search_job;
int av1mi_lr_search_units(int width, int height, int unit_size);       /* units of a frame's three planes together */
size_t av1mi_lr_search_scratch_bytes(int width, int height, int unit_size, int nframes);
int av1mi_lr_search_candidate(int chroma, int c, int8_t record[8]);    /* candidate c's record; AV1MI_E_INVAL outside 0 .. 8 */
int av1mi_lr_search_bits(int chroma, int c);                           /* bits_c; -1 outside 0 .. 8 */
long long av1mi_lr_search_lambda(int qindex, int bit_depth);
int av1mi_lr_search(av1mi_ctx *ctx, const av1mi_lr_search_job *job);

/* ---- the intra-only segment pipeline (BASELINE config 2): what stands in for the encode the reference delegates
 * to `ffmpeg -c:v:0 av1_vaapi` (transcode.go:120) for key frames.  One launch codes `nframes` frames that are
 * stacked in the plane buffers (frame f starts at row f*height of the luma planes, f*height/2 of the chroma planes).
 * Every 64x64 superblock is an independent tile; blocks are block_size x block_size (8 or 16; width and height must
 * be multiples of it), transform = block size, DCT_DCT, mode chosen per block by SAD among all 13 intra modes (DC, V, H, 6
 * diagonals, SMOOTH, PAETH, SMOOTH_V, SMOOTH_H; angle delta 0).  Outputs: reconstruction planes, int16 levels (block-contiguous, raster order of blocks, per plane),
 * one mode byte per block for luma and one for the chroma pair. */
typedef struct av1mi_intra_job {
  int width, height, bit_depth, nframes, qindex, block_size;   /* block_size 8 (the session), 16 or 32 (32: closed loop only) */
  int stride_y, stride_uv;                 /* samples; multiples of 4 */
  const void *d_src_y, *d_src_u, *d_src_v; /* source frames */
  void *d_rec_y, *d_rec_u, *d_rec_v;       /* reconstruction (output) */
  int16_t *d_lev_y, *d_lev_u, *d_lev_v;    /* quantised levels (output): nframes * width*height (/4 for chroma) */
  uint8_t *d_modes_y, *d_modes_uv;         /* nframes * (width/bs)*(height/bs) each */
  int open_loop;                           /* mode decision: 0 = closed loop (13 candidates predicted from the reconstruction, inside the
                                              tile's serial chain), 1 = open loop (decided for all blocks at once from the SOURCE frame's
                                              neighbours, then one prediction per block in the chain).  The GOP session codes its key frames closed
                                              loop (AV1MI_INTRA_OPEN_LOOP=1 in the environment switches a session over, for measurements) */
  int frame_rows;                          /* 0 = height.  Otherwise the job codes a BAND of `height` rows of every frame: the frames of a plane
                                              are frame_rows luma rows apart (levels likewise), the pointers address the band's first row */
  int modes_frame_stride;                  /* 0 = the job's blocks per frame; otherwise the mode bytes of consecutive frames are this far apart */
} av1mi_intra_job;
int av1mi_intra_encode(av1mi_ctx *ctx, const av1mi_intra_job *job);

/* ---- the inter (P-frame) pipeline (BASELINE config 3): every 8x8 block predicted from ONE reference frame
 * (the previous reconstructed, loop-filtered frame): integer full search +-search_range (0..15) by SAD, half- and
 * quarter-pel refinement with the regular 8-tap filter, luma + chroma motion compensation (spec §7.11.3.4), then the
 * same DCT_DCT residual coding as the intra pipeline.  nframes independent frames are stacked like in av1mi_intra_job
 * (typically the t-th frames of many closed-GOP segments).  Outputs additionally: one vector per block (int16 x, y in
 * 1/8 luma samples) and one skip byte per block (1 = no non-zero level in Y, U and V). */
typedef struct av1mi_inter_job {
  int width, height, bit_depth, nframes, qindex, search_range;
  int stride_y, stride_uv;
  const void *d_src_y, *d_src_u, *d_src_v;
  const void *d_ref_y, *d_ref_u, *d_ref_v;
  void *d_rec_y, *d_rec_u, *d_rec_v;
  int16_t *d_lev_y, *d_lev_u, *d_lev_v;
  int16_t *d_mvs;       /* nframes * (w/8)*(h/8) * 2 */
  uint8_t *d_skip;      /* nframes * (w/8)*(h/8) */
  /* optional (NULL = not used): the reference per frame and plane without a copy.  d_ref_sel[f * 3 + p] == 0 makes frame f predict
   * plane p from d_ref_alt_* (the CDEF output of the previous frame: its restoration was switched off, av1mi_lr_frames_decide)
   * instead of d_ref_* (the restored planes).  d_ref_sel: 4-byte aligned, allocated up to a multiple of 4 bytes (read as dwords). */
  const void *d_ref_alt_y, *d_ref_alt_u, *d_ref_alt_v;
  const uint8_t *d_ref_sel;
  int coarse_range;     /* 0 (default): the integer search runs around the zero vector.  Otherwise a multiple of 4 up to 64: the coarse search
                           ("motion search" below) gives every 64x64 tile a centre first; its quarter planes and centres live in the context
                           (allocated at the first such job, reused and grown afterwards) */
} av1mi_inter_job;
int av1mi_inter_encode(av1mi_ctx *ctx, const av1mi_inter_job *job);

/* ---- motion search: the optional coarse search in front of the integer search (av1-go_amd/csrc/me_coarse_kernels.hip), and the integer
 * search around its centres (k_me_int, inter_kernels.hip).  Integer arithmetic, bit exact by definition; P = a luma plane of one
 * frame, w x h (multiples of 8).
 *   8-bit view     m8(v) = v >> (bit_depth - 8): what the integer search has always compared.
 *   quarter plane  Q[y][x] = (sum over i, j < 4 of m8(P[4 y + i][4 x + j]) + 8) >> 4, one byte per sample, (w / 4) x (h / 4).  Built for
 *                  the source luma and for the luma plane the frame predicts from (d_ref_y, or d_ref_alt_y where d_ref_sel[f * 3] == 0).
 *   coarse search  per 64x64 tile (tx, ty) of a frame, Rc = coarse_range / 4: the 16 x 16 block of the SOURCE's quarter plane at
 *                  (16 tx, 16 ty) against the reference's quarter plane displaced by every (dx, dy) in [-Rc, Rc]^2; score = the sum of
 *                  absolute differences over all 256 samples; every coordinate of either plane is clamped into [0, w / 4 - 1] x
 *                  [0, h / 4 - 1] (edge replication; this also defines partial tiles).  The winner is the minimum of
 *                  (SAD << 16) | rank, rank = 0 for (0, 0), else 1 + (dy + Rc) (2 Rc + 1) + dx + Rc: ties go to the zero displacement,
 *                  then to raster order.  SAD <= 65 280 and rank <= 1 089: both halves fit.  Centre of the tile = (4 dx, 4 dy) luma samples.
 *   integer search per 8x8 block at (x, y), c = the centre of its tile, R = search_range: every d in [-R, R]^2, score = the sum over the
 *                  block's EVEN rows of |m8(S[y + r][x + k]) - m8(Ref[clamp(y + r + c.y + d.y)][clamp(x + k + c.x + d.x)])| (clamped into
 *                  the plane), winner = the minimum of (SAD << 16) | rank with rank = 0 for d = (0, 0) — the centre itself —, else
 *                  1 + (d.y + R) (2 R + 1) + d.x + R.  The vector handed to the refinement is (c + d) * 8, in 1/8 luma samples.
 *                  Without a coarse search c = (0, 0): the search as it has always been.
 *   range          coarse_range is 0 (off) or a multiple of 4 up to 64; the reach is coarse_range + search_range <= 79 samples: vectors
 *                  stay below 2^10 eighth samples, far inside AV1's +-2^14 and int16. */
/* The search alone, without coding — the per-stage entry the parity tests use.  `job` as for av1mi_inter_encode, of which only the
 * geometry, bit_depth, nframes, search_range, coarse_range, stride_y, d_src_y, d_ref_y, d_ref_alt_y, d_ref_sel and d_mvs are read
 * (the other pointers may be null).  Outputs, all in device memory: d_mvs receives the INTEGER vectors ((c + d) * 8 per block);
 * d_centres (nframes * tiles int16 pairs (x, y), tiles = ceil(w / 64) * ceil(h / 64), raster per frame; 4-byte aligned) the centres —
 * zeros when coarse_range is 0 —; d_q_src / d_q_ref (nframes * (w / 4) * (h / 4) bytes each, rows w / 4 bytes apart, frames stacked;
 * either may be null; untouched when coarse_range is 0) the quarter planes.  Asynchronous on the context's stream. */
int av1mi_me_search(av1mi_ctx *ctx, const av1mi_inter_job *job, uint8_t *d_q_src, uint8_t *d_q_ref, int16_t *d_centres);

/* ---- K9: the AV1 tile entropy coder on the GPU (av1-go_amd/csrc/av1_entropy_kernels.hip).  Codes the outputs
 * of av1mi_intra_encode (key = 1) or av1mi_inter_encode (key = 0) of `nframes` stacked frames in AV1's tile syntax — the tool
 * set of the block pipeline: 8x8 blocks, one 64x64 superblock per tile, TX_MODE_LARGEST, DCT_DCT luma, cdef_bits = 0, Wiener
 * restoration on 64x64 units — byte-identical to the host writer (include/av1mi_host.h), which dav1d verifies.  Output: the tile
 * payloads of all frames back to back in tile order (frame-major, raster inside a frame) in d_out, their sizes in d_tile_size
 * (nframes * tiles entries; tiles = ceil(w / 64) * ceil(h / 64)), and d_total[0] = total bytes, d_total[1] = status (0 = OK; bit 0 /
 * 1: a tile exceeded the coder's op / payload capacity, bit 2: out_cap too small — then the batch must be coded on the host).
 * The frame header and the tile-size fields are added by the host (av1mi_obu_assemble_temporal_unit): they depend on the
 * largest tile.  lr_on / lr_unit_*: the restoration parameters the frames were filtered with (av1mi_frame_params). */
typedef struct av1mi_av1_entropy_job {
  int width, height, nframes, key, base_q_idx;
  const int16_t *d_lev_y, *d_lev_u, *d_lev_v;
  const uint8_t *d_modes_y, *d_modes_uv;       /* key = 1 */
  const int16_t *d_mvs; const uint8_t *d_skip; /* key = 0 */
  int lr_on[3];
  int8_t lr_unit_y[8], lr_unit_uv[8];
  uint8_t *d_out; size_t out_cap;
  uint32_t *d_tile_size;
  uint64_t *d_total;                           /* 2 entries, 8-byte aligned */
  const uint8_t *d_lr_on;                      /* optional: [frame * 3 + plane] 0 switches lr_on[plane] off for that frame */
  int visible_width, visible_height;           /* the true frame size when width / height are it rounded up to 8 (the restoration units
                                                  a tile codes tile the TRUE frame); 0 = width / height */
  int key_rows32;                              /* key = 1: the first key_rows32 luma rows (whole superblock rows; width % 32 == 0) are coded in
                                                  32x32 blocks: their modes one per 32x32 block from entry 0 of d_modes_*, their levels
                                                  block-contiguous over the 32x32 grid; the rows below in 8x8 blocks at their usual places */
} av1mi_av1_entropy_job;
/* The restoration units' own records for a job (the restoration search's choice), beside the job and not inside it: callers built
 * against the job as it stands hand over a struct that ends at key_rows32, and a field behind it would be read from their memory.
 * d_units[p] (Y, U, V): 8-byte records (type 0 none / 1 Wiener), per frame rows x cols in raster order as the units tile the TRUE
 * frame — what av1mi_lr_search writes; null = lr_unit_y / lr_unit_uv serve every unit of the plane.  frame_stride[p]: units between
 * the frames of d_units[p], 0 = one frame's records serve all.  The three pointers are all given or all null, and 8-byte aligned (a
 * record is read as one word); anything else is AV1MI_E_INVAL.  units = NULL: av1mi_av1_entropy_encode_on. */
typedef struct av1mi_av1_entropy_units { const int8_t *d_units[3]; size_t frame_stride[3]; } av1mi_av1_entropy_units;
int av1mi_av1_entropy_encode_units(av1mi_ctx *ctx, const av1mi_av1_entropy_job *job, const av1mi_av1_entropy_units *units, void *stream);
/* The superblocks' CDEF indices for a job (the CDEF search's choice), beside the job for the same reason.  cdef_bits 1 .. 3: every
 * tile codes its superblock's index d_idx[frame * frame_stride + sb] (sb in raster order) as cdef_bits literal bits behind the skip
 * symbol of its first block that is not skipped; d_idx null = index 0 everywhere.  cdef_bits 0 (or cdef = NULL): nothing is coded.
 * Anything else is AV1MI_E_INVAL.  Either side struct may be NULL. */
typedef struct av1mi_av1_entropy_cdef { int cdef_bits; const uint8_t *d_idx; size_t frame_stride; } av1mi_av1_entropy_cdef;
int av1mi_av1_entropy_encode_sides(av1mi_ctx *ctx, const av1mi_av1_entropy_job *job, const av1mi_av1_entropy_units *units,
                                   const av1mi_av1_entropy_cdef *cdef, void *stream);
int av1mi_av1_entropy_encode(av1mi_ctx *ctx, const av1mi_av1_entropy_job *job);
/* the same on another HIP stream of the caller's (hipStream_t passed as void *; NULL = the context's stream) */
int av1mi_av1_entropy_encode_on(av1mi_ctx *ctx, const av1mi_av1_entropy_job *job, void *stream);
uint32_t av1mi_av1_entropy_ops_per_tile(void);
/* measurement: 32-bit list words (one per syntax element) the most recent job handed from the tokenizer to the range coder, summed
 * over its tiles; synchronises the device */
int av1mi_av1_entropy_last_list_words(av1mi_ctx *ctx, uint64_t *words);
uint32_t av1mi_av1_entropy_slot_bytes(void);

/* ---- input formats: the layouts a source batch (segments stacked, stride = width, `rows` = segments * height luma rows) may
 * arrive in.  Every kernel of the block pipeline reads PLANAR; the other three are wire / surface formats that one streaming
 * kernel (av1-go_amd/csrc/input_kernels.hip) turns into planar planes on the device.
 *   PACKED10 halves the zeros on the PCIe link: a 10-bit sample in a 16-bit container carries 6 padding bits, packed planes are
 *     5 / 8 of the bytes.  Normative layout: each plane is ONE little-endian bit string in the planar plane's raster order, sample
 *     i occupies bits [10 i, 10 i + 10).  Equivalently bytes 5k .. 5k + 4 hold samples s0..s3 = 4k .. 4k + 3 as
 *       s0 & 0xff, (s0 >> 8) | (s1 & 0x3f) << 2, (s1 >> 6) | (s2 & 0x0f) << 4, (s2 >> 4) | (s3 & 0x03) << 6, s3 >> 2.
 *     No row or segment padding: width and height are multiples of 8, so a segment's luma plane is a multiple of 64 samples (80
 *     bytes) and its chroma plane a multiple of 16 samples (20 bytes): every segment starts on a 4-byte boundary.
 *   P010 / NV12 are what hardware and most software decoders leave in memory (the reference hands its encoder exactly these,
 *     internal/ffmpeg/transcode.go:99-111,173-178): the luma plane as in PLANAR (P010: the value in bits 15..6 of a uint16, the
 *     low 6 bits are ignored), then ONE plane of rows / 2 rows of width / 2 interleaved (U, V) pairs of the luma's element type. */
enum av1mi_input_format {
  AV1MI_INPUT_PLANAR   = 0,  /* Y, U, V planes, uint8 (8-bit) or uint16 with the value in the low bits (10-bit) */
  AV1MI_INPUT_PACKED10 = 1,  /* bit_depth 10 only: Y, U, V planes, 10 bits per sample, no padding */
  AV1MI_INPUT_P010     = 2,  /* bit_depth 10 only: Y plane uint16 with the value in bits 15..6, then one plane of interleaved U,V pairs */
  AV1MI_INPUT_NV12     = 3   /* bit_depth 8 only: Y plane uint8, then one plane of interleaved U,V pairs */
};
/* bytes of plane 0..2 of a stack of `rows` luma rows (multiple of 8, like width) in `format`; 0 for an invalid combination of
 * format and bit depth, a bad size, and for plane 2 of the semi-planar formats.  No GPU needed. */
size_t av1mi_input_plane_bytes(int format, int bit_depth, int plane, int width, int rows);
/* planar planes in (uint8 / uint16 as PLANAR), the format's planes out (av1mi_input_plane_bytes each; out2 unused by the
 * semi-planar formats); plain host code, no GPU needed.  PACKED10 packs any 4-byte-aligned run of whole 16-sample groups on its
 * own, so the segments of a batch can be packed by different threads into their byte ranges of one buffer (the product's reader
 * threads do).  AV1MI_OK or AV1MI_E_INVAL (null pointer, invalid combination). */
int av1mi_input_pack(int format, int bit_depth, int width, int rows, const void *y, const void *u, const void *v, void *out0, void *out1, void *out2);
/* the conversion on the device, one launch for the three planes: d_in0..2 in `format` (d_in2 ignored by the semi-planar formats)
 * -> planar d_y, d_u, d_v.  Asynchronous on the context's stream; all pointers 16-byte aligned; PLANAR is refused (nothing to do). */
int av1mi_input_convert(av1mi_ctx *ctx, int format, int bit_depth, int width, int rows, const void *d_in0, const void *d_in1, const void *d_in2,
                        void *d_y, void *d_u, void *d_v);

/* ---- chroma formats: sources that are not 4:2:0, or deeper than the coded depth (av1-go_amd/csrc/input_kernels.hip, k_chroma_convert).
 * A source has a chroma layout, source_chroma (4:2:0, 4:2:2, 4:4:4 or 4:0:0 = grey), and a depth, source_bit_depth (8, 10 or 12).  It is
 * coded as 4:2:0 at bit_depth: 8 -> 8, 10 -> 10, 12 -> 10; no other pair of depths is valid.  Integer arithmetic, bit exact by definition.
 * With d = source_bit_depth - bit_depth (0 or 2) and max = (1 << bit_depth) - 1:
 *   layout   the planes of a frame of TRUE luma size w x h lie in buffers of that size rounded up to 8 in both directions, W8 x H8 (uint8
 *            for an 8-bit source, uint16 with the value in the low bits otherwise; frames stacked, no row padding):
 *              luma W8 x H8;  chroma 4:2:0 W8 / 2 x H8 / 2,  4:2:2 W8 / 2 x H8,  4:4:4 W8 x H8,  4:0:0 none.
 *            The TRUE chroma plane size w_p x h_p is ceil(w / 2) x ceil(h / 2), ceil(w / 2) x h and w x h (luma: w x h).
 *   reads    in(x, y) = plane[min(y, h_p - 1)][min(max(x, 0), w_p - 1)]: clamped at the TRUE size.  Nothing beyond it is read; the
 *            buffers' padding may be undefined.
 *   writes   every sample of the 4:2:0 output planes (W8 x H8 luma, W8 / 2 x H8 / 2 chroma; uint8 at bit_depth 8, else uint16), padding
 *            included, by ONE rule:  out = min((S + (1 << (s - 1))) >> s, max), and out = S where s = 0:
 *              luma, and 4:2:0 chroma   S = in(x, y)                                                              s = d
 *              4:2:2 chroma             S = in(x, 2 y) + in(x, 2 y + 1)                                           s = 1 + d
 *              4:4:4 chroma             S = sum over r in {2 y, 2 y + 1} of in(2 x - 1, r) + 2 in(2 x, r) + in(2 x + 1, r)   s = 3 + d
 *              4:0:0                    both chroma planes are 1 << (bit_depth - 1) everywhere
 *            Each output sample is rounded once (all-max 12-bit: (4095 + 2) >> 2 = 1024, hence the min).  The chroma ends up co-sited
 *            with the even luma column and midway between two luma rows: the siting of C420mpeg2, and of what 4:2:2 video carries.
 * The sequence header keeps chroma_sample_position 0 and mono_chrome 0: a grey source is coded as 4:2:0 with flat chroma. */
enum av1mi_source_chroma { AV1MI_CHROMA_420 = 0, AV1MI_CHROMA_422 = 1, AV1MI_CHROMA_444 = 2, AV1MI_CHROMA_400 = 3 };
/* bytes of plane 0..2 of a source stacked to `rows` luma rows (multiple of 8, like width: the buffers' size) in the layout above; 0 for
 * an invalid layout / depth / size and for the chroma planes of a grey source.  No GPU needed. */
size_t av1mi_source_plane_bytes(int source_chroma, int source_bit_depth, int plane, int width, int rows);
/* the conversion on the device, ONE launch for all planes of `frames` stacked frames of TRUE luma size width x height (8 .. 16384):
 * d_in0..2 in the layout above (d_in1 / d_in2 ignored for a grey source) -> the 4:2:0 planes d_y, d_u, d_v at bit_depth.  Where the
 * depths are equal (d = 0) the source's luma plane IS the output's: it is not part of the launch, d_in0 and d_y are ignored and may be
 * null.  Asynchronous on the context's stream; all pointers 16-byte aligned; an invalid layout, pair of depths or size is
 * AV1MI_E_INVAL.  Counted under AV1MI_K_INPUT in the profile. */
int av1mi_chroma_convert(av1mi_ctx *ctx, int source_chroma, int source_bit_depth, int bit_depth, int width, int height, int frames,
                         const void *d_in0, const void *d_in1, const void *d_in2, void *d_y, void *d_u, void *d_v);

/* ---- scaling: the resampler of the input stage (av1-go_amd/csrc/scale_kernels.hip).  Integer arithmetic, bit exact by definition.
 * One dimension, N true source samples -> M output samples, N / M in [1/4, 4]:
 *   taps     T = 2 * ceil(3 * max(N, M) / M) (evaluated in integers: 6 when enlarging or copying, 12 for 2:1, at most 24);
 *   stretch  s = max(N, M) / M;
 *   output j: centre c = ((2 j + 1) N - M) / (2 M)  (= (j + 0.5) N / M - 0.5), first tap first[j] = floor(c) - T / 2 + 1 (floor in integers),
 *            weight of tap k = L((first[j] + k - c) / s), L(x) = sinc(x) sinc(x / 3) for |x| < 3 and 0 beyond (sinc(x) = sin(pi x) / (pi x)), in
 *            double precision; the weights are normalised to sum 1, multiplied by 16384 and rounded to nearest (floor(x + 0.5)); the
 *            rounding remainder 16384 - sum goes to the tap of largest magnitude (the first of equals): EVERY ROW SUMS TO EXACTLY 16384;
 *   source index of tap k = clamp(first[j] + k, 0, N - 1): edge replication at the TRUE size.
 * A plane is resampled horizontally first, t = (sum coef * x + (1 << 9)) >> 10 — a signed 16-bit intermediate that keeps 4 extra bits
 * and is not clamped (>> is the arithmetic shift) —, then vertically, out = clamp((sum coef * t + (1 << 17)) >> 18, 0, 2^bit_depth - 1).
 * Y, U and V are resampled independently by the same rule at their own sizes: chroma N = (N_luma + 1) / 2, M = M_luma / 2, no
 * chroma-siting shift.  N == M gives the unit impulse in every row: that pass is the identity.  Bounds: the largest sum of |coef| of a
 * row is below 1.6 * 16384, so the intermediate stays below 2^15 at 10 bits, a coefficient (at most 16385) fits int16 and both sums int32. */
/* the table for src_n -> dst_n samples (8 .. 4096 each, ratio within [1/4, 4]; else AV1MI_E_INVAL): *taps = T; first[dst_n] and
 * coef[dst_n * T] (row j = the taps of output j) are filled unless first == NULL (then only T is returned, to size coef).  Plain host
 * code, no GPU needed. */
int av1mi_scale_filter(int src_n, int dst_n, int *taps, int32_t *first, int16_t *coef);
/* `frames` stacked frames of three planar planes (uint8 for 8-bit, uint16 otherwise) of TRUE luma size src_w x src_h, in buffers of that
 * size rounded up to 8 in both directions (stride and rows per frame; the half for chroma; nothing beyond the true size is read), ->
 * the planes scaled to dst_w x dst_h in buffers of THAT size rounded up to 8 (the coded size); the padding of the destination receives
 * the last true column / row.  Sizes 16 .. 4096, ratios within [1/4, 4].  One launch, asynchronous on the context's stream; all
 * pointers 16-byte aligned.  Counted under AV1MI_K_INPUT in the profile. */
int av1mi_scale_planes(av1mi_ctx *ctx, int bit_depth, int src_w, int src_h, int dst_w, int dst_h, int frames, const void *const d_src[3],
                       void *const d_dst[3]);

/* ---- quality: per-plane squared error and SSIM of a decoded picture b against the source a (av1-go_amd/csrc/quality_kernels.hip; the
 * arithmetic, shared with the host, in av1-go_amd/csrc/quality.hpp).  Each plane is handled on its own over its TRUE size W x H: luma the
 * frame's true size, chroma (W_luma + 1) / 2 x (H_luma + 1) / 2.  Normative:
 *   sse       sum (a - b)^2 over all W H samples, exact; columns and rows beyond the last whole 4x4 block included.
 *             PSNR (derived on the host) = 10 log10(L^2 W H / sse), L = 2^bit_depth - 1; inf when sse = 0.
 *   SSIM      the 8x8-window, step-4 form of the x264 / FFmpeg `ssim` filter.  4x4 blocks over floor(W / 4) x floor(H / 4), a partial
 *             block at the right or bottom is ignored; per block s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b.  One
 *             window for every (x, y) in [0, floor(W / 4) - 1) x [0, floor(H / 4) - 1): the sum of blocks (x, y), (x + 1, y), (x, y + 1),
 *             (x + 1, y + 1).  Per window, in 64-bit integers:
 *               vars = 64 ss - s1^2 - s2^2,  covar = 64 s12 - s1 s2,
 *               c1 = floor(0.01^2 L^2 64 + 0.5),  c2 = floor(0.03^2 L^2 64 63 + 0.5)      (8 bit: 416, 235963; 10 bit: 6698, 3797644)
 *             then each of the four factors converted to double (all below 2^35: exact) and
 *               ssim = ((2 s1 s2 + c1) (2 covar + c2)) / ((s1^2 + s2^2 + c1) (vars + c2)):
 *             one product above, one below, one IEEE division; no addition follows a product (nothing to contract).
 *   ssim_sum  the sum of the windows' values in double, `windows` their count; the reported SSIM is ssim_sum / windows.  The order of
 *             the additions is fixed per implementation: the device gives the same bits run to run, and agrees with the host twin to
 *             rounding (relative 1e-12).
 *   "All"     SSIM: (4 Y + U + V) / 6; PSNR: from the summed sse over the summed sample counts.
 * A plane with no window cannot be measured: a true luma size under 16 x 16 is AV1MI_E_INVAL. */
typedef struct av1mi_quality { uint64_t sse; double ssim_sum; uint32_t samples, windows; } av1mi_quality;
/* The records of `frames` stacked 4:2:0 frames of TRUE luma size width x height, planar planes (uint8 for 8-bit, uint16 otherwise) in
 * buffers of that size rounded up to 8 in both directions (stride and rows per frame; the half for chroma; nothing beyond the true
 * size is read).  Per (frame, plane) the decoded picture is read from d_dec0, or from d_dec1 where d_select[frame * 3 + plane] == 0
 * (the layout and meaning of the session's restoration flags: 1 = the restored plane, the first candidate); d_select NULL = always
 * d_dec0, and d_dec1 may then be NULL too.  d_out: frames * 3 records [frame * 3 + plane], 8-byte aligned; planes 16-byte aligned.
 * Two launches (tiles, then a fixed-order sum: no atomics), asynchronous on the context's stream; AV1MI_K_QUALITY in the profile.
 * The CPU twin on host pointers, av1mi_quality_planes_host, and the derived figures av1mi_quality_psnr / av1mi_quality_ssim are
 * exported by libav1mi_host.so and declared beside the arithmetic in av1-go_amd/csrc/quality.hpp. */
int av1mi_quality_planes(av1mi_ctx *ctx, int bit_depth, int width, int height, int frames, const void *const d_src[3], const void *const d_dec0[3],
                         const void *const d_dec1[3], const uint8_t *d_select, av1mi_quality *d_out);

/* ---- scene analysis: how much of every frame of a run of consecutive frames its predecessor explains (av1-go_amd/csrc/scene_kernels.hip),
 * and the gather that builds a batch from frames held in device memory.  Integer arithmetic, bit exact by definition; P_f = the luma
 * plane of frame f, in a buffer of W8 x H8 samples (the true size rounded up to 8, the last column / row replicated into the padding).
 *   quarter plane  Q_f, exactly as "motion search" defines it: m8(v) = v >> (bit_depth - 8), Q_f[y][x] = (sum over i, j < 4 of
 *                  m8(P_f[4 y + i][4 x + j]) + 8) >> 4, (W8 / 4) x (H8 / 4) samples.
 *   blocks         8 x 8 quarter samples (32 x 32 luma): block (bx, by), bx < ceil(W8 / 32), by < ceil(H8 / 32), covers the quarter
 *                  samples (x, y) in [8 bx, 8 bx + 8) x [8 by, 8 by + 8).  Q(x, y) below reads Q[clamp(y, 0, H8 / 4 - 1)][clamp(x, 0,
 *                  W8 / 4 - 1)]: every coordinate, displaced or not, is clamped into the plane, so partial blocks replicate the edge.
 *   per frame f >= 1 of the run and block b:
 *                  inter(b) = the minimum over (dx, dy) in [-2, 2]^2 of the sum over the block's 64 samples of
 *                             |Q_f(x, y) - Q_{f-1}(x + dx, y + dy)|;
 *                  intra(b) = the sum of |Q_f(x, y) - m|, m = (sum of Q_f(x, y) + 32) >> 6.
 *                  The frame's record: inter_sad and intra_sad are the sums over all blocks, blocks their number.  Frame 0 of a run has
 *                  no predecessor: inter_sad = 0.  Every sum fits: a block's is at most 64 x 255 = 16 320.
 *   determinism    two stages like the quality records: per-block pairs, then one fixed-order sum per frame; the only atomic is an
 *                  integer minimum.  A run gives the same bytes every time.
 *   a cut          frame f is a cut iff 100 inter_sad >= (100 - scenecut) intra_sad and intra_sad > 0, scenecut in 1..99 the
 *                  sensitivity (the host's rule: av1-go_amd/host/sceneplan.hpp; the product's default is AV1MI_SCENECUT_DEFAULT there).
 * Fades, flashes and cuts nearer to the start of a GOP than its minimum length are not handled. */
typedef struct av1mi_scene_record { uint64_t inter_sad, intra_sad; uint32_t blocks, reserved; } av1mi_scene_record;
/* The records of `frames` (1 .. 65535) consecutive frames whose luma planes are stacked in d_luma: width x height samples each, both
 * multiples of 8 (the buffers' size), uint8 at bit_depth 8, uint16 at 10 or 12.  d_records: `frames` records in device memory, 8-byte
 * aligned; d_luma 16-byte aligned.  Three launches (quarter planes, blocks, sum), asynchronous on the context's stream; the quarter
 * planes and block results live in the context (grown on demand).  AV1MI_K_SCENE in the profile. */
int av1mi_scene_analyse(av1mi_ctx *ctx, int bit_depth, int width, int height, int frames, const void *d_luma, av1mi_scene_record *d_records);
/* The gather, ONE launch: for every segment s < segments and plane p < 3, plane_bytes[p] bytes from d_src_table[s * 3 + p] — a table of
 * segments * 3 device pointers IN DEVICE MEMORY, each 16-byte aligned, or null for a flat slot, which is written as zeros — to
 * d_dst[p] + s * plane_bytes[p]: the stacked layout every stage of a batch reads.  plane_bytes: multiples of 4 (0 = no such plane);
 * d_dst[p] 16-byte aligned.  A 4:2:0 plane of a frame whose size is a multiple of 8 is a multiple of 16 bytes (the smallest: 8 x 8
 * luma = 64 bytes, 4 x 4 chroma = 16) and moves in 16-byte units; any other in single dwords.  Asynchronous on the context's stream;
 * AV1MI_K_SCENE in the profile. */
int av1mi_frames_gather(av1mi_ctx *ctx, const size_t plane_bytes[3], int segments, const void *const *d_src_table, void *const d_dst[3]);

/* ---- bar detection: the black margins of every frame of a sample of frames (av1-go_amd/csrc/crop_kernels.hip), from which the host plans a
 * crop window (av1-go_amd/host/cropplan.hpp).  Integer arithmetic, bit exact by definition; P_f = the luma plane of frame f, TRUE size w x h
 * inside a buffer of W8 x H8 samples (the true size rounded up to 8); m8(v) = v >> (bit_depth - 8), as in "motion search".
 *   sums           row(y) = the sum over x < w of m8(P_f[y][x]);  col(x) = the sum over y < h of m8(P_f[y][x]).  Both fit in 32 bits
 *                  (16384 x 255).  Nothing at or beyond the true size is read: the buffer's padding may be undefined.
 *   dark           a row is dark iff row(y) <= limit * w, a column iff col(x) <= limit * h; limit 0 .. 255 (a MEAN 8-bit level: FFmpeg's
 *                  cropdetect compares the same way; its default is 24).  Column darkness is judged over the full height, bars included.
 *   the record     top = the number of consecutive dark rows from y = 0, bottom = from y = h - 1; left / right the same over columns from
 *                  x = 0 / x = w - 1.  A frame whose rows are all dark has top = bottom = h; all columns dark: left = right = w.
 *   determinism    two stages like the quality and scene records: integer partials in scratch with ONE writer each (per row and tile
 *                  column, per tile row and column), then one workgroup per frame adds them in an order fixed by geometry.  The only
 *                  atomics are integer minima over the indices of the rows / columns that are not dark: the order changes nothing. */
typedef struct av1mi_crop_record { uint32_t top, bottom, left, right; } av1mi_crop_record;
/* The records of `frames` (1 .. 65535) frames whose luma planes are stacked in d_luma as for av1mi_scene_analyse: width x height samples
 * each, both multiples of 8 (the buffers' size), uint8 at bit_depth 8, uint16 at 10 or 12; true_width x true_height the picture inside,
 * less than 8 below the buffer's size.  d_records: `frames` records in device memory, 4-byte aligned; d_luma 16-byte aligned.  Two
 * launches (k_crop_sums reads every sample once and makes both families of sums; k_crop_margins), asynchronous on the context's stream;
 * the partials live in the context (grown on demand).  AV1MI_K_SCENE in the profile. */
int av1mi_crop_analyse(av1mi_ctx *ctx, int bit_depth, int width, int height, int true_width, int true_height, int frames, const void *d_luma, int limit,
                       av1mi_crop_record *d_records);

/* ---- noise records: how much of a source changes from frame to frame where the picture stands still (av1-go_amd/csrc/noise_kernels.hip),
 * from which the host plans the strength of "denoising" below (av1-go_amd/host/noiseplan.hpp, av1mi_plan_denoise of libav1mi_host.so).
 * Integer arithmetic, bit exact by definition; luma only.
 *   pairs          a record describes a pair (A, B) of consecutive frames: planes of TRUE size w x h inside buffers of W8 x H8 samples (the
 *                  true size rounded up to 8); m8(v) = v >> (bit_depth - 8), as in "motion search".
 *   blocks         only the 8 x 8 blocks that lie wholly inside the true size are looked at: block (bx, by), bx < floor(w / 8),
 *                  by < floor(h / 8), covers the samples [8 bx, 8 bx + 8) x [8 by, 8 by + 8).  Nothing at or beyond the true size is read:
 *                  the buffer's padding may be undefined (a true size under 8 in either direction has no block).
 *   per block      on native samples, over the block's 64 samples: S = sum |A - B|;  M = sum m8(A);  S8 = S >> (bit_depth - 8).
 *   eligible       a block is eligible iff 16 x 64 <= M <= 235 x 64.  A block whose mean lies outside the nominal video range is clipped
 *                  or synthetic (black bars, credits, burnt whites): it carries no noise and would pull any low percentile to zero on
 *                  a letterboxed film (has the same trap for the grain records).
 *   bin            min(255, S8 >> 2): one bin is 1/16 of an 8-bit code of mean absolute difference; bin 255 = "16 codes or more", which
 *                  is motion, not noise.
 *   the record     hist[b] = the eligible blocks of bin b; eligible = their number (the sum of hist); blocks = floor(w / 8) x floor(h / 8).
 *   determinism    two stages like the crop, scene and telecine records: per workgroup a histogram in LDS (integer atomics: integer
 *                  addition gives the same bytes in any order), written as integer partials with ONE writer each, then one workgroup per
 *                  pair adds them in an order fixed by geometry.
 *   the plan       (host, av1mi_plan_denoise; a pure function of the records)
 *                  per pair: counted = the sum of hist[0 .. 254].  The pair is VALID iff counted >= 1, 4 counted >= eligible and
 *                  eligible >= floor(blocks / 16): at least a quarter of what could be judged stood still enough to be judged.  Its
 *                  level q = the smallest bin whose cumulative count over bins 0 .. 254 reaches ceil(counted / 4): the lower quartile
 *                  (motion, and texture that moved, only ever add to S: the still blocks are at the low end).
 *                  per file: the valid pairs' q sorted ascending, Q = the one at index floor((n - 1) / 4) (noise is a property of the
 *                  file; motion in some pairs only adds to it).  No valid pair: strength 0.
 *                  sigma in 1/16 code: s16 = (227 Q + 128) >> 8 (the mean |difference| of two independent noises of sigma is 1.128 sigma;
 *                  227 / 256 = 1 / 1.128).
 *                  strength = 0 if s16 < 8 (sigma under half a code: rounding to 8 bits alone gives 0.29), else min(16, (3 s16 + 31) >> 5)
 *                  = ceil(1.5 sigma).  The 1.5 follows from "denoising" below: w_F = 16 - floor(16 MAD / (3 T)), and a sample counts as
 *                  grain iff w_P + w_N >= 24, i.e. w >= 12 per neighbour, i.e. MAD <= 3 T / 4; with MAD = 1.128 sigma that needs
 *                  T >= 1.5 sigma: the smallest strength at which a still, noisy sample is on average counted as grain.
 * The estimate is temporal: a file that moves everywhere in every pair plans 0. */
typedef struct av1mi_noise_record { uint32_t hist[256]; uint32_t eligible, blocks; } av1mi_noise_record;
/* The records of `pairs` (1 .. 32767) pairs whose 2 x pairs luma planes are stacked in d_luma as for av1mi_crop_analyse (pair i = planes
 * 2 i and 2 i + 1): width x height samples each, both multiples of 8 (the buffers' size), uint8 at bit_depth 8, uint16 at 10 or 12;
 * true_width x true_height the picture inside, less than 8 below the buffer's size.  d_records: `pairs` records in device memory, 4-byte
 * aligned; d_luma 16-byte aligned.  Two launches (k_noise_blocks reads every sample of the whole blocks of both planes once, in whole
 * 16-byte units where the rows allow; k_noise_sum), asynchronous on the context's stream; the partials live in the context (grown on
 * demand).  AV1MI_K_SCENE in the profile. */
int av1mi_noise_analyse(av1mi_ctx *ctx, int bit_depth, int width, int height, int true_width, int true_height, int pairs, const void *d_luma,
                        av1mi_noise_record *d_records);

/* ---- peak records: how bright a PQ source gets, per frame, as the histogram of the very code that indexes the tone map's gain[]
 * (av1-go_amd/csrc/peak_kernels.hip), from which the host plans the peak of "tone mapping" below (av1-go_amd/host/peakplan.hpp,
 * av1mi_plan_peak of libav1mi_host.so).  Integer arithmetic, bit exact by definition; restated in numpy in tests/peak_ref.py.
 *   frames         planar 4:2:0 frames of uint16 samples: luma of TRUE size w x h inside a buffer of W8 x H8 samples (the true size rounded
 *                  up to 8), chroma in buffers of W8 / 2 x H8 / 2.  Nothing at or beyond the true size is read (luma x >= w or y >= h,
 *                  chroma x >= ceil(w / 2) or y >= ceil(h / 2)): the buffers' padding may be undefined.
 *   per pixel      (x, y) of the true picture: Y = min(luma[y][x], 1023), U = min(chromaU[y >> 1][x >> 1], 1023), V likewise; then steps 1
 *                  and 2 of "tone mapping" verbatim with u = U - 512, v = V - 512: the same AV1MI_TONE_TO_RGB_* constants, the same >> 14,
 *                  the same clamps to 0 .. 1023, M = max(R', G', B').  With the clamp at 1023 every intermediate fits 32 bits
 *                  (|TO_RGB_Y (Y - 64) + 8192| < 2^25, |TO_RGB_BU u| < 2^25, the sums below 2^26).
 *   the record     hist[M] counts the pixels of code M; pixels = w x h = the sum of hist (16384 x 16384 pixels fit 32 bits).
 *   determinism    two stages like the crop, scene and noise records: per workgroup (a strip of rows of one frame) a histogram in LDS
 *                  (integer atomics: integer addition gives the same bytes in any order), written as integer partials with ONE writer
 *                  each, then one workgroup per frame adds them in an order fixed by geometry.
 *   the plan       (host, av1mi_plan_peak; a pure function of the records and of lin[], the table of av1mi_tone_map_tables, which does
 *                  not depend on the peak)
 *                  per frame: skip = pixels >> 14 (0.006 % of the frame: 506 pixels at 3840 x 2160, 0 for frames under 16384 pixels), so
 *                  that specular glints and hot pixels go.  The frame's code c_f = the largest c with hist[c] + .. + hist[1023] > skip,
 *                  or 0 if there is none.
 *                  per file: C = the maximum of c_f.  The peak belongs to the brightest scene: a maximum, not a quantile over frames.
 *                  peak = min(max((lin[C] + 255) >> 8, 400), 10000) cd/m2 (lin[] is in 2^-8 cd/m2: rounded up).  The floor of 400 is the
 *                  low end of the range over which "tone mapping" bounds gain[]'s monotonicity fix (at most 6 steps, peaks 400 .. 10000);
 *                  it also keeps a dark sample of a bright film from planning a hard clip.
 *                  frames < 1, or a record with pixels == 0: -1.
 *                  The >> 14 and the 400 are POLICY, not measurements: nobody has tuned them on real footage. */
typedef struct av1mi_peak_record { uint32_t hist[1024]; uint32_t pixels; } av1mi_peak_record;
/* The records of `frames` (1 .. 65535) frames whose planes are stacked in d_y, d_u, d_v: luma width x height samples per frame, both
 * multiples of 8 (8 .. 16384: the buffers' size, as for av1mi_crop_analyse), chroma width / 2 x height / 2, uint16; true_width x
 * true_height the picture inside, less than 8 below the buffer's size.  d_records: `frames` records in device memory, 4-byte aligned; the
 * planes 16-byte aligned.  AV1MI_E_INVAL and a text otherwise.  Two launches (k_peak_rows reads every sample of the true picture once, luma
 * in whole 16-byte units, chroma in 8-byte units, a chroma sample once per 2x2 quad; k_peak_sum), asynchronous on the context's stream;
 * the partials live in the context (grown on demand).  AV1MI_K_SCENE in the profile. */
int av1mi_peak_analyse(av1mi_ctx *ctx, int width, int height, int true_width, int true_height, int frames, const void *d_y, const void *d_u, const void *d_v,
                       av1mi_peak_record *d_records);

/* ---- deinterlacing: an interlaced source becomes progressive frames inside the gather (av1-go_amd/csrc/deint_kernels.hip).  AV1 has no
 * interlaced coding and no field signalling: combing that is coded stays in the picture.  The filter is SAME-RATE: one output frame per
 * input frame, at the time of the frame's FIRST field.  Integer arithmetic, bit exact by definition.
 *   geometry  every plane of the fed layout is filtered on its own: true size w x h, buffer size = the true size rounded up to 8 in luma
 *             terms.  Parity k = 0 for top field first (the even lines are the first field and are kept), 1 for bottom field first.  A
 *             run is the frames 0 .. n - 1 of a store; for frame f: C = frame f, P = frame max(f - 1, 0), N = frame min(f + 1, n - 1).
 *             The ends of a run have no neighbour and take the frame itself, as frame 0 of a run has no predecessor in the scene analysis.
 *   lines     lines with y mod 2 == k are copied.  The others are missing; for a missing line y: up = y - 1 if y >= 1 else y + 1,
 *             dn = y + 1 if y + 1 <= h - 1 else y - 1: both are kept lines.  All x arguments below clamp to [0, w - 1].  A plane with
 *             h == 1 is copied.
 *   spatial   a(j) = C[up][x + j], b(j) = C[dn][x + j].  For d in the order 0, -1, +1, -2, +2: score(d) = sum over j in -1 .. 1 of
 *             |a(j + d) - b(j - d)|; the first d whose score is strictly smaller than every earlier one's wins; s = (a(d) + b(-d) + 1) >> 1.
 *   temporal  t0 = P[y][x] (the other field of the previous frame, one field before the kept one), t1 = C[y][x] (one field after it),
 *             t = (t0 + t1 + 1) >> 1.
 *   bound     m = the maximum of (|t0 - t1| + 1) >> 1, (|P[up][x] - a(0)| + |P[dn][x] - b(0)| + 1) >> 1 and the same expression with N
 *             in place of P.
 *   output    min(max(s, t - m), t + m).  A still picture gives m = 0 and the weave, exactly; motion opens the bound to the edge-directed
 *             value.  The buffer's sample at (x, y) beyond the true size is the filter's value at (min(x, w - 1), min(y, h - 1)): the
 *             padding of the output replicates its own edge, which is what the analysis and the block pipeline expect of a fed frame.
 *             Nothing beyond the true size is read: the input's padding may be undefined.
 * FIELD-RATE OUTPUT ("bob": one progressive frame per FIELD, 25i -> 50p).  A run of n source frames gives 2 n output frames; output
 * o = 2 f + phi comes from source frame f with phase phi in {0, 1}, at the time of that frame's first (phi = 0) or second (phi = 1)
 * field.  With k the parity above:
 *   phi = 0   exactly the filter above for frame f: the kept parity is k, t0 = P[y][x], t1 = C[y][x].
 *   phi = 1   the kept lines are those with y mod 2 == 1 - k: up, dn, spatial and output are defined as above on C's lines of THAT
 *             parity.  temporal changes: t0 = C[y][x] (the first field of this frame, one field earlier), t1 = N[y][x] (the first field
 *             of the next frame, one field later).  bound is unchanged: P[up] / P[dn] and N[up] / N[dn] are the fields of the kept
 *             parity before and after.
 *   ends      P and N clamp at the ends of the run as above, so the last frame's second field sees t0 = t1 (and the first frame's first
 *             field, as ever, too).
 * A still picture gives the weave in both phases, exactly; the padding rule is unchanged.  CONSEQUENCE: output (f, phi = 1) is the
 * same-rate filter applied to the time-reversed triple with the opposite parity — filter(P = N, C = C, N = P, parity 1 - k) — because t,
 * the first term of m and the pair of bound terms are symmetric in P and N.
 * Film carried by 3:2 pulldown is not this filter's business: see "inverse telecine" below.  Neighbours across the boundaries of a
 * deinterlacer's run are not built. */
/* The gather with the filter in it, ONE launch for all planes and segments.  d_table: segments * 9 device pointers IN DEVICE MEMORY,
 * [(s * 3 + p) * 3 + i] = plane p of segment s's frame P (i = 0), C (1) and N (2), the run's clamping applied by whoever fills it; a null
 * C makes the slot flat (zeros).  Planes whose rows are whole 16-byte units must be 16-byte aligned, any other 4-byte.  plane_w x
 * plane_h: the buffers' size in samples (0 = no such plane; rows of whole dwords), true_w x true_h the size the filter works at, less than
 * 8 below it.  bit_depth 8 (uint8 samples), 10 or 12 (uint16); parity 0 or 1.  The filtered plane goes to d_dst[p] + s * the plane's
 * bytes (16-byte aligned).  The sources are only read.  Asynchronous on the context's stream; AV1MI_K_SCENE in the profile, like the
 * gather it stands in for. */
int av1mi_deinterlace_gather(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int parity,
                             int segments, const void *const *d_table, void *const d_dst[3]);
/* The same at field rate ("FIELD-RATE OUTPUT" above), ONE launch (k_deint_gather's field-rate instantiation): av1mi_deinterlace_gather's
 * arguments and rules, plus d_phase: `segments` bytes IN DEVICE MEMORY, the phase of each segment's output.  Phases may differ from
 * segment to segment inside one launch.  A value outside 0 .. 1 cannot be checked on the device: only the low bit is read.  A launch
 * whose phases are all 0 writes the bytes av1mi_deinterlace_gather writes.  parity stays the SOURCE's (0 = top field first); the table
 * holds P, C, N of the SOURCE frame o >> 1 of output o. */
int av1mi_deinterlace_gather_fields(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int parity,
                                    int segments, const void *const *d_table, const uint8_t *d_phase, void *const d_dst[3]);

/* ---- inverse telecine: film carried in 30000/1001 video by 3:2 pulldown becomes its 24000/1001 film frames again
 * (av1-go_amd/csrc/telecine_kernels.hip; the plan: av1-go_amd/host/telecineplan.hpp).  Two of every five video frames of such a source hold
 * the fields of two different film frames, and one field of every five is a repeat.  Nothing is filtered: the right fields are WOVEN
 * back together and the frame that carries the repeat is dropped.  Integer arithmetic, bit exact by definition.
 *   fields     the TOP field of a frame is its even lines, the BOTTOM field its odd lines.  The bottom field of every source frame is
 *              kept; its top field is chosen among three candidates.  This covers both field orders and all five phases of the cadence:
 *              the film frame of a combed video frame has its top field in the frame before or after, and the video frame that repeats
 *              a film frame repeats its bottom field.
 *   records    luma only, on m8(v) = v >> (bit_depth - 8), TRUE size w x h inside the buffer; nothing at or beyond the true size is
 *              read.  A run is frames 0 .. n - 1.  For frame f: B = frame f; T_p, T_c, T_n = frames max(f - 1, 0), f, min(f + 1, n - 1)
 *              (an absent neighbour equals c).  For j in p, c, n (comb[0], comb[1], comb[2]):
 *                comb[j] = the sum over even y with 2 <= y <= h - 2 and over x < w of
 *                          max(0, |2 T_j[y][x] - B[y - 1][x] - B[y + 1][x]| - |B[y - 1][x] - B[y + 1][x]| - 8)
 *              : how far the candidate top line lies outside what the kept field's two lines around it explain, above a noise floor of
 *              8.  (h <= 3 has no such line: comb = 0.)
 *                bdiff   = the sum over odd y < h and x < w of |B_f[y][x] - B_{f-1}[y][x]|; frame 0 of a run has no predecessor and
 *                          gets 2^64 - 1.
 *              Every sum fits 64 bits with room (16384 x 16384 x 510 < 2^38).
 *   the plan   (host, av1mi_plan_telecine) the run's first `front` (0 or 1) and last `back` (0 or 1) frames are CONTEXT: analysed, matched
 *              against, never output and never counted.  The n own frames are counted in cycles of 5 from the first own frame.
 *                match   of frame f: the candidate with the smallest comb, ties going to the earlier in the order c, p, n.  The top
 *                        source is f (c), f - 1 (p) or f + 1 (n), clamped into the run; the bottom source is f.
 *                drop    in every complete cycle the frame with the smallest bdiff is dropped, the first on ties; a tail of fewer than
 *                        5 frames drops none.  n frames give n - floor(n / 5) outputs, in order.
 *              PROPERTY: a sequence cut into runs of any multiple of 5 frames, each given the frame before and the frame after as
 *              context where the sequence has one, has the plan of the sequence as one run (every comb and bdiff the plan reads is then
 *              computed from the same three frames).
 *   the weave  every plane is woven on its own by its own row parity: output row y of a plane of true size w x h comes from row
 *              r = min(y, h - 1) of the TOP source if r is even, else of the BOTTOM source; columns at or beyond w repeat column w - 1 of
 *              the same row.  So the output's padding replicates its own edge (the deinterlacer's rule) and the input's padding may be
 *              undefined.  A plane with h == 1 is the top source's row.  Equal sources give that source's true area.
 *   determinism  the records in two stages like the crop and quality records: integer partials in scratch with ONE writer each (per
 *              frame and band of rows), then one workgroup per frame adds them in an order fixed by geometry.  No atomics. */
typedef struct av1mi_telecine_record { uint64_t comb[3]; uint64_t bdiff; } av1mi_telecine_record;
/* The records of a run of `frames` (1 .. 65535) frames whose luma planes are stacked in d_luma as for av1mi_crop_analyse: width x height
 * samples each (multiples of 8, the buffers' size), uint8 at bit_depth 8, uint16 at 10 or 12; true_width x true_height the picture
 * inside, less than 8 below.  d_records: `frames` records in device memory (or pinned host memory), 8-byte aligned; d_luma 16-byte
 * aligned.  Two launches (k_telecine_rows walks the run once per band of rows and reads every sample once per role; k_telecine_sum),
 * asynchronous on the context's stream; the partials live in the context (grown on demand).  AV1MI_K_SCENE in the profile. */
int av1mi_telecine_analyse(av1mi_ctx *ctx, int bit_depth, int width, int height, int true_width, int true_height, int frames, const void *d_luma,
                           av1mi_telecine_record *d_records);
/* The weave gather, ONE launch for all planes and segments; it stands where av1mi_frames_gather stands.  d_table: segments * 6 device
 * pointers IN DEVICE MEMORY, [(s * 3 + p) * 2 + i] = plane p of segment s's top (i = 0) and bottom (1) source; a null top makes the slot
 * flat (zeros).  Planes whose rows are whole 16-byte units must be 16-byte aligned and move in 16-byte units, any other 4-byte aligned, in
 * dwords.  plane_w x plane_h, true_w x true_h, bit_depth (8: uint8 samples; 10 or 12: uint16) and d_dst as av1mi_deinterlace_gather's.
 * The sources are only read.  Asynchronous on the context's stream; AV1MI_K_SCENE in the profile. */
int av1mi_telecine_gather(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int segments,
                          const void *const *d_table, void *const d_dst[3]);

/* ---- denoising: a temporal filter inside the gather (av1-go_amd/csrc/grain_kernels.hip), the deinterlacer's sibling: it removes what
 * changes from frame to frame while the picture stands still — film grain, sensor noise — so that the coder does not spend its bits on
 * it; "grain records" below measure what was removed, and the bitstream asks the decoder to put statistically equal grain back (film
 * grain synthesis; av1-go_amd/host/filmgrain.hpp).  Integer arithmetic, bit exact by definition; samples of 8 or 10 bits.
 *   geometry  as "deinterlacing": every plane of the fed layout is filtered on its own at its true size w x h; a run is the frames
 *             0 .. n - 1 of a store; for frame f: C = frame f, P = frame max(f - 1, 0), N = frame min(f + 1, n - 1).  All coordinates
 *             clamp to [0, w - 1] x [0, h - 1].  The buffer's sample at (x, y) beyond the true size is the output at (min(x, w - 1),
 *             min(y, h - 1)): the padding of the output replicates its own edge.  Nothing beyond the true size is read.
 *   ends      a frame at an end of its run (f = 0 or f = n - 1: P or N is the frame itself) PASSES THROUGH: out = C, and it adds
 *             nothing to the records.  (Averaging with one neighbour would leave 1/2 of the grain's variance where a middle frame
 *             leaves 1/3, and the records' model below would not hold; a run of one or two frames is not filtered at all.)
 *   measure   strength 1 .. 16 in 8-bit code values, T = strength << (bit_depth - 8).  For F in {P, N}:
 *               D_F(x, y) = the sum over the 3x3 neighbourhood of |C - F|                                   (<= 9 x 1023)
 *               w_F = max(0, 16 - floor(16 D_F / (27 T))), computed without a division as
 *               w_F = 16 - ((16 min(D_F, 27 T) R) >> 32),  R = floor(2^32 / (27 T)) + 1                     (a 32 x 32 -> high 32 product)
 *             which is the same number for every D_F and T (16 D R < 2^63; the error of R, below 16 x 27 T / 2^32, cannot reach the
 *             next multiple of 1 / (27 T)).  A mean absolute difference of 3 T / 16 costs one step of weight; at 3 T the weight is 0.
 *   output    den = 16 + w_P + w_N (16 .. 48), num = 16 C + w_P P + w_N N, out = (num K[den] + 2^15) >> 16 with K[den] = round(65536 / den):
 *               K[16 .. 48] = 4096 3855 3641 3449 3277 3121 2979 2849 2731 2621 2521 2427 2341 2260 2185 2114 2048 1986 1928 1872 1820
 *                             1771 1725 1680 1638 1598 1560 1524 1489 1456 1425 1394 1365
 *             This IS the definition, not an approximation of a division.  |den K[den] - 65536| <= 20, so equal samples v <= 1023 give
 *             v back (the error is below 1023 x 20 / 65536 < 1/2): a still, clean picture comes out unchanged, and a sample whose
 *             neighbourhood moved (both weights 0) keeps C exactly.  With 12-bit samples neither would hold: not accepted.
 * ---- grain records: what the filter removed, by intensity.  Per (segment, plane) of a batch a record of 16 bins; a sample of a middle
 * frame of a run inside the true size is COUNTED iff w_P + w_N >= 24 (at least half of the possible weight: its neighbourhood stood
 * still, so r is grain and not motion) and goes to bin out >> (bit_depth - 4), the OUTPUT sample's top four bits, with r = C - out:
 *   sum_sq += r^2, count += 1.
 * All integers: per-workgroup partials in scratch, then one sum per (segment, plane); no floating point, and integer addition gives the
 * same bytes in any order, run to run.  A flat slot and the ends of a run have all-zero records. */
#define AV1MI_GRAIN_BINS 16
typedef struct av1mi_grain_bin { uint64_t sum_sq; uint32_t count, reserved; } av1mi_grain_bin;
typedef struct av1mi_grain_record { av1mi_grain_bin bin[AV1MI_GRAIN_BINS]; } av1mi_grain_record;
/* The gather with the denoiser in it: av1mi_deinterlace_gather's arguments and rules (the table of P, C, N per segment and plane with the
 * run's clamping applied by whoever fills it — an entry P or N EQUAL to C marks an end of the run; a null C makes the slot flat), with
 * strength 1 .. 16 in place of the parity, bit_depth 8 or 10, and the last 16-byte cell of every row starting inside the true width
 * (true of every buffer that is its true size rounded up to 8 in luma terms).  d_records: segments * 3 records [segment * 3 + plane]
 * in device memory (or pinned host memory), 8-byte aligned, written by a second launch (k_grain_sum); NULL = nothing is measured and
 * only k_denoise_gather is launched.  The partials live in the context (grown on demand).  Asynchronous on the context's stream;
 * AV1MI_K_SCENE in the profile, like the gathers it stands in for. */
int av1mi_denoise_gather(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int strength,
                         int segments, const void *const *d_table, void *const d_dst[3], av1mi_grain_record *d_records);

/* ---- motion-compensated denoising: the temporal filter follows the picture.  "denoising" compares a sample with the sample at the same
 * coordinates of P and N; where the picture moves both weights fall to 0 and nothing is removed.  Here a block search stands in front of
 * the filter and the filter reads its neighbours DISPLACED.  Integers only, bit exact by definition.  Everything "denoising" says about
 * geometry, the ends of a run, T, R, K[den], the output's padding and the records holds unchanged; with all vectors 0 this IS that filter.
 *   blocks    the luma plane's true size w0 x h0 is tiled from (0, 0) in blocks of 16 x 16: ceil(w0 / 16) x ceil(h0 / 16) blocks; the last
 *             block of a row or column may be partial, with n samples inside the true size.  A sample (x, y) of plane p, subsampled by
 *             (ssx, ssy) in {0, 1}^2 against luma (from the fed layout's plane sizes: 4:2:0, 4:2:2, 4:4:4 and grey all occur), belongs to
 *             block ((x << ssx) >> 4, (y << ssy) >> 4).
 *   search    range 4 or 8.  For each F in {P, N} every block gets one integer vector (dx, dy), |dx|, |dy| <= range:
 *               SAD(v)  = the sum over the block's n luma samples of |C(x, y) - F(clamp(x + dx), clamp(y + dy))|, full-depth samples,
 *                         coordinates clamped to the true size: every one of the (2 range + 1)^2 candidates is valid at every block;
 *               cost(v) = SAD(v) + (v != 0 ? (n T) >> 2 : 0), T the luma threshold strength << (bit_depth - 8);
 *               the vector is the candidate with the smallest key (cost << 11 | rank); rank 0 is (0, 0), the others follow in raster
 *               order of (dy, dx) from (-range, -range): the zero vector wins ties, then the earliest candidate.
 *             cost <= 256 x 1023 + 256 x (16 << 2) / 4 < 2^19 and rank < 2^11: the key is a dword, and an integer minimum over it is the
 *             same in any order.  The bias keeps still, grainy content at the zero vector: without it the minimum over 289 candidates
 *             picks the neighbour whose noise happens to correlate with C's, and the filter keeps more grain than the records' model
 *             assumes.  It costs real motion half a sigma per sample at T = 2 sigma.
 *   filter    for a sample (x, y) of plane p, its block's vector for F scaled to the plane as (vx, vy) = (dx >> ssx, dy >> ssy)
 *             (arithmetic shifts: floor):
 *               D_F(x, y) = the sum over the 3x3 neighbourhood, (cx, cy) clamped, of |C(cx, cy) - F(clamp(cx + vx), clamp(cy + vy))|.
 *             All nine terms use the vector of the block that holds (x, y), never a neighbouring block's.  The F that enters num is
 *             F(clamp(x + vx), clamp(y + vy)).  Weights, den, K, out, the "counted" rule, the bins and r = C - out are "denoising"'s.
 *             An end of a run passes through and is not searched; a flat slot is zeros.
 *   vectors   one av1mi_denoise_vec per block in block raster order, per segment; an end of a run and a flat slot have zeros.
 * Sub-sample vectors, overlapped blocks and a hierarchical search are not built. */
typedef struct av1mi_denoise_vec { int8_t dx_p, dy_p, dx_n, dy_n; } av1mi_denoise_vec;
/* av1mi_denoise_gather with the search in front of it: its arguments and rules, plus range (4 or 8), a luma plane (plane 0 must exist:
 * it is what is searched), and chroma true sizes that are the luma plane's, halved upwards where the plane is subsampled.  d_vectors:
 * segments * ceil(true_w[0] / 16) * ceil(true_h[0] / 16) records in device memory, 4-byte aligned, [segment * blocks + block]; NULL = the
 * vectors live in the context (grown on demand).  Launches: k_denoise_search (luma, all segments, both neighbours), k_denoise_mc_gather
 * (all planes and segments), and k_grain_sum where d_records is given.  Asynchronous on the context's stream; AV1MI_K_SCENE in the
 * profile. */
int av1mi_denoise_mc_gather(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int strength,
                            int range, int segments, const void *const *d_table, void *const d_dst[3], av1mi_grain_record *d_records, av1mi_denoise_vec *d_vectors);

/* ---- grain covariance: how what the filter removed correlates with its neighbours (av1-go_amd/csrc/grain_cov_kernels.hip).  The grain
 * records say how STRONG the grain was; white grain of that strength on a picture whose grain had a size looks like another, sharper
 * noise.  For a plane of a frame, r(x, y) = C(x, y) - out(x, y) inside the true size w x h, C the fed sample and out what either
 * denoising gather wrote.  For dy = 0 .. 3 and dx = -6 .. 6:
 *   sum[dy][dx + 6] = the sum of r(x, y) r(x + dx, y + dy) over all (x, y) with 0 <= x, x + dx < w and 0 <= y, y + dy < h
 * as signed 64-bit integers (|r| <= 1023, a product is below 2^20).  The entries with dy = 0, dx < 0 follow the same formula and equal
 * their mirror images: one rule, no special case.  Nothing beyond the true size is read; a plane narrower or lower than an offset has no
 * such pair and the entry is 0.  One record per (segment, plane), [segment * 3 + plane], like the grain records.  Integers only, bit
 * exact by definition, and integer addition gives the same bytes in any order, run to run.
 *   offsets   up to (+-6, 3) is what the Yule-Walker equations of AV1's lag-3 neighbourhood need: 24 causal neighbours with dy in -3 .. 0
 *             and dx in -3 .. 3, whose differences reach (+-6, +-3); the covariance at (-dx, -dy) is the one at (dx, dy).
 *   no mask   there is no "counted" rule here, and none is needed.  A sample whose neighbourhood moved keeps C exactly: r = 0, it adds
 *             nothing to any sum, sum[0][6] (the sum of r^2) included.  An end of a run passes through (out = C) and a flat slot has no
 *             C: both give all-zero records without a path of their own.  Only the ratios sum[d] / sum[0][6] are used downstream
 *             (av1-go_amd/host/filmgrain.hpp), so samples that were filtered with part of the weight scale numerator and denominator alike.
 *   limit     a slow change of the picture that the filter half removes is spatially correlated and enters the sums. */
typedef struct av1mi_grain_cov { int64_t sum[4][13]; } av1mi_grain_cov_record;      /* (the plain name is the function's below) */
/* Runs BEHIND av1mi_denoise_gather or av1mi_denoise_mc_gather, with their arguments and rules for the planes, the segments and the table
 * (of which only the C entries are read; a null C means zeros were fed); d_out: the planes that gather wrote (its d_dst), only read here.
 * d_cov: segments * 3 records [segment * 3 + plane] in device memory (or pinned host memory), 8-byte aligned.  Two launches: k_grain_cov
 * (all planes and segments) and k_grain_cov_sum.  The partials live in the context (grown on demand).  Asynchronous on the context's
 * stream; AV1MI_K_SCENE in the profile. */
int av1mi_grain_cov(av1mi_ctx *ctx, int bit_depth, const int plane_w[3], const int plane_h[3], const int true_w[3], const int true_h[3], int segments,
                    const void *const *d_table, void *const d_out[3], av1mi_grain_cov_record *d_cov);

/* ---- tone mapping: an HDR10 source (BT.2020 non-constant luminance, PQ, limited range, 10 bit) becomes BT.709 limited-range SDR at 10 bits
 * (av1-go_amd/csrc/tonemap_kernels.hip, k_tone_map).  Pointwise per 2x2 luma QUAD of planar 4:2:0 planes (four luma samples, one U, one V, the
 * chroma applied to all four), in place.  Integers throughout, bit exact by definition; restated in numpy in tests/tonemap_ref.py.  Every
 * constant below is its formula times 16384, rounded to nearest.  >> is the arithmetic shift.  Per quad, u = U - 512, v = V - 512, and per pixel:
 *   1. R'G'B' as 10-bit full-range PQ codes, from E = (Y - 64) / 876, Cb = u / 896, Cr = v / 896 with Kr = 0.2627, Kb = 0.0593, Kg = 1 - Kr - Kb:
 *        y = TO_RGB_Y * (Y - 64) + 8192;  R' = (y + TO_RGB_RV * v) >> 14;  G' = (y - TO_RGB_GV * v - TO_RGB_GU * u) >> 14;  B' = (y + TO_RGB_BU * u) >> 14
 *      each clamped to 0 .. 1023 (TO_RGB_Y = 1023 / 876, _RV = 2 (1 - Kr) 1023 / 896, _GV = 2 Kr (1 - Kr) / Kg 1023 / 896, _GU = 2 Kb (1 - Kb) / Kg
 *      1023 / 896, _BU = 2 (1 - Kb) 1023 / 896).  Y, U, V outside 64 .. 940 / 64 .. 960 are legal input.
 *   2. M = max(R', G', B').
 *   3. r, g, b = lin[R'], lin[G'], lin[B']: the PQ EOTF (SMPTE ST 2084) of code / 1023 in units of 2^-8 cd/m2 (10000 cd/m2 = 2 560 000).
 *   4. gamut: c_i = max((GAMUT[i][0] r + GAMUT[i][1] g + GAMUT[i][2] b + 8192) >> 14, 0) (64-bit sums).  GAMUT = inverse(RGB709 -> XYZ) *
 *      (RGB2020 -> XYZ) from the primaries' chromaticities and D65 = (0.3127, 0.3290); the rounding remainder of a row goes to its entry of
 *      largest magnitude: EVERY ROW SUMS TO EXACTLY 16384, so grey stays grey.
 *   5. gain: c_i = min((c_i * gain[M] + 32768) >> 16, 25600): the curve, in Q16, then the clamp at 100 cd/m2.
 *   6. BT.709 OETF (4.5 L below 0.018, else 1.099 L^0.45 - 0.099, L = c / 25600) to a code 0 .. 1023: c < 512: oetf_lo[c] (direct).  Otherwise
 *      k = floor(log2 c) (9 .. 14), sh = k - 6, i = (k - 9) * 64 + (c >> sh) - 64, f = c & ((1 << sh) - 1): every octave has 64 intervals, the
 *      nodes oetf_hi[] hold 64 * code (Q6), and the code is min((oetf_hi[i] * ((1 << sh) - f) + oetf_hi[i + 1] * f + (1 << (sh + 5))) >> (sh + 6), 1023).
 *      The interpolation error is below 0.01 code (the curvature falls as fast as the intervals grow).
 *   7. BT.709 Y'CbCr limited (Kr = 0.2126, Kb = 0.0722; scales 876 / 1023 and 896 / 1023): with d(k) = k[0] R + k[1] G + k[2] B over the codes of 6,
 *        Y = 64 + ((d(TO_YUV[0]) + 8192) >> 14) per pixel;  U = 512 + ((sum over the quad of d(TO_YUV[1]) + 32768) >> 16), V with TO_YUV[2]:
 *      the mean of the four pixels' Cb / Cr, rounded once.  The Cb and Cr rows SUM TO EXACTLY 0 (remainder to the entry of largest magnitude).
 *      All three clamped to 0 .. 1023.
 * A neutral quad (U = V = 512) comes out with U = V = 512 exactly, and on that axis Y out never falls as Y in rises.
 * The curve is the BT.2390 EETF from a source of 0 .. peak cd/m2 to a display of 0 .. 100 cd/m2 (black level 0): on PQ signals, e1 = min(e /
 * pq(peak), 1), maxLum = pq(100) / pq(peak), KS = 1.5 maxLum - 0.5, e2 = e1 below KS and the Hermite spline P(e1) of the Report above it, out =
 * e2 pq(peak).  Only the host-built table knows it: gain[M] = round(65536 * eotf(out) / eotf(e)) for e = M / 1023 (65536 where the light is 0),
 * then raised by single steps (at most 6 in all, 0.03 % of the light, for the peaks 400 .. 10000) wherever step 5's result for r = g = b = lin[M] would fall below that for M - 1 (rounding alone can do that where
 * the curve is flat, at and above the peak; the clamp at 100 cd/m2 keeps the steps from adding up). */
#define AV1MI_TONE_LO 512        /* direct OETF entries */
#define AV1MI_TONE_HI 385        /* OETF nodes: 6 octaves of 64 intervals + the last node */
#define AV1MI_TONE_TO_RGB_Y 19133
#define AV1MI_TONE_TO_RGB_RV 27584
#define AV1MI_TONE_TO_RGB_GV 10688
#define AV1MI_TONE_TO_RGB_GU 3078
#define AV1MI_TONE_TO_RGB_BU 35194
#define AV1MI_TONE_GAMUT { { 27206, -9628, -1194 }, { -2041, 18562, -137 }, { -297, -1648, 18329 } }
#define AV1MI_TONE_TO_YUV { { 2983, 10034, 1013 }, { -1644, -5531, 7175 }, { 7175, -6517, -658 } }
typedef struct av1mi_tone_tables {
  uint32_t lin[1024], gain[1024], oetf_lo[AV1MI_TONE_LO], oetf_hi[AV1MI_TONE_HI + 3];      /* what the kernel reads (the last three entries pad to 16 bytes) */
  int32_t to_rgb[5], gamut[3][3], to_yuv[3][3];      /* the constants above, for callers that restate the arithmetic */
  int32_t peak;
} av1mi_tone_tables;
/* all tables for a source peak of 100 .. 10000 cd/m2 (else AV1MI_E_INVAL).  Plain host code in double precision, no GPU needed. */
int av1mi_tone_map_tables(int peak, av1mi_tone_tables *out);
/* `frames` stacked frames of planar 4:2:0 10-bit planes (uint16; luma width x height, width a multiple of 4, height even, up to 16384 each) tone-mapped
 * IN PLACE.  d_tables: an av1mi_tone_tables in device memory, 16-byte aligned; the planes 16-byte aligned.  One launch, asynchronous on the
 * context's stream.  Counted under AV1MI_K_INPUT in the profile. */
int av1mi_tone_map(av1mi_ctx *ctx, int width, int height, int frames, void *d_y, void *d_u, void *d_v, const av1mi_tone_tables *d_tables);

/* ---- depth reduction: 10-bit planar 4:2:0 planes become the 8-bit planes that are coded (av1-go_amd/csrc/depth_kernels.hip, k_depth_reduce;
 * numpy twin: tests/depth_ref.py).  Pointwise, out of place, integer arithmetic, bit exact by definition.  Input: the three planes of `frames`
 * stacked frames, uint16 samples v (0 .. 1023 is what a 10-bit picture holds; the arithmetic below is defined, and computed exactly, for every
 * uint16), at their BUFFER size: W8 x H8 luma, W8 / 2 x H8 / 2 chroma, both multiples of 8.  Output: uint8 planes of the same sizes.  Every
 * sample of the buffers is processed, padding included.  With (x, y) the sample's position in its own plane and p = 0, 1, 2 for Y, U, V:
 *   mode 0 (round)     out = min((v + 2) >> 2, 255)
 *   mode 1 (ordered)   out = min((v + t_p(x, y)) >> 2, 255),  t_p(x, y) = T[y & 1][(x + p) & 1],  T = { { 0, 2 }, { 3, 1 } }
 * The pattern depends on the position only, never on the frame: a still picture stays still, and a P frame does not code the dither again.
 * Over any aligned 2x2 cell of constant v the thresholds are 0, 1, 2, 3 once each, so the four outputs sum to exactly v (where no clamp is
 * hit: v <= 1020): the dither preserves the mean, and a larger (Bayer 8x8) matrix could add nothing to a reduction by two bits.  Plane p's
 * pattern is plane 0's shifted by p columns, so U and V do not dither in step.  Limited range maps onto limited range in both modes: 64 -> 16,
 * 940 -> 235 (multiples of 4 pass every threshold unchanged).  H8 and H8 / 2 are even, so a row's parity inside a batch plane of frames x
 * height rows is its parity inside its frame: the kernel treats the batch as one plane. */
enum av1mi_depth_mode { AV1MI_DEPTH_ROUND = 0, AV1MI_DEPTH_ORDERED = 1 };
/* d_in[p] -> d_out[p], p = Y, U, V: `frames` stacked frames of width x height luma samples (multiples of 8, 8 .. 16384: the buffers' size) and
 * the half-size chroma planes; uint16 in, uint8 out, all six 4-byte aligned, no output overlapping an input.  One launch, asynchronous on the
 * context's stream; counted under AV1MI_K_INPUT in the profile.  AV1MI_E_INVAL for an unknown mode, a size that is not a multiple of 8 or
 * outside 8 .. 16384, frames < 1 (or frames x height beyond 65535 x 32 rows), a null or misaligned plane. */
int av1mi_depth_reduce(av1mi_ctx *ctx, int mode, int width, int height, int frames, const void *const d_in[3], void *const d_out[3]);

/* ---- GOP session: the encoder object a cgo replacement of RunTranscode drives (reference call site
 * internal/daemon/daemon.go:101 -> internal/ffmpeg/transcode.go:194; SURVEY.md §8b "av1mi_open(config) / av1mi_encode /
 * av1mi_flush").  It owns the closed-GOP orchestration and the encoder's filter-parameter POLICY, so that no caller
 * re-implements them: `segments` independent closed GOPs are coded in lockstep (the t-th frames of all of them share every
 * launch: SURVEY.md §8e shards by closed-GOP segment), frame t = 0 of a GOP is a key frame, the others are P frames
 * predicted from the previous frame after deblocking + CDEF + loop restoration.
 *
 * Data path per frame batch: the caller fills the session's pinned host buffers with the source planes
 * (av1mi_gop_acquire_input), av1mi_gop_submit() queues the upload (own copy stream), the block pipeline + in-loop filters
 * (the context's stream) and the download of the frame's SYMBOLS (modes or vectors + skip flags + int16 levels; own copy
 * stream) into pinned host memory; av1mi_gop_collect() waits for the oldest submitted batch and hands those symbols out
 * together with the frame-header parameters the policy chose — exactly what the host bitstream writer
 * (av1-go_amd/host/av1_bitstream.hpp, entropy coding stays on the host cores) needs.  av1mi_gop_max_in_flight() = 3 batches
 * can be in flight: submit(t + 2) before collect(t) overlaps the upload of one batch, the kernels of the next, the GPU coder
 * of the third and the host's work on what was collected. */
typedef struct av1mi_gop_config {
  int width, height;     /* luma samples, multiples of 8 */
  int bit_depth;         /* 8 or 10 */
  int base_q_idx;        /* 1..255 (the reference's only quality knob is DetermineQuality, transcode.go:157-165) */
  int gop_length;        /* frames per closed GOP, >= 1 */
  int segments;          /* closed GOPs coded in lockstep, >= 1 */
  int search_range;      /* integer motion search range in samples, 0..15 */
  int gpu_entropy;       /* 0: the symbols are downloaded, the host entropy-codes them (north_star's split);
                            1: the AV1 tile entropy coder runs on the GPU (side stream), only tile payloads are downloaded;
                            2: both (tests compare the two) */
  /* Sources whose size is not a multiple of 8: width / height above are the CODED size (the true size rounded up to 8; the caller
   * replicates the source's last column / row into the padding of the input planes) and these the TRUE size that goes into the
   * sequence header (av1mi_obu_frame.visible_*); coded - visible < 8; 0 = the coded size.  The session then does what makes a
   * decoder — which works at the coded size except where the spec says FrameWidth / FrameHeight — reconstruct the same pictures:
   * deblocking units that start beyond the true size are not filtered (spec 7.14.2 onScreen), the true last column / row of the
   * deblocked, CDEF and restored planes is replicated into the padding (what the decoder's clamps at lastX / lastY, 7.11.3.4, and
   * PlaneEndX / PlaneEndY, 7.17, read), the restoration units of the tile syntax are counted on the true size. */
  int visible_width, visible_height;
  /* gpu_entropy != 0: where the tile coder runs.  0 (default) = tokenizer + chains on a side stream and the range coder on a third,
   * beside the next batches' block pipeline (fastest); 1 = the whole coder on one side stream; 2 = on the main stream, serialised
   * behind the filters — slower, but every kernel then runs ALONE on the GPU: the arrangement for per-kernel measurements (bench.py
   * `kernels_isolated`, rocprofv3 passes).  The environment variable AV1MI_CODER_STREAMS = split | side | main overrides it. */
  int coder_streams;
  int key_block_size;    /* 0 / 8: key frames in 8x8 blocks like every frame.  32: key frames in 32x32 blocks (luma 32x32 DCT, chroma 16x16,
                            transform type by mode) over every COMPLETE superblock row, 8x8 blocks in a last partial row: +3.7 dB at equal
                            size on the synthetic key frames at q 128, +1.85 dB at q 24.  Needs width % 32 == 0 */
  int input_format;      /* enum av1mi_input_format: the layout of the source the session is fed (pinned buffers of av1mi_gop_acquire_input,
                            device buffers of av1mi_gop_submit_device).  0 = planar.  Anything else adds one conversion launch per batch
                            in front of the block pipeline (k_input_convert) and changes nothing about what is coded */
  /* Scaling (0, 0 = none).  Otherwise the TRUE size of the frames the session is fed; width / height / visible_* above keep their
   * meaning for the coded frame, whose true size (visible_*, or width x height) is the scaling target.  The buffers of
   * av1mi_gop_acquire_input / av1mi_gop_submit_device then hold SOURCE frames, in the session's input_format, at the source size rounded
   * up to 8 in both directions (stacked with that many rows per segment; the padding may be left undefined, it is never read), and
   * one launch per batch (av1mi_scale_planes' kernel, after k_input_convert where the format is not planar) fills the planar planes
   * of the coded size, which are device-only.  16 .. 4096 each, ratio to the target within [1/4, 4]; a source equal to the target is
   * accepted and takes the scaling path (the identity). */
  int source_width, source_height;
  /* != 0: every batch is measured (stage measure_quality behind the in-loop filters: av1mi_quality_planes' two launches on the planar
   * source at the coded size — the scaled / converted frame where the session scales or converts — against the picture a decoder
   * outputs: the restored plane, or the CDEF plane where restoration was switched off) and av1mi_gop_frame.quality carries the
   * records.  0 (default): nothing is launched or allocated.  Needs a true luma size of at least 16 x 16.  Changes nothing about what
   * is coded. */
  int quality_stats;
  /* 0 (default): P frames search +-search_range around the zero vector, as ever; nothing else is allocated or launched.  A multiple of
   * 4 up to 64: the coarse search ("motion search" above; two launches at the head of every P batch, k_me_down + k_me_coarse) gives
   * every 64x64 tile of every segment a centre for the integer search: vectors reach coarse_range + search_range samples.  The
   * quarter planes and centres exist once per session. */
  int coarse_range;
  /* Chroma formats (0, 0 = none: a 4:2:0 source at bit_depth, the session as it has always been — same allocations, same launches).
   * source_chroma: enum av1mi_source_chroma; source_bit_depth: 8, 10 or 12, 0 = bit_depth.  Otherwise the session is FED the source in
   * the layout of "chroma formats" above at the fed size (buffers of av1mi_gop_acquire_input / av1mi_gop_submit_device: sizes
   * av1mi_source_plane_bytes with rows = segments * the fed height; no chroma planes for a grey source), and the stage "chroma" (one
   * launch per batch, k_chroma_convert) runs between "convert" and "scale": it reads the fed buffers at their TRUE size (source_width x
   * source_height where the session scales, else visible_* or width x height) and writes the planar 4:2:0 planes the scaler or the
   * block pipeline reads.  Where the depths are equal the fed luma plane IS the planar luma plane (the caller still replicates the luma
   * edge into its padding when the session does not scale; chroma padding may be undefined).  input_format must be PLANAR.  Scaling,
   * visible_*, quality_stats (measured against the converted frame) and coarse_range work unchanged behind the stage. */
  int source_chroma, source_bit_depth;
  /* The frame store (0 = none: nothing below is allocated, launched or accepted).  Otherwise the session owns TWO stores of store_frames
   * fed frames each, in the fed layout (what av1mi_gop_acquire_input hands out, one frame = one segment's share of it), plus the scene
   * analysis' quarter planes and block results for one store and pinned records.  A group of frames is put into a store in FILE ORDER
   * (av1mi_gop_store_put), analysed (av1mi_gop_store_analyse) and then coded in any layout of segments and positions
   * (av1mi_gop_submit_stored): one launch (k_frames_gather) builds each batch's fed buffers from the store in place of the upload.
   * input_format must be PLANAR; source_chroma / source_bit_depth / scaling work unchanged, because the store holds what the session is
   * fed.  The analysis reads the luma planes' padding: the caller replicates the edge into it (also where the session scales).  Such
   * a session is fed through the store or av1mi_gop_submit_device; av1mi_gop_submit is refused.  At 4K 10-bit, 12 segments x 30
   * frames, the two stores are 2 x 9 GB. */
  int store_frames;
  /* Deinterlacing (0 = none: nothing new is allocated, launched or accepted; 1 = top field first, 2 = bottom field first; "deinterlacing"
   * above).  Needs store_frames > 0 (and with it a planar input_format): the filter looks at the frames before and after each frame, which
   * only the store holds.  av1mi_gop_submit_stored then launches k_deint_gather in place of k_frames_gather: the slot's fed buffers
   * receive the filtered frames, with a run = the frames 0 .. n - 1 the store was last filled with (the highest position put since the
   * store's position 0 was put), and the store itself is never written.  Everything behind the fed buffers is untouched: chroma
   * conversion, scaling, visible_*, quality records (measured against the deinterlaced frame), coarse_range, rate control.
   * av1mi_gop_store_analyse keeps reading the frames AS FED: averaging 4x4 samples blends the two fields, so cuts are found as before.
   * av1mi_gop_submit_device does not deinterlace. */
  int deinterlace;
  /* Denoising (0 = none: nothing new is allocated, launched or accepted; 1 .. 16 = the strength; "denoising" above).  Needs
   * store_frames > 0, like deinterlace and for the same reason; fed samples of 8 or 10 bits; refused together with deinterlace (the
   * chain of the two needs a third copy of a group: DESIGN section 7).  av1mi_gop_submit_stored then launches k_denoise_gather in place
   * of k_frames_gather, with the deinterlacer's table of P, C, N and its run: the slot's fed buffers receive the filtered frames, the
   * first and the last frame of a run pass through, and av1mi_gop_frame.grain carries the batch's grain records.  Everything behind the
   * fed buffers is untouched (the quality records are measured against the denoised frame); av1mi_gop_store_analyse keeps reading the
   * frames as fed; av1mi_gop_submit_device does not denoise. */
  int denoise;
  /* The crop window (0, 0, 0, 0 = none: same allocations, same launches, same bytes as ever).  Otherwise a rectangle (crop_x, crop_y,
   * crop_width, crop_height) of the planar 4:2:0 frame at the fed TRUE size; it applies after "convert" / "chroma" and before "scale".
   * Such a session is fed WHOLE source frames exactly as a scaling session is: source_width x source_height is their true size and is
   * required, the buffers are that size rounded up to 8 (padding undefined, never read), and av1mi_gop_source_layout describes that.
   * Rules: the four numbers are even, the window lies inside the true size and is at least 16 x 16.  The coded true size (visible_*, or
   * width x height) is the target:
   *   equal to the window's size   nothing is resampled: one launch per batch (k_crop_copy, crop_kernels.hip) copies the window to the
   *                                coded planes and replicates the WINDOW's last column / row into their <= 7 padding columns / rows,
   *                                which is what the block pipeline expects of a fed frame;
   *   any other size               the scaler resamples the window to the target exactly as it would a fed frame that WAS the window
   *                                ("scaling" with N = the window's size): its edge clamps sit at the window's edges, not the frame's.
   * MECHANISM: no stage of its own and no plane between.  The window is handed to the last input stage as an origin (crop_y * stride +
   * crop_x samples, the half of either for chroma) and the fed planes' stride: to k_scale, or where nothing is resampled to k_crop_copy,
   * which takes k_scale's place in the chain.  Either way one launch per batch, and neither kernel assumes any alignment of the window's
   * rows beyond the sample's own (an even crop_x starts 8-bit luma rows at any even byte, chroma rows at any byte).
   * DEFINING PROPERTY: nothing outside the window influences anything the session produces.  Fed whole frames, it yields the same tile
   * payloads, symbols, references, quality records and av1mi_gop_download_reference planes, byte for byte, as a session without a
   * window fed the pre-cropped frames.  It composes with every input_format, with source_chroma / source_bit_depth (a 4:4:4 source is
   * cropped after the conversion), the frame store, deinterlace and denoise (which run in the gather on the WHOLE fed frame, before
   * the window), quality_stats (measured against the cropped frame), coarse_range and rate control.
   * KNOWN LIMIT: av1mi_gop_store_analyse and the grain records keep reading whole fed frames, bars included: black bars count as still
   * picture in the scene records and as clean samples in bin 0 of the grain records. */
  int crop_x, crop_y, crop_width, crop_height;
  /* The range of the denoiser's block search (0 = none: nothing new is allocated, launched or accepted; 4 or 8; "motion-compensated
   * denoising" above).  Needs denoise.  av1mi_gop_submit_stored then launches k_denoise_search + k_denoise_mc_gather where it launches
   * k_denoise_gather at range 0; the session owns one scratch of segments x blocks vectors, whose users the main stream orders.  Events,
   * av1mi_gop_frame.grain and everything behind the fed buffers are as with denoise alone; av1mi_gop_submit_device still does not
   * denoise. */
  int denoise_range;
  /* Tone mapping (0 = none: nothing new is allocated, launched or accepted; 1 = BT.2390; "tone mapping" above).  Needs bit_depth 10.  The source
   * is taken to be BT.2020 non-constant luminance, PQ, limited range; every batch becomes BT.709 limited-range SDR at 10 bits before the block
   * pipeline sees it: ONE launch (k_tone_map) behind the last input stage, whatever the chain was, in place on the planar planes at the coded
   * size, over all segments, padding included (the padding of a fed frame replicates its edge, and stays a replica: the map is pointwise per
   * quad and the true size's odd last column / row shares its quad with its replica).  No stage of the chain and no plane of its own; the
   * tables (av1mi_tone_map_tables) are built and uploaded at open.  tone_map_peak: the source's peak in cd/m2, 100 .. 10000; 0 = 1000.
   * Refused with av1mi_gop_submit_device (it would overwrite the caller's planes) and with denoise (the grain records would be measured in the
   * wrong light).  The scene analysis keeps reading the frames as fed; the quality records measure against the tone-mapped source, which is
   * the source as coded; with zero input stages av1mi_gop_download_fed returns the tone-mapped planes (the fed buffer IS the coded plane). */
  int tone_map, tone_map_peak;
  /* The grain covariance (0 = none: nothing new is allocated, launched or accepted, and the session produces the bytes it always did; 1 =
   * on; "grain covariance" above).  Needs denoise; works with and without denoise_range.  av1mi_gop_submit_stored then makes one more
   * pair of launches (k_grain_cov, k_grain_cov_sum) behind the batch's denoising gather, on the same stream and in front of the same
   * event as the grain records; av1mi_gop_frame.grain_cov carries the batch's records.  The fed buffers and everything behind them are
   * untouched: the coded bytes are those of the session without it. */
  int grain_cov;
  /* restoration search ("restoration search"): 0 = every unit of a plane is filtered with the policy's one record, as ever; 1 = a
   * Wiener record or none is chosen per 64 x 64 unit and frame (k_lr_search, k_lr_pick in front of the restoration, on the same
   * stream), the restoration and its per-plane ON / OFF decision run with the chosen units, the GPU coder codes them, and
   * av1mi_gop_frame.lr_units carries them.  Per slot: the three unit arrays, the cost table and the index bytes.  Refused where the
   * units of the coded size and of the true size form different grids.  With 0 nothing of this is allocated or launched. */
  int lr_search;
  /* CDEF search ("CDEF search"): 0 = every superblock is filtered with the policy's one strength set and the stream carries
   * cdef_bits = 0, as ever; N = 1, 2, 3 = cdef_bits = N: one of the first 1 << N sets of av1mi_cdef_search_sets is chosen per 64 x 64
   * superblock and frame against the source.  Every frame size then takes the filters one by one on the main stream —
   * av1mi_deblock_frames per plane, av1mi_cdef_search (k_cdef_search), av1mi_cdef_frames with the chosen records — because the search
   * reads whole deblocked planes; the GPU coder codes the indices, and av1mi_gop_frame.cdef_bits / cdef_y / cdef_uv / cdef_idx carry
   * what the frame header and the host writer need.  Per slot: the cost table, the strength records, the index bytes and their pinned
   * mirror, an event.  Anything outside 0 .. 3 is refused.  With 0 nothing of this is allocated or launched. */
  int cdef_search;
  /* deblocking search ("deblocking search"): 0 = every frame of a batch is deblocked at the policy's levels from one shared map, as
   * ever; 1 = in front of the first deblocking launch of a batch, on the main stream, av1mi_lf_search (k_lf_search, k_lf_pick,
   * k_mi_levels_frames) chooses the levels of every segment's frame against the source and writes a map per frame, which all three
   * deblocking paths (the fused kernel, the unfused path of padded sizes and of cdef_search) then read with a frame stride;
   * av1mi_gop_frame.lf_levels / lf_choice carry the choice and av1mi_session_temporal_unit writes it into the frame header.  Per
   * session: the per-frame maps (the batches are serial on the main stream), the scratch table and the sums; per slot: the level and
   * choice bytes with pinned mirrors, an event.  Anything outside 0 / 1 is refused.  With 0 nothing of this is allocated or launched. */
  int lf_search;
  /* Depth reduction ("depth reduction"; 0, 0 = none: the session codes at bit_depth as it always has — same allocations, same launches, same
   * bytes).  coded_bit_depth: 0 = bit_depth; 8 is valid with bit_depth 10 only (with bit_depth 8 there is nothing to do, and it is refused; 10 with bit_depth 10 means 0).  bit_depth KEEPS
   * its meaning for everything in front of the stage — wire formats, source_bit_depth, chroma conversion, crop, scaler, tone map, frame store,
   * scene analysis, deinterlacing: the depth the input stages work at — and the stage runs at the end of the input chain, BEHIND the tone
   * map: one launch per batch (k_depth_reduce, under AV1MI_K_INPUT) reads the planar planes at the coded size where the chain left them and
   * writes the slot's own uint8 planes.  Per slot: those 10-bit planes (in a session without input stages they are the fed buffers).  In a
   * batch of av1mi_gop_submit_device the stage may read the caller's planes and never writes them (a tone_map session still refuses device
   * batches: the MAP runs in place on the planes it is given).  Everything from the block pipeline on
   * is an 8-bit session: planes and strides, av1mi_policy_frame_params, both intra pipelines and the inter pipeline, motion search, the loop
   * filters and their three searches (against the 8-bit source), tokenizers and coder, the quantiser tables, av1mi_gop_frame.bit_depth, and
   * the quality records (against the source AS CODED, the 8-bit planes: L = 255).  It yields, byte for byte, what a bit_depth 8 session
   * fed the reduced planes yields.  depth_dither: 0 = round, 1 = ordered (enum av1mi_depth_mode); needs coded_bit_depth 8.  Refused with
   * denoise: the grain records are measured in 10-bit codes and the grain would be synthesised into an 8-bit stream. */
  int coded_bit_depth, depth_dither;
  /* Field-rate deinterlacing ("FIELD-RATE OUTPUT" under "deinterlacing"; 0 = none: nothing new is allocated, launched or accepted; 1 =
   * one output frame per field).  Needs deinterlace 1 / 2 and is refused without it.  A store's run of n source frames then stands for
   * 2 n OUTPUT frames, and the index[s] of av1mi_gop_submit_stored is an output position o in 0 .. 2 run - 1 (source frame o >> 1,
   * phase o & 1; -1 stays a flat slot); the gather is k_deint_gather's field-rate instantiation, and the slot's table carries one phase
   * byte per segment behind its pointers, in the same copy.  av1mi_gop_store_put / av1mi_gop_store_analyse keep SOURCE positions and
   * store_frames keeps counting source frames.  Everything behind the gather is unchanged. */
  int deinterlace_fields;
  /* Inverse telecine ("inverse telecine"; 0 = none: nothing new is allocated, launched or accepted; 1 = on).  Needs store_frames > 0; refused
   * together with deinterlace, denoise and AV1MI_INPUT_PACKED10.  Each store then holds store_frames + 2 frames, room for one context
   * frame in front of a group and one behind it: positions 0 .. store_frames + 1 for av1mi_gop_store_put, av1mi_gop_store_telecine and
   * av1mi_gop_submit_woven, which weaves every segment's frame from two store positions (k_telecine_gather in place of k_frames_gather).
   * av1mi_gop_submit_stored keeps its meaning (its positions run over the context frames' room too).  Everything behind the gather sees
   * ordinary fed frames. */
  int telecine;
} av1mi_gop_config;

/* The source layout: what a session opened with a config is FED, as one description.  Everything a caller sizes or strides by — the
 * pinned buffers of av1mi_gop_acquire_input, the device planes of av1mi_gop_submit_device, a frame of the store, what
 * av1mi_gop_download_fed writes — follows from it, and the session itself reads its geometry from nothing else.  One FED frame (one
 * segment's share of a batch) has up to three planes; a batch's plane is `segments` frames stacked: segments * frame_bytes bytes,
 * frame s at byte s * frame_bytes.  (av1mi_input_plane_bytes / av1mi_source_plane_bytes give the same numbers for rows = segments *
 * height: both are linear in the rows.) */
typedef struct av1mi_source_layout {
  int width, height;            /* luma size of a fed frame's BUFFER: the coded size, or where the session scales or crops the source size rounded up to 8 */
  int true_width, true_height;  /* the picture inside it: source_width x source_height where the session scales or crops, else the visible size */
  int bit_depth;                /* of the fed samples: source_bit_depth, or bit_depth */
  struct {
    int width, height;          /* in samples; 0 x 0 = no such plane (the chroma of a grey source, the third plane of P010 / NV12).  The
                                   interleaved plane of P010 / NV12 counts U and V: width x height / 2; PACKED10 counts the samples it packs */
    size_t frame_bytes;         /* one frame of it; 0 = no such plane */
  } plane[3];
} av1mi_source_layout;
/* cfg -> its layout.  Plain host code, no GPU needed.  AV1MI_E_INVAL (and *out untouched) for a null pointer and for every config
 * av1mi_gop_open refuses. */
int av1mi_gop_source_layout(const av1mi_gop_config *cfg, av1mi_source_layout *out);

/* Frame-header parameters chosen by the session's policy for one frame (non-normative encoder choices; the bitstream carries
 * them): deblocking level from the quantiser step (libaom's LPF_PICK_FROM_Q fit, key / inter frames differ for 8-bit), one
 * CDEF strength set and damping from the step, Wiener restoration with fixed taps on 64x64 units. */
typedef struct av1mi_frame_params {
  int frame_type;        /* 0 key frame, 1 inter frame */
  int base_q_idx;
  int lf_level[4];       /* luma vertical, luma horizontal, U, V */
  int lf_sharpness;
  int cdef_damping;
  uint8_t cdef_y, cdef_uv;      /* (primary strength << 2) | secondary code */
  int lr_unit_size;             /* luma and chroma restoration unit size in samples of the plane */
  int8_t lr_unit_y[8], lr_unit_uv[8];   /* the unit record every unit of the plane uses (layout of av1mi_lr_frames) */
} av1mi_frame_params;
/* the policy alone (tests build the oracle's chain from it) */
int av1mi_policy_frame_params(int base_q_idx, int bit_depth, int frame_type, av1mi_frame_params *out);

typedef struct av1mi_gop_frame {    /* one collected frame batch; host pointers into the session's pinned buffers, valid until
                                       the next av1mi_gop_submit */
  av1mi_frame_params params;
  int segments;                     /* batch size */
  size_t blocks_per_frame;          /* (width / 8) * (height / 8); per-block arrays hold segments * blocks_per_frame entries */
  /* the symbols: NULL with gpu_entropy = 1 (the host gets the coded payloads only), unless the GPU coder gave the batch back */
  const uint8_t *y_mode, *uv_mode;  /* key frames: intra modes per 8x8 block (0 DC .. 12 PAETH) */
  const int16_t *mv;                /* inter frames: (x, y) per block in 1/8 luma samples */
  const uint8_t *skip;              /* inter frames: 1 = no non-zero level in the block */
  const int16_t *lev_y, *lev_u, *lev_v;   /* 64 / 16 / 16 levels per block, row-major inside a block */
  /* gpu_entropy != 0: the finished tile payloads of the batch, frame-major / raster inside a frame, back to back */
  int tiles_per_frame;
  const uint32_t *tile_size;        /* segments * tiles_per_frame entries */
  const uint8_t *tile_payload;
  uint64_t payload_bytes;
  /* restoration ON (1) / OFF (0) per segment and plane, [segment * 3 + plane]: the encoder keeps params.lr_unit_* for a plane only
   * where it lowered the squared error against the source; an OFF plane is signalled with lr_type NONE in the frame header */
  const uint8_t *lr_on;
  int key_block_size;               /* of this frame: 8, or 32 (key frames of a key_block_size 32 session).  32: y_mode / uv_mode hold, per
                                       segment (stride key_modes_stride bytes), the modes of the 32x32 blocks of the complete superblock rows in
                                       raster order from entry 0, and from byte offset key_modes_band (their place in the 8x8 grid) the 8x8
                                       blocks of the last partial row; the levels
                                       are block-contiguous per region in the same planes (a region's blocks tile its rows of the plane) */
  int key_modes_stride, key_modes_band;
  /* av1mi_gop_config.quality_stats: segments * 3 records [segment * 3 + plane] of this batch (source against the decoded picture, over
   * the true frame size), in pinned memory; NULL when the option is off */
  const av1mi_quality *quality;
  /* av1mi_gop_config.denoise: segments * 3 grain records [segment * 3 + plane] of this batch ("grain records"), in pinned memory; NULL
   * when the option is off (and for a batch of av1mi_gop_submit_device) */
  const av1mi_grain_record *grain;
  /* av1mi_gop_config.grain_cov: segments * 3 covariance records [segment * 3 + plane] of this batch ("grain covariance"), in pinned
   * memory, valid where `grain` is; NULL when the option is off (and for a batch of av1mi_gop_submit_device) */
  const av1mi_grain_cov_record *grain_cov;
  /* av1mi_gop_config.lr_search: the chosen unit records of this batch per plane (Y, U, V), [segment][unit of the plane][8], in pinned
   * memory (what av1mi_obu_frame.lr_units takes for a segment), lr_units_per_frame[p] units per segment; lr_choice: the chosen
   * candidates' indices, [segment][units of Y, U, V end to end].  NULL / 0 when the option is off */
  const int8_t *lr_units[3];
  int lr_units_per_frame[3];
  const uint8_t *lr_choice;
  /* av1mi_gop_config.cdef_search: cdef_bits of this batch's frames, their 1 << cdef_bits strength sets (av1mi_cdef_search_sets of
   * `params`: the batch's frame type and quantiser) and the chosen indices [segment][superblock in raster order] in pinned memory: what
   * av1mi_obu_frame.cdef_bits / cdef_y / cdef_uv / cdef_idx take for a segment.  0 / NULL when the option is off */
  int cdef_bits;
  uint8_t cdef_y[8], cdef_uv[8];
  const uint8_t *cdef_idx;
  /* av1mi_gop_config.lf_search: the deblocking levels of this batch's frames, [segment][4] (luma vertical, luma horizontal, U, V: what
   * av1mi_obu_frame.lf_level takes for a segment, in place of params.lf_level), and the chosen candidates [segment][2] (luma, chroma),
   * in pinned memory.  NULL when the option is off */
  const uint8_t *lf_levels;
  const uint8_t *lf_choice;
  int bit_depth;                    /* of what was coded: av1mi_gop_config.coded_bit_depth, or bit_depth.  What the sequence header and every
                                       writer of this batch's frames take */
} av1mi_gop_frame;

typedef struct av1mi_gop av1mi_gop;
int av1mi_gop_open(av1mi_ctx *ctx, const av1mi_gop_config *cfg, av1mi_gop **out);
void av1mi_gop_close(av1mi_gop *g);
/* pinned host planes for the NEXT batch: segment s occupies rows [s * height, (s + 1) * height) of the luma plane
 * (stride = width samples, uint8 for 8-bit, uint16 otherwise) and the matching rows of the half-size chroma planes.
 * Blocks until the upload that last used these buffers has finished.
 * A session whose input_format is not PLANAR hands out the buffers in THAT format (sizes: av1mi_input_plane_bytes with rows =
 * segments * height): PACKED10 three byte buffers, P010 / NV12 the luma plane in *y, the interleaved plane in *u and *v = NULL.
 * A session with source_chroma / source_bit_depth hands out planes of av1mi_source_plane_bytes each; grey sources: *u = *v = NULL.
 * av1mi_gop_source_layout says all of this for a config: plane p holds segments * plane[p].frame_bytes bytes, NULL where that is 0. */
int av1mi_gop_acquire_input(av1mi_gop *g, void **y, void **u, void **v);
/* queue the batch in the acquired buffers.  frame_type: 0 key, 1 inter, -1 = by position in the GOP (gop_length).
 * AV1MI_E_INVAL when av1mi_gop_max_in_flight() batches are already in flight (collect first).
 * An explicit frame type is all the session needs to know about a GOP: gop_length only drives frame_type -1, and no buffer, table or
 * counter is sized by it.  A caller that gives types may place its key batches freely; the product's planner (host/sceneplan.hpp) lets
 * up to 3/2 gop_length batches lie between two of them. */
int av1mi_gop_submit(av1mi_gop *g, int frame_type);
/* The same for a batch whose source planes are ALREADY in device memory (same layout as the pinned planes: segments stacked, stride =
 * width; in the session's input_format, d_v ignored by P010 / NV12, 16-byte aligned unless PLANAR): no upload is queued, the kernels
 * read the caller's buffers, which must stay valid and unchanged until the batch has been
 * collected.  No av1mi_gop_acquire_input() before it.  (A decoder that leaves its frames in HBM feeds the session this way; bench.py
 * times this path, the bench contract's "inputs already resident in HBM".) */
int av1mi_gop_submit_device(av1mi_gop *g, const void *d_y, const void *d_u, const void *d_v, int frame_type);
/* The quantiser belongs to the BATCH.  Every batch submitted after this call (av1mi_gop_submit, av1mi_gop_submit_device) is coded at
 * base_q_idx, until the next call; a session on which it is never called codes every batch at av1mi_gop_config.base_q_idx and allocates
 * and launches what it always did.  1..255, else AV1MI_E_INVAL (with a text, and nothing changes).  Batches already in flight keep the
 * quantiser they were submitted with.  One value per batch: all its segments share it (the stacked launches take one).  From it follow
 * the batch's av1mi_frame_params (av1mi_policy_frame_params(base_q_idx, bit_depth, frame type): what av1mi_gop_collect hands out in
 * av1mi_gop_frame.params, base_q_idx included), the quantiser of the block pipeline, the default CDF set of the tile coder, the
 * deblocking levels, the CDEF strengths and damping.  The call neither synchronises nor copies anything from the host: where the
 * device-side deblocking maps and CDEF records hold another quantiser's levels than the batch's, one small launch (k_mi_levels) in
 * front of the batch's filters patches the level fields in place. */
int av1mi_gop_set_base_q_idx(av1mi_gop *g, int base_q_idx);
/* ---- the frame store (av1mi_gop_config.store_frames).  `store` is 0 or 1.
 * av1mi_gop_store_put: the count <= segments frames the caller wrote into the buffers of av1mi_gop_acquire_input (frame i where segment
 * i of a batch would lie) go to positions first .. first + count - 1 of the store, on the upload stream; nothing is coded.  In a session
 * with a store av1mi_gop_acquire_input rotates over the session's pinned buffers whatever is in flight, and waits only for the copy that
 * last read the buffer it hands out.  The copy waits (an event, not the host) for every batch submitted so far that reads this store. */
int av1mi_gop_store_put(av1mi_gop *g, int store, int first, int count);
/* The scene analysis over frames 0 .. frames - 1 of the store (a run: frame 0 gets inter_sad 0), `frames` records copied to out.  It
 * runs on the upload stream behind the puts and waits for ITS records only: batches of the other store that are in flight keep running. */
int av1mi_gop_store_analyse(av1mi_gop *g, int store, int frames, av1mi_scene_record *out);
/* A batch from the store: index[s] (segments entries) = the store position of segment s's frame, or -1 for a flat slot (zeros, as the
 * product feeds a segment that has no frame; its output is to be dropped).  The gather stands in for the upload, the stages follow as
 * ever.  frame_type must be 0 or 1: the layout is the caller's.  A later av1mi_gop_store_put into the same store is ordered behind this
 * batch's gather by an event.  In a session with deinterlace_fields index[s] is an OUTPUT position (source position * 2 + phase). */
int av1mi_gop_submit_stored(av1mi_gop *g, int store, const int32_t *index, int frame_type);
/* Inverse telecine (av1mi_gop_config.telecine; both are refused in a session without it).  av1mi_gop_store_telecine: the field-match records
 * ("inverse telecine") of the run of frames 0 .. frames - 1 of the store, context frames included (frames up to store_frames + 2), copied
 * to out; av1mi_gop_store_analyse's sibling: on the upload stream behind the puts, and it waits for ITS records only.
 * av1mi_gop_submit_woven: av1mi_gop_submit_stored with TWO store positions per segment: segment s's frame is woven from the top field
 * (even lines) of position top[s] and the bottom field of position bottom[s]; top[s] = -1 is a flat slot.  The weave gather is launched in
 * place of k_frames_gather and is ordered against later puts by the same event. */
int av1mi_gop_store_telecine(av1mi_gop *g, int store, int frames, av1mi_telecine_record *out);
int av1mi_gop_submit_woven(av1mi_gop *g, int store, const int32_t *top, const int32_t *bottom, int frame_type);
/* wait for the oldest batch in flight and describe its symbols; AV1MI_E_INVAL when nothing is in flight */
int av1mi_gop_collect(av1mi_gop *g, av1mi_gop_frame *out);
/* number of batches in flight (0..av1mi_gop_max_in_flight()) */
int av1mi_gop_max_in_flight(void);
int av1mi_gop_pending(av1mi_gop *g);
/* gpu_entropy != 0: batches whose tiles exceeded the GPU coder's capacity so far.  Such a batch is handed out by
 * av1mi_gop_collect with tile_size == NULL and the symbols filled in instead (the caller entropy-codes it on the host). */
long av1mi_gop_entropy_fallbacks(av1mi_gop *g);
/* the reference frame(s) produced by the LAST submitted batch (after all in-loop filters): host buffers of the stacked-plane
 * sizes; synchronises the session.  For tests and PSNR. */
int av1mi_gop_download_reference(av1mi_gop *g, void *y, void *u, void *v);
/* the fed buffers of the LAST submitted batch as the input stages read them (the session's own device buffers: what the upload, the
 * gather or the deinterlacing gather wrote; not a batch of av1mi_gop_submit_device): host buffers of the sizes av1mi_gop_acquire_input
 * hands out, a null u / v is skipped; synchronises the session.  For tests. */
int av1mi_gop_download_fed(av1mi_gop *g, void *y, void *u, void *v);

/* ---- host-pointer single-block forms (SURVEY.md §8b "per-stage test entry points"): copy in, run the
 * same kernels, copy out, synchronous. */
int av1mi_inv_txfm2d_add(av1mi_ctx *ctx, const int32_t *coef, void *dst, int stride, int tx_size, int tx_type, int bd);
int av1mi_fwd_txfm2d(av1mi_ctx *ctx, const int16_t *resid, int stride, int32_t *coef, int tx_size, int tx_type);

#ifdef __cplusplus
}
#endif
#endif /* AV1MI_H */
