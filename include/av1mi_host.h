/*
 * av1mi_host.h — C ABI of libav1mi_host.so: the host side of the MI355X AV1 backend (entropy coding, OBU packing and the
 * transcode-job contract stay on the host cores).  Together with include/av1mi.h this is everything a
 * cgo replacement of the reference's transcode step binds:
 *
 *   av1mi_run_transcode            stands in for  internal/ffmpeg/transcode.go:194  RunTranscode(ffmpegPath, args) (int, error)
 *   av1mi_obu_assemble_temporal_unit  frame header + tile group around tile payloads the GPU coder produced
 *   av1mi_obu_write_temporal_unit  the bitstream writer alone, for callers that drive the GOP session (av1mi.h av1mi_gop_*)
 *                                  themselves: symbols of one frame in, one AV1 temporal unit (Section-5 OBUs) out
 *
 * Plain C, no C++ types, no exceptions across the boundary, no callbacks; thread-safe (no global state).
 */
#ifndef AV1MI_HOST_H
#define AV1MI_HOST_H
#include <stddef.h>
#include <stdint.h>

#include "av1mi.h"
#include "av1mi_rc.h"   /* the one-pass rate controller: av1mi_rc_open / _next_q / _collected / _close / _qstep / _defaults */

#ifdef __cplusplus
extern "C" {
#endif

/* Film grain synthesis parameters of one frame: the fields of film_grain_params (AV1 spec 5.9.30, semantics 6.8.20) the writer codes,
 * with update_grain = 1 always (no reference's parameters are loaded).  av1mi_film_grain_from_records (av1-go_amd/host/filmgrain.hpp)
 * fills one from a frame's grain records (include/av1mi.h "grain records"); any legal set may be given. */
typedef struct av1mi_film_grain {
  int32_t apply_grain;             /* 0: the frame gets no grain, nothing else is coded */
  int32_t grain_seed;              /* 0 .. 65535 */
  int32_t num_y_points;            /* 0 .. 14 points of the luma scaling function, values strictly increasing */
  uint8_t point_y_value[14], point_y_scaling[14];
  int32_t chroma_scaling_from_luma;
  int32_t num_cb_points, num_cr_points;      /* 0 .. 10; must be 0 when num_y_points is 0 (4:2:0) or chroma_scaling_from_luma is set */
  uint8_t point_cb_value[10], point_cb_scaling[10], point_cr_value[10], point_cr_scaling[10];
  int32_t grain_scaling_minus_8;   /* 0 .. 3 */
  int32_t ar_coeff_lag;            /* 0 .. 3 */
  uint8_t ar_coeffs_y_plus_128[24], ar_coeffs_cb_plus_128[25], ar_coeffs_cr_plus_128[25];
  int32_t ar_coeff_shift_minus_6, grain_scale_shift;      /* 0 .. 3 each */
  int32_t cb_mult, cb_luma_mult, cb_offset;               /* 8, 8 and 9 bits */
  int32_t cr_mult, cr_luma_mult, cr_offset;
  int32_t overlap_flag, clip_to_restricted_range;
} av1mi_film_grain;

/* Colour description and HDR10 static metadata of a stream: what its sequence header says in color_config (AV1 spec 5.5.2, code points of
 * ITU-T H.273) and what the metadata OBUs behind every sequence header carry (spec 5.8.3 / 5.8.4).  A stream has one; give the same record
 * with every frame.  primaries = transfer = matrix = 2 (unspecified), full_range = 0 and no metadata: every byte is what it is without a
 * record.  matrix 0 (identity) is refused: the spec's sRGB special case implies 4:4:4, which is not coded; so are code points above 255. */
typedef struct av1mi_colour {
  int32_t primaries, transfer, matrix;   /* color_primaries, transfer_characteristics, matrix_coefficients; 2 = unspecified */
  int32_t full_range;                    /* color_range: 0 studio swing, 1 full swing */
  int32_t have_mdcv;                     /* the mastering display colour volume below is given (metadata_type 2) */
  uint16_t primary_x[3], primary_y[3];   /* R, G, B chromaticities, 0.16 fixed point */
  uint16_t white_x, white_y;             /* 0.16 fixed point */
  uint32_t luminance_max;                /* cd/m2, 24.8 fixed point */
  uint32_t luminance_min;                /* cd/m2, 18.14 fixed point */
  int32_t have_cll;                      /* the content light level below is given (metadata_type 1) */
  uint16_t max_cll, max_fall;            /* cd/m2 */
} av1mi_colour;

/* Frame description for the bitstream writer.  All block arrays are raster order over the (width/8) x (height/8) grid of
 * 8x8 luma blocks; host pointers.  The tool set that can be described is listed in av1-go_amd/host/av1_bitstream.hpp. */
/* Frame description (plain C: also bound from Python through libav1mi_host.so, and by the cgo shim of INTEGRATION.md). */
/* All block arrays are raster order over the (width/8) x (height/8) grid of 8x8 luma blocks. */
typedef struct av1mi_obu_frame {
  int32_t width, height;       /* luma samples, multiples of 8 */
  int32_t bit_depth;           /* 8 or 10 */
  int32_t frame_type;          /* 0 key frame, 1 inter frame (reference LAST = the previously coded frame) */
  int32_t base_q_idx;          /* 1..255 */
  int32_t lf_level[4];         /* deblocking levels: luma vertical edges, luma horizontal edges, U, V (0..63) */
  int32_t lf_sharpness;        /* 0..7 */
  int32_t cdef_damping;        /* 3..6 */
  int32_t cdef_bits;           /* 0..3: 1 << cdef_bits strength sets */
  uint8_t cdef_y[8];           /* per set: (primary strength 0..15) << 2 | secondary code 0..3 (3 stands for strength 4) */
  uint8_t cdef_uv[8];
  const uint8_t *cdef_idx;     /* per 64x64 superblock (raster), index of its strength set; NULL = all 0 */
  int32_t lr_type[3];          /* per plane: 0 none, 1 Wiener, 2 self-guided, 3 switchable (frame restoration type) */
  int32_t lr_unit_shift;       /* luma restoration unit = 64 << shift (0..2) */
  int32_t lr_uv_shift;         /* chroma unit = luma unit >> lr_uv_shift (0 or 1) */
  const int8_t *lr_units[3];   /* per plane: unit rows x unit cols records of 8 bytes as in include/av1mi.h (av1mi_lr_frames) */
  int32_t reduced_tx_set;      /* 0 or 1 */
  int32_t disable_cdf_update;  /* 0 or 1 */
  int32_t tile_cols_log2, tile_rows_log2;  /* -1 = one superblock per tile (what the GPU pipeline's prediction assumes) */
  const uint8_t *y_mode;       /* intra blocks: 0 DC .. 12 PAETH */
  const int8_t *angle_y;       /* -3..3 for directional modes; NULL = 0 */
  const uint8_t *uv_mode;      /* 0..12, 13 = chroma from luma */
  const int8_t *angle_uv;      /* NULL = 0 */
  const int8_t *cfl_alpha;     /* 2 per block (U, V), -16..16, used where uv_mode == 13; NULL = none */
  const uint8_t *skip;         /* 1 = block coded with skip (no residual); NULL = 0 */
  const uint8_t *tx_type;      /* luma transform type per block (enum av1mi_tx_type); NULL = DCT_DCT */
  const uint8_t *is_inter;     /* inter frames: 1 = inter block (NULL = all inter) */
  const int16_t *mv;           /* inter blocks: (x, y) in 1/8 luma samples, multiples of 2 (quarter-sample precision) */
  const int16_t *lev_y;        /* 64 levels per block, row-major (row = vertical frequency) */
  const int16_t *lev_u, *lev_v;/* 16 levels per block */
  /* The size the decoder outputs, when the source is not a multiple of 8: width / height above are then the CODED size (the
   * true size rounded up to 8, the source edge replicated into the padding) and these the true one, written to the sequence
   * header; coded - visible < 8.  0 = same as width / height.  What the encoder loop must do for such a frame so that a decoder
   * reconstructs the same pictures: av1mi.h, av1mi_gop_config.visible_width. */
  int32_t visible_width, visible_height;
  /* Film grain.  film_grain_present says what the stream's SEQUENCE header says (film_grain_params_present; one value for all frames of a
   * stream): when set, every frame header ends in film_grain_params, written from *film_grain, or as apply_grain = 0 where film_grain is
   * NULL.  A film_grain pointer in a frame whose sequence flag is off is refused.  Both 0 / NULL (the default): every byte is what it
   * was before the fields existed. */
  int32_t film_grain_present;
  const av1mi_film_grain *film_grain;
  /* Colour description + HDR10 static metadata (above).  Read only where a sequence header is written: it goes into color_config, and the
   * metadata OBUs follow the sequence header directly.  NULL (the default): every byte is what it was before the field existed. */
  const av1mi_colour *colour;
} av1mi_obu_frame;

/* One temporal unit: temporal delimiter [+ sequence header] + OBU_FRAME.  threads > 1 codes the tiles on that many host
 * threads.  Returns the size in bytes (the bytes are copied into out when they fit in cap), or -1 when the description
 * cannot be coded (text in err). */
long long av1mi_obu_write_temporal_unit(const av1mi_obu_frame *f, int with_sequence_header, int threads, uint8_t *out, long long cap,
                                        char *err, int errcap);

/* The same temporal unit when the tile payloads were coded by the GPU tile entropy coder (av1mi.h: av1mi_av1_entropy_encode, or
 * the GOP session with gpu_entropy != 0): f carries only the header fields (geometry, base_q_idx, filter parameters; the symbol
 * pointers are not read), payloads = the frame's ntiles finished tile payloads back to back in raster order, sizes[t] bytes each. */
long long av1mi_obu_assemble_temporal_unit(const av1mi_obu_frame *f, const uint8_t *payloads, const uint32_t *sizes, int ntiles,
                                           int with_sequence_header, uint8_t *out, long long cap, char *err, int errcap);

/* A collected GOP-session batch (av1mi.h av1mi_gop_collect) -> the temporal unit of its segment `seg`: what a caller that drives the
 * session itself does per frame (INTEGRATION.md §3 collect()).  Fills the frame description from fr->params and the restoration
 * decision fr->lr_on, then either wraps the segment's GPU-coded tile payloads (fr->tile_size != NULL) or entropy-codes its symbols
 * on `threads` host threads (gpu_entropy = 0, or a batch the GPU coder gave back).  width x height: the CODED size of the session;
 * visible_*: the true size when that is not a multiple of 8 (0 = the coded size).  Same return convention as above. */
long long av1mi_session_temporal_unit(const av1mi_gop_frame *fr, int seg, int width, int height, int bit_depth, int visible_width,
                                      int visible_height, int with_sequence_header, int threads, uint8_t *out, long long cap, char *err,
                                      int errcap);

/* av1mi_session_temporal_unit_grain (include/av1mi_filmgrain.h) is this entry with film grain parameters. */

/* ---- general block structure: every AV1 block size 4x4 .. 64x64 (incl. the 1:2 / 2:1 / 1:4 / 4:1 shapes), every partition type,
 * every transform size (TX_MODE_LARGEST or TX_MODE_SELECT) and all 16 transform types, the four interpolation filters.  It is
 * what the encoder behind transcode.go:120 (`-c:v:0 av1_vaapi`) may emit and what north_star's "4x4-64x64" names; the 8x8
 * description above is the subset the GPU block pipeline produces today.  Symbols are ARBITRARY (tests hand the writer random
 * ones and compare dav1d's decode with the oracle primitives, tests/test_av1_blocks.py).
 * Inter blocks: single reference LAST, coded as NEWMV against an EMPTY prediction list — the writer refuses an inter block that
 * has another inter block of the same tile within the reach of the MV prediction scan (5 units of 4 samples above / to the
 * left, one to the right); av1_bitstream.cpp has the full list for 8x8 blocks. */
typedef struct av1mi_obu_block {
  uint16_t mi_row, mi_col;     /* position in units of 4 luma samples */
  uint8_t bsize;               /* AV1 BLOCK_* order: 4X4 4X8 8X4 8X8 8X16 16X8 16X16 16X32 32X16 32X32 32X64 64X32 64X64 (12), then
                                  4X16 = 16, 16X4, 8X32, 32X8, 16X64, 64X16 = 21 */
  uint8_t skip;                /* no residual */
  uint8_t is_inter;            /* inter frames only */
  uint8_t y_mode, uv_mode;     /* intra blocks: 0 DC .. 12 PAETH; uv_mode 13 = chroma from luma (blocks up to 32x32) */
  int8_t angle_y, angle_uv;    /* -3..3, directional modes of blocks >= 8x8 (BLOCK_* order: also 4x16 / 16x4) */
  int8_t cfl_alpha_u, cfl_alpha_v;
  uint8_t tx_depth;            /* TX_MODE_SELECT: 0..2 halvings of the block's largest transform (intra: tx_depth, inter: txfm_split
                                  down to that depth everywhere); TX_MODE_LARGEST: must be 0 */
  uint8_t interp_filter;       /* inter blocks when the frame's filter is switchable: 0 regular, 1 smooth, 2 sharp */
  uint8_t reserved;
  int16_t mv_x, mv_y;          /* inter blocks: 1/8 luma samples, multiples of 2 */
  uint32_t tx_type_off;        /* first entry of the block in tx_type[]: one byte per LUMA transform block, coding order */
  uint32_t lev_off[3];         /* first level of the block's Y / U / V transform blocks in levels[]: the plane's transform blocks back
                                  to back in coding order, each min(h, 32) rows x min(w, 32) columns, row-major (row = vertical
                                  frequency).  Transform blocks that start outside the frame are not stored (nor coded). */
} av1mi_obu_block;

typedef struct av1mi_obu_blocks {
  av1mi_obu_frame hdr;         /* geometry, quantiser, filter parameters, tiles; its per-8x8 symbol pointers are not read */
  int32_t tx_mode_select;      /* 0 TX_MODE_LARGEST, 1 TX_MODE_SELECT */
  int32_t interp_filter;       /* inter frames: 0 regular, 1 smooth, 2 sharp, 3 bilinear for every block; 4 = switchable per block */
  int32_t high_precision_mv;   /* inter frames: allow_high_precision_mv (vectors in 1/8 luma samples: odd values allowed) */
  const uint8_t *partition;    /* one partition type (0 NONE, 1 HORZ, 2 VERT, 3 SPLIT, 4 HORZ_A, 5 HORZ_B, 6 VERT_A, 7 VERT_B, 8 HORZ_4,
                                  9 VERT_4) per decode_partition() call that starts inside the frame with a block of 8x8 or more, in
                                  decoding order (tiles in raster order, superblocks in raster order inside a tile) */
  size_t n_partition;
  const av1mi_obu_block *blocks;  /* in decoding order */
  size_t n_blocks;
  const uint8_t *tx_type;      /* enum av1mi_tx_type order (DCT_DCT 0 .. H_FLIPADST 15) */
  const int16_t *levels;
} av1mi_obu_blocks;

/* One temporal unit for a general block description; same return convention as av1mi_obu_write_temporal_unit. */
long long av1mi_obu_write_blocks_temporal_unit(const av1mi_obu_blocks *f, int with_sequence_header, uint8_t *out, long long cap,
                                               char *err, int errcap);

/* The drop-in for RunTranscode (transcode.go:194-315): argv as TranscodeArgs (transcode.go:17) builds it — the backend reads
 * "-i <input.y4m>", "-global_quality:v:0 <q>" and the output path (last argument), plus its own "-g", "-av1mi_device",
 * "-av1mi_segments", "-av1mi_gpu_entropy", "-av1mi_key_block_size", "-av1mi_tracks", "-threads", "-av1mi_scale WxH"; "-vf:v:0 <chain>"
 * is evaluated on the source (its scale filters are applied on the GPU, a filter that cannot be applied is an error: INTEGRATION.md §1);
 * "-av1mi_denoise N" (0 = default: off; 1 .. 16 = the strength of the temporal denoiser in the gather, include/av1mi.h "denoising"; the job
 * runs through the frame store; not with -av1mi_pack10 1 or -av1mi_deinterlace), "-av1mi_denoise auto" (the strength is planned per file before the session
 * opens: up to 16 pairs of consecutive frames of a seekable file are measured on the GPU, include/av1mi.h "noise records", and the job is the job
 * -av1mi_denoise N from there on, or with N = 0 the job without the option; refused with everything -av1mi_denoise N is refused with), "-av1mi_denoise_range N" (0 = default, 4 or 8: the filter
 * follows the picture by a block search of that range, include/av1mi.h "motion-compensated denoising"; an error without -av1mi_denoise),
 * "-av1mi_film_grain 0 | 1" (1 by default when denoising:
 * film grain synthesis parameters from what was removed, av1mi_filmgrain.h; an error without -av1mi_denoise);
 * "-av1mi_deinterlace off | auto | tff | bff" (off = default; auto deinterlaces a source whose Y4M header says It / Ib on the GPU, at the
 * same frame rate, and refuses Im; a chain that names yadif, bwdif or deinterlace_vaapi — bare, mode=0 or mode=send_frame — means auto;
 * include/av1mi.h "deinterlacing", av1mi_gop_config.deinterlace); "-av1mi_deinterlace_rate frame | field" (frame = default; field = one
 * output frame per FIELD where the job deinterlaces, at twice the source's frame rate: "-g" then counts output frames and must be even;
 * av1mi_gop_config.deinterlace_fields; the chain's own field-rate spellings stay refused); "-av1mi_ivtc 0 | 1" (0 = default; 1 = inverse
 * telecine, whatever the source's header's I parameter says, from a file or a stream: 4 output frames per 5 source frames at fps x 4 / 5, "-g" counts
 * output frames and must be a multiple of 4; include/av1mi.h "inverse telecine", av1mi_gop_config.telecine; not with -av1mi_deinterlace,
 * -av1mi_denoise, -av1mi_pack10 1 or -av1mi_scenecut);
 * "-av1mi_tonemap_peak N | auto" (with -av1mi_tonemap bt2390 or tonemap_vaapi in the chain: the source's peak in cd/m2, 100 .. 10000; auto =
 * planned per file before the session opens: up to 32 frames of a seekable 4:2:0 10-bit file are measured on the GPU, include/av1mi.h "peak
 * records", and the job is the job -av1mi_tonemap_peak N from there on; the first line of the stats file then holds " peak:auto>N");
 * everything else is accepted and ignored.  Returns 0 and leaves the output file in place on
 * success; -1 when the backend could not run at all (no HIP device: transcode.go:311); another non-zero code on failure.
 * err receives the reference-shaped text ("av1mi failed with exit code N: ...", at most 800 characters + "..."). */
int av1mi_run_transcode(int argc, const char *const *argv, char *err, size_t errcap);

/* libav1mi_host.so also exports the job's plans as functions of their own, for callers that drive the analyses themselves; like
 * av1mi_plan_denoise they are listed here and not declared (tests/test_abi.py pins this header's declarations to the drop-in and the
 * bitstream writers):
 *   int av1mi_plan_peak(const av1mi_peak_record *records, int frames, int32_t *frame_code);
 * the plan of -av1mi_tonemap_peak auto (av1-go_amd/host/peakplan.hpp; the rule: include/av1mi.h "peak records", the plan): `frames` >= 1
 * records of av1mi_peak_analyse in host memory -> the source peak in cd/m2, 400 .. 10000, or -1 (frames < 1, no records, a record with
 * pixels == 0).  frame_code (may be null): `frames` entries, every frame's code c_f.  Plain host code, no GPU. */

#ifdef __cplusplus
}
#endif
#endif /* AV1MI_HOST_H */
