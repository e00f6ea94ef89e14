// av1mi_internal.hpp — declarations shared by the kernel translation units and the C ABI (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/av1mi.h"

namespace av1mi {

// XCD-aware block order (cdna_hip_programming.md T1).  The dispatcher deals consecutive workgroup ids to the 8 XCDs in turn, and
// each XCD has its own L2: with a plain raster grid every neighbour of a tile (left, right, above, below) runs on another XCD,
// so the halo rows and columns that adjacent tiles share are fetched through several L2s (the filter kernels read 3-4x their
// algorithmic bytes by FETCH_SIZE).  The remap gives the ids that share an XCD (id % 8) one contiguous run of `nwg / 8` tiles in
// raster order, bijective for any nwg; it is an affinity hint only, nothing depends on where a block actually runs.
__device__ __forceinline__ unsigned xcd_swizzle(unsigned bid, unsigned nwg) {
  const unsigned q = nwg >> 3, r = nwg & 7u, xcd = bid & 7u;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
// row * stride of a plane row: both operands are below 2^24 and the product below 2^32 (the C ABI admits frames up to 16384 x
// 16384), so it is ONE full-rate 24-bit multiply; written as (size_t)row * stride it is a 64-bit multiply-add, four passes.
__device__ __forceinline__ size_t row_off(int row, int stride) { return (size_t)__umul24((unsigned)row, (unsigned)stride); }
// the 64x64 superblocks of a w x h frame (at most 256 x 256 of them)
__host__ __device__ inline int sb_count(int w, int h) { return ((w + 63) / 64) * ((h + 63) / 64); }

// The hand-off between lanes of one wave that share a block (a group): LDS traffic is in order per wave, this only stops the compiler
// moving LDS accesses across the hand-off (and drains lgkmcnt).
#define AV1MI_GROUP_SYNC()                                   \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   \
    __builtin_amdgcn_wave_barrier();                         \
  } while (0)

// raster tile index -> (x, y, z) of a gx x gy x gz grid
struct Tile3 { int x, y, z; };
// ... of workgroup `bid` out of the `nwg` that share the grid (a launch whose 1-D grid holds several such grids end to end)
__device__ __forceinline__ Tile3 xcd_tile(unsigned gx, unsigned gy, unsigned gz, unsigned bid, unsigned nwg) {
  (void)gz;   // the grid is exactly gx * gy * gz workgroups (every launch_* computes it from the same expressions)
  const unsigned t = xcd_swizzle(bid, nwg);
  const unsigned z = t / (gx * gy), rem = t - z * gx * gy, y = rem / gx;
  return { (int)(rem - y * gx), (int)y, (int)z };
}
__device__ __forceinline__ Tile3 xcd_tile(unsigned gx, unsigned gy, unsigned gz) { return xcd_tile(gx, gy, gz, blockIdx.x, gridDim.x); }

// One transform launch: either a block list or an implicit grid of equal blocks.
struct TxLaunch {
  int32_t *coef;            // int32 coefficients (K2: in, K1: out)
  void *plane;              // K2: uint8/uint16 prediction->reconstruction; K1: int16 residual
  int stride;               // samples
  int nblocks;
  const av1mi_txb *list;    // non-null: list form
  const uint8_t *tx_types;  // grid form: per-block type or null
  int uniform_type;
  int blocks_per_row;
};

// K3: a list of equally-sized blocks predicted from `ref` into `dst`
struct IntraLaunch {
  const void *ref; void *dst;
  int ref_stride, dst_stride, bd, nblocks;
  const av1mi_intra_blk *blocks;
};
hipError_t launch_intra_pred(int tx_size, const IntraLaunch &L, hipStream_t s);
struct CflLaunch {
  const void *luma; void *dst;
  int luma_stride, dst_stride, bd, nblocks;
  const av1mi_cfl_blk *blocks;
};
hipError_t launch_cfl_pred(int tx_size, const CflLaunch &L, hipStream_t s);

// K5: one plane, source -> destination (different allocations)
struct DeblockLaunch {
  const void *src; void *dst;
  int src_stride, dst_stride, w, h, bd, is_chroma;
  const uint32_t *mi; int mi_stride;   // (h/4) x (w/4) units of 4 bytes, see av1mi.h
  int sharpness;
  int nframes; size_t mi_frame_stride;   // frames stacked vertically (h rows each); mi units between frames, 0 = shared
};
hipError_t launch_deblock(const DeblockLaunch &L, hipStream_t s);

// fused intra-only pipeline over a segment of stacked frames
struct IntraPipeLaunch {
  const void *src[3]; void *rec[3]; int16_t *lev[3];
  uint8_t *modes_y, *modes_uv;
  int w, h, stride_y, stride_uv, bd, nframes, dc_q, ac_q;
  int dc_quant, ac_quant;   // (1 << 16) / step (libaom quant_fp): computed once by the host, see block_code.hpp
  int open_loop;            // 1: the modes are decided on the source first (k_intra_modes), the chain predicts each block once
  int frame_rows;           // luma rows between the stacked frames of a plane (= h, or more when the job codes a band of rows of every frame)
  int modes_stride;         // mode bytes between frames (= blocks of the job, or more)
};
hipError_t launch_intra_pipe(const IntraPipeLaunch &L, int bs, hipStream_t s);

// K4: a list of equally-sized blocks predicted from `ref` into `dst`
struct McLaunch {
  const void *ref; void *dst;
  int ref_stride, dst_stride, plane_w, plane_h, bd, nblocks;
  const av1mi_mc_blk *blocks;
};
hipError_t launch_mc(int size_id, const McLaunch &L, hipStream_t s);

// K6: CDEF of 4:2:0 frames stacked vertically
struct CdefLaunch {
  const void *src[3]; void *dst[3];
  int w, h, stride_y, stride_uv, bd, damping, nframes;
  const uint8_t *sb_strength; size_t sb_frame_stride;   // 4 bytes per 64x64; entries between frames (0 = shared)
  const uint8_t *skip8; size_t skip_frame_stride;       // 1 byte per 8x8 luma block; bytes between frames (0 = shared)
};
hipError_t launch_cdef(const CdefLaunch &L, hipStream_t s);

// The CDEF search (cdef_search_kernel.hip k_cdef_search; av1mi.h "CDEF search"): per superblock the squared error of ncand candidate
// strength sets against the source over the true size (tw x th), and the arg-min
struct CdefSearchLaunch {
  const void *src[3], *orig[3];                         // deblocked planes, source planes: the same geometry
  int w, h, tw, th, stride_y, stride_uv, bd, damping, nframes, ncand;
  const uint8_t *skip8; size_t skip_frame_stride;       // as CdefLaunch
  uint32_t sets[8];                                     // candidate c as a CdefLaunch strength record: y_pri | y_sec << 8 | uv_pri << 16 | uv_sec << 24
  unsigned long long *sse;                              // [frame][sb][8]
  uint8_t *strength, *idx;                              // [frame][sb][4], [frame][sb]
};
hipError_t launch_cdef_search(const CdefSearchLaunch &L, hipStream_t s);

// K5 + K6 in one kernel (deblock_cdef_kernel.hip): reconstruction -> CDEF output, and the rows of the deblocked planes that K7 reads
struct DeblockCdefLaunch {
  const void *rec[3]; void *dbl[3]; void *dst[3];
  int w, h, rec_stride_y, rec_stride_uv, dbl_stride_y, dbl_stride_uv, dst_stride_y, dst_stride_uv, bd, damping, sharpness, nframes;
  const uint32_t *mi_y, *mi_uv; int mi_stride_y, mi_stride_uv;   // deblocking mode info of the luma / chroma planes, as DeblockLaunch
  size_t mi_frame_stride_y, mi_frame_stride_uv;
  const uint8_t *sb_strength; size_t sb_frame_stride;            // as CdefLaunch
  const uint8_t *skip8; size_t skip_frame_stride;
};
hipError_t launch_deblock_cdef(const DeblockCdefLaunch &L, hipStream_t s);

// K7: loop restoration of one plane, frames stacked vertically
struct LrLaunch {
  const void *cdef = nullptr, *dbl = nullptr; void *out = nullptr;
  int stride = 0, w = 0, h = 0, bd = 0, ss = 0, unit_size = 0, nframes = 0;
  const int8_t *units = nullptr; size_t unit_frame_stride = 0;   // 8 bytes per unit; units between frames (0 = shared)
  // the on/off decision (orig != nullptr): the source plane, and per (frame, stripe) two 64-bit sums: squared error of the restored
  // samples, of the CDEF samples (zeroed by the caller; sse_stripes = LrGeom::stripes)
  const void *orig = nullptr; unsigned long long *sse = nullptr; int sse_stripes = 0;
  // two-pass form of the decision (pass 0 = everything in one launch): pass 1 restores only the tiles the sums run over, pass 2 the
  // others, and only in the frames whose flag keep[f * keep_stride] (written by the decision between the two) is set
  int pass = 0; const uint8_t *keep = nullptr; int keep_stride = 0;
  int no_sgr = 0;   // the caller's promise that no unit is self-guided (type 2): the kernel without that path's LDS
};
// K7's geometry, host and device: the ONE place it is computed (the launchers, the C ABI's scratch sizes and the kernels read it).  A
// workgroup owns the intersection of a stripe (64 rows, 32 for 4:2:0 chroma, offset 8 luma rows upwards) with a column band no wider
// than a unit or 64 samples; workgroups = bands x stripes x frames.
struct LrGeom {
  int w, h, unit_size, nframes, stripe_h, stripe_off, tile_w, bands, stripes, unit_rows, unit_cols;
  __host__ __device__ static int stripes_of(int h, int ss) { return (h + (8 >> ss) + (64 >> ss) - 1) / (64 >> ss); }
  __host__ __device__ LrGeom(int w_, int h_, int ss, int unit_size_, int nframes_) : w(w_), h(h_), unit_size(unit_size_), nframes(nframes_) {
    stripe_h = 64 >> ss; stripe_off = 8 >> ss; tile_w = unit_size < 64 ? unit_size : 64;
    bands = (w + tile_w - 1) / tile_w; stripes = stripes_of(h, ss);
    unit_rows = (h + (unit_size >> 1)) / unit_size; unit_cols = (w + (unit_size >> 1)) / unit_size;
    if (unit_rows < 1) unit_rows = 1;
    if (unit_cols < 1) unit_cols = 1;
  }
  explicit LrGeom(const LrLaunch &L) : LrGeom(L.w, L.h, L.ss, L.unit_size, L.nframes) {}
  __host__ __device__ unsigned workgroups() const { return (unsigned)(bands * stripes * nframes); }
  // the stripe's first row (the first stripe starts above the picture); a tile writes the stripe's rows inside the picture
  __host__ __device__ int first_row(int stripe) const { return stripe * stripe_h - stripe_off; }
  // the unit of the tile whose first written sample is (x0, y0)
  __host__ __device__ size_t unit_index(int x0, int y0) const {
    const int ur = (y0 + stripe_off) / unit_size, uc = x0 / unit_size;
    return (size_t)(ur < unit_rows - 1 ? ur : unit_rows - 1) * unit_cols + (uc < unit_cols - 1 ? uc : unit_cols - 1);
  }
  // The decision's sums run over an EIGHTH of the plane — the 64-column x stripe tiles with (column + stripe) % 8 == 0, a diagonal
  // pattern over the whole picture (every tile when the plane has fewer than 32) — so the decision costs an eighth of a source read.
  __host__ __device__ bool sampled(int x0, int stripe) const { return ((w + 63) >> 6) * stripes < 32 || (((x0 >> 6) + stripe) & 7) == 0; }
  // the decision's scratch: per (frame, stripe) one pair of 64-bit sums
  __host__ __device__ size_t sum_pairs() const { return (size_t)nframes * stripes; }
};
// the first pair of plane p in the scratch of a 4:2:0 frame's three planes (luma geometry y, chroma geometry c), end to end
__host__ __device__ inline size_t lr_first_pair(const LrGeom &y, const LrGeom &c, int p) { return p ? y.sum_pairs() + (p - 1) * c.sum_pairs() : 0; }
hipError_t launch_lr(const LrLaunch &L, hipStream_t s);
// the three planes of 4:2:0 frames in ONE launch: their grids end to end, a workgroup takes its plane from its index.  The planes
// share bd, unit_size, nframes, pass and no_sgr; plane 0 is the luma plane (ss 0), planes 1 and 2 are subsampled (ss 1)
struct LrYuvLaunch { LrLaunch plane[3]; unsigned first[3]; };      // first: filled in by launch_lr_yuv (plane p's first workgroup)
hipError_t launch_lr_yuv(LrYuvLaunch &Y, hipStream_t s);
hipError_t launch_zero16(void *p, size_t bytes, hipStream_t s);
hipError_t launch_extend(void *plane, int stride, int w, int h, int vw, int vh, int bd, int nframes, hipStream_t s);
// the decision over the sums of nplanes = 1 plane (geometry y) or the 3 of 4:2:0 frames (y, c, c): lr_kernel.hip k_lr_decide
hipError_t launch_lr_decide(unsigned long long *sse, const LrGeom &y, const LrGeom &c, int nplanes, uint8_t *on, int on_stride, bool clear, hipStream_t s);

// The restoration search over the three planes of 4:2:0 frames (lr_kernel.hip k_lr_search, k_lr_pick; av1mi.h "restoration search").
// The cost table holds 9 sums per unit, the units of a frame's planes end to end: [frame][unit_first[p] + unit][candidate].
struct LrSearchLaunch {
  const void *cdef[3], *dbl[3], *orig[3];
  int stride[3], w[3], h[3], bd, unit_size, nframes;
  unsigned long long *sums;                    // zeroed by the caller
  unsigned unit_first[3], units_frame;         // plane p's first unit in a frame's run of units, and the run's length
  unsigned first[3];                           // filled in by launch_lr_search (plane p's first workgroup)
  int8_t taps[2][3][3];                        // [luma / chroma][filter][tap0 tap1 tap2]
  // the pick: J = sum + lambda * bits[class][candidate]; the chosen record per unit, its index per unit
  long long lambda; int bits[2][9];
  int8_t *units[3]; uint8_t *choice;
};
hipError_t launch_lr_search(LrSearchLaunch &S, hipStream_t s);
hipError_t launch_lr_pick(const LrSearchLaunch &S, hipStream_t s);
// the search's tables, host side (lr_kernel.hip): candidate c's record for a luma / chroma plane, and the exact bits of that record
void lr_search_record(int chroma, int c, int8_t rec[8]);
int lr_search_bits(int chroma, int c);
void lr_search_tables(LrSearchLaunch *S);      // the launch's taps (the table itself) and bits

// inter (P-frame) pipeline over the t-th frames of a batch of segments, stacked like the intra job
struct InterLaunch {
  const void *src[3]; const void *ref[3]; void *rec[3]; int16_t *lev[3];
  int16_t *mvs; uint8_t *skip;
  int w, h, stride_y, stride_uv, bd, nframes, dc_q, ac_q, range;
  int dc_quant, ac_quant;   // (1 << 16) / step (libaom quant_fp): computed once by the host, see block_code.hpp
  const void *ref_alt[3]; const uint8_t *ref_sel;   // optional: ref_sel[f * 3 + p] == 0 -> frame f predicts plane p from ref_alt[p]
  const int16_t *centres = nullptr;                 // optional (k_me_int): a search centre (x, y) in luma samples per 64x64 tile and frame, multiples of 4
};
hipError_t launch_me_int(const InterLaunch &L, hipStream_t s);
// the coarse search (me_coarse_kernels.hip): where its quarter planes and centres lie in a scratch area of `bytes` bytes (16-byte
// aligned): the source's quarter planes at 0, the reference's at off_ref (qw x qh samples per frame, rows qs = qw rounded up to 4
// bytes apart, frames stacked), the centres (an int16 pair per tile and frame) at off_centres
struct MeLayout { int qw, qh, qs, tiles; size_t off_ref, off_centres, bytes; };
MeLayout me_layout(int w, int h, int nframes);
hipError_t launch_me_coarse(const InterLaunch &L, int coarse_range, void *scratch, hipStream_t s);

// the input stage (input_kernels.hip): the planes of a batch in a wire / surface format (enum av1mi_input_format, not PLANAR) ->
// planar planes; ny luma and nc chroma samples per plane.  The unit counts are filled in by the launcher.
struct InputLaunch {
  const void *in[3]; void *out[3];
  size_t ny, nc;
  size_t units, units_y, units_c;
};
hipError_t launch_input_convert(int format, InputLaunch L, hipStream_t s);
// the chroma stage (input_kernels.hip, include/av1mi.h "chroma formats"): `frames` stacked frames of TRUE luma size w x h in the
// source's layout -> 4:2:0 planes at bit depth bd; in[0] / out[0] are unused where src_bd == bd (the luma plane is not converted)
struct ChromaLaunch {
  const void *in[3]; void *out[3];
  int chroma, src_bd, bd, w, h, frames;
};
// the argument rules shared by av1mi_chroma_convert and the session: null = fine, else the reason
const char *chroma_format_error(int chroma, int src_bd, int bd);
hipError_t launch_chroma_convert(const ChromaLaunch &L, hipStream_t s);
hipError_t launch_inter_pipe(const InterLaunch &L, hipStream_t s);

// the resampler of the input stage (scale_kernels.hip): a plan holds the device tables of one geometry (true luma size of the source ->
// target luma size, both buffers at their sizes rounded up to 8); one launch scales the three planes of `frames` stacked frames
// A crop window (include/av1mi.h "crop window"): the rectangle (x, y, w, h), all even, of planar 4:2:0 frames of TRUE luma size frame_w x
// frame_h (their buffers: that rounded up to 8).  The chroma planes' window is the half of every number.
struct CropWindow { int x, y, w, h, frame_w, frame_h; };
struct ScalePlan;
// window != null: sw x sh is the WINDOW's size and the source planes are the frames it lies in: the plan reads from the window's origin
// with the frames' strides, and clamps at the window's edges
hipError_t scale_plan_create(int bd, int sw, int sh, int dw, int dh, ScalePlan **out, const CropWindow *window = nullptr);      // synchronous (allocates, uploads)
void scale_plan_destroy(ScalePlan *P);
bool scale_plan_is(const ScalePlan *P, int bd, int sw, int sh, int dw, int dh);
hipError_t launch_scale(const ScalePlan *P, int frames, const void *const *src, void *const *dst, hipStream_t s);
// the argument rules shared by av1mi_scale_planes and the session: null = fine, else the reason
const char *scale_geometry_error(int sw, int sh, int dw, int dh);

// the window alone, nothing resampled (crop_kernels.hip, k_crop_copy): the window of `frames` stacked frames -> the coded planes of dst_w x
// dst_h luma samples (the window's size rounded up to 8; the window's last column / row replicated into the padding).  ONE launch
hipError_t launch_crop_copy(const CropWindow &W, int bd, int dst_w, int dst_h, int frames, const void *const *src, void *const *dst, hipStream_t s);
// tone mapping in place (tonemap_kernels.hip, include/av1mi.h "tone mapping"): `frames` stacked frames of planar 4:2:0 10-bit planes of luma size
// w x h (w a multiple of 4, h even), tables = an av1mi_tone_tables in device memory (16-byte aligned); one launch
hipError_t launch_tone_map(int w, int h, int frames, void *const planes[3], const void *tables, hipStream_t s);
// depth reduction (depth_kernels.hip, include/av1mi.h "depth reduction"): `frames` stacked frames of planar 4:2:0 uint16 planes of luma BUFFER size
// w x h (multiples of 8) -> uint8 planes of the same sizes, mode = enum av1mi_depth_mode; all planes 4-byte aligned; one launch
hipError_t launch_depth_reduce(int mode, int w, int h, int frames, const void *const in[3], void *const out[3], hipStream_t s);
// bar detection (crop_kernels.hip, include/av1mi.h "bar detection"): `frames` stacked luma planes of TRUE size w x h in buffers of stride x
// rows samples -> one record of margins per frame, two launches.  scratch: crop_layout().bytes bytes, 4-byte aligned: a partial per
// (row, tile column) at 0, a partial per (tile row, column) at off_cols
struct CropLayout { int tiles_x, tiles_y; size_t off_cols, bytes; };
CropLayout crop_layout(int bd, int w, int h, int frames);
struct CropAnalyseLaunch {
  int bd, stride, rows, w, h, frames, limit;
  const void *luma; void *scratch; av1mi_crop_record *out;
};
hipError_t launch_crop_analyse(const CropAnalyseLaunch &A, hipStream_t s);
// noise records (noise_kernels.hip, include/av1mi.h "noise records"): `pairs` pairs of stacked luma planes (pair i = planes 2 i, 2 i + 1) of
// TRUE size w x h in buffers of stride x rows samples -> one record per pair, two launches.  scratch: noise_layout().bytes bytes, 4-byte
// aligned: 256 partials per (pair, tile).  bw x bh: the 8x8 blocks that lie wholly inside the true size
struct NoiseLayout { int bw, bh, tiles_x, tiles_y; size_t bytes; };
NoiseLayout noise_layout(int bd, int w, int h, int pairs);
struct NoiseAnalyseLaunch {
  int bd, stride, rows, w, h, pairs;
  const void *luma; void *scratch; av1mi_noise_record *out;
};
hipError_t launch_noise_analyse(const NoiseAnalyseLaunch &A, hipStream_t s);
// peak records (peak_kernels.hip, include/av1mi.h "peak records"): `frames` stacked planar 4:2:0 uint16 frames of TRUE luma size tw x th in
// buffers of w8 x h8 luma samples (chroma w8 / 2 x h8 / 2) -> one record per frame, two launches.  scratch: peak_layout().bytes bytes,
// 16-byte aligned: 1024 partials per (frame, strip of rows)
struct PeakLayout { int strips; size_t bytes; };
PeakLayout peak_layout(int th, int frames);
struct PeakAnalyseLaunch {
  int w8, h8, tw, th, frames;
  const void *y, *u, *v; void *scratch; av1mi_peak_record *out;
};
hipError_t launch_peak_analyse(const PeakAnalyseLaunch &A, hipStream_t s);

// the quality records (quality_kernels.hip): source against the decoded picture, three planes of `frames` stacked frames of TRUE luma
// size w x h in buffers of that size rounded up to 8; two launches (tiles, then a fixed-order sum per frame and plane).  dec1 / sel
// may be null; scratch: quality_scratch_bytes() bytes, 8-byte aligned; out: frames * 3 records (device memory or pinned host memory)
struct QualityLaunch {
  int bd, w, h, frames;
  const void *const *src, *const *dec0, *const *dec1;
  const uint8_t *sel;
  void *scratch; av1mi_quality *out;
};
size_t quality_scratch_bytes(int bd, int w, int h, int frames);
hipError_t launch_quality(const QualityLaunch &Q, hipStream_t s);

// the scene analysis (scene_kernels.hip, include/av1mi.h "scene analysis"): `frames` stacked luma planes of w x h samples (multiples of
// 8; uint8 at bd 8, else uint16 viewed through >> (bd - 8)) -> one record per frame, three launches.  scratch: scene_layout().bytes
// bytes, 16-byte aligned: the quarter planes at 0 (rows qs bytes apart, frames stacked), a pair (inter, intra) per block at off_blocks;
// out: `frames` records (device memory or pinned host memory)
struct SceneLayout { int qw, qh, qs, nbx, nby; size_t off_blocks, bytes; };
SceneLayout scene_layout(int w, int h, int frames);
struct SceneLaunch {
  int bd, w, h, frames;
  const void *luma; void *scratch; av1mi_scene_record *out;
};
hipError_t launch_scene(const SceneLaunch &S, hipStream_t s);
// the gather (scene_kernels.hip): table[segment * 3 + plane] = where that segment's plane of plane_bytes[plane] bytes lies in device
// memory (16-byte aligned), or null = zeros -> dst[plane] + segment * plane_bytes[plane]; ONE launch.  table is device memory.
hipError_t launch_frames_gather(const size_t plane_bytes[3], int segments, const void *const *table, void *const dst[3], hipStream_t s);
// the fed planes of a filtering gather (gather_cells.hpp): table[(segment * 3 + plane) * 3 + {0, 1, 2}] = that segment's plane of frames
// P, C and N in device memory (the run's clamping applied by the caller; C null = zeros); plane_w x plane_h: the buffers' size in samples
// (0 = no such plane), true_w x true_h the size the filter works at, less than 8 below it; bd 8 = uint8 samples, else uint16
struct GatherPlanes {
  int bd, segments;
  int plane_w[3], plane_h[3], true_w[3], true_h[3];
  const void *const *table; void *dst[3];
};
// the deinterlacing gather (deint_kernels.hip, include/av1mi.h "deinterlacing"): the gather above with the filter in it; parity 0 = the
// even lines are kept.  ONE launch.
struct DeintLaunch : GatherPlanes {
  int parity;
};
hipError_t launch_deint_gather(const DeintLaunch &L, hipStream_t s);
// the same at field rate (include/av1mi.h "field-rate output"): phase[segment] in device memory, low bit 0 = the frame's first field
// (the launch above, exactly), 1 = its second: the opposite parity is kept and the temporal pair is (C, N).  ONE launch.
struct DeintFieldsLaunch : DeintLaunch {
  const uint8_t *phase;
};
hipError_t launch_deint_gather_fields(const DeintFieldsLaunch &L, hipStream_t s);

// inverse telecine (telecine_kernels.hip, include/av1mi.h "inverse telecine").  The records of a run of `frames` stacked luma planes of TRUE
// size w x h in buffers of stride x rows samples: two launches.  scratch: telecine_layout().bytes bytes, 16-byte aligned: per (frame,
// tile, wave) four 32-bit partials; out: `frames` records (device memory or pinned host memory)
struct TelecineLayout { int tiles_x, tiles_y, chunks; size_t per_frame, bytes; };
TelecineLayout telecine_layout(int bd, int w, int h, int frames);
struct TelecineLaunch {
  int bd, stride, rows, w, h, frames;
  const void *luma; void *scratch; av1mi_telecine_record *out;
};
hipError_t launch_telecine_analyse(const TelecineLaunch &A, hipStream_t s);
// the weave gather: a GatherPlanes whose table holds TWO pointers per (segment, plane), [(segment * 3 + plane) * 2 + {0, 1}] = the top and
// the bottom source (top null = zeros).  ONE launch.
hipError_t launch_telecine_gather(const GatherPlanes &L, hipStream_t s);

// the denoising gather (grain_kernels.hip, include/av1mi.h "denoising" / "grain records"): a strength (1 .. 16) in place of the parity; bd
// 8 or 10.  records: segments * 3 records (device or pinned host memory), or null = nothing is measured, ONE launch; else two, and
// scratch holds grain_scratch_bytes(L) bytes (8-byte aligned) of per-workgroup partials.
struct DenoiseLaunch : GatherPlanes {
  int strength;
  void *scratch; av1mi_grain_record *records;
};
size_t grain_scratch_bytes(const DenoiseLaunch &L);      // 0 for a geometry the launch refuses
hipError_t launch_denoise_gather(const DenoiseLaunch &L, hipStream_t s);
// the same with a block search in front (include/av1mi.h "motion-compensated denoising"): range 4 or 8; vectors: segments x blocks records
// (denoise_mc_vector_bytes(L) bytes, 4-byte aligned, never null), written by k_denoise_search and read by k_denoise_mc_gather; scratch holds
// denoise_mc_scratch_bytes(L) bytes where records are asked for.  Two launches, three with records.
struct DenoiseMcLaunch : DenoiseLaunch {
  int range;
  av1mi_denoise_vec *vectors;
};
size_t denoise_mc_scratch_bytes(const DenoiseMcLaunch &L);      // 0 for a geometry the launch refuses
size_t denoise_mc_vector_bytes(const DenoiseMcLaunch &L);       // likewise
hipError_t launch_denoise_mc_gather(const DenoiseMcLaunch &L, hipStream_t s);
// the grain covariance (grain_cov_kernels.hip, include/av1mi.h "grain covariance"), launched BEHIND either gather above on the same planes:
// of the table only the C entries are read, dst are the planes the gather wrote (only read here); bd 8 or 10.  cov: segments * 3 records
// (device or pinned host memory); scratch holds grain_cov_scratch_bytes(L) bytes (8-byte aligned) of per-workgroup partials.  Two launches.
struct GrainCovLaunch : GatherPlanes {
  void *scratch; av1mi_grain_cov_record *cov;
};
size_t grain_cov_scratch_bytes(const GatherPlanes &L);      // 0 for a geometry the launch refuses
hipError_t launch_grain_cov(const GrainCovLaunch &L, hipStream_t s);

// side information that follows a batch's quantiser (levels_kernels.hip): up to three arrays of dwords patched in place in one launch,
// word = (word & keep) | bits unless (word & hold) != 0
struct LevelsLaunch {
  struct Array { uint32_t *words; size_t n; uint32_t keep, bits, hold; } a[3];
  int arrays;
};
hipError_t launch_mi_levels(const LevelsLaunch &L, hipStream_t s);
// ... and its grid-wide sibling (k_mi_levels_frames): the level bytes come from levels[frame][4] in DEVICE memory (the deblocking search's
// pick: luma vertical, luma horizontal, U, V) and the patched words go to a map of their own per frame, dense (w / 4 units a row, h / 4
// rows a frame; chroma: of the chroma plane), read from base maps with their strides (frame stride 0 = shared).  The hold rule as above
struct LevelsFramesLaunch {
  const uint8_t *levels;
  const uint32_t *base[2]; uint32_t *out[2];              // luma, chroma; a null out[k] is skipped
  int cols[2], rows[2], stride[2]; size_t frame_stride[2];
  int nframes;
};
hipError_t launch_mi_levels_frames(const LevelsFramesLaunch &L, hipStream_t s);

// The deblocking search (lf_search_kernel.hip k_lf_search, k_lf_pick; av1mi.h "deblocking search"): per (frame, superblock) the squared
// error against the source of the planes deblocked at each of 8 candidate levels, luma and chroma apart, over the true size (tw x th);
// then per frame the sums over the superblocks, the two arg-mins and the four header levels
struct LfSearchLaunch {
  const void *rec[3], *orig[3];                            // reconstruction, source: the same geometry
  int w, h, tw, th, stride_y, stride_uv, bd, sharpness, nframes;
  const uint32_t *mi_y, *mi_uv; int mi_stride_y, mi_stride_uv;      // the base maps, as DeblockCdefLaunch
  size_t mi_frame_stride_y, mi_frame_stride_uv;
  uint8_t lvl[8][4];                                       // candidate c: luma vertical, luma horizontal, chroma, chroma
  uint8_t first[2][8];                                     // [luma / chroma][c]: the lowest candidate with c's levels (c itself: not a twin)
  unsigned long long *table;                               // scratch: [frame][sb][2][8]
  unsigned long long *sse; uint8_t *choice, *levels;       // [frame][2][8], [frame][2], [frame][4]
};
hipError_t launch_lf_search(const LfSearchLaunch &L, hipStream_t s);
hipError_t launch_lf_pick(const LfSearchLaunch &L, hipStream_t s);

int tx_width(int tx_size);
int tx_height(int tx_size);
hipError_t launch_inv_txfm(int tx_size, const TxLaunch &L, int bd, hipStream_t s);
hipError_t launch_fwd_txfm(int tx_size, const TxLaunch &L, hipStream_t s);
hipError_t launch_quantize(const int32_t *coef, int16_t *levels, int32_t *dqcoef, long long n, int coef_per_blk,
                           int dc_q, int ac_q, int log_scale, hipStream_t s);
hipError_t launch_dequantize(const int16_t *levels, int32_t *dqcoef, long long n, int coef_per_blk, int dc_q,
                             int ac_q, int log_scale, int bd, hipStream_t s);

// the AV1 tile entropy coder's per-context scratch (av1_entropy_kernels.hip); created on first use, freed by av1mi_close
struct av1mi_av1ent_state_fwd;
}  // namespace av1mi
struct av1mi_av1ent_state;
namespace av1mi {
av1mi_av1ent_state *av1ent_new();
void av1ent_free(av1mi_av1ent_state *st);
av1mi_av1ent_state *ctx_av1ent(av1mi_ctx *ctx);
hipStream_t ctx_side_stream(av1mi_ctx *ctx);      // these two are created at their first use; null = creation failed
hipStream_t ctx_back_stream(av1mi_ctx *ctx);
// Optional pinned host mirrors of a coder job's results.  The gather stores them itself, with plain stores, beside the payloads it
// already writes into pinned memory: every tile's workgroup its size, the last tile's workgroup the total, the status and the job's
// restoration flags (d_lr_on, lr_on_bytes of them).  They are valid where the payloads are: after an event recorded behind the back
// half.  Null members are skipped; without the record a caller gets the job's device arrays and nothing else.
struct Av1EntMirrors {
  uint32_t *h_tile_size;
  uint64_t *h_total;      // [0] total bytes, [1] status: the layout of av1mi_av1_entropy_job::d_total
  uint8_t *h_lr_on; uint32_t lr_on_bytes;
};
// the AV1 tile coder of include/av1mi.h's av1mi_av1_entropy_job in two halves: info + tokens + chains on `front`, the serial range
// coder + gather on `back` (the same stream, or a second one: the lists are double-buffered, so the front half of the next
// job runs beside the back half of this one)
int av1_entropy_submit(av1mi_ctx *ctx, const struct av1mi_av1_entropy_job *j, hipStream_t front, hipStream_t back, const Av1EntMirrors *mirrors = nullptr,
                       const struct av1mi_av1_entropy_units *units = nullptr, const struct av1mi_av1_entropy_cdef *cdef = nullptr);
// ... and the halves on their own: the back half of a job may be launched later (the session defers the range coder of batch t behind
// the filters of batch t + 1 on the main stream); at most two jobs' back halves can be outstanding (the list sets)
int av1_entropy_front(av1mi_ctx *ctx, const struct av1mi_av1_entropy_job *j, hipStream_t front, int *ticket, const struct av1mi_av1_entropy_units *units = nullptr,
                      const struct av1mi_av1_entropy_cdef *cdef = nullptr);
int av1_entropy_back(av1mi_ctx *ctx, int ticket, hipStream_t back, const Av1EntMirrors *mirrors = nullptr);
// accessors of the opaque context for translation units other than capi.hip (gop_session.hip)
hipStream_t ctx_stream(av1mi_ctx *ctx);
int ctx_device(av1mi_ctx *ctx);
int ctx_fail(av1mi_ctx *ctx, int code, const char *fmt, ...);
// the per-kernel profile (av1mi_prof_*) for launches made outside capi.hip, on any stream of the context: an event pair around the
// launch(es) while profiling is enabled, nothing otherwise
struct ProfToken { hipEvent_t e0 = nullptr; int kind = 0; };
// av1mi_inter_encode with the coarse search's scratch area given by the caller (the GOP session owns one); d_me is unused, and may be
// null, when the job's coarse_range is 0
int inter_encode_with(av1mi_ctx *ctx, const struct av1mi_inter_job *j, void *d_me);
// av1mi_lr_yuv_decide for a caller that owns its scratch: scratch_clean = the sums are known to be zero (capi.hip: the rule)
int lr_yuv_decide_with(av1mi_ctx *ctx, const struct av1mi_lr_decide_job *j, bool scratch_clean);
ProfToken ctx_prof_begin(av1mi_ctx *ctx, int kind, hipStream_t st);
void ctx_prof_end(av1mi_ctx *ctx, const ProfToken &t, hipStream_t st);
// ... and the same as a scope around the launch(es); st null = the context's stream
struct ProfScope {
  av1mi_ctx *ctx; hipStream_t st; ProfToken t;
  ProfScope(av1mi_ctx *c, int kind, hipStream_t s = nullptr) : ctx(c), st(s ? s : ctx_stream(c)), t(ctx_prof_begin(c, kind, st)) {}
  ~ProfScope() { ctx_prof_end(ctx, t, st); }
};

}  // namespace av1mi
