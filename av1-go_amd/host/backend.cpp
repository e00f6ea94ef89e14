// backend.cpp — the part of RunTranscode that replaces the FFmpeg child (internal/ffmpeg/transcode.go:194-203): raw frames in,
// an AV1 elementary stream out.  A THIN caller: closed-GOP orchestration, filter-parameter policy and PCIe plumbing live in
// libav1mi.so's GOP session (include/av1mi.h av1mi_gop_*), entropy coding + OBU packing in av1_bitstream.cpp on the host
// cores, so nothing about the encoder is decided here.
//
// Input is Y4M (4:2:0, 8- or 10-bit; with a job that converts to 4:2:0 also 4:2:2, 4:4:4 and grey, up to 12 bits), from a file or from a stream ("-i -", a FIFO: y4m.hpp), because demux / H.264 decode stay
// FFmpeg's job (SURVEY.md §8b "Gap to flag"): any decoder process can pipe its frames in.
// Output, chosen by the file name: ".obu" = Section-5 low-overhead OBU stream (what `dav1d -i x.obu` / `aomdec --obu` read),
// ".ivf" = IVF, anything else (the reference's "<base>.av1-tmp.mkv") = Matroska with one V_AV1 video track (mux.cpp);
// audio / subtitle copy (transcode.go:134-137) needs a demuxer and is not done.
//
// With -av1mi_deinterlace (or a deinterlacer in the chain) an interlaced source takes the same stored path, without the analysis unless
// -av1mi_scenecut asks for it: the session's gather deinterlaces every frame on its way from the store (av1mi_gop_config.deinterlace).
// With -av1mi_scenecut the GOPs of a group do not start every `gop` frames but where the scene analysis finds cuts: the group's frames go
// into the session's frame store in file order (av1mi_gop_store_put), are analysed there (av1mi_gop_store_analyse), the planner
// (sceneplan.hpp) lays the GOPs out, and every batch is gathered from the store (av1mi_gop_submit_stored).  The session has two stores:
// the next group's frames are read and put while this group's batches run.
//
// A crop window — a crop= filter in front of the chain, -av1mi_crop W:H:X:Y, or the bars that -av1mi_crop auto finds — is settled BEFORE the
// session is opened: auto reads up to 32 frames spread evenly over a seekable file, uploads their luma planes, runs av1mi_crop_analyse
// and plans the window (cropplan.hpp).  The session is then opened with the window (av1mi_gop_config.crop_*) and fed whole frames; the
// rest of the chain sees the window's size.  No window = the path below as it has always been.
//
// `segments` closed GOPs of the file are coded in lockstep (the session's batch dimension); while the host codes the
// symbols of frame t the GPU already works on frames t + 1 and t + 2 (three batches in flight).
#include "filmgrain.hpp"
#include "backend.hpp"
#include <sys/stat.h>
#include <unistd.h>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#include "../../include/av1mi.h"
#include "../csrc/quality.hpp"
#include "av1_bitstream.hpp"
#include "cropplan.hpp"
#include "mux.hpp"
#include "ratecontrol.hpp"
#include "sceneplan.hpp"
#include "y4m.hpp"

namespace av1mi_host {

void DescribeSessionFrame(const av1mi_gop_frame &fr, int seg, int width, int height, int bit_depth, SessionFrameDesc *d, int visible_width, int visible_height) {
  const av1mi_frame_params &p = fr.params;
  av1mi_obu_frame &f = d->f;
  memset(&f, 0, sizeof(f));
  f.width = width; f.height = height; f.bit_depth = bit_depth; f.frame_type = p.frame_type; f.base_q_idx = p.base_q_idx;
  f.visible_width = visible_width; f.visible_height = visible_height;
  for (int i = 0; i < 4; i++) f.lf_level[i] = p.lf_level[i];
  f.lf_sharpness = p.lf_sharpness; f.cdef_damping = p.cdef_damping; f.cdef_bits = 0; f.cdef_y[0] = p.cdef_y; f.cdef_uv[0] = p.cdef_uv;
  auto units = [&](int n) { const int u = (n + p.lr_unit_size / 2) / p.lr_unit_size; return u > 1 ? u : 1; };
  const int vw = visible_width ? visible_width : width, vh = visible_height ? visible_height : height;      // the units tile the TRUE frame
  const size_t uy = (size_t)units(vh) * units(vw), uc = (size_t)units((vh + 1) / 2) * units((vw + 1) / 2);
  d->lr_y.resize(uy * 8); d->lr_uv.resize(uc * 8);
  for (size_t i = 0; i < uy; i++) memcpy(&d->lr_y[i * 8], p.lr_unit_y, 8);
  for (size_t i = 0; i < uc; i++) memcpy(&d->lr_uv[i * 8], p.lr_unit_uv, 8);
  // restoration per plane: the policy's type where the encoder kept it ON for this segment's frame (fr.lr_on), NONE elsewhere
  const uint8_t *on = fr.lr_on ? fr.lr_on + (size_t)seg * 3 : nullptr;
  f.lr_type[0] = (!on || on[0]) ? p.lr_unit_y[0] : 0;
  f.lr_type[1] = (!on || on[1]) ? p.lr_unit_uv[0] : 0;
  f.lr_type[2] = (!on || on[2]) ? p.lr_unit_uv[0] : 0;
  f.lr_unit_shift = p.lr_unit_size == 64 ? 0 : p.lr_unit_size == 128 ? 1 : 2; f.lr_uv_shift = 0;
  f.lr_units[0] = d->lr_y.data(); f.lr_units[1] = f.lr_units[2] = d->lr_uv.data();
  f.tile_cols_log2 = f.tile_rows_log2 = -1;      // one superblock per tile: the independence the GPU pipeline's prediction assumes
  const size_t nb = fr.blocks_per_frame, o = (size_t)seg * nb;
  if (fr.y_mode) { f.y_mode = fr.y_mode + o; f.uv_mode = fr.uv_mode + o; }       // the symbols are absent when the tiles were coded on the GPU
  if (fr.mv) { f.mv = fr.mv + o * 2; f.skip = fr.skip + o; }
  if (fr.lev_y) { f.lev_y = fr.lev_y + o * 64; f.lev_u = fr.lev_u + o * 16; f.lev_v = fr.lev_v + o * 16; }     // absent when the tiles were coded on the GPU
}

// A key frame of a key_block_size 32 session (av1mi_gop_frame.key_block_size == 32): 32x32 blocks over the complete superblock rows,
// 8x8 blocks in a last partial row — written by the general block writer (av1_blockstream.cpp) from the session's symbols.
static bool Key32TemporalUnit(const av1mi_gop_frame &fr, int seg, const SessionFrameDesc &desc, int width, int height, bool with_sequence_header, int threads,
                              std::vector<uint8_t> *out, std::string *err) {
  if (!fr.y_mode || !fr.lev_y) { if (err) *err = "a key frame in 32x32 blocks needs its symbols (gpu_entropy 0)"; return false; }
  const int hA = (height / 64) * 64, mi_rows = height / 4, mi_cols = width / 4;
  const size_t ny = (size_t)width * height, nc = ny / 4;
  const uint8_t *my = fr.y_mode + (size_t)seg * fr.key_modes_stride, *muv = fr.uv_mode + (size_t)seg * fr.key_modes_stride;
  std::vector<int16_t> lev(ny + 2 * nc);
  memcpy(lev.data(), fr.lev_y + (size_t)seg * ny, ny * 2);
  memcpy(lev.data() + ny, fr.lev_u + (size_t)seg * nc, nc * 2);
  memcpy(lev.data() + ny + nc, fr.lev_v + (size_t)seg * nc, nc * 2);
  std::vector<uint8_t> parts;
  std::vector<av1mi_obu_block> blocks;
  auto block = [&](int r, int c, int bsize, int mode_y, int mode_uv, size_t oy, size_t oc) {
    av1mi_obu_block b;
    memset(&b, 0, sizeof(b));
    b.mi_row = (uint16_t)r; b.mi_col = (uint16_t)c; b.bsize = (uint8_t)bsize; b.y_mode = (uint8_t)mode_y; b.uv_mode = (uint8_t)mode_uv;
    b.tx_type_off = 0;                                   // every luma transform is DCT_DCT: one shared entry
    b.lev_off[0] = (uint32_t)oy; b.lev_off[1] = (uint32_t)(ny + oc); b.lev_off[2] = (uint32_t)(ny + nc + oc);
    blocks.push_back(b);
  };
  const int w32 = width / 32, w8 = width / 8;
  std::vector<size_t> starts;          // per tile (= superblock): its first block, its first partition symbol; the writer's threads start there
  for (int sr = 0; sr * 16 < mi_rows; sr++)
    for (int sc = 0; sc * 16 < mi_cols; sc++) {
      starts.push_back(blocks.size()); starts.push_back(parts.size());
      if (sr * 64 < hA) {                                // PARTITION_SPLIT at 64x64, four 32x32 blocks (two where the frame ends mid-superblock)
        parts.push_back(3);
        for (int k = 0; k < 4; k++) {
          const int r32 = sr * 2 + (k >> 1), c32 = sc * 2 + (k & 1);
          if (c32 >= w32) continue;
          const size_t i = (size_t)r32 * w32 + c32;
          parts.push_back(0);
          block(r32 * 8, c32 * 8, 9 /* BLOCK_32X32 */, my[i], muv[i], i * 1024, i * 256);
        }
      } else {                                           // the last, partial superblock row: split down to 8x8 wherever the frame reaches
        const size_t oyB = (size_t)hA * width, ocB = oyB / 4;
        const uint8_t *myB = my + fr.key_modes_band, *muvB = muv + fr.key_modes_band;
        for (int k = 0; k < 64; k++) {                   // z-order over the superblock's 8x8 blocks; a level's symbol precedes its first block
          int bx = 0, by = 0;
          for (int i = 0; i < 3; i++) { bx |= ((k >> (2 * i)) & 1) << i; by |= ((k >> (2 * i + 1)) & 1) << i; }
          const int r = sr * 16 + by * 2, c = sc * 16 + bx * 2;
          for (int n8 = 8; n8 >= 2; n8 >>= 1)            // 64, 32, 16: PARTITION_SPLIT at every level that starts here, inside the frame
            if (!(bx & (n8 - 1)) && !(by & (n8 - 1)) && r < mi_rows && c < mi_cols) parts.push_back(3);
          if (r >= mi_rows || c >= mi_cols) continue;
          parts.push_back(0);
          const size_t i = (size_t)(r / 2 - hA / 8) * w8 + c / 2;
          block(r, c, 3 /* BLOCK_8X8 */, myB[i], muvB[i], oyB + i * 64, ocB + i * 16);
        }
      }
    }
  av1mi_obu_blocks d;
  memset(&d, 0, sizeof(d));
  d.hdr = desc.f;
  const uint8_t dct = 0;
  d.partition = parts.data(); d.n_partition = parts.size(); d.blocks = blocks.data(); d.n_blocks = blocks.size(); d.tx_type = &dct; d.levels = lev.data();
  starts.push_back(blocks.size()); starts.push_back(parts.size());
  std::string werr;
  if (!av1::blocks_temporal_unit(d, with_sequence_header, out, &werr, threads, reinterpret_cast<const size_t (*)[2]>(starts.data()))) {
    if (err) *err = "bitstream writer: " + werr;
    return false;
  }
  return true;
}

bool SessionTemporalUnit(const av1mi_gop_frame &fr, int seg, int width, int height, int bit_depth, int visible_width, int visible_height,
                         bool with_sequence_header, int threads, std::vector<uint8_t> *out, std::string *err, bool film_grain_present,
                         const av1mi_film_grain *film_grain, const av1mi_colour *colour) {
  SessionFrameDesc desc;
  DescribeSessionFrame(fr, seg, width, height, bit_depth, &desc, visible_width, visible_height);
  desc.f.film_grain_present = film_grain_present; desc.f.film_grain = film_grain; desc.f.colour = colour;
  std::string werr;
  if (fr.tile_size) {      // tiles coded on the GPU: frame header + tile group around them
    const uint32_t *sz = fr.tile_size + (size_t)seg * fr.tiles_per_frame;
    size_t off = 0;
    for (size_t i = 0; i < (size_t)seg * fr.tiles_per_frame; i++) off += fr.tile_size[i];
    std::vector<uint8_t> frame;
    if (!av1::frame_obu_from_tiles(desc.f, fr.tile_payload + off, sz, fr.tiles_per_frame, &frame, &werr)) { if (err) *err = "bitstream assembly: " + werr; return false; }
    *out = av1::temporal_delimiter_obu();
    if (with_sequence_header) av1::append_sequence_obus(av1::sequence_params(desc.f), out);
    out->insert(out->end(), frame.begin(), frame.end());
    return true;
  }
  if (fr.key_block_size == 32) return Key32TemporalUnit(fr, seg, desc, width, height, with_sequence_header, threads, out, err);      // symbols of a key frame in 32x32 blocks
  if (!av1::temporal_unit(desc.f, with_sequence_header, threads, out, &werr)) { if (err) *err = "bitstream writer: " + werr; return false; }
  return true;
}

int RunBackend(const BackendJob &job, std::string *err) {
  av1mi_ctx *ctx = nullptr;
  if (av1mi_device_count() <= 0 || av1mi_open(job.device, &ctx) != AV1MI_OK) {
    *err = "Error: no usable HIP device for the av1mi backend (device " + std::to_string(job.device) + ")";
    return -1;
  }
  Y4mSource y;
  av1mi_gop *gop = nullptr;
  StreamSink sink;
  int code = 0;
#define CHK(call)                                                                                   \
  do { int rc_ = (call); if (rc_ != AV1MI_OK) { *err = std::string(#call) + ": " + av1mi_last_error(ctx); code = 2; goto done; } } while (0)
  if (!y.open(job.input, err, job.to_420)) { code = 1; goto done; }
  {
    // the target: what the argv's filter chain yields on this source (transcode.go:92-115), or -av1mi_scale; no chain = the source
    // the window first: -av1mi_crop stands in front of the chain, whose filters then see the window's size
    CropRect win;
    if (job.crop_mode == 2) {
      win = job.crop;
      if (win.w > y.w || win.h > y.h || win.x > y.w - win.w || win.y > y.h - win.h) {
        *err = "Invalid argument: -av1mi_crop " + std::to_string(win.w) + ":" + std::to_string(win.h) + ":" + std::to_string(win.x) + ":" + std::to_string(win.y) +
               " lies outside the " + std::to_string(y.w) + "x" + std::to_string(y.h) + " picture";
        code = 1; goto done;
      }
    } else if (job.crop_mode == 1) {
      // cropping by a stream's first frames would crop by its opening credits, and what is cropped is gone
      if (!y.seekable()) { *err = "Invalid argument: -av1mi_crop auto needs a seekable file: it samples frames from all over the input, not from a pipe or FIFO"; code = 1; goto done; }
      const long have = y.prepare(0, y.known_frames(), err);
      if (have < 0) { code = 1; goto done; }
      const int n = (int)std::min<long>(kCropSampleFrames, have), W8 = (y.w + 7) & ~7, H8 = (y.h + 7) & ~7;
      const size_t plane = (size_t)W8 * H8 * (y.src_bd == 8 ? 1 : 2);
      std::vector<unsigned char> luma(plane * (size_t)std::max(n, 1)), cu(plane), cv(plane);      // (the chroma planes are read and dropped)
      for (int i = 0; i < n; i++)
        if (!y.read((long)i * have / n, W8, H8, luma.data() + plane * (size_t)i, cu.data(), cv.data())) { *err = job.input + ": Invalid data found when processing input (truncated frame)"; code = 1; goto done; }
      std::vector<av1mi_crop_record> rec((size_t)std::max(n, 1));
      if (n > 0) {
        void *d_luma = nullptr, *d_rec = nullptr;
        int rc = av1mi_malloc(ctx, &d_luma, luma.size());
        if (rc == AV1MI_OK) rc = av1mi_malloc(ctx, &d_rec, rec.size() * sizeof(av1mi_crop_record));
        if (rc == AV1MI_OK) rc = av1mi_upload(ctx, d_luma, luma.data(), luma.size());
        if (rc == AV1MI_OK) rc = av1mi_crop_analyse(ctx, y.src_bd, W8, H8, y.w, y.h, n, d_luma, job.crop_limit, (av1mi_crop_record *)d_rec);
        if (rc == AV1MI_OK) rc = av1mi_download(ctx, rec.data(), d_rec, rec.size() * sizeof(av1mi_crop_record));
        if (rc != AV1MI_OK) *err = std::string("av1mi_crop_analyse: ") + av1mi_last_error(ctx);
        if (d_luma) (void)av1mi_free(ctx, d_luma);
        if (d_rec) (void)av1mi_free(ctx, d_rec);
        if (rc != AV1MI_OK) { code = 2; goto done; }
      }
      if (!PlanCrop(rec.data(), n, y.w, y.h, &win) || !win.trims(y.w, y.h)) win = CropRect();      // no bars: today's path, exactly
    }
    const int pw = win.w ? win.w : y.w, ph = win.w ? win.h : y.h;      // the picture the chain works on
    int tw = pw, th = ph;
    bool square = y.sar_n == y.sar_d;
    CropRect chain_crop;
    if (job.have_vf && !ChainTarget(pw, ph, y.sar_n, y.sar_d, job.vf, &tw, &th, &square, err, nullptr, nullptr, &chain_crop)) { code = 1; goto done; }
    if (chain_crop.w) win = chain_crop;      // (ParseBackendJob: never together with -av1mi_crop)
    if (job.scale_w) { tw = job.scale_w; th = job.scale_h; square = true; }
    const bool scaling = win.w != 0 || tw != y.w || th != y.h || job.scale_w != 0;      // a window is fed like a source to be scaled: whole frames
    const int G = job.gop, w = (tw + 7) & ~7, h = (th + 7) & ~7;       // the coded size; tw x th is what a decoder outputs
    int S = std::max(job.segments, 1);
    if (y.known_frames() >= 0) S = (int)std::max<long>(1, std::min<long>(S, (y.known_frames() + G - 1) / G));      // no more segments than the file has GOPs
    long total_frames = 0;
    const int threads = job.threads > 0 ? job.threads : (int)std::max(1u, std::thread::hardware_concurrency());
    av1mi_gop_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    if (w != tw || h != th) { cfg.visible_width = tw; cfg.visible_height = th; }
    if (scaling) { cfg.source_width = y.w; cfg.source_height = y.h; }
    if (win.w) { cfg.crop_x = win.x; cfg.crop_y = win.y; cfg.crop_width = win.w; cfg.crop_height = win.h; }
    cfg.width = w; cfg.height = h; cfg.bit_depth = y.bd; cfg.base_q_idx = job.quality < 1 ? 1 : job.quality; cfg.gop_length = G; cfg.segments = S;
    cfg.search_range = 8;
    cfg.coarse_range = job.me_range;      // -av1mi_me_range: the coarse search in front of it
    cfg.gpu_entropy = job.gpu_entropy ? 1 : 0;
    // -av1mi_stats / -av1mi_min_psnr: the session measures every batch on the GPU; the records arrive with the collected batch
    const bool measure = !job.stats_path.empty() || job.min_psnr > 0;
    cfg.quality_stats = measure ? 1 : 0;
    std::string stats;                 // the stats file's lines, in presentation order
    av1mi::quality::Summary summary;
    long long total_bytes = 0;
    // key frames in 32x32 blocks where the frame allows it (the coded width a multiple of 32)
    cfg.key_block_size = (job.key_block_size == 32 && (w & 31) == 0) ? 32 : 8;
    // -av1mi_pack10 1: a 10-bit source crosses PCIe at 10 bits per sample; the session's pinned buffers are then three packed planes
    // A source that is not 4:2:0 at the coded depth (only a job that converts opens one): fed in its own layout, converted on the GPU
    const bool convert = y.chroma != AV1MI_CHROMA_420 || y.src_bd != y.bd;
    if (convert) { cfg.source_chroma = y.chroma; cfg.source_bit_depth = y.src_bd; }
    const bool packed = job.pack10 && y.bd == 10 && !convert;      // (planar 4:2:0 10-bit only)
    if (packed) cfg.input_format = AV1MI_INPUT_PACKED10;
    // -av1mi_deinterlace: auto follows the header's I parameter, tff / bff force a parity
    int dei = job.deinterlace == 2 ? 1 : job.deinterlace == 3 ? 2 : 0;
    if (job.deinterlace == 1) {
      if (y.interlace == 3) { *err = "Invalid argument: -av1mi_deinterlace auto: the source is mixed-mode interlaced (Im); field-rate output and inverse telecine are not built"; code = 1; goto done; }
      dei = y.interlace;
    }
    cfg.deinterlace = dei;
    // -av1mi_scenecut, or a job that deinterlaces: the frame store holds one group (the deinterlacer's run)
    // -av1mi_denoise: the same store, the denoiser in the gather; -av1mi_film_grain (1 unless told otherwise): parameters in every frame header
    cfg.denoise = job.denoise;
    cfg.denoise_range = job.denoise_range;
    // the stream's colour record: the job's options, the header's range; a tone-mapped job says what the kernel makes
    const av1mi_colour colour = JobColour(job, y.colour_range);
    if (const char *why = av1::colour_error(colour)) { *err = std::string("Invalid argument: ") + why; code = 1; goto done; }
    if (job.tonemap) {
      if (y.bd != 10) { *err = "Invalid argument: tone mapping needs a 10-bit source (an 8-bit HDR10 source does not exist)"; code = 1; goto done; }
      if (y.colour_range == 1) { *err = "Invalid argument: tone mapping takes a limited-range source; the Y4M header says XCOLORRANGE=FULL"; code = 1; goto done; }
      cfg.tone_map = 1;
      cfg.tone_map_peak = job.tonemap_peak ? job.tonemap_peak : job.hdr.have_mdcv ? (int)std::min<uint32_t>(std::max<uint32_t>(job.hdr.luminance_max >> 8, 100), 10000) : 0;
    }
    const bool grainy = job.denoise > 0 && job.film_grain != 0;
    const bool analysed = job.scenecut > 0, stored = analysed || dei != 0 || job.denoise > 0;
    if (stored) cfg.store_frames = S * G;
    // What the reader threads deliver, one segment's share of the pinned buffers: frames of the coded size (the source's edge replicated
    // into the padding) or, when the GPU scales, of the source size rounded up to 8; no chroma planes for a grey source.  (A config the
    // layout refuses, av1mi_gop_open refuses below, with the reason.)
    av1mi_source_layout fed = {};
    (void)av1mi_gop_source_layout(&cfg, &fed);
    auto at = [&](void *plane, int p, int i) { return (unsigned char *)plane + fed.plane[p].frame_bytes * (size_t)i; };      // frame i of a pinned plane
    std::vector<std::vector<unsigned char>> scratch(packed ? (size_t)S : 0);          // per reader thread: one planar frame to pack from
    CHK(av1mi_gop_open(ctx, &cfg, &gop));
    av1::SequenceParams sp; sp.width = tw; sp.height = th; sp.bit_depth = y.bd; sp.film_grain = grainy; sp.colour = colour;
    const av1mi_colour *const stream_colour = sp.has_colour() ? &colour : nullptr;
    // pixels that stay non-square: the track at least says at which shape to show them
    if (!square) sink.set_display_size((int)((long)tw * y.sar_n / y.sar_d), th);
    for (const std::string &side : job.tracks)
      if (!sink.add_side_file(side, err)) { code = 1; goto done; }
    if (!sink.open(job.output, sp, y.fps_n, y.fps_d, err)) { code = 1; goto done; }
    std::vector<std::vector<std::vector<uint8_t>>> units((size_t)S);   // [segment][frame] temporal units of the batch in flight
    struct Rec { av1mi_quality q[3]; };
    std::vector<std::vector<Rec>> records((size_t)S);                  // ... and their quality records (measure)
    // A target (-b:v:0 / -av1mi_target_bpp): the controller lives across the groups.  It is asked at ONE point of the loop (before each
    // submit) and told at one (after each assemble), so the quantisers, and with them the output bytes, are a function of the input alone.
    std::unique_ptr<RateControl> rc;
    std::vector<std::vector<int>> grains((size_t)S);                   // ... and, denoising, their luma scaling at mid grey (the stats file's grain:)
    std::vector<std::vector<int>> qs((size_t)S);                       // ... and, with a target, their quantisers (the stats file's q:)
    long long rc_bytes = 0, rc_frames = 0;
    if (job.bitrate || job.target_bpp_u) {
      av1mi_rc_params rp;
      memset(&rp, 0, sizeof(rp));
      av1mi_rc_defaults(&rp);
      if (job.bitrate) { rp.target_num = job.bitrate * y.fps_d; rp.target_den = 8ll * y.fps_n; }
      else { rp.target_num = job.target_bpp_u * tw * th; rp.target_den = 8000000; }
      if (job.qmin) rp.qmin = job.qmin;
      if (job.qmax) rp.qmax = job.qmax;
      rp.gop_length = G; rp.bit_depth = y.bd;
      rp.start_q = std::min(std::max(cfg.base_q_idx, rp.qmin), rp.qmax);
      if (const char *why = RateControl::ParamError(rp)) { *err = std::string("Invalid argument: rate control: ") + why; code = 1; goto done; }
      rc.reset(new RateControl(rp));
    }
    const int lag = av1mi_gop_max_in_flight() - 1;      // batches the GPU holds while the host works on the oldest
    // the layout of the group in flight: GOP s holds frames start[s] .. start[s] + len[s] - 1 of the group.  Fixed (s G, up to G frames)
    // unless the planner moves the boundaries onto cuts (stored)
    std::vector<int32_t> start((size_t)S), len((size_t)S), index((size_t)S);
    std::vector<uint8_t> cut;                           // stored: the frames of the group the analysis flagged
    std::vector<av1mi_scene_record> scene;
    int cur_store = 0;
    long next_frames = -1;                              // stored: frames of the group that is (being) put into the other store; -1 = not asked yet
    // One chunk of a group -> a store (stored): frames f0 .. f0 + n - 1 of the group the reader has prepared, read by one thread each into
    // the session's pinned buffers IN FILE ORDER, then put.  begin starts the threads, end joins them and queues the copy.
    struct Reads {
      std::vector<std::thread> th; std::vector<char> ok;
      bool join() { for (auto &x : th) if (x.joinable()) x.join(); th.clear(); for (char c : ok) if (!c) return false; return true; }
      ~Reads() { for (auto &x : th) if (x.joinable()) x.join(); }
    };
    Reads puts;
    auto put_begin = [&](long f0, int n) -> bool {
      void *py, *pu, *pv;
      if (av1mi_gop_acquire_input(gop, &py, &pu, &pv) != AV1MI_OK) { *err = std::string("av1mi_gop_acquire_input: ") + av1mi_last_error(ctx); return false; }
      puts.ok.assign((size_t)n, 1);
      for (int i = 0; i < n; i++)
        puts.th.emplace_back([&, i, f0, py, pu, pv]() {
          puts.ok[(size_t)i] = y.read(f0 + i, fed.width, fed.height, at(py, 0, i), at(pu, 1, i), at(pv, 2, i));
        });
      return true;
    };
    auto put_end = [&](int store, long f0, int n) -> int {      // 0, or the exit code
      if (!puts.join()) { *err = job.input + ": Invalid data found when processing input (truncated frame)"; return 1; }
      if (av1mi_gop_store_put(gop, store, (int)f0, n) != AV1MI_OK) { *err = std::string("av1mi_gop_store_put: ") + av1mi_last_error(ctx); return 2; }
      return 0;
    };
    for (long g0 = 0;; g0 += S) {
      for (auto &u : units) u.clear();
      for (auto &r : records) r.clear();
      for (auto &v : qs) v.clear();
      for (auto &v : grains) v.clear();
      // the next GROUP of S GOPs: a file is read in place, a stream one group ahead of the encoder (y4m.hpp)
      long have_frames;
      if (stored && next_frames >= 0) have_frames = next_frames;      // already in the store: it was put while the group before ran
      else {
        have_frames = y.prepare(g0 * G, (long)S * G, err);
        if (have_frames < 0) { code = 1; goto done; }
        for (long f0 = 0; stored && f0 < have_frames; f0 += S) {      // the first group: nothing runs beside it
          const int n = (int)std::min<long>(S, have_frames - f0);
          if (!put_begin(f0, n)) { code = 2; goto done; }
          if ((code = put_end(cur_store, f0, n)) != 0) goto done;
        }
      }
      if (have_frames == 0) break;
      total_frames += have_frames;
      for (int s = 0; s < S; s++) { start[(size_t)s] = s * G; len[(size_t)s] = (int32_t)std::max<long>(0, std::min<long>(G, have_frames - (long)s * G)); }
      if (analysed) {
        scene.resize((size_t)have_frames); cut.assign((size_t)have_frames, 0);
        CHK(av1mi_gop_store_analyse(gop, cur_store, (int)have_frames, scene.data()));
        for (long f = 0; f < have_frames; f++) cut[(size_t)f] = (uint8_t)av1mi_scene_is_cut(&scene[(size_t)f], job.scenecut);
        if (av1mi_plan_gops((int)have_frames, G, S, job.min_gop, cut.data(), start.data(), len.data()) < 0) { *err = "Invalid argument: -av1mi_min_gop does not fit the GOP length"; code = 1; goto done; }
      }
      if (stored) {      // (a job that only deinterlaces keeps the nominal layout above)
        // the group after this one: prepared now (this group's frames are all in the store), put chunk by chunk beside the batches below
        next_frames = y.prepare((g0 + S) * G, (long)S * G, err);
        if (next_frames < 0) { code = 1; goto done; }
      }
      long next_put = 0;                                  // stored: frames of the next group already put
      // frames of this group that exist: segment s, position t -> frame start[s] + t of the group
      auto exists = [&](int s, int t) { return t < len[(size_t)s]; };
      int T = 0;
      for (int s = 0; s < S; s++) T = std::max(T, (int)len[(size_t)s]);
      av1mi_gop_frame fr;
      auto collect_oldest = [&]() -> bool {
        if (av1mi_gop_collect(gop, &fr) != AV1MI_OK) { *err = std::string("av1mi_gop_collect: ") + av1mi_last_error(ctx); return false; }
        return true;
      };
      auto assemble = [&](int t) -> bool {         // the collected batch t -> temporal units (frame header + tile group, or the host coder)
        long long batch_bytes = 0;
        for (int s = 0; s < S; s++) {
          if (!exists(s, t)) continue;
          std::vector<uint8_t> tu;
          av1mi_film_grain fg;
          if (job.denoise) {      // what the gather removed from this frame -> the parameters that put it back (none for the ends of a run)
            if (!fr.grain) { *err = "the session returned no grain records"; return false; }
            FilmGrainFromRecords(fr.grain + (size_t)s * 3, y.bd, (int)(g0 * G + start[(size_t)s] + t), &fg);
            grains[(size_t)s].push_back(FilmGrainMidGrey(fg));
          }
          if (!SessionTemporalUnit(fr, s, w, h, y.bd, cfg.visible_width, cfg.visible_height, t == 0, threads, &tu, err, grainy, grainy ? &fg : nullptr, stream_colour)) return false;
          batch_bytes += (long long)tu.size();
          if (rc) qs[(size_t)s].push_back(fr.params.base_q_idx);
          units[(size_t)s].push_back(std::move(tu));
          if (measure) {
            if (!fr.quality) { *err = "the session returned no quality records"; return false; }
            Rec r;
            memcpy(r.q, fr.quality + (size_t)s * 3, sizeof(r.q));
            records[(size_t)s].push_back(r);
          }
        }
        if (rc) {      // the truth replaces the controller's prediction for this batch; segments that do not exist count nowhere
          rc_bytes += batch_bytes;
          if (rc->Collected(batch_bytes) != 0) { *err = "rate control: nothing in flight"; return false; }
        }
        return true;
      };
      // The frames of batch t + 1 are read (one thread per segment) WHILE the host assembles batch t - lag: the session hands out
      // the next input buffers as soon as the oldest batch has been collected.
      Reads reads;
      auto start_reads = [&](int t) -> bool {
        void *py, *pu, *pv;
        if (av1mi_gop_acquire_input(gop, &py, &pu, &pv) != AV1MI_OK) { *err = std::string("av1mi_gop_acquire_input: ") + av1mi_last_error(ctx); return false; }
        reads.ok.assign((size_t)S, 1);
        for (int s = 0; s < S; s++) {
          if (!exists(s, t)) {
            // a shorter last GOP / fewer GOPs than segments: the slot is coded (the batch is one launch) and its output dropped.  Flat
            // planes, not whatever the pinned buffer held: stale pixels could cost the GPU coder's tile capacity for the whole batch
            // (zero samples pack to zero bytes)
            void *const plane[3] = { py, pu, pv };
            for (int p = 0; p < 3; p++) if (fed.plane[p].frame_bytes) memset(at(plane[p], p, s), 0, fed.plane[p].frame_bytes);
            continue;
          }
          reads.th.emplace_back([&, s, t, py, pu, pv]() {
            if (!packed) {
              reads.ok[(size_t)s] = y.read((long)start[(size_t)s] + t, fed.width, fed.height, at(py, 0, s), at(pu, 1, s), at(pv, 2, s));
              return;
            }
            // the frame (edge padding included) into this thread's scratch, then packed into the segment's byte range of the pinned planes
            std::vector<unsigned char> &f = scratch[(size_t)s];
            const size_t fy = (size_t)fed.width * fed.height * 2, fc = fy / 4;      // planar 10-bit planes
            f.resize(fy + 2 * fc);
            reads.ok[(size_t)s] = y.read((long)start[(size_t)s] + t, fed.width, fed.height, f.data(), f.data() + fy, f.data() + fy + fc) &&
                                  av1mi_input_pack(AV1MI_INPUT_PACKED10, 10, fed.width, fed.height, f.data(), f.data() + fy, f.data() + fy + fc, at(py, 0, s), at(pu, 1, s), at(pv, 2, s)) == AV1MI_OK;
          });
        }
        return true;
      };
      if (!stored && T > 0 && !start_reads(0)) { code = 2; goto done; }
      for (int t = 0; t < T; t++) {
        if (!stored && !reads.join()) { *err = job.input + ": Invalid data found when processing input (truncated frame)"; code = 1; goto done; }
        if (rc) {
          int frames = 0;
          for (int s = 0; s < S; s++) frames += exists(s, t) ? 1 : 0;
          rc_frames += frames;
          const int q = rc->NextQ(t == 0 ? 0 : 1, frames);
          if (q < 1) { *err = "rate control: no quantiser for the next batch"; code = 2; goto done; }
          CHK(av1mi_gop_set_base_q_idx(gop, q));
        }
        if (stored) {
          for (int s = 0; s < S; s++) index[(size_t)s] = exists(s, t) ? start[(size_t)s] + t : -1;      // (-1: a flat slot, its output dropped)
          CHK(av1mi_gop_submit_stored(gop, cur_store, index.data(), t == 0 ? 0 : 1));
        } else CHK(av1mi_gop_submit(gop, t == 0 ? 0 : 1));
        const bool have = t >= lag;
        if (have && !collect_oldest()) { code = 2; goto done; }            // the GPU works on the frames after it meanwhile
        // what is read beside the host's work on the oldest batch: the next batch's frames, or (stored) the next chunk of the next group
        const int chunk = stored ? (int)std::min<long>(S, next_frames - next_put) : 0;
        if (!stored && t + 1 < T && !start_reads(t + 1)) { code = 2; goto done; }
        if (chunk > 0 && !put_begin(next_put, chunk)) { code = 2; goto done; }
        if (have && !assemble(t - lag)) { code = 2; goto done; }
        if (chunk > 0) { if ((code = put_end(cur_store ^ 1, next_put, chunk)) != 0) goto done; next_put += chunk; }
      }
      for (int t = std::max(0, T - lag); t < T; t++)
        if (!collect_oldest() || !assemble(t)) { code = 2; goto done; }
      for (; stored && next_put < next_frames; ) {      // (a group of short GOPs has fewer batches than the next group has chunks)
        const int n = (int)std::min<long>(S, next_frames - next_put);
        if (!put_begin(next_put, n)) { code = 2; goto done; }
        if ((code = put_end(cur_store ^ 1, next_put, n)) != 0) goto done;
        next_put += n;
      }
      for (int s = 0; s < S; s++)
        for (size_t t = 0; t < units[(size_t)s].size(); t++)
          if (!sink.write(units[(size_t)s][t], t == 0, err)) { code = 1; goto done; }
      if (measure)
        for (int s = 0; s < S; s++)
          for (size_t t = 0; t < units[(size_t)s].size(); t++) {
            char line[512];
            int n = snprintf(line, sizeof(line), "n:%ld type:%c bytes:%zu", summary.frames, t == 0 ? 'K' : 'P', units[(size_t)s][t].size());
            n += av1mi::quality::format_figures(av1mi::quality::frame_figures(records[(size_t)s][t].q, y.bd), line + n, sizeof(line) - (size_t)n);
            if (win.w && summary.frames == 0) n += snprintf(line + n, sizeof(line) - (size_t)n, " crop:%dx%d+%d+%d", win.w, win.h, win.x, win.y);
            if (sp.described() && summary.frames == 0) n += snprintf(line + n, sizeof(line) - (size_t)n, " colour:%d/%d/%d/%d", colour.primaries, colour.transfer, colour.matrix, colour.full_range);
            if (rc) n += snprintf(line + n, sizeof(line) - (size_t)n, " q:%d", qs[(size_t)s][t]);
            if (job.denoise) n += snprintf(line + n, sizeof(line) - (size_t)n, " grain:%d", grains[(size_t)s][t]);
            if (analysed && cut[(size_t)start[(size_t)s] + t]) n += snprintf(line + n, sizeof(line) - (size_t)n, " cut:1");
            stats.append(line, (size_t)n); stats += '\n';
            summary.add(records[(size_t)s][t].q, y.bd);
            total_bytes += (long long)units[(size_t)s][t].size();
          }
      if (stored) cur_store ^= 1;
    }
    if (total_frames == 0) { *err = job.input + ": Invalid data found when processing input (no frames)"; code = 1; goto done; }
    if (!sink.close(err)) { code = 1; goto done; }
    if (rc && rc_frames > 0) {
      const av1mi_rc_params &rp = rc->params();
      const double fps = (double)y.fps_n / y.fps_d, px = (double)tw * th, want = 8.0 * rp.target_num / rp.target_den, got = 8.0 * rc_bytes / rc_frames;
      fprintf(stderr, "[av1mi] rate control: target %.0f bit/s (%.4f bit/pixel), achieved %.0f bit/s (%.4f bit/pixel) over %lld frames\n", want * fps, want / px,
              got * fps, got / px, rc_frames);
    }
    if (measure) {
      const av1mi::quality::Figures f = summary.figures(y.bd);
      if (!job.stats_path.empty()) {
        char line[512];
        int n = snprintf(line, sizeof(line), "summary frames:%ld bytes:%lld", summary.frames, total_bytes);
        n += av1mi::quality::format_figures(f, line + n, sizeof(line) - (size_t)n);
        stats.append(line, (size_t)n); stats += '\n';
        FILE *sf = fopen(job.stats_path.c_str(), "wb");
        const bool ok = sf && fwrite(stats.data(), 1, stats.size(), sf) == stats.size();
        if ((sf && fclose(sf)) || !ok) { *err = job.stats_path + ": could not write the stats file"; remove(job.output.c_str()); code = 1; goto done; }
      }
      if (job.min_psnr > 0 && f.psnr[0] < job.min_psnr) {      // the quality gate: the file is not good enough to stand in for its source
        char why[160];
        snprintf(why, sizeof(why), "quality gate: psnr_y %.6f dB below the bound %.6f dB", f.psnr[0], job.min_psnr);
        *err = why;
        remove(job.output.c_str());
        code = 3; goto done;
      }
    }
  }
done:
  sink.abort();
  if (gop) av1mi_gop_close(gop);
  y.close();
  av1mi_close(ctx);
  return code;
#undef CHK
}

}  // namespace av1mi_host
