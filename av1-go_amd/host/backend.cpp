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
// With -av1mi_deinterlace_rate field it makes two output frames of every stored frame: the groups, their layouts and the stored batches'
// indices then count OUTPUT frames, the reader and the store source frames (SessionPlan::out_per_src; fieldrate.hpp).
// With -av1mi_ivtc 1 a group of segments x gop OUTPUT frames is segments x gop x 5 / 4 source frames (fieldrate.hpp's ratio): they are put into
// the store with one context frame on either side, the session gives their field-match records (av1mi_gop_store_telecine), the plan
// (telecineplan.hpp) drops one frame of every five and names the two frames each kept one is woven from, and the batches are submitted as
// woven pairs (av1mi_gop_submit_woven): run_groups_telecine.
// With -av1mi_scenecut the GOPs of a group do not start every `gop` frames but where the scene analysis finds cuts: the group's frames go
// into the session's frame store in file order (av1mi_gop_store_put), are analysed there (av1mi_gop_store_analyse), the planner
// (sceneplan.hpp) lays the GOPs out, and every batch is gathered from the store (av1mi_gop_submit_stored).  The session has two stores:
// the next group's frames are read and put while this group's batches run.
//
// A crop window — a crop= filter in front of the chain, -av1mi_crop W:H:X:Y, or the bars that -av1mi_crop auto finds — is settled BEFORE the
// session is opened: auto reads up to 32 frames spread evenly over a seekable file, uploads their luma planes, runs av1mi_crop_analyse
// and plans the window (cropplan.hpp).  The session is then opened with the window (av1mi_gop_config.crop_*) and fed whole frames; the
// rest of the chain sees the window's size.  No window = the path below as it has always been.
// -av1mi_denoise auto is settled at the same point, the same way: up to 16 pairs of consecutive frames spread over a seekable file, their
// luma uploaded as the file holds it, av1mi_noise_analyse, and the plan (noiseplan.hpp) makes the job the job -av1mi_denoise N.
// -av1mi_tonemap_peak auto likewise: up to 32 frames in the crop sampler's slots, all three planes, av1mi_peak_analyse, and the plan
// (peakplan.hpp) makes the job the job -av1mi_tonemap_peak N.
//
// `segments` closed GOPs of the file are coded in lockstep (the session's batch dimension); while the host codes the
// symbols of frame t the GPU already works on frames t + 1 and t + 2 (three batches in flight).
//
// RunBackend is a list of steps, each a method of Run (the job's state; its destructor releases what the steps opened) that returns the
// exit code, 0 = go on: settle_window, settle_denoise, settle_peak, session_config (SessionConfig: the policy, a pure function), open_session, run_groups, finish.
#include "filmgrain.hpp"
#include "backend.hpp"
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <thread>
#include <vector>
#include "av1_bitstream.hpp"
#include "cropplan.hpp"
#include "fieldrate.hpp"
#include "noiseplan.hpp"
#include "peakplan.hpp"
#include "ratecontrol.hpp"
#include "sceneplan.hpp"
#include "telecineplan.hpp"
#include "y4m.hpp"

namespace av1mi_host {

int ExplicitWindow(const BackendJob &job, int w, int h, CropRect *win, std::string *err) {
  *win = job.crop;
  if (win->w <= w && win->h <= h && win->x <= w - win->w && win->y <= h - win->h) return 0;
  *err = "Invalid argument: -av1mi_crop " + std::to_string(win->w) + ":" + std::to_string(win->h) + ":" + std::to_string(win->x) + ":" + std::to_string(win->y) +
         " lies outside the " + std::to_string(w) + "x" + std::to_string(h) + " picture";
  return 1;
}

int SessionConfig(const BackendJob &job, const SourceFacts &src, const CropRect &window, SessionPlan *plan, std::string *err) {
  auto refuse = [&](const std::string &why) { *err = "Invalid argument: " + why; return 1; };
  *plan = SessionPlan();      // (a refused job leaves a plan of zeros, never an indeterminate one)
  // the target: what the argv's filter chain yields on this source (transcode.go:92-115), or -av1mi_scale; no chain = the source
  // the window first: -av1mi_crop stands in front of the chain, whose filters then see the window's size
  CropRect &win = plan->win = window;
  const int pw = win.w ? win.w : src.w, ph = win.w ? win.h : src.h;      // the picture the chain works on
  int &tw = plan->tw = pw, &th = plan->th = ph;
  plan->square = src.sar_n == src.sar_d;
  CropRect chain_crop;
  if (job.have_vf && !ChainTarget(pw, ph, src.sar_n, src.sar_d, job.vf, &tw, &th, &plan->square, err, nullptr, nullptr, &chain_crop)) return 1;
  if (chain_crop.w) win = chain_crop;      // (ParseBackendJob: never together with -av1mi_crop)
  if (job.scale_w) { tw = job.scale_w; th = job.scale_h; plan->square = true; }
  const bool scaling = win.w != 0 || tw != src.w || th != src.h || job.scale_w != 0;      // a window is fed like a source to be scaled: whole frames
  const int G = job.gop, w = (tw + 7) & ~7, h = (th + 7) & ~7;       // the coded size; tw x th is what a decoder outputs
  int S = std::max(job.segments, 1);
  // the output: -av1mi_deinterlace_rate field makes two frames of each source frame, at twice the rate; G counts OUTPUT frames
  const JobOutput output = JobOutputOf(job, src.interlace, src.fps_n, src.fps_d, src.known_frames);
  plan->out_per_src = output.per_source; plan->fps_n = output.fps_n; plan->fps_d = output.fps_d;
  if (job.ivtc && (G & 3)) return refuse("with -av1mi_ivtc -g counts output frames, four per five source frames, and must be a multiple of 4: not -g " + std::to_string(G));
  if (output.per_source == 2 && (G & 1)) return refuse("with -av1mi_deinterlace_rate field -g counts output frames, two per source frame, and must be even: not -g " + std::to_string(G));
  if (output.frames >= 0) S = (int)std::max<long>(1, std::min<long>(S, (output.frames + G - 1) / G));      // no more segments than the file has GOPs
  av1mi_gop_config &cfg = plan->cfg;
  if (w != tw || h != th) { cfg.visible_width = tw; cfg.visible_height = th; }
  if (scaling) { cfg.source_width = src.w; cfg.source_height = src.h; }
  if (win.w) { cfg.crop_x = win.x; cfg.crop_y = win.y; cfg.crop_width = win.w; cfg.crop_height = win.h; }
  cfg.width = w; cfg.height = h; cfg.bit_depth = src.bd; cfg.base_q_idx = job.quality < 1 ? 1 : job.quality; cfg.gop_length = G; cfg.segments = S;
  cfg.search_range = 8;
  cfg.coarse_range = job.me_range;      // -av1mi_me_range: the coarse search in front of it
  cfg.gpu_entropy = job.gpu_entropy ? 1 : 0;
  cfg.lr_search = job.lr_search;        // -av1mi_lr_search: a restoration record chosen per unit
  cfg.cdef_search = job.cdef_search;    // -av1mi_cdef_search: cdef_bits, a CDEF strength set chosen per superblock
  cfg.lf_search = job.lf_search;        // -av1mi_lf_search: the deblocking levels chosen per frame
  // -av1mi_stats / -av1mi_min_psnr: the session measures every batch on the GPU; the records arrive with the collected batch
  plan->measure = !job.stats_path.empty() || job.min_psnr > 0;
  cfg.quality_stats = plan->measure ? 1 : 0;
  // key frames in 32x32 blocks where the frame allows it (the coded width a multiple of 32)
  cfg.key_block_size = (job.key_block_size == 32 && (w & 31) == 0) ? 32 : 8;
  // A source that is not 4:2:0 at the coded depth (only a job that converts opens one): fed in its own layout, converted on the GPU
  const bool convert = src.chroma != AV1MI_CHROMA_420 || src.src_bd != src.bd;
  if (convert) { cfg.source_chroma = src.chroma; cfg.source_bit_depth = src.src_bd; }
  // -av1mi_pack10 1: a 10-bit source crosses PCIe at 10 bits per sample; the session's pinned buffers are then three packed planes
  plan->packed = job.pack10 && src.bd == 10 && !convert;      // (planar 4:2:0 10-bit only)
  if (plan->packed) cfg.input_format = AV1MI_INPUT_PACKED10;
  // -av1mi_deinterlace: auto follows the header's I parameter, tff / bff force a parity
  int dei = job.deinterlace == 2 ? 1 : job.deinterlace == 3 ? 2 : 0;
  if (job.deinterlace == 1) {
    if (src.interlace == 3) return refuse("-av1mi_deinterlace auto: the source is mixed-mode interlaced (Im); field-rate output and inverse telecine are not built");
    dei = src.interlace;
  }
  cfg.deinterlace = dei;
  cfg.deinterlace_fields = output.per_source == 2;
  // -av1mi_ivtc: whatever the header's I parameter says; the session weaves what the plan asks for (telecineplan.hpp)
  plan->telecine = job.ivtc != 0;
  cfg.telecine = plan->telecine ? 1 : 0;
  // -av1mi_scenecut, or a job that deinterlaces: the frame store holds one group (the deinterlacer's run)
  // -av1mi_denoise: the same store, the denoiser in the gather; -av1mi_film_grain (1 unless told otherwise): parameters in every frame header
  cfg.denoise = job.denoise;
  cfg.denoise_range = job.denoise_range;
  cfg.grain_cov = job.grain_lag > 0;      // -av1mi_grain_lag: the covariance behind the gather, from which the AR coefficients follow
  // the stream's colour record: the job's options, the header's range; a tone-mapped job says what the kernel makes
  plan->colour = JobColour(job, src.colour_range);
  if (const char *why = av1::colour_error(plan->colour)) return refuse(why);
  if (job.tonemap) {
    if (job.tonemap_peak_auto && (src.chroma != AV1MI_CHROMA_420 || src.src_bd != 10))
      return refuse("-av1mi_tonemap_peak auto measures 4:2:0 10-bit frames as the file holds them: a 4:2:2, 4:4:4, grey, 8- or 12-bit source is not measured (give the peak as a number)");
    if (src.bd != 10) return refuse("tone mapping needs a 10-bit source (an 8-bit HDR10 source does not exist)");
    if (src.colour_range == 1) return refuse("tone mapping takes a limited-range source; the Y4M header says XCOLORRANGE=FULL");
    cfg.tone_map = 1;
    cfg.tone_map_peak = job.tonemap_peak ? job.tonemap_peak : job.hdr.have_mdcv ? (int)std::min<uint32_t>(std::max<uint32_t>(job.hdr.luminance_max >> 8, 100), 10000) : 0;
  }
  // -av1mi_depth: the depth that is coded.  The session's bit_depth stays the depth its input stages work at
  const int want = job.depth == -1 ? job.chain_depth : job.depth;      // 0 = the source's
  plan->coded_bd = src.bd;
  if (want == 10 && src.bd == 8)
    return refuse(std::string(job.depth == -1 ? "-av1mi_depth chain: the chain's last format= names a 10-bit format" : "-av1mi_depth 10") + " and the source has 8 bits: 8 -> 10 bits is not built");
  if (want == 8 && src.bd == 10) {
    if (job.denoise || job.denoise_auto) return refuse("a depth reduction together with -av1mi_denoise is not built: the grain records are measured in 10-bit codes and the grain would be synthesised into an 8-bit stream");
    cfg.coded_bit_depth = 8; cfg.depth_dither = job.dither != 0;      // (ordered unless -av1mi_dither round)
    plan->coded_bd = 8; plan->reduced_from = src.src_bd;
  }
  plan->grainy = job.denoise > 0 && job.film_grain != 0;
  plan->analysed = job.scenecut > 0;
  plan->stored = plan->analysed || dei != 0 || job.denoise > 0 || plan->telecine;
  if (plan->stored) cfg.store_frames = (int)((long)S * G * output.den / output.num);      // SOURCE frames: a group of S G output frames (the session adds the context frames' room)
  // What the reader threads deliver, one segment's share of the pinned buffers: frames of the coded size (the source's edge replicated
  // into the padding) or, when the GPU scales, of the source size rounded up to 8; no chroma planes for a grey source.  (A config the
  // layout refuses, av1mi_gop_open refuses, with the reason.)
  (void)av1mi_gop_source_layout(&cfg, &plan->fed);
  return 0;
}

std::string StatsFrameLine(long n, bool key, const FrameOut &f, int bit_depth, const StatsTags &tags, bool cut) {
  char line[512];
  int k = snprintf(line, sizeof(line), "n:%ld type:%c bytes:%zu", n, key ? 'K' : 'P', f.unit.size());
  k += av1mi::quality::format_figures(av1mi::quality::frame_figures(f.q, bit_depth), line + k, sizeof(line) - (size_t)k);
  if (tags.win.w && n == 0) k += snprintf(line + k, sizeof(line) - (size_t)k, " crop:%dx%d+%d+%d", tags.win.w, tags.win.h, tags.win.x, tags.win.y);
  if (tags.denoise_auto >= 0 && n == 0) k += snprintf(line + k, sizeof(line) - (size_t)k, " denoise:auto>%d", tags.denoise_auto);
  if (tags.peak_auto >= 0 && n == 0) k += snprintf(line + k, sizeof(line) - (size_t)k, " peak:auto>%d", tags.peak_auto);
  if (tags.depth_from && n == 0) k += snprintf(line + k, sizeof(line) - (size_t)k, " depth:%d>%d", tags.depth_from, tags.depth_to);
  if (tags.colour && n == 0) k += snprintf(line + k, sizeof(line) - (size_t)k, " colour:%d/%d/%d/%d", tags.colour->primaries, tags.colour->transfer, tags.colour->matrix, tags.colour->full_range);
  if (tags.q) k += snprintf(line + k, sizeof(line) - (size_t)k, " q:%d", f.base_q_idx);
  if (tags.grain) k += snprintf(line + k, sizeof(line) - (size_t)k, " grain:%d", f.grain);
  if (tags.ar) k += snprintf(line + k, sizeof(line) - (size_t)k, " ar:%d", f.ar);
  if (tags.lr) k += snprintf(line + k, sizeof(line) - (size_t)k, " lr:%d/%d", f.lr_filtered, f.lr_units);
  if (tags.cdef) k += snprintf(line + k, sizeof(line) - (size_t)k, " cdef:%d/%d", f.cdef_moved, f.cdef_sbs);
  if (tags.lf) k += snprintf(line + k, sizeof(line) - (size_t)k, " lf:%d/%d", f.lf_y, f.lf_uv);
  if (tags.ivtc) k += snprintf(line + k, sizeof(line) - (size_t)k, " ivtc:%ld/%ld", f.ivtc_top, f.ivtc_bottom);
  if (cut) k += snprintf(line + k, sizeof(line) - (size_t)k, " cut:1");
  return std::string(line, (size_t)k);
}

std::string StatsSummaryLine(const av1mi::quality::Summary &sum, long long bytes, int bit_depth) {
  char line[512];
  int k = snprintf(line, sizeof(line), "summary frames:%ld bytes:%lld", sum.frames, bytes);
  k += av1mi::quality::format_figures(sum.figures(bit_depth), line + k, sizeof(line) - (size_t)k);
  return std::string(line, (size_t)k);
}

namespace {

// reader threads at work on the session's pinned planes; join() = all of them delivered their frame (false: a truncated one)
struct Reads {
  std::vector<std::thread> th; std::vector<char> ok;
  bool join() { for (auto &x : th) if (x.joinable()) x.join(); th.clear(); for (char c : ok) if (!c) return false; return true; }
  ~Reads() { for (auto &x : th) if (x.joinable()) x.join(); }
};
typedef std::vector<std::vector<FrameOut>> GroupOut;      // [segment][t]: the coded frames of the group in flight

struct Run {
  BackendJob job;              // the caller's, until settle_denoise / settle_peak write what they planned into it
  std::string *err;
  av1mi_ctx *ctx = nullptr;
  Y4mSource y;
  av1mi_gop *gop = nullptr;
  StreamSink sink;
  CropRect window;             // settle_window: -av1mi_crop's, given or found (w == 0: none)
  int planned_denoise = -1;    // settle_denoise: what -av1mi_denoise auto planned (-1: the job did not ask)
  int planned_peak = -1;       // settle_peak: what -av1mi_tonemap_peak auto planned, cd/m2 (-1: the job did not ask)
  SessionPlan plan = {};       // session_config
  av1::SequenceParams sp;
  int S = 0, G = 0, threads = 1, lag = 0;
  std::vector<std::vector<unsigned char>> scratch;      // packed: per reader thread, one planar frame to pack from
  // A target (-b:v:0 / -av1mi_target_bpp): the controller lives across the groups.  It is asked at ONE point of the loop (before each
  // submit) and told at one (after each assemble), so the quantisers, and with them the output bytes, are a function of the input alone.
  std::unique_ptr<RateControl> rc;
  long long rc_bytes = 0, rc_frames = 0;
  long g0 = 0, total_frames = 0;      // the group in flight starts at GOP g0 of the input
  int cur_store = 0;
  long next_frames = -1, next_put = 0;      // stored: frames of the group that goes into the other store (-1 = not asked yet), and those already put
  av1mi_gop_frame oldest;      // the batch collected last, until it is assembled
  // -av1mi_ivtc: the plan of the group in the current store (output k of the group is woven from store positions ivtc_top[k] / ivtc_bottom[k]),
  // and the file-wide number of the source frame at store position 0
  std::vector<int32_t> ivtc_top, ivtc_bottom;
  long ivtc_base = 0;
  int put_offset = 0;          // the store position of frame 0 of the group put_chunk puts (-av1mi_ivtc: 1 behind a context frame)
  std::vector<unsigned char> kept[3];      // -av1mi_ivtc: the last source frame of the group in flight, the next group's context
  std::string stats;           // the stats file's lines, in presentation order
  av1mi::quality::Summary summary;
  long long total_bytes = 0;

  Run(const BackendJob &j, std::string *e) : job(j), err(e) {}
  ~Run() {
    if (!ctx) return;
    sink.abort();
    if (gop) av1mi_gop_close(gop);
    y.close();
    av1mi_close(ctx);
  }
  int fail(int code, const std::string &text) { *err = text; return code; }
  int lib_error(const char *call) { return fail(2, std::string(call) + ": " + av1mi_last_error(ctx)); }
  int truncated() { return fail(1, job.input + ": Invalid data found when processing input (truncated frame)"); }
  unsigned char *at(void *plane, int p, int i) const { return (unsigned char *)plane + plan.fed.plane[p].frame_bytes * (size_t)i; }      // frame i of a pinned plane

  // The crop window, settled before the session is opened: -av1mi_crop W:H:X:Y as given, or what auto finds in a sample of the file
  int settle_window() {
    if (job.crop_mode == 2) return ExplicitWindow(job, y.w, y.h, &window, err);
    if (job.crop_mode != 1) return 0;
    // cropping by a stream's first frames would crop by its opening credits, and what is cropped is gone
    if (!y.seekable()) return fail(1, "Invalid argument: -av1mi_crop auto needs a seekable file: it samples frames from all over the input, not from a pipe or FIFO");
    const long have = y.prepare(0, y.known_frames(), err);
    if (have < 0) return 1;
    const int n = (int)std::min<long>(kCropSampleFrames, have), W8 = (y.w + 7) & ~7, H8 = (y.h + 7) & ~7;
    const size_t plane = (size_t)W8 * H8 * (y.src_bd == 8 ? 1 : 2);
    std::vector<unsigned char> luma(plane * (size_t)std::max(n, 1)), cu(plane), cv(plane);      // (the chroma planes are read and dropped)
    for (int i = 0; i < n; i++)
      if (!y.read((long)i * have / n, W8, H8, luma.data() + plane * (size_t)i, cu.data(), cv.data())) return truncated();
    std::vector<av1mi_crop_record> rec((size_t)std::max(n, 1));
    if (n > 0) {
      void *d_luma = nullptr, *d_rec = nullptr;
      int rc = av1mi_malloc(ctx, &d_luma, luma.size());
      if (rc == AV1MI_OK) rc = av1mi_malloc(ctx, &d_rec, rec.size() * sizeof(av1mi_crop_record));
      if (rc == AV1MI_OK) rc = av1mi_upload(ctx, d_luma, luma.data(), luma.size());
      if (rc == AV1MI_OK) rc = av1mi_crop_analyse(ctx, y.src_bd, W8, H8, y.w, y.h, n, d_luma, job.crop_limit, (av1mi_crop_record *)d_rec);
      if (rc == AV1MI_OK) rc = av1mi_download(ctx, rec.data(), d_rec, rec.size() * sizeof(av1mi_crop_record));
      if (rc != AV1MI_OK) lib_error("av1mi_crop_analyse");
      if (d_luma) (void)av1mi_free(ctx, d_luma);
      if (d_rec) (void)av1mi_free(ctx, d_rec);
      if (rc != AV1MI_OK) return 2;
    }
    if (!PlanCrop(rec.data(), n, y.w, y.h, &window) || !window.trims(y.w, y.h)) window = CropRect();      // no bars: the path without a window, exactly
    return 0;
  }

  // The denoiser's strength, settled before the session is opened: -av1mi_denoise auto measures up to 16 pairs of consecutive frames
  // spread evenly over the file (noiseplan.hpp NoisePairSlot), luma as the file holds it, and plans.  From here on the job IS the job
  // -av1mi_denoise N; planned 0 = the job without the denoiser, and what only shapes the denoiser goes with it.  (Its own read of the
  // file: sharing the sample with -av1mi_crop auto is not built.)
  int settle_denoise() {
    if (!job.denoise_auto) return 0;
    if (!y.seekable()) return fail(1, "Invalid argument: -av1mi_denoise auto needs a seekable file: it samples frame pairs from all over the input, not from a pipe or FIFO");
    // validity does not depend on content: what the job would be refused for with a strength, it is refused for before anything is read
    SessionPlan dry;
    if (const int code = SessionConfig(job, facts(), window, &dry, err)) return code;
    const long have = y.prepare(0, y.known_frames(), err);
    if (have < 0) return 1;
    const int P = NoiseSamplePairs(have), W8 = (y.w + 7) & ~7, H8 = (y.h + 7) & ~7;
    int strength = 0;      // a file of fewer than 2 frames
    if (P > 0) {
      const size_t plane = (size_t)W8 * H8 * (y.src_bd == 8 ? 1 : 2);
      std::vector<unsigned char> luma(plane * 2 * (size_t)P), cu(plane), cv(plane);      // (the chroma planes are read and dropped)
      for (int i = 0; i < P; i++)
        for (int k = 0; k < 2; k++)
          if (!y.read(2 * NoisePairSlot(i, have) + k, W8, H8, luma.data() + plane * (size_t)(2 * i + k), cu.data(), cv.data())) return truncated();
      std::vector<av1mi_noise_record> rec((size_t)P);
      void *d_luma = nullptr, *d_rec = nullptr;
      int rc = av1mi_malloc(ctx, &d_luma, luma.size());
      if (rc == AV1MI_OK) rc = av1mi_malloc(ctx, &d_rec, rec.size() * sizeof(av1mi_noise_record));
      if (rc == AV1MI_OK) rc = av1mi_upload(ctx, d_luma, luma.data(), luma.size());
      if (rc == AV1MI_OK) rc = av1mi_noise_analyse(ctx, y.src_bd, W8, H8, y.w, y.h, P, d_luma, (av1mi_noise_record *)d_rec);
      if (rc == AV1MI_OK) rc = av1mi_download(ctx, rec.data(), d_rec, rec.size() * sizeof(av1mi_noise_record));
      if (rc != AV1MI_OK) lib_error("av1mi_noise_analyse");
      if (d_luma) (void)av1mi_free(ctx, d_luma);
      if (d_rec) (void)av1mi_free(ctx, d_rec);
      if (rc != AV1MI_OK) return 2;
      if ((strength = PlanDenoise(rec.data(), P, nullptr, nullptr)) < 0) return fail(2, "the denoise plan refused its arguments");
    }
    planned_denoise = job.denoise = strength;
    if (!strength) { job.denoise_range = 0; job.film_grain = -1; job.grain_lag = 0; }      // nothing is left for them to shape
    fprintf(stderr, "[av1mi] denoise: auto planned strength %d from %d pairs of frames\n", strength, P);
    return 0;
  }

  // The tone map's peak, settled before the session is opened: -av1mi_tonemap_peak auto measures up to 32 frames spread evenly over the
  // file (the crop sampler's slots and I/O budget), all three planes as the file holds them, and plans.  From here on the job IS the job
  // -av1mi_tonemap_peak N.  The whole frame is measured, in front of crop and scale: black bars only add to `pixels`, and a crop window
  // does not change the plan.  (Its own read of the file: together with -av1mi_crop auto the file is sampled twice; sharing is not built.)
  int settle_peak() {
    if (!job.tonemap_peak_auto) return 0;
    if (!y.seekable()) return fail(1, "Invalid argument: -av1mi_tonemap_peak auto needs a seekable file: it samples frames from all over the input, not from a pipe or FIFO");
    // validity does not depend on content: what the job would be refused for with a number, it is refused for before anything is read
    SessionPlan dry;
    if (const int code = SessionConfig(job, facts(), window, &dry, err)) return code;
    const long have = y.prepare(0, y.known_frames(), err);
    if (have < 0) return 1;
    const int n = PeakSampleFrames(have), W8 = (y.w + 7) & ~7, H8 = (y.h + 7) & ~7;
    if (n < 1) return fail(1, job.input + ": -av1mi_tonemap_peak auto found no frame to measure");
    const size_t luma = (size_t)W8 * H8 * 2, chroma = luma / 4;
    std::vector<unsigned char> py(luma * (size_t)n), pu(chroma * (size_t)n), pv(chroma * (size_t)n);
    for (int i = 0; i < n; i++)
      if (!y.read(PeakSampleSlot(i, have), W8, H8, py.data() + luma * (size_t)i, pu.data() + chroma * (size_t)i, pv.data() + chroma * (size_t)i)) return truncated();
    std::vector<av1mi_peak_record> rec((size_t)n);
    void *d[3] = { nullptr, nullptr, nullptr }, *d_rec = nullptr;
    int rc = av1mi_malloc(ctx, &d[0], py.size());
    if (rc == AV1MI_OK) rc = av1mi_malloc(ctx, &d[1], pu.size());
    if (rc == AV1MI_OK) rc = av1mi_malloc(ctx, &d[2], pv.size());
    if (rc == AV1MI_OK) rc = av1mi_malloc(ctx, &d_rec, rec.size() * sizeof(av1mi_peak_record));
    if (rc == AV1MI_OK) rc = av1mi_upload(ctx, d[0], py.data(), py.size());
    if (rc == AV1MI_OK) rc = av1mi_upload(ctx, d[1], pu.data(), pu.size());
    if (rc == AV1MI_OK) rc = av1mi_upload(ctx, d[2], pv.data(), pv.size());
    if (rc == AV1MI_OK) rc = av1mi_peak_analyse(ctx, W8, H8, y.w, y.h, n, d[0], d[1], d[2], (av1mi_peak_record *)d_rec);
    if (rc == AV1MI_OK) rc = av1mi_download(ctx, rec.data(), d_rec, rec.size() * sizeof(av1mi_peak_record));
    if (rc != AV1MI_OK) lib_error("av1mi_peak_analyse");
    for (void *p : d) if (p) (void)av1mi_free(ctx, p);
    if (d_rec) (void)av1mi_free(ctx, d_rec);
    if (rc != AV1MI_OK) return 2;
    av1mi_tone_tables tables;      // (lin[] does not depend on the peak)
    if (av1mi_tone_map_tables(1000, &tables) != AV1MI_OK) return fail(2, "av1mi_tone_map_tables refused its arguments");
    const int peak = PlanPeak(rec.data(), n, tables.lin, nullptr);
    if (peak < 0) return fail(2, "the peak plan refused its arguments");
    planned_peak = job.tonemap_peak = peak;
    fprintf(stderr, "[av1mi] tone map: auto planned a source peak of %d cd/m2 from %d frames\n", peak, n);
    return 0;
  }

  SourceFacts facts() const { return { y.w, y.h, y.bd, y.src_bd, y.chroma, y.sar_n, y.sar_d, y.fps_n, y.fps_d, y.interlace, y.colour_range, y.known_frames() }; }
  int session_config() {
    if (const int code = SessionConfig(job, facts(), window, &plan, err)) return code;
    S = plan.cfg.segments; G = plan.cfg.gop_length;
    threads = job.threads > 0 ? job.threads : (int)std::max(1u, std::thread::hardware_concurrency());
    scratch.resize(plan.packed ? (size_t)S : 0);
    return 0;
  }

  // the session, the sink (display size, side tracks) and the rate controller
  int open_session() {
    if (av1mi_gop_open(ctx, &plan.cfg, &gop) != AV1MI_OK) return lib_error("av1mi_gop_open");
    sp.width = plan.tw; sp.height = plan.th; sp.bit_depth = plan.coded_bd; sp.film_grain = plan.grainy; sp.colour = plan.colour;
    // pixels that stay non-square: the track at least says at which shape to show them
    if (!plan.square) sink.set_display_size((int)((long)plan.tw * y.sar_n / y.sar_d), plan.th);
    for (const std::string &side : job.tracks)
      if (!sink.add_side_file(side, err)) return 1;
    if (!sink.open(job.output, sp, plan.fps_n, plan.fps_d, err)) return 1;
    if (job.bitrate || job.target_bpp_u) {
      av1mi_rc_params rp;
      memset(&rp, 0, sizeof(rp));
      av1mi_rc_defaults(&rp);
      if (job.bitrate) { rp.target_num = job.bitrate * plan.fps_d; rp.target_den = 8ll * plan.fps_n; }      // bytes per OUTPUT frame
      else { rp.target_num = job.target_bpp_u * plan.tw * plan.th; rp.target_den = 8000000; }
      if (job.qmin) rp.qmin = job.qmin;
      if (job.qmax) rp.qmax = job.qmax;
      rp.gop_length = G; rp.bit_depth = plan.coded_bd;
      rp.start_q = std::min(std::max(plan.cfg.base_q_idx, rp.qmin), rp.qmax);
      if (const char *why = RateControl::ParamError(rp)) return fail(1, std::string("Invalid argument: rate control: ") + why);
      rc.reset(new RateControl(rp));
    }
    lag = av1mi_gop_max_in_flight() - 1;      // batches the GPU holds while the host works on the oldest
    return 0;
  }

  // THE reader of frames into the session's pinned planes: slot i of the next input buffers receives frame frame[i] of the group the
  // reader has prepared, read (and, where the job packs, packed) by a thread of its own; -1 = a flat slot.  Every call is followed by
  // exactly one submit or store_put.  0, or the exit code; reads->join() then tells whether every frame was whole.
  int start_reads(const std::vector<int32_t> &frame, Reads *reads) {
    void *py, *pu, *pv;
    if (av1mi_gop_acquire_input(gop, &py, &pu, &pv) != AV1MI_OK) return lib_error("av1mi_gop_acquire_input");
    const av1mi_source_layout &fed = plan.fed;
    reads->ok.assign(frame.size(), 1);
    for (int i = 0; i < (int)frame.size(); i++) {
      if (frame[(size_t)i] < 0) {
        // a shorter last GOP / fewer GOPs than segments: the slot is coded (the batch is one launch) and its output dropped.  Flat
        // planes, not whatever the pinned buffer held: stale pixels could cost the GPU coder's tile capacity for the whole batch
        // (zero samples pack to zero bytes)
        void *const plane[3] = { py, pu, pv };
        for (int p = 0; p < 3; p++) if (fed.plane[p].frame_bytes) memset(at(plane[p], p, i), 0, fed.plane[p].frame_bytes);
        continue;
      }
      reads->th.emplace_back([this, reads, &fed, i, f = (long)frame[(size_t)i], py, pu, pv]() {
        if (!plan.packed) { reads->ok[(size_t)i] = y.read(f, fed.width, fed.height, at(py, 0, i), at(pu, 1, i), at(pv, 2, i)); return; }
        // the frame (edge padding included) into this thread's scratch, then packed into the slot's byte range of the pinned planes
        std::vector<unsigned char> &b = scratch[(size_t)i];
        const size_t fy = (size_t)fed.width * fed.height * 2, fc = fy / 4;      // planar 10-bit planes
        b.resize(fy + 2 * fc);
        reads->ok[(size_t)i] = y.read(f, fed.width, fed.height, b.data(), b.data() + fy, b.data() + fy + fc) &&
                               av1mi_input_pack(AV1MI_INPUT_PACKED10, 10, fed.width, fed.height, b.data(), b.data() + fy, b.data() + fy + fc, at(py, 0, i), at(pu, 1, i), at(pv, 2, i)) == AV1MI_OK;
      });
    }
    return 0;
  }
  // The next chunk (up to S frames, IN FILE ORDER) of the `frames` frames the reader has prepared -> a store; *put counts the frames
  // put so far.  The chunk is read while `beside` (if any) runs; nothing left to put = `beside` alone.
  int put_chunk(int store, long frames, long *put, const std::function<int()> &beside = nullptr) {
    const int n = (int)std::min<long>(S, frames - *put);
    Reads reads;
    std::vector<int32_t> frame((size_t)std::max(n, 0));
    for (int i = 0; i < n; i++) frame[(size_t)i] = (int32_t)*put + i;
    int code = n > 0 ? start_reads(frame, &reads) : 0;
    if (code || (beside && (code = beside())) || n <= 0) return code;
    if (!reads.join()) return truncated();
    if (av1mi_gop_store_put(gop, store, put_offset + (int)*put, n) != AV1MI_OK) return lib_error("av1mi_gop_store_put");
    *put += n;
    return 0;
  }
  // -av1mi_ivtc's context frames, one frame each.  put_one: frame i of the group the reader has prepared -> position pos of a store.
  // keep_frame: frame i of the prepared group -> host memory (before the reader moves on to the next group); put_kept: that frame ->
  // position pos of a store.
  int put_one(int store, int pos, long i) {
    Reads reads;
    if (const int code = start_reads(std::vector<int32_t>(1, (int32_t)i), &reads)) return code;
    if (!reads.join()) return truncated();
    return av1mi_gop_store_put(gop, store, pos, 1) == AV1MI_OK ? 0 : lib_error("av1mi_gop_store_put");
  }
  int keep_frame(long i) {
    for (int p = 0; p < 3; p++) kept[p].resize(plan.fed.plane[p].frame_bytes);
    return y.read(i, plan.fed.width, plan.fed.height, kept[0].data(), kept[1].data(), kept[2].data()) ? 0 : truncated();
  }
  int put_kept(int store, int pos) {
    void *plane[3];
    if (av1mi_gop_acquire_input(gop, &plane[0], &plane[1], &plane[2]) != AV1MI_OK) return lib_error("av1mi_gop_acquire_input");
    for (int p = 0; p < 3; p++) if (!kept[p].empty()) memcpy(plane[p], kept[p].data(), kept[p].size());
    return av1mi_gop_store_put(gop, store, pos, 1) == AV1MI_OK ? 0 : lib_error("av1mi_gop_store_put");
  }
  int put_all(int store, long frames, long *put) {
    for (int code; *put < frames;) if ((code = put_chunk(store, frames, put))) return code;
    return 0;
  }

  // THE place a group is laid out: the nominal layout (GOP s = frames s G .. of the group), or with -av1mi_scenecut the planner's, its
  // boundaries moved onto the cuts the analysis of the store finds.  (A job that only deinterlaces or denoises keeps the nominal layout.)
  // frames: the group's OUTPUT frames.  At field rate the analysis still reads the source frames, and FieldRateCuts places their cuts.
  int lay_out(long frames, Group *g) {
    g->frames = frames; g->start.resize((size_t)S); g->len.resize((size_t)S);
    for (int s = 0; s < S; s++) { g->start[(size_t)s] = s * G; g->len[(size_t)s] = (int32_t)std::max<long>(0, std::min<long>(G, frames - (long)s * G)); }
    if (!plan.analysed) return 0;
    const long n = frames / plan.out_per_src;      // source frames
    std::vector<av1mi_scene_record> scene((size_t)n);
    g->cut.assign((size_t)frames, 0);
    if (av1mi_gop_store_analyse(gop, cur_store, (int)n, scene.data()) != AV1MI_OK) return lib_error("av1mi_gop_store_analyse");
    for (long f = 0; f < n; f++) g->cut[(size_t)f] = (uint8_t)av1mi_scene_is_cut(&scene[(size_t)f], job.scenecut);
    if (plan.out_per_src == 2) {
      const std::vector<uint8_t> source_cut(g->cut.begin(), g->cut.begin() + n);
      FieldRateCuts(source_cut.data(), n, g->cut.data());
    }
    if (av1mi_plan_gops((int)frames, G, S, job.min_gop, g->cut.data(), g->start.data(), g->len.data()) < 0) return fail(1, "Invalid argument: -av1mi_min_gop does not fit the GOP length");
    return 0;
  }

  // ask the rate controller, then submit batch t
  int submit(const Group &group, int t) {
    if (rc) {
      int frames = 0;
      for (int s = 0; s < S; s++) frames += group.exists(s, t) ? 1 : 0;
      rc_frames += frames;
      const int q = rc->NextQ(t == 0 ? 0 : 1, frames);
      if (q < 1) return fail(2, "rate control: no quantiser for the next batch");
      if (av1mi_gop_set_base_q_idx(gop, q) != AV1MI_OK) return lib_error("av1mi_gop_set_base_q_idx");
    }
    if (!plan.stored) return av1mi_gop_submit(gop, t == 0 ? 0 : 1) == AV1MI_OK ? 0 : lib_error("av1mi_gop_submit");
    if (plan.telecine) {      // the group's output frames -> the two store positions the plan weaves each from
      std::vector<int32_t> top = group.slots(t), bottom = top;
      for (size_t s = 0; s < top.size(); s++)
        if (top[s] >= 0) { bottom[s] = ivtc_bottom[(size_t)top[s]]; top[s] = ivtc_top[(size_t)top[s]]; }
      return av1mi_gop_submit_woven(gop, cur_store, top.data(), bottom.data(), t == 0 ? 0 : 1) == AV1MI_OK ? 0 : lib_error("av1mi_gop_submit_woven");
    }
    return av1mi_gop_submit_stored(gop, cur_store, group.slots(t).data(), t == 0 ? 0 : 1) == AV1MI_OK ? 0 : lib_error("av1mi_gop_submit_stored");
  }
  int collect() { return av1mi_gop_collect(gop, &oldest) == AV1MI_OK ? 0 : lib_error("av1mi_gop_collect"); }
  // the collected batch t -> one FrameOut per segment that exists (frame header + tile group, or the host coder); tells the controller
  int assemble(const Group &group, int t, GroupOut *out) {
    long long batch_bytes = 0;
    for (int s = 0; s < S; s++) {
      if (!group.exists(s, t)) continue;
      FrameOut f = {};
      av1mi_film_grain fg;
      if (job.denoise) {      // what the gather removed from this frame -> the parameters that put it back (none for the ends of a run)
        if (!oldest.grain) return fail(2, "the session returned no grain records");
        const int index = (int)(g0 * G + group.start[(size_t)s] + t);
        if (job.grain_lag > 0) {      // coloured grain: the covariance of the same residual shapes it
          if (!oldest.grain_cov) return fail(2, "the session returned no grain covariance");
          FilmGrainFromRecordsAr(oldest.grain + (size_t)s * 3, oldest.grain_cov + (size_t)s * 3, y.bd, index, job.grain_lag, &fg);
          f.ar = fg.apply_grain ? fg.ar_coeff_lag : 0;
        } else FilmGrainFromRecords(oldest.grain + (size_t)s * 3, y.bd, index, &fg);
        f.grain = FilmGrainMidGrey(fg);
      }
      if (!SessionTemporalUnit(oldest, s, plan.cfg.width, plan.cfg.height, plan.coded_bd, plan.cfg.visible_width, plan.cfg.visible_height, t == 0, threads, &f.unit, err, plan.grainy,
                               plan.grainy ? &fg : nullptr, sp.has_colour() ? &plan.colour : nullptr)) return 2;
      batch_bytes += (long long)f.unit.size();
      f.base_q_idx = oldest.params.base_q_idx;
      if (job.lr_search) {      // the units of the three planes that are filtered: a Wiener record chosen, in a plane whose restoration stayed ON
        if (!oldest.lr_choice) return fail(2, "the session returned no restoration choices");
        const int per[3] = { oldest.lr_units_per_frame[0], oldest.lr_units_per_frame[1], oldest.lr_units_per_frame[2] }, all = per[0] + per[1] + per[2];
        const uint8_t *choice = oldest.lr_choice + (size_t)s * all, *on = oldest.lr_on ? oldest.lr_on + (size_t)s * 3 : nullptr;
        for (int p = 0, u = 0; p < 3; p++)
          for (int i = 0; i < per[p]; i++, u++) f.lr_filtered += choice[u] != 0 && (!on || on[p]);
        f.lr_units = all;
      }
      if (job.cdef_search) {    // the superblocks that left the policy's strength set
        if (!oldest.cdef_idx) return fail(2, "the session returned no CDEF indices");
        f.cdef_sbs = ((plan.cfg.width + 63) / 64) * ((plan.cfg.height + 63) / 64);
        for (int i = 0; i < f.cdef_sbs; i++) f.cdef_moved += oldest.cdef_idx[(size_t)s * f.cdef_sbs + i] != 0;
      }
      if (job.lf_search) {      // the frame's chosen levels: luma vertical, chroma
        if (!oldest.lf_levels) return fail(2, "the session returned no deblocking levels");
        f.lf_y = oldest.lf_levels[(size_t)s * 4]; f.lf_uv = oldest.lf_levels[(size_t)s * 4 + 2];
      }
      if (plan.telecine) { const int32_t k = group.index(s, t); f.ivtc_top = ivtc_base + ivtc_top[(size_t)k]; f.ivtc_bottom = ivtc_base + ivtc_bottom[(size_t)k]; }
      if (plan.measure) {
        if (!oldest.quality) return fail(2, "the session returned no quality records");
        memcpy(f.q, oldest.quality + (size_t)s * 3, sizeof(f.q));
      }
      (*out)[(size_t)s].push_back(std::move(f));
    }
    if (rc) {      // the truth replaces the controller's prediction for this batch; segments that do not exist count nowhere
      rc_bytes += batch_bytes;
      if (rc->Collected(batch_bytes) != 0) return fail(2, "rate control: nothing in flight");
    }
    return 0;
  }

  // The batches of a group.  The frames of batch t + 1 (stored: the next chunk of the next group) are read WHILE the host assembles batch
  // t - lag: the session hands out the next input buffers as soon as the oldest batch has been collected.  The order inside a step is
  // what overlaps the reads with the assembly and keeps the quantisers a function of the input alone.
  int code_group(const Group &group, GroupOut *out) {
    const int T = group.T();
    const bool stored = plan.stored;
    Reads reads;
    int code = !stored && T > 0 ? start_reads(group.slots(0), &reads) : 0;
    for (int t = 0; t < T && !code; t++) {
      if (!stored && !reads.join()) return truncated();
      if ((code = submit(group, t))) return code;
      const bool have = t >= lag;
      if (have && (code = collect())) return code;            // the GPU works on the frames after it meanwhile
      if (!stored && t + 1 < T && (code = start_reads(group.slots(t + 1), &reads))) return code;
      auto assemble_oldest = [&] { return have ? assemble(group, t - lag, out) : 0; };
      code = stored ? put_chunk(cur_store ^ 1, next_frames, &next_put, assemble_oldest) : assemble_oldest();
    }
    for (int t = std::max(0, T - lag); t < T && !code; t++)
      if (!(code = collect())) code = assemble(group, t, out);
    if (code || !stored) return code;
    return put_all(cur_store ^ 1, next_frames, &next_put);      // (a group of short GOPs has fewer batches than the next group has chunks)
  }

  // the group's frames in presentation order: each unit to the sink, its line to the stats
  int write_group(const Group &group, const GroupOut &out) {
    StatsTags tags;
    tags.depth_from = plan.reduced_from; tags.depth_to = plan.coded_bd;
    tags.win = plan.win; tags.colour = sp.described() ? &plan.colour : nullptr; tags.q = rc != nullptr; tags.grain = job.denoise != 0; tags.ar = job.grain_lag > 0; tags.lr = job.lr_search != 0; tags.cdef = job.cdef_search != 0; tags.lf = job.lf_search != 0; tags.ivtc = plan.telecine; tags.denoise_auto = planned_denoise; tags.peak_auto = planned_peak;
    for (int s = 0; s < S; s++)
      for (size_t t = 0; t < out[(size_t)s].size(); t++) {
        const FrameOut &f = out[(size_t)s][t];
        if (!sink.write(f.unit, t == 0, err)) return 1;
        if (!plan.measure) continue;
        stats += StatsFrameLine(summary.frames, t == 0, f, plan.coded_bd, tags, plan.analysed && group.cut[(size_t)group.index(s, (int)t)]) + '\n';
        summary.add(f.q, plan.coded_bd);
        total_bytes += (long long)f.unit.size();
      }
    return 0;
  }

  // The loop over GROUPS of S GOPs: a file is read in place, a stream one group ahead of the encoder (y4m.hpp).  Stored: the group's
  // frames are in the current store before its batches run — the first group's are put here, nothing runs beside it; every later one was
  // put into the other store while the group before ran (code_group) — and the stores swap per group.
  // -av1mi_ivtc: a group of S G output frames is S G 5 / 4 source frames.  They go into the store between the last source frame of the group
  // before and the first of the group after (context: analysed and matched against, never output), the records are taken on the GPU, the
  // plan says which frame of every five is dropped and which two frames each kept one is woven from, and the batches are submitted as
  // woven pairs.  Every source frame is read ONCE, in order, so a pipe or FIFO feeds the job like a file: the group's last frame is kept on
  // the host for the next group, and the next group's first frame is read one ahead.  The next group is put beside this group's batches
  // like every stored job's (code_group).
  int run_groups_telecine() {
    const long per_group = (long)S * G * kTelecineCycle / (kTelecineCycle - 1);      // source frames
    int code;
    long have = y.prepare(0, per_group, err), put = 0;
    if (have < 0) return 1;
    if ((code = put_all(cur_store, have, &put))) return code;      // the first group: from position 0, nothing in front of it
    put_offset = 1;                                                  // every later group lies behind its context frame
    for (long k = 0, front = 0; have > 0; k++, g0 += S, front = 1) {
      // the group's last frame, kept for the next group before the reader moves on; then the next group is prepared (a stream: it has
      // been read ahead) and its first frame is this group's context behind
      if ((code = keep_frame(have - 1))) return code;
      if ((next_frames = y.prepare((k + 1) * per_group, per_group, err)) < 0) return 1;
      next_put = 0;
      const long back = next_frames > 0 ? 1 : 0, run = front + have + back;
      if (back && (code = put_one(cur_store, (int)(front + have), 0))) return code;
      std::vector<av1mi_telecine_record> rec((size_t)run);
      if (av1mi_gop_store_telecine(gop, cur_store, (int)run, rec.data()) != AV1MI_OK) return lib_error("av1mi_gop_store_telecine");
      ivtc_top.assign((size_t)have, 0); ivtc_bottom.assign((size_t)have, 0);
      const int outs = PlanTelecine(rec.data(), (int)run, (int)front, (int)back, ivtc_top.data(), ivtc_bottom.data());
      if (outs < 0) return fail(2, "the telecine plan refused its arguments");
      ivtc_base = k * per_group - front;
      total_frames += outs;
      Group group;
      if ((code = lay_out(outs, &group))) return code;
      // the next group into the other store: its context in front now, its own frames chunk by chunk beside this group's batches
      if (back && (code = put_kept(cur_store ^ 1, 0))) return code;
      GroupOut out((size_t)S);
      if ((code = code_group(group, &out)) || (code = write_group(group, out))) return code;
      cur_store ^= 1;
      have = next_frames;
    }
    return 0;
  }

  int run_groups() {
    if (plan.telecine) return run_groups_telecine();
    for (int code;; g0 += S) {
      long have = next_frames;
      const int F = plan.out_per_src;      // g0 and G count OUTPUT frames; the reader and the store count source frames (G is even where F is 2)
      if (!plan.stored || have < 0) {
        if ((have = y.prepare(g0 * G / F, (long)S * G / F, err)) < 0) return 1;
        long put = 0;
        if (plan.stored && (code = put_all(cur_store, have, &put))) return code;
      }
      if (have == 0) return 0;
      total_frames += have;
      Group group;
      if ((code = lay_out(have * F, &group))) return code;
      if (plan.stored) {
        // the group after this one: prepared now (this group's frames are all in the store), put chunk by chunk beside the batches
        if ((next_frames = y.prepare((g0 + S) * G / F, (long)S * G / F, err)) < 0) return 1;
        next_put = 0;
      }
      GroupOut out((size_t)S);
      if ((code = code_group(group, &out)) || (code = write_group(group, out))) return code;
      if (plan.stored) cur_store ^= 1;
    }
  }

  // the end of the job: the container, the rate-control report, the stats file and the quality gate
  int finish() {
    if (total_frames == 0) return fail(1, job.input + ": Invalid data found when processing input (no frames)");
    if (!sink.close(err)) return 1;
    if (rc && rc_frames > 0) {
      const av1mi_rc_params &rp = rc->params();
      const double fps = (double)plan.fps_n / plan.fps_d, px = (double)plan.tw * plan.th, want = 8.0 * rp.target_num / rp.target_den, got = 8.0 * rc_bytes / rc_frames;
      fprintf(stderr, "[av1mi] rate control: target %.0f bit/s (%.4f bit/pixel), achieved %.0f bit/s (%.4f bit/pixel) over %lld frames\n", want * fps, want / px,
              got * fps, got / px, rc_frames);
    }
    if (!plan.measure) return 0;
    if (!job.stats_path.empty()) {
      stats += StatsSummaryLine(summary, total_bytes, plan.coded_bd) + '\n';
      FILE *sf = fopen(job.stats_path.c_str(), "wb");
      const bool ok = sf && fwrite(stats.data(), 1, stats.size(), sf) == stats.size();
      if ((sf && fclose(sf)) || !ok) { remove(job.output.c_str()); return fail(1, job.stats_path + ": could not write the stats file"); }
    }
    const av1mi::quality::Figures f = summary.figures(plan.coded_bd);
    if (job.min_psnr > 0 && f.psnr[0] < job.min_psnr) {      // the quality gate: the file is not good enough to stand in for its source
      char why[160];
      snprintf(why, sizeof(why), "quality gate: psnr_y %.6f dB below the bound %.6f dB", f.psnr[0], job.min_psnr);
      remove(job.output.c_str());
      return fail(3, why);
    }
    return 0;
  }
};

}  // namespace

int RunBackend(const BackendJob &job, std::string *err, BackendReport *report) {
  Run r(job, err);
  struct Tell { Run &r; BackendReport *to; ~Tell() { if (to) to->denoise = r.planned_denoise; } } tell = { r, report };      // (whichever way the job ends)
  if (av1mi_device_count() <= 0 || av1mi_open(job.device, &r.ctx) != AV1MI_OK) {
    r.ctx = nullptr;
    *err = "Error: no usable HIP device for the av1mi backend (device " + std::to_string(job.device) + ")";
    return -1;
  }
  if (!r.y.open(job.input, err, job.to_420)) return 1;
  int code;
  if ((code = r.settle_window()) || (code = r.settle_denoise()) || (code = r.settle_peak()) || (code = r.session_config()) || (code = r.open_session()) || (code = r.run_groups())) return code;
  return r.finish();
}

}  // namespace av1mi_host
