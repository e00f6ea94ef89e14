// capi_host.cpp — extern "C" hooks over the host mirror so that the CPU test-suite (ctypes) can pin it against
// values read off the reference source.
#include <cstring>
#include "filmgrain.hpp"
#include "daemon.hpp"
#include "av1_bitstream.hpp"
#include "mux.hpp"
#include "y4m.hpp"
#include "backend.hpp"
#include "fieldrate.hpp"
#include "noiseplan.hpp"
#include "peakplan.hpp"
#include "../csrc/quality.hpp"

using namespace av1mi_host;

// the test hooks' list convention: strings joined with '\n' (an argv, a list of paths)
static std::vector<std::string> split_lines(const std::string &s) {
  std::vector<std::string> a;
  size_t p = 0, q;
  while ((q = s.find('\n', p)) != std::string::npos) { a.push_back(s.substr(p, q - p)); p = q + 1; }
  a.push_back(s.substr(p));
  return a;
}

extern "C" {
int av1mi_host_determine_quality(int height) { return DetermineQuality(height); }
int av1mi_host_check_size_gate(long long orig, long long neu, double ratio) { return CheckSizeGate(orig, neu, ratio) ? 1 : 0; }
// argv joined with '\n' into buf; returns the number of arguments, -1 on the reference's error (text in buf)
int av1mi_host_transcode_args(const char *in, const char *out, int has_video, int index, int height, int webrip, char *buf, int cap) {
  ProbeResult pr; pr.has_video_stream = has_video != 0; pr.VideoStream.Index = index; pr.VideoStream.Height = height;
  std::vector<std::string> a; std::string err;
  const bool ok = TranscodeArgs("ffmpeg", in, out, pr, webrip != 0, &a, &err);
  std::string j;
  if (ok) for (size_t i = 0; i < a.size(); i++) j += (i ? "\n" : "") + a[i]; else j = err;
  strncpy(buf, j.c_str(), cap - 1); buf[cap - 1] = 0;
  return ok ? (int)a.size() : -1;
}
// the argv ProcessJob runs: the reference's (TranscodeArgs) plus what a TranscodeConfig with TargetBitsPerPixel adds; same convention
int av1mi_host_job_args(const char *in, const char *out, int height, int webrip, double target_bpp, char *buf, int cap) {
  ProbeResult pr; pr.has_video_stream = true; pr.VideoStream.Height = height;
  std::vector<std::string> a; std::string err;
  if (!TranscodeArgs("ffmpeg", in, out, pr, webrip != 0, &a, &err)) return -1;
  TranscodeConfig cfg; cfg.TargetBitsPerPixel = target_bpp;
  AppendConfigArgs(cfg, &a);
  std::string j;
  for (size_t i = 0; i < a.size(); i++) j += (i ? "\n" : "") + a[i];
  strncpy(buf, j.c_str(), cap - 1); buf[cap - 1] = 0;
  return (int)a.size();
}
// ParseBackendJob's view of the rate options for an argv joined with '\n': 0 and out = { bits per second, millionths of a bit per pixel,
// qmin, qmax, quality }, or -1 with the text in err
int av1mi_host_parse_rate_options(const char *joined, long long *out, char *err, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  out[0] = job.bitrate; out[1] = job.target_bpp_u; out[2] = job.qmin; out[3] = job.qmax; out[4] = job.quality;
  return ok ? 0 : -1;
}
// Y4mSource (y4m.hpp) alone, for the CPU tests: reads the whole input in groups of `group` frames the way RunBackend does and
// returns the number of frames (-1 on error, text in err); *sum = a checksum over every frame's padded planes; *seekable = the mode
long long av1mi_host_y4m_scan(const char *path, int group, unsigned long long *sum, int *seekable, int *geometry, char *err, int cap) {
  Y4mSource y;
  std::string e;
  auto fail = [&]() { strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0; return -1LL; };
  if (!y.open(path, &e)) return fail();
  const int cw = (y.w + 7) & ~7, ch = (y.h + 7) & ~7;
  const size_t bps = y.bd == 8 ? 1 : 2;
  std::vector<unsigned char> Y((size_t)cw * ch * bps), U((size_t)cw * ch * bps / 4), V((size_t)cw * ch * bps / 4);
  unsigned long long acc = 1469598103934665603ull;
  long long total = 0;
  for (long first = 0;; first += group) {
    const long n = y.prepare(first, group, &e);
    if (n < 0) return fail();
    if (n == 0) break;
    for (long i = 0; i < n; i++) {
      if (!y.read(i, cw, ch, Y.data(), U.data(), V.data())) { e = "read failed"; return fail(); }
      for (const auto *pl : { &Y, &U, &V }) for (unsigned char b : *pl) acc = (acc ^ b) * 1099511628211ull;
    }
    total += n;
  }
  *sum = acc; *seekable = y.seekable() ? 1 : 0;
  geometry[0] = y.w; geometry[1] = y.h; geometry[2] = y.bd; geometry[3] = y.fps_n; geometry[4] = y.fps_d;
  return total;
}
// Y4mSource::open alone, with or without the job's opt-in to other layouts than 4:2:0 (any_layout): 0 and geometry = { w, h, coded bit
// depth, chroma layout (enum av1mi_source_chroma), source bit depth }, *frame_bytes = one frame's samples in the file, *frames = the
// frames a seekable file holds (-1 for a stream); -1 with the text in err when the source is refused
int av1mi_host_y4m_layout(const char *path, int any_layout, int *geometry, unsigned long long *frame_bytes, long long *frames, char *err, int cap) {
  Y4mSource y;
  std::string e;
  if (!y.open(path, &e, any_layout != 0)) { strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0; return -1; }
  geometry[0] = y.w; geometry[1] = y.h; geometry[2] = y.bd; geometry[3] = y.chroma; geometry[4] = y.src_bd;
  *frame_bytes = y.frame_bytes(); *frames = y.known_frames();
  return 0;
}
// ParseBackendJob's view of the conversion to 4:2:0 (BackendJob::to_420) for an argv joined with '\n': 1 / 0, or -1 with the text in err
int av1mi_host_parse_format_option(const char *joined, char *err, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  return ok ? (job.to_420 ? 1 : 0) : -1;
}
// the header's sample aspect ratio as Y4mSource keeps it; 0, or -1 when the file does not open
int av1mi_host_y4m_sar(const char *path, int *sar) {
  Y4mSource y;
  std::string e;
  if (!y.open(path, &e)) return -1;
  sar[0] = y.sar_n; sar[1] = y.sar_d;
  return 0;
}
// the header's I parameter as Y4mSource keeps it (0 progressive, 1 It, 2 Ib, 3 Im); -1 when the file does not open
int av1mi_host_y4m_interlace(const char *path) {
  Y4mSource y;
  std::string e;
  if (!y.open(path, &e)) return -1;
  return y.interlace;
}
// ParseBackendJob's view of -av1mi_deinterlace and the chain's deinterlacers for an argv joined with '\n': BackendJob::deinterlace (0 off,
// 1 auto, 2 tff, 3 bff), or -1 with the text in err
int av1mi_host_parse_deinterlace_option(const char *joined, char *err, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  return ok ? job.deinterlace : -1;
}
// ParseBackendJob's view of -av1mi_deinterlace_rate for an argv joined with '\n': BackendJob::deint_rate (0 frame, 1 field), or -1 with the
// text in err
int av1mi_host_parse_deinterlace_rate(const char *joined, char *err, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  return ok ? job.deint_rate : -1;
}
// JobOutputOf (fieldrate.hpp) for an argv joined with '\n' on a source with the header's I parameter `interlace` (0 progressive, 1 It, 2 Ib,
// 3 Im), fps_n / fps_d and `frames` frames (-1 = a stream): 0 and out = { output frames per source frame, fps_n, fps_d, frames }, or -1
// with the text in err
int av1mi_host_job_output(const char *joined, int interlace, int fps_n, int fps_d, long long frames, long long *out, char *err, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  if (!ok) return -1;
  const JobOutput o = JobOutputOf(job, interlace, fps_n, fps_d, (long)frames);
  out[0] = o.per_source; out[1] = o.fps_n; out[2] = o.fps_d; out[3] = o.frames;
  return 0;
}
// the same with the ratio: out = { output frames per source frame, fps_n, fps_d, frames, num, den } (num output frames per den source frames)
int av1mi_host_job_output_ratio(const char *joined, int interlace, int fps_n, int fps_d, long long frames, long long *out, char *err, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  if (!ok) return -1;
  const JobOutput o = JobOutputOf(job, interlace, fps_n, fps_d, (long)frames);
  out[0] = o.per_source; out[1] = o.fps_n; out[2] = o.fps_d; out[3] = o.frames; out[4] = o.num; out[5] = o.den;
  return 0;
}
// ParseBackendJob's view of -av1mi_ivtc for an argv joined with '\n': BackendJob::ivtc (0, 1), or -1 with the text in err
int av1mi_host_parse_ivtc_option(const char *joined, char *err, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  return ok ? job.ivtc : -1;
}
// PlanTelecine (telecineplan.hpp): the woven outputs of a run of `frames` records with `front` / `back` context frames; the number of
// outputs, or -1
int av1mi_plan_telecine(const av1mi_telecine_record *rec, int frames, int front, int back, int32_t *top, int32_t *bottom) {
  return PlanTelecine(rec, frames, front, back, top, bottom);
}
// PlanDenoise (noiseplan.hpp): the strength 0 .. 16 that `pairs` noise records plan, or -1; pair_q (may be null): every pair's level or -1
// for a pair that is not valid; s16 (may be null): the file's sigma in 1/16 of an 8-bit code, -1 without a valid pair
int av1mi_plan_denoise(const av1mi_noise_record *rec, int pairs, int32_t *pair_q, int32_t *s16) { return PlanDenoise(rec, pairs, pair_q, s16); }
// the pair slots -av1mi_denoise auto samples in a file of n frames (noiseplan.hpp NoisePairSlot): their number, slots[i] = the slot of pair i
// (frames 2 slot, 2 slot + 1); slots holds 16 entries
int av1mi_host_noise_pair_slots(long long n, int32_t *slots) {
  const int P = NoiseSamplePairs((long)n);
  for (int i = 0; i < P; i++) slots[i] = (int32_t)NoisePairSlot(i, (long)n);
  return P;
}
// PlanPeak (peakplan.hpp) with lin[] of av1mi_tone_map_tables: the source peak in cd/m2 (400 .. 10000) that `frames` peak records plan,
// or -1; frame_code (may be null): every frame's code
int av1mi_plan_peak(const av1mi_peak_record *rec, int frames, int32_t *frame_code) {
  av1mi_tone_tables t;      // (lin[] does not depend on the peak)
  if (av1mi_tone_map_tables(1000, &t) != AV1MI_OK) return -1;
  return PlanPeak(rec, frames, t.lin, frame_code);
}
// the frames -av1mi_tonemap_peak auto samples in a file of n frames (peakplan.hpp PeakSampleSlot): their number; slots holds 32 entries
int av1mi_host_peak_sample_slots(long long n, int32_t *slots) {
  const int P = PeakSampleFrames((long)n);
  for (int i = 0; i < P; i++) slots[i] = (int32_t)PeakSampleSlot(i, (long)n);
  return P;
}
// ParseBackendJob's view of the tone map's options for an argv joined with '\n': 0 and out = { tonemap, tonemap_peak, tonemap_peak_auto },
// or -1 with the text in err
int av1mi_host_parse_peak_options(const char *joined, int *out, char *err, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  out[0] = job.tonemap; out[1] = job.tonemap_peak; out[2] = job.tonemap_peak_auto ? 1 : 0;
  return ok ? 0 : -1;
}
// ParseBackendJob's view of the denoiser's options for an argv joined with '\n': 0 and out = { denoise, denoise_auto, denoise_range,
// film_grain, grain_lag }, or -1 with the text in err
int av1mi_host_parse_denoise_options(const char *joined, int *out, char *err, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  out[0] = job.denoise; out[1] = job.denoise_auto ? 1 : 0; out[2] = job.denoise_range; out[3] = job.film_grain; out[4] = job.grain_lag;
  return ok ? 0 : -1;
}
// the argv ProcessJob runs for a TranscodeConfig whose Denoise is `denoise` ("" = not given); av1mi_host_job_args's convention
int av1mi_host_job_args_denoise(const char *in, const char *out, int height, const char *denoise, char *buf, int cap) {
  ProbeResult pr; pr.has_video_stream = true; pr.VideoStream.Height = height;
  std::vector<std::string> a; std::string err;
  if (!TranscodeArgs("ffmpeg", in, out, pr, false, &a, &err)) return -1;
  TranscodeConfig cfg; cfg.Denoise = denoise ? denoise : "";
  AppendConfigArgs(cfg, &a);
  std::string j;
  for (size_t i = 0; i < a.size(); i++) j += (i ? "\n" : "") + a[i];
  strncpy(buf, j.c_str(), cap - 1); buf[cap - 1] = 0;
  return (int)a.size();
}
// FieldRateCuts (fieldrate.hpp): n source frames' cut flags -> 2 n output frames'
void av1mi_host_field_rate_cuts(const uint8_t *cut, int n, uint8_t *out) { FieldRateCuts(cut, n, out); }
// ScaleTarget (transcode.hpp): the size a filter chain yields on a source; 0, or -1 for a chain with an unsupported filter
int av1mi_host_scale_target(int iw, int ih, int sar_n, int sar_d, const char *chain, int *w, int *h) {
  std::string e;
  bool square = false;
  return ScaleTarget(iw, ih, sar_n, sar_d, chain ? chain : "", w, h, &square, &e) ? 0 : -1;
}
// the chain with crop= accepted (ChainTarget): the size the chain yields in *w, *h and the window in win[4] = x, y, width, height (width 0: the
// chain does not crop); -1 and the text in err (may be null) for a chain that is refused
int av1mi_host_chain_target(int iw, int ih, int sar_n, int sar_d, const char *chain, int *w, int *h, int *win, char *err, int errcap) {
  std::string e;
  bool square = false;
  CropRect c;
  const bool ok = ChainTarget(iw, ih, sar_n, sar_d, chain ? chain : "", w, h, &square, &e, nullptr, nullptr, &c);
  if (win) { win[0] = c.x; win[1] = c.y; win[2] = c.w; win[3] = c.h; }
  if (err && errcap > 0) { strncpy(err, e.c_str(), (size_t)errcap - 1); err[errcap - 1] = 0; }
  return ok ? 0 : -1;
}
// the crop plan (cropplan.hpp PlanCrop): n records of frames of true size w x h -> win[4] = x, y, width, height; 1 = a window, 0 = none (win zeroed)
int av1mi_host_crop_plan(const av1mi_crop_record *rec, int n, int w, int h, int *win) {
  CropRect c;
  const bool ok = PlanCrop(rec, n, w, h, &c);
  if (win) { win[0] = c.x; win[1] = c.y; win[2] = c.w; win[3] = c.h; }
  return ok ? 1 : 0;
}
// StreamSink (mux.hpp) alone, for the CPU tests: n_units byte strings (unit i = bytes [off[i], off[i + 1]) of `units`, standing in for
// temporal units; unit i is a key frame when i % gop == 0) muxed at fps_n / fps_d together with the tracks of the Matroska side files
// `sides` (paths separated by '\n').  Returns 0, or -1 with the text in err.
int av1mi_host_mux_selftest(const char *out_path, int width, int height, int bit_depth, int fps_n, int fps_d, const unsigned char *units,
                            const long long *off, int n_units, int gop, const char *sides, char *err, int cap) {
  std::string e;
  auto fail = [&]() { strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0; return -1; };
  StreamSink sink;
  for (std::string rest = sides ? sides : ""; !rest.empty();) {
    const size_t nl = rest.find('\n');
    const std::string one = rest.substr(0, nl);
    rest = nl == std::string::npos ? "" : rest.substr(nl + 1);
    if (!one.empty() && !sink.add_side_file(one, &e)) return fail();
  }
  av1::SequenceParams sp;
  sp.width = width; sp.height = height; sp.bit_depth = bit_depth;
  if (!sink.open(out_path, sp, fps_n, fps_d, &e)) return fail();
  for (int i = 0; i < n_units; i++) {
    const std::vector<uint8_t> tu(units + off[i], units + off[i + 1]);
    if (!sink.write(tu, i % gop == 0, &e)) { sink.abort(); return fail(); }
  }
  if (!sink.close(&e)) return fail();
  return 0;
}
// StreamSink with a colour record, for the CPU tests: av1mi_host_mux_units with the sequence's colour (null = none)
int av1mi_host_mux_units_colour(const char *path, int w, int h, int bd, int fps_n, int fps_d, const uint8_t *data, const long long *sizes, const uint8_t *keys, int n,
                                const av1mi_colour *colour) {
  StreamSink sink; std::string err;
  av1::SequenceParams sp; sp.width = w; sp.height = h; sp.bit_depth = bd;
  if (colour) sp.colour = *colour;
  if (!sink.open(path, sp, fps_n, fps_d, &err)) return 1;
  for (int i = 0; i < n; i++) {
    std::vector<uint8_t> tu(data, data + sizes[i]);
    data += sizes[i];
    if (!sink.write(tu, keys[i] != 0, &err)) { sink.abort(); return 2; }
  }
  return sink.close(&err) ? 0 : 3;
}
// ParseBackendJob's view of the colour and tone mapping options for an argv joined with '\n': 0, *out = the record JobColour gives with the Y4M range
// y4m_range, tone[2] = { tonemap, tonemap_peak }; or -1 with the text in err
int av1mi_host_parse_colour_options(const char *joined, int y4m_range, av1mi_colour *out, int *tone, char *err, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  if (!ok) return -1;
  *out = JobColour(job, y4m_range);
  tone[0] = job.tonemap; tone[1] = job.tonemap_peak;
  return 0;
}
// the header's XCOLORRANGE as Y4mSource keeps it (-1 absent, 0 LIMITED, 1 FULL); -2 when the file does not open
int av1mi_host_y4m_colour_range(const char *path) {
  Y4mSource y;
  std::string e;
  if (!y.open(path, &e)) return -2;
  return y.colour_range;
}
// The drop-in for internal/ffmpeg/transcode.go:194 `RunTranscode(ffmpegPath string, args []string) (int, error)`: what the cgo
// shim of INTEGRATION.md binds.  Returns the exit code of the contract (0 = output written, -1 = could not run, else failed);
// the error text (<= 800 chars + "...", transcode.go:295-297) goes to err.  Declared in include/av1mi_host.h.
int av1mi_run_transcode(int argc, const char *const *argv, char *err, size_t errcap) {
  std::vector<std::string> a;
  for (int i = 0; i < argc; i++) a.push_back(argv[i] ? argv[i] : "");
  const RunResult rr = RunTranscode("av1mi", a);
  if (err && errcap) { strncpy(err, rr.err.c_str(), errcap - 1); err[errcap - 1] = 0; }
  return rr.exitCode;
}
// runs the replacement RunTranscode on an argv joined with '\n'; error text into buf; returns the exit code
int av1mi_host_run_transcode(const char *joined, char *buf, int cap) {
  const std::vector<std::string> a = split_lines(joined);
  const RunResult rr = RunTranscode("av1mi", a);
  strncpy(buf, rr.err.c_str(), cap - 1); buf[cap - 1] = 0;
  return rr.exitCode;
}
// av1mi_host_run_transcode with the job's report: *denoise = the strength -av1mi_denoise auto planned, -1 = the job did not ask
int av1mi_host_run_transcode_report(const char *joined, char *buf, int cap, int *denoise) {
  const RunResult rr = RunTranscode("av1mi", split_lines(joined));
  strncpy(buf, rr.err.c_str(), cap - 1); buf[cap - 1] = 0;
  *denoise = rr.denoise;
  return rr.exitCode;
}
// ProcessJob on a source file; returns 0 when the reference would return nil; status and reason into the buffers
int av1mi_host_process_job(const char *source, long long orig_size, double ratio, const char *state_dir, int wait_s, int replace_source,
                           char *status, char *reason, int cap) {
  Job job; job.ID = "test"; job.SourcePath = source; job.OriginalSize = orig_size;
  TranscodeConfig cfg; cfg.MaxSizeRatio = ratio; cfg.JobStateDir = state_dir ? state_dir : ""; cfg.StableWaitSeconds = wait_s;
  cfg.ReplaceSource = replace_source != 0;
  ProbeResult pr; pr.HasVideo = true; pr.has_video_stream = true; pr.VideoStream.Height = 720;
  const std::string e = ProcessJob(&job, "av1mi", pr, cfg);
  strncpy(status, job.Status.c_str(), cap - 1); status[cap - 1] = 0;
  strncpy(reason, job.Reason.c_str(), cap - 1); reason[cap - 1] = 0;
  return e.empty() ? 0 : 1;
}
// ProcessJob with the quality gate: the argument list above plus TranscodeConfig::MinPSNR (dB, 0 = off)
int av1mi_host_process_job_q(const char *source, long long orig_size, double ratio, const char *state_dir, int wait_s, int replace_source,
                             char *status, char *reason, int cap, double min_psnr) {
  Job job; job.ID = "test"; job.SourcePath = source; job.OriginalSize = orig_size;
  TranscodeConfig cfg; cfg.MaxSizeRatio = ratio; cfg.JobStateDir = state_dir ? state_dir : ""; cfg.StableWaitSeconds = wait_s;
  cfg.ReplaceSource = replace_source != 0; cfg.MinPSNR = min_psnr;
  ProbeResult pr; pr.HasVideo = true; pr.has_video_stream = true; pr.VideoStream.Height = 720;
  const std::string e = ProcessJob(&job, "av1mi", pr, cfg);
  strncpy(status, job.Status.c_str(), cap - 1); status[cap - 1] = 0;
  strncpy(reason, job.Reason.c_str(), cap - 1); reason[cap - 1] = 0;
  return e.empty() ? 0 : 1;
}
// the quality records on the host (csrc/quality.hpp): the CPU twin of av1mi_quality_planes and the derived figures
int av1mi_quality_planes_host(int bit_depth, int width, int height, int frames, const void *const src[3], const void *const dec0[3], const void *const dec1[3],
                              const uint8_t *select, av1mi_quality *out) {
  return av1mi::quality::planes_host(bit_depth, width, height, frames, src, dec0, dec1, select, out);
}
double av1mi_quality_psnr(const av1mi_quality *q, int bit_depth) { return av1mi::quality::psnr_from_sse((double)q->sse, (double)q->samples, bit_depth); }
double av1mi_quality_ssim(const av1mi_quality *q) { return q->ssim_sum / (double)q->windows; }
// test hooks: the constants, ParseBackendJob's view of the two options, and the stats file's summary line from n frames' records
// (q: n * 3 records; bytes: n temporal unit sizes); returns the line's length
void av1mi_host_quality_constants(int bit_depth, long long *c1, long long *c2) { *c1 = av1mi::quality::ssim_c1(bit_depth); *c2 = av1mi::quality::ssim_c2(bit_depth); }
int av1mi_host_parse_quality_options(const char *joined, char *stats_path, int cap, double *min_psnr, char *err, int errcap) {
  const std::vector<std::string> a = split_lines(joined);
  BackendJob job; std::string e;
  const bool ok = ParseBackendJob(a, &job, &e);
  strncpy(stats_path, job.stats_path.c_str(), cap - 1); stats_path[cap - 1] = 0;
  strncpy(err, e.c_str(), errcap - 1); err[errcap - 1] = 0;
  *min_psnr = job.min_psnr;
  return ok ? 0 : -1;
}
int av1mi_host_quality_summary_line(const av1mi_quality *q, const long long *bytes, int n, int bit_depth, char *buf, int cap) {
  av1mi::quality::Summary sum;
  long long total = 0;
  for (int i = 0; i < n; i++) { sum.add(q + 3 * i, bit_depth); total += bytes[i]; }
  const std::string line = StatsSummaryLine(sum, total, bit_depth);
  if ((long long)line.size() >= cap) return -1;
  memcpy(buf, line.c_str(), line.size() + 1);
  return (int)line.size();
}
// SessionConfig (backend.hpp) for an argv joined with '\n' whose -i names a Y4M file (only its header is read): what RunBackend opens the
// session with, found without a device.  auto_win (may be null) = x, y, width, height standing for what -av1mi_crop auto found; without it
// the window is -av1mi_crop W:H:X:Y's, or none.  0 and *cfg, target[3] = the target's width, height and whether its pixels are square,
// switches[5] = packed, stored, analysed, grainy, measure; or the exit code 1 with the text in err
int av1mi_host_session_config(const char *joined, const int *auto_win, av1mi_gop_config *cfg, int *target, int *switches, char *err, int cap) {
  BackendJob job; std::string e;
  Y4mSource y;
  CropRect win;
  SessionPlan plan;
  int code = ParseBackendJob(split_lines(joined), &job, &e) && y.open(job.input, &e, job.to_420) ? 0 : 1;
  if (!code && auto_win) { win.x = auto_win[0]; win.y = auto_win[1]; win.w = auto_win[2]; win.h = auto_win[3]; }
  else if (!code && job.crop_mode == 2) code = ExplicitWindow(job, y.w, y.h, &win, &e);
  if (!code) code = SessionConfig(job, { y.w, y.h, y.bd, y.src_bd, y.chroma, y.sar_n, y.sar_d, y.fps_n, y.fps_d, y.interlace, y.colour_range, y.known_frames() }, win, &plan, &e);
  strncpy(err, e.c_str(), cap - 1); err[cap - 1] = 0;
  if (code) return code;
  *cfg = plan.cfg;
  target[0] = plan.tw; target[1] = plan.th; target[2] = plan.square;
  const bool sw[5] = { plan.packed, plan.stored, plan.analysed, plan.grainy, plan.measure };
  for (int i = 0; i < 5; i++) switches[i] = sw[i];
  return 0;
}
// AV1 bitstream writer (av1_bitstream.hpp): one temporal unit (delimiter [+ sequence header] + frame) for a frame description.
// Returns the size in bytes (copied into out when it fits in cap), -1 on a description the writer cannot code (text in err).
long long av1mi_obu_write_temporal_unit(const av1mi_obu_frame *f, int with_sequence_header, int threads, uint8_t *out, long long cap,
                                        char *err, int errcap) {
  std::vector<uint8_t> b; std::string e;
  if (!av1::temporal_unit(*f, with_sequence_header != 0, threads, &b, &e)) {
    if (err && errcap > 0) { strncpy(err, e.c_str(), errcap - 1); err[errcap - 1] = 0; }
    return -1;
  }
  if ((long long)b.size() <= cap && out) memcpy(out, b.data(), b.size());
  return (long long)b.size();
}
// One segment of a collected session batch -> its temporal unit (include/av1mi_host.h; session_unit.cpp SessionTemporalUnit)
long long av1mi_session_temporal_unit(const av1mi_gop_frame *fr, int seg, int width, int height, int bit_depth, int visible_width, int visible_height,
                                      int with_sequence_header, int threads, uint8_t *out, long long cap, char *err, int errcap) {
  std::vector<uint8_t> b; std::string e;
  if (!fr || seg < 0 || seg >= fr->segments) e = "bad batch / segment";
  else if (SessionTemporalUnit(*fr, seg, width, height, bit_depth, visible_width, visible_height, with_sequence_header != 0, threads, &b, &e)) {
    if ((long long)b.size() <= cap && out) memcpy(out, b.data(), b.size());
    return (long long)b.size();
  }
  if (err && errcap > 0) { strncpy(err, e.c_str(), errcap - 1); err[errcap - 1] = 0; }
  return -1;
}
long long av1mi_session_temporal_unit_grain(const av1mi_gop_frame *fr, int seg, int width, int height, int bit_depth, int visible_width, int visible_height,
                                            int with_sequence_header, int threads, int film_grain_present, const av1mi_film_grain *film_grain, uint8_t *out,
                                            long long cap, char *err, int errcap) {
  std::vector<uint8_t> b; std::string e;
  if (!fr || seg < 0 || seg >= fr->segments) e = "bad batch / segment";
  else if (SessionTemporalUnit(*fr, seg, width, height, bit_depth, visible_width, visible_height, with_sequence_header != 0, threads, &b, &e, film_grain_present != 0,
                               film_grain)) {
    if ((long long)b.size() <= cap && out) memcpy(out, b.data(), b.size());
    return (long long)b.size();
  }
  if (err && errcap > 0) { strncpy(err, e.c_str(), errcap - 1); err[errcap - 1] = 0; }
  return -1;
}
int av1mi_film_grain_from_records(const av1mi_grain_record *records, int bit_depth, int frame_index, av1mi_film_grain *out) {
  return FilmGrainFromRecords(records, bit_depth, frame_index, out) ? 0 : -1;
}
int av1mi_film_grain_from_records_ar(const av1mi_grain_record *records, const av1mi_grain_cov_record *cov, int bit_depth, int frame_index, int lag, av1mi_film_grain *out) {
  return FilmGrainFromRecordsAr(records, cov, bit_depth, frame_index, lag, out) ? 0 : -1;
}
int av1mi_film_grain_mid_grey(const av1mi_film_grain *g) { return g ? FilmGrainMidGrey(*g) : 0; }
// The general block description (av1_blockstream.cpp): any block / transform size, any partition
long long av1mi_obu_write_blocks_temporal_unit(const av1mi_obu_blocks *f, int with_sequence_header, uint8_t *out, long long cap, char *err, int errcap) {
  std::vector<uint8_t> b; std::string e;
  if (!f || !av1::blocks_temporal_unit(*f, with_sequence_header != 0, &b, &e)) {
    if (err && errcap > 0) { strncpy(err, f ? e.c_str() : "null description", errcap - 1); err[errcap - 1] = 0; }
    return -1;
  }
  if ((long long)b.size() <= cap && out) memcpy(out, b.data(), b.size());
  return (long long)b.size();
}
// One temporal unit from tile payloads coded by the GPU tile entropy coder (include/av1mi.h av1mi_av1_entropy_encode / the GOP
// session with gpu_entropy): `f` needs only its header fields (geometry, quantiser, filter parameters); payloads = the frame's
// ntiles finished tile payloads back to back in raster order, sizes[t] bytes each.  Same return convention as
// av1mi_obu_write_temporal_unit.  Declared in include/av1mi_host.h.
long long av1mi_obu_assemble_temporal_unit(const av1mi_obu_frame *f, const uint8_t *payloads, const uint32_t *sizes, int ntiles,
                                           int with_sequence_header, uint8_t *out, long long cap, char *err, int errcap) {
  std::vector<uint8_t> fr; std::string e;
  if (!av1::frame_obu_from_tiles(*f, payloads, sizes, ntiles, &fr, &e)) {
    if (err && errcap > 0) { strncpy(err, e.c_str(), errcap - 1); err[errcap - 1] = 0; }
    return -1;
  }
  std::vector<uint8_t> b = av1::temporal_delimiter_obu();
  if (with_sequence_header) av1::append_sequence_obus(av1::sequence_params(*f), &b);
  b.insert(b.end(), fr.begin(), fr.end());
  if ((long long)b.size() <= cap && out) memcpy(out, b.data(), b.size());
  return (long long)b.size();
}
// the op-stream path on the host (av1_opstream.cpp): same contract as av1mi_obu_write_temporal_unit; -2 = outside its tool set
// key_rows32 > 0: a key frame whose first key_rows32 luma rows are coded in 32x32 blocks (symbol arrays in the session's layout, see
// av1_opstream.cpp opstream_tiles)
long long av1mi_host_opstream_key32_temporal_unit(const av1mi_obu_frame *f, int key_rows32, int with_sequence_header, uint8_t *out, long long cap, char *err,
                                                  int errcap) {
  std::vector<std::vector<uint8_t>> tiles; std::string e;
  auto fail = [&](long long code) { if (err && errcap > 0) { strncpy(err, e.c_str(), errcap - 1); err[errcap - 1] = 0; } return code; };
  if (!av1::opstream_supported(*f, &e)) return fail(-2);
  if (!av1::opstream_tiles(*f, &tiles, &e, key_rows32)) return fail(-1);
  std::vector<uint8_t> cat; std::vector<uint32_t> sizes;
  for (auto &t : tiles) { sizes.push_back((uint32_t)t.size()); cat.insert(cat.end(), t.begin(), t.end()); }
  std::vector<uint8_t> fr;
  if (!av1::frame_obu_from_tiles(*f, cat.data(), sizes.data(), (int)sizes.size(), &fr, &e)) return fail(-1);
  std::vector<uint8_t> b = av1::temporal_delimiter_obu();
  if (with_sequence_header) av1::append_sequence_obus(av1::sequence_params(*f), &b);
  b.insert(b.end(), fr.begin(), fr.end());
  if ((long long)b.size() <= cap && out) memcpy(out, b.data(), b.size());
  return (long long)b.size();
}
int av1mi_host_opstream_slots(void) { return av1::opstream_slots(); }
// one tile (superblock sbr, sbc) of a key frame's 32x32 band through the tile tokenizer of csrc/av1_ops32.hpp, into the caller's list
// (ops_cap words), grouped entries (ops_cap + 4 * slots words) and per-slot totals / bases (av1mi_host_opstream_slots() entries each): the list words, -1 = the tile does not fit, -2 = outside the tool set
int av1mi_host_opstream_tile32(const av1mi_obu_frame *f, int sbr, int sbc, uint32_t ops_cap, uint32_t *list, uint32_t *grouped, uint16_t *slot_total,
                               uint16_t *slot_base) {
  if (!f || !list || !grouped || !slot_total || !slot_base) return -2;
  std::string e;
  return av1::opstream_tile32(*f, sbr, sbc, ops_cap, list, grouped, slot_total, slot_base, &e);
}
// the same for one tile of 8x8 blocks of a key or an inter frame (csrc/av1_ops8.hpp); -1 = the tile is refused (more than ops_cap words, or one
// of the tokenizer's own capacities): every slot total is 0, nothing else is written
int av1mi_host_opstream_tile8(const av1mi_obu_frame *f, int sbr, int sbc, uint32_t ops_cap, uint32_t *list, uint32_t *grouped, uint16_t *slot_total,
                              uint16_t *slot_base) {
  if (!f || !list || !grouped || !slot_total || !slot_base) return -2;
  std::string e;
  return av1::opstream_tile8(*f, sbr, sbc, ops_cap, list, grouped, slot_total, slot_base, &e);
}
long long av1mi_host_opstream_temporal_unit(const av1mi_obu_frame *f, int with_sequence_header, uint8_t *out, long long cap, char *err, int errcap) {
  return av1mi_host_opstream_key32_temporal_unit(f, 0, with_sequence_header, out, cap, err, errcap);
}
// job record + GPU probe hooks for the CPU tests
int av1mi_host_job_json(const char *id, const char *source, const char *status, const char *reason, long long orig, long long neu, char *buf, int cap) {
  Job j; j.ID = id; j.SourcePath = source; j.Status = status; j.Reason = reason; j.OriginalSize = orig; j.NewSize = neu; j.CreatedAt = "2026-01-02T03:04:05Z";
  const std::string s = JobToJSON(j);
  strncpy(buf, s.c_str(), cap - 1); buf[cap - 1] = 0;
  return (int)s.size();
}
double av1mi_host_gpu_usage(int device, const char *sysfs_root) { return GetGPUUsage(device, sysfs_root ? sysfs_root : "/sys"); }
// container hook for the CPU tests: writes `n` temporal units (concatenated in data, sizes[i] bytes each) to path; 0 = OK
int av1mi_host_mux_units(const char *path, int w, int h, int bd, int fps_n, int fps_d, const uint8_t *data, const long long *sizes,
                         const uint8_t *keys, int n) {
  return av1mi_host_mux_units_colour(path, w, h, bd, fps_n, fps_d, data, sizes, keys, n, nullptr);
}
// av1mi_host_mux_units with a display size on the video track (0, 0 = none)
int av1mi_host_mux_units_display(const char *path, int w, int h, int bd, int fps_n, int fps_d, const uint8_t *data, const long long *sizes,
                                 const uint8_t *keys, int n, int display_w, int display_h) {
  StreamSink sink; std::string err;
  av1::SequenceParams sp; sp.width = w; sp.height = h; sp.bit_depth = bd;
  if (display_w || display_h) sink.set_display_size(display_w, display_h);
  if (!sink.open(path, sp, fps_n, fps_d, &err)) return 1;
  for (int i = 0; i < n; i++) {
    std::vector<uint8_t> tu(data, data + sizes[i]);
    data += sizes[i];
    if (!sink.write(tu, keys[i] != 0, &err)) { sink.abort(); return 2; }
  }
  return sink.close(&err) ? 0 : 3;
}
// RunJobPool over `n` source files joined with '\n'; statuses joined with '\n' into buf; returns the number of successes
int av1mi_host_job_pool(const char *sources, int workers, int ngpus, double ratio, const char *state_dir, char *buf, int cap) {
  std::vector<Job> jobs;
  for (const std::string &path : split_lines(sources)) {
    Job j; j.ID = "pool" + std::to_string(jobs.size()); j.SourcePath = path;
    FILE *f = fopen(path.c_str(), "rb");
    if (f) { fseek(f, 0, SEEK_END); j.OriginalSize = ftell(f); fclose(f); }
    jobs.push_back(j);
  }
  TranscodeConfig cfg; cfg.MaxSizeRatio = ratio; cfg.JobStateDir = state_dir ? state_dir : ""; cfg.StableWaitSeconds = 0;
  ProbeResult pr; pr.HasVideo = true; pr.has_video_stream = true; pr.VideoStream.Height = 720;
  std::vector<std::string> errs;
  const PoolStats ps = RunJobPool(&jobs, workers, ngpus, pr, cfg, &errs);
  std::string out;
  for (size_t i = 0; i < jobs.size(); i++) out += (i ? "\n" : "") + jobs[i].Status + (errs[i].empty() ? "" : ": " + errs[i]);
  strncpy(buf, out.c_str(), cap - 1); buf[cap - 1] = 0;
  return ps.succeeded;
}
}
