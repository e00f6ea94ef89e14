// transcode.hpp — host-side mirror of the reference's transcode-job API for the MI355X backend.
//
// The reference is Go and the image has no Go toolchain, so the host side above the C ABI is C++
// with the same names, argument meaning and error behaviour as
//   internal/ffmpeg/transcode.go:17   TranscodeArgs(ffmpegPath, inputPath, outputPath, probeResult, isWebRipLike)
//   internal/ffmpeg/transcode.go:157  DetermineQuality(height)
//   internal/ffmpeg/transcode.go:194  RunTranscode(ffmpegPath, args) (int, error)
//   internal/metadata/probe.go:14-46  ProbeResult / StreamInfo (the fields the path consumes)
// RunTranscode here does not spawn ffmpeg: it drives libav1mi.so (include/av1mi.h) on raw frames.
#pragma once
#include "../../include/av1mi_host.h"
#include <string>
#include <vector>
#include "cropplan.hpp"

namespace av1mi_host {

struct StreamInfo {       // metadata.StreamInfo, probe.go:35-46 (consumed fields only)
  int Index = 0;
  std::string CodecName, CodecType;
  int Width = 0, Height = 0;
  std::string AvgFrameRate;
  int BitDepth = 0;
};
struct ProbeResult {      // metadata.ProbeResult, probe.go:14-22
  bool HasVideo = false, HasAV1 = false, IsWebRipLike = false;
  bool has_video_stream = false;   // VideoStream != nil
  StreamInfo VideoStream;
};

// transcode.go:157-165
int DetermineQuality(int height);
// transcode.go:174-179 (dead code upstream; kept because a 10-bit capable backend needs it)
std::string determineSurfaceFormat(int bitDepth);
// transcode.go:182-191
std::string joinFilterParts(const std::vector<std::string> &parts);

// transcode.go:17-151.  Returns false and sets *err ("no video stream found in probe result") when VideoStream is nil,
// otherwise fills `args` with exactly the argv the reference builds.
bool TranscodeArgs(const std::string &ffmpegPath, const std::string &inputPath, const std::string &outputPath,
                   const ProbeResult &probeResult, bool isWebRipLike, std::vector<std::string> *args, std::string *err);

// What the MI355X backend takes from that argv: input (last "-i"), output (last argument), quality
// ("-global_quality:v:0"), and the bit depth policy.  The reference forces 8-bit NV12 (transcode.go:99-110).
struct BackendJob {
  std::string input, output;
  int quality = 25;        // FFmpeg global_quality; av1_vaapi uses it directly as the AV1 base_q_idx [ext]
  int gop = 30;            // closed-GOP segment length
  int device = 0;
  int segments = 4;        // closed GOPs coded in lockstep (the GOP session's batch)
  int threads = 0;         // host threads for entropy coding; 0 = all cores
  int gpu_entropy = 1;     // 1 = the AV1 tile entropy coder runs on the GPU (the host only assembles frames); 0 = north_star's split:
                           // symbols are downloaded and coded on the host cores.  Same bytes either way.
  int key_block_size = 32; // -av1mi_key_block_size 8 | 32: key frames in 32x32 blocks where the coded width (the source's rounded up to 8) is a multiple of 32 (av1mi_gop_config.key_block_size;
                           // +3.7 dB at equal size on the synthetic key frames at q 128 for ~9 % of the throughput), else 8x8 like every other frame
  int pack10 = 0;          // -av1mi_pack10 0 | 1: with a 10-bit source, pack the frames to 10 bits per sample on the reader threads before the PCIe upload
                           // (av1mi.h AV1MI_INPUT_PACKED10: 5 / 8 of the bytes on the link and in the pinned buffers; same output bytes).  Accepted and
                           // without effect with an 8-bit source
  bool have_vf = false;    // "-vf:v:0" / "-vf" was given: the filter chain below is evaluated on the source's size and sample aspect ratio
  std::string vf;          // (ScaleTarget) and the frames are scaled on the GPU to what it yields; absent = the source size is coded as before
  int scale_w = 0, scale_h = 0;      // -av1mi_scale WxH: an explicit target (16 .. 4096 each); wins over the chain
  std::string stats_path;  // -av1mi_stats <file>: per-frame PSNR / SSIM of the decoded picture against the source as coded, measured on the GPU
                           // (av1mi_gop_config.quality_stats), one line per frame in presentation order + a summary line
  double min_psnr = 0;     // -av1mi_min_psnr <dB>: the quality gate on the summary's psnr_y (0 = off), with or without a stats file: below it the
                           // transcode fails with exit code 3, "quality gate: psnr_y ...", and the output is removed
  int lr_search = 0;       // -av1mi_lr_search 0 | 1: 1 = a Wiener record or none chosen per restoration unit on the GPU (av1mi_gop_config.lr_search); the
                           // stats file's frame lines gain " lr:<units filtered>/<units>"
  int cdef_search = 0;     // -av1mi_cdef_search 0 .. 3: N > 0 = cdef_bits N: one of 1 << N CDEF strength sets chosen per 64x64 superblock on the GPU
                           // (av1mi_gop_config.cdef_search); the stats file's frame lines gain " cdef:<superblocks not on set 0>/<superblocks>"
  int lf_search = 0;       // -av1mi_lf_search 0 | 1: 1 = the deblocking levels chosen per frame on the GPU against the source (av1mi_gop_config.lf_search);
                           // the stats file's frame lines gain " lf:<luma vertical level>/<chroma level>"
  int me_range = 0;        // -av1mi_me_range N: 0 (default), or a multiple of 4 up to 64: P frames search around a coarse centre per 64x64 tile
                           // (av1mi_gop_config.coarse_range): vectors reach N + 8 samples per frame instead of 8
  // A target instead of the fixed quantiser (host/ratecontrol.hpp: one quantiser per batch, chosen from the bytes of the batches before).
  // -b:v:0 N (alias -b:v; FFmpeg's k / M suffixes): bits per second of the video; -av1mi_target_bpp X: bits per pixel per frame of the coded
  // picture's true size, the form of the reference's own estimate (cmd/av1d/main.go:413-427: 0.15 / 0.12 / 0.10).  One of the two at most.
  // -global_quality:v:0 is then the START quantiser; -qmin / -qmax (only with a target) bound what the controller may choose.  0 = not given
  long long bitrate = 0;
  long long target_bpp_u = 0;   // in millionths of a bit per pixel
  int qmin = 0, qmax = 0;
  bool to_420 = false;     // the job converts its source to 4:2:0: the chain has a format= filter naming a 4:2:0 format (nv12, p010, p010le, yuv420p,
                           // yuv420p10le — the reference's chain always does, transcode.go:99-110), or -av1mi_format 420 was given.  The source may then be
                           // 4:2:2, 4:4:4 or grey, at 8, 10 or 12 bits (Y4mSource::open's any_layout); it is converted on the GPU (av1mi.h "chroma formats").
                           // The coded depth follows the SOURCE (8 -> 8, 10 -> 10, 12 -> 10) unless -av1mi_depth says otherwise.  Without it such a source is refused
  int scenecut = 0;        // -av1mi_scenecut N: 0 (default) = off; 1 .. 99 = the sensitivity of the scene-cut rule (include/av1mi.h "scene analysis";
                           // host/sceneplan.hpp AV1MI_SCENECUT_DEFAULT is the measured middle).  Every group of segments x gop frames is put into the
                           // session's frame store in file order, analysed on the GPU, and its GOP boundaries are moved onto the cuts found
                           // (av1mi_plan_gops): key frames land on the cuts, GOPs are min_gop .. 3/2 gop frames long.  Not with -av1mi_pack10 1
  int deinterlace = 0;     // -av1mi_deinterlace off | auto | tff | bff (0 .. 3).  off (default): every source is coded as its frames are.  auto: a source whose
                           // Y4M header says It / Ib is deinterlaced on the GPU with that parity (include/av1mi.h "deinterlacing": same-rate, one
                           // frame per frame unless -av1mi_deinterlace_rate field), a progressive one is coded as ever, Im is refused (film by
                           // pulldown is -av1mi_ivtc's business).  tff / bff force a parity, for sources whose header lies.  A chain that names yadif, bwdif or deinterlace_vaapi
                           // (bare, mode=0 or mode=send_frame) means auto.  The job then runs through the frame store.  Not with -av1mi_pack10 1
  int deint_rate = 0;      // -av1mi_deinterlace_rate frame | field (0, 1).  frame (default): one output frame per source frame.  field: one per FIELD
                           // (include/av1mi.h "FIELD-RATE OUTPUT", av1mi_gop_config.deinterlace_fields): twice the frames at twice the rate
                           // (host/fieldrate.hpp), -g counts OUTPUT frames and must be even, a group holds segments x gop / 2 source frames.  It has
                           // a meaning only where the job deinterlaces: with -av1mi_deinterlace off, or auto on a progressive source, the job
                           // runs as ever.  The chain's own field-rate spellings (yadif=1, bwdif=mode=send_field ...) stay refused
  int ivtc = 0;            // -av1mi_ivtc 0 | 1.  1: inverse telecine (include/av1mi.h "inverse telecine", av1mi_gop_config.telecine), whatever the Y4M header's I
                           // parameter says, Im included: film carried by 3:2 pulldown is woven back from the right fields and the repeated frame of
                           // every five is dropped.  -g counts OUTPUT frames and must be a multiple of 4; a group of segments x gop output frames is
                           // segments x gop x 5 / 4 source frames, put into the store between the last frame of the group before and the first of the
                           // group after (context), analysed on the GPU, planned (host/telecineplan.hpp) and submitted as woven pairs.  Rate and count
                           // follow host/fieldrate.hpp (30000/1001 -> 24000/1001).  On material that is not telecined it drops one frame in five.  Not
                           // with -av1mi_deinterlace, -av1mi_denoise, -av1mi_pack10 1 or -av1mi_scenecut
  int denoise = 0;         // -av1mi_denoise N: 0 (default) = off; 1 .. 16 = the strength of the temporal denoiser (include/av1mi.h "denoising",
                           // av1mi_gop_config.denoise).  The job then runs through the frame store (one group), also without -av1mi_scenecut; the
                           // first and last frame of a group pass through.  Not with -av1mi_pack10 1, not with -av1mi_deinterlace
  bool denoise_auto = false;   // -av1mi_denoise auto: the strength is PLANNED per file before the session opens (host/noiseplan.hpp): needs a seekable
                           // file; up to 16 pairs of consecutive frames spread evenly over it are uploaded and measured on the GPU
                           // (av1mi_noise_analyse, include/av1mi.h "noise records").  Planned N >= 1: the job -av1mi_denoise N runs, byte for byte.
                           // Planned 0: the job without -av1mi_denoise, byte for byte; -av1mi_denoise_range, -av1mi_film_grain and
                           // -av1mi_grain_lag are then dropped with it.  Everything -av1mi_denoise N is refused with, auto is refused with,
                           // whatever is planned later.  `denoise` stays 0 until the plan is made
  int denoise_range = 0;   // -av1mi_denoise_range N: 0 (default), 4 or 8 = the range of the denoiser's block search (include/av1mi.h "motion-compensated
                           // denoising", av1mi_gop_config.denoise_range); an error without -av1mi_denoise
  int grain_lag = 0;       // -av1mi_grain_lag N: 0 (default, white grain) .. 3 = the lag of the film grain's autoregressive filter, its coefficients from the
                           // covariance of what the denoiser removed (host/filmgrain.hpp "coloured"; av1mi_gop_config.grain_cov); an error without
                           // -av1mi_denoise or with -av1mi_film_grain 0
  int film_grain = -1;     // -av1mi_film_grain 0 | 1: with -av1mi_denoise, 1 (the default there) signals film grain synthesis parameters derived from
                           // what the denoiser removed (host/filmgrain.hpp), 0 codes the clean frames alone; an error without -av1mi_denoise
  int min_gop = 0;         // -av1mi_min_gop M: the shortest GOP the planner makes, 1 .. gop - gop / 2; 0 = max(1, gop / 4).  Only with -av1mi_scenecut
  int crop_mode = 0;       // -av1mi_crop off | auto | W:H:X:Y (0, 1, 2).  off (default): only a crop= filter of the chain crops.  W:H:X:Y: that window of the
                           // source (rounded down to even like the chain's crop=), in front of the chain.  auto: needs a seekable file; up to 32 frames
                           // spread evenly over it are uploaded and analysed on the GPU (av1mi_crop_analyse at -av1mi_crop_limit, default 24:
                           // FFmpeg cropdetect's), host/cropplan.hpp turns the margins into a window, and the session is opened with it
                           // (av1mi_gop_config.crop_*); no bars found = the path without a window, exactly.  auto or W:H:X:Y together with a crop=
                           // in the chain is refused.  Not with -av1mi_pack10 1 (the window is cut from planar planes; the packed upload would need
                           // a second planar copy of the whole frame)
  CropRect crop;           // -av1mi_crop W:H:X:Y as given
  int crop_limit = kCropLimitDefault;   // -av1mi_crop_limit N (0 .. 255)
  // Colour.  -color_primaries / -color_trc / -colorspace / -color_range (FFmpeg's output options, bare or with a :v / :v:0 suffix; FFmpeg's
  // names or plain numbers 0 .. 255): the description the stream carries (av1mi_colour: sequence header, Matroska Colour).  -1 = not given:
  // unspecified (2); the range then follows the Y4M header's XCOLORRANGE.  -av1mi_master_display "G(x,y)B(x,y)R(x,y)WP(x,y)L(max,min)" (the
  // x265 / FFmpeg string: chromaticities in 0.00002, luminance in 0.0001 cd/m2) and -av1mi_max_cll "cll,fall": HDR10 static metadata.
  int color_primaries = -1, color_trc = -1, colorspace = -1, color_range = -1;
  av1mi_colour hdr = {};   // have_mdcv / have_cll and their numbers; the four fields above fill the rest when the job runs
  // -av1mi_tonemap off | bt2390 (a tonemap_vaapi in the chain means bt2390): the PQ / BT.2020 source becomes BT.709 SDR on the GPU
  // (av1mi_gop_config.tone_map); -av1mi_tonemap_peak N: the source's peak in cd/m2 (else the mastering display's maximum, else 1000).  The
  // output is then described as 1 / 1 / 1 limited without metadata, and -color_* describe the SOURCE (bt2020 / smpte2084 / bt2020nc / tv or nothing)
  int tonemap = 0, tonemap_peak = 0;
  // -av1mi_tonemap_peak auto: the peak is PLANNED per file before the session opens (host/peakplan.hpp): needs tone mapping, a seekable file
  // and a source that is 4:2:0 at 10 bits in the file; up to 32 frames spread evenly over it (the crop sampler's slots) are uploaded, all
  // three planes, and measured on the GPU (av1mi_peak_analyse, include/av1mi.h "peak records").  The job -av1mi_tonemap_peak N then runs,
  // byte for byte.  `tonemap_peak` stays 0 until the plan is made
  bool tonemap_peak_auto = false;
  // -av1mi_depth 8 | 10 | source | chain: the depth that is CODED (av1mi_gop_config.coded_bit_depth).  source (0, the default): the source's, as
  // ever (8 -> 8, 10 -> 10, 12 -> 10).  8: a 10- or 12-bit source is reduced to 8 bits on the GPU at the end of the input chain, behind the
  // scaler and the tone map; nothing happens to an 8-bit source.  chain (-1): the LAST format= of the chain decides (chain_depth: nv12, yuv420p = 8;
  // p010, p010le, yuv420p10le = 10; none = source): what the reference's argv means by format=nv12.  10, or a chain asking for 10, with an 8-bit
  // source is refused when the source is known: 8 -> 10 bits is not built.  -av1mi_dither ordered | round (1, 0; -1 = not given: ordered): the
  // reduction's rounding (include/av1mi.h "depth reduction"); an error without -av1mi_depth.  Not together with -av1mi_denoise
  int depth = 0, dither = -1, chain_depth = 0;
  std::vector<std::string> tracks;   // -av1mi_tracks <file.mka> (repeatable): Matroska side files whose audio / subtitle tracks are copied
                                     // next to the video (the reference's `-c:a copy -c:s copy`, transcode.go:134-137, after an external demux)
};
bool ParseBackendJob(const std::vector<std::string> &args, BackendJob *job, std::string *err);
// the colour record a job's stream carries: the options, the Y4M header's range (-1 = none) where -color_range is absent, and what tone mapping forces
av1mi_colour JobColour(const BackendJob &job, int y4m_range);

// The video filter chain of the argv (transcode.go:92-115), evaluated as it is written on a source of iw x ih samples with sample aspect
// ratio sar_n : sar_d.  Recognised, literally: the reference's SAR scale (transcode.go:97: (w, h) = sar < 1 ? (iw, iw / sar) :
// (iw * sar, ih), truncated to integers — the first branch divides iw, as written upstream), its even-size scale (:98 / :107: each
// dimension rounded up to even), `hwdownload`, `hwupload`, `setsar=1` (no effect on planar 4:2:0 frames), `format=` naming a 4:2:0
// format (nv12, p010, p010le, yuv420p, yuv420p10le: no effect on the size; *to_420, when given, is set — BackendJob::to_420; any other
// format is "Invalid argument: unsupported filter format=<name>"), the deinterlacers `yadif`, `bwdif` and `deinterlace_vaapi`, bare or with
// `mode=0` / `mode=send_frame` (one frame per frame: *deint, when given, is set — BackendJob::deinterlace auto; any other argument is
// "Invalid argument: unsupported filter argument <filter>=<argument> ..."), and
// `scale=W:H` / `scale_vaapi=w=W:h=H` with plain integers.  Returns false and "Invalid argument: unsupported filter <name>" for
// anything else.  *square: the chain leaves square pixels (it resampled by the SAR, or to an explicit size).
bool ScaleTarget(int iw, int ih, int sar_n, int sar_d, const std::string &chain, int *w, int *h, bool *square, std::string *err, bool *to_420 = nullptr,
                 bool *deint = nullptr);

// The same evaluation with `crop=` accepted (ScaleTarget keeps refusing it: "unsupported filter crop").  Forms: positional crop=W:H[:X:Y] and
// named w= / out_w= / h= / out_h= / x= / y=, plain integers only; x and y default to the centre, (iw - W) / 2 and (ih - H) / 2.  All four
// values are rounded down to even: what FFmpeg's crop does on 4:2:0 frames without exact=1 [ext].  exact=0 and keep_aspect=0 (the defaults)
// are accepted.  "Invalid argument: unsupported filter argument crop=... (reason)" for expressions, exact=1, keep_aspect, a crop after a
// scale filter and a window outside the picture (or smaller than 16x16).  *crop receives the window in SOURCE samples (w == 0: the chain
// does not crop; a second crop composes with the first), and every later filter of the chain sees the window's size.  geometry = false
// checks the syntax alone, for a chain whose source size is not known yet: *w, *h and the window are then meaningless.
bool ChainTarget(int iw, int ih, int sar_n, int sar_d, const std::string &chain, int *w, int *h, bool *square, std::string *err, bool *to_420, bool *deint,
                 CropRect *crop, bool geometry = true, bool *tonemap = nullptr);
// (`tonemap_vaapi`, bare or with format=nv12|p010 and t / m / p = bt709, sets *tonemap — BackendJob::tonemap; any other argument of it, and the
// software filters tonemap= and zscale=, are refused)

// transcode.go:194-315 contract: (0, "") on success AND the output file exists; (code, text <= 800 chars) on failure;
// (-1, text) when the backend could not run at all (no HIP device, library error before any frame).  Exit code 3 is the quality gate
// (-av1mi_min_psnr): its text is handed on as it is, "quality gate: psnr_y ...", for ProcessJob to treat like the size gate.
// denoise: the strength -av1mi_denoise auto planned for the file (0 .. 16), for the caller's log; -1 = the job did not ask, or did not get that far.
struct RunResult { int exitCode; std::string err; int denoise = -1; };
RunResult RunTranscode(const std::string &backendPath, const std::vector<std::string> &args);

}  // namespace av1mi_host
