// backend.hpp — the part of RunTranscode that replaces the ffmpeg child: raw frames in, an AV1 stream out; everything
// per-pixel on the GPU through the GOP session of libav1mi.so, entropy coding + OBU packing on the host cores.
#pragma once
#include <string>
#include "../../include/av1mi.h"
#include "../csrc/quality.hpp"
#include "mux.hpp"
#include "transcode.hpp"

namespace av1mi_host {
// 0 = OK and job.output written; > 0 = failed after starting (bad input, I/O, device error mid-run);
// < 0 = could not run (no HIP device / library unusable).  *err carries the text.
// report (may be null): what the job found out about its source, for the caller's log.
struct BackendReport { int denoise = -1; };      // the strength -av1mi_denoise auto planned (0 .. 16); -1 = not asked, or the job did not get that far
int RunBackend(const BackendJob &job, std::string *err, BackendReport *report = nullptr);

// What a job's session is opened with, as a pure function (SessionConfig): of the job, of the source's facts as plain values (the Y4M
// header's, Y4mSource's fields of the same names; known_frames -1 = a stream) and of the settled crop window (w == 0: none).
struct SourceFacts { int w, h, bd, src_bd, chroma, sar_n, sar_d, fps_n, fps_d, interlace, colour_range; long known_frames; };
struct SessionPlan {
  av1mi_gop_config cfg;
  av1mi_source_layout fed;      // what the reader threads deliver, one segment's share of the pinned buffers (av1mi_gop_source_layout)
  int tw, th;                   // the target: what a decoder outputs (cfg.width x cfg.height is it rounded up to 8)
  bool square;                  // the target's pixels are square (else the track says at which shape to show them)
  CropRect win;                 // the window the session cuts: the settled one, or the chain's crop=
  av1mi_colour colour;          // the stream's colour record
  // packed: the frames cross PCIe at 10 bits per sample; stored: the job runs through the frame store; analysed: its groups are laid out
  // on scene cuts; grainy: film grain parameters in every frame header; measure: the session returns quality records
  bool packed, stored, analysed, grainy, measure;
  bool telecine;                // -av1mi_ivtc: the session weaves (cfg.telecine); the store's groups are planned by telecineplan.hpp
  int coded_bd;                 // the depth of the stream (-av1mi_depth): what the sequence header, the sink, the rate controller and the figures take
  int reduced_from;             // the source's depth where the job reduces it (10 or 12), else 0
  // the job's OUTPUT (fieldrate.hpp JobOutputOf): output frames per source frame (2 = field rate: -g, the groups' layouts and the
  // indices of av1mi_gop_submit_stored count output frames, the reader and the store source frames) and the rate the sink, the rate
  // controller and the report take
  int out_per_src, fps_n, fps_d;
};
// -av1mi_crop W:H:X:Y against a w x h picture: 0 and *win, or 1 and the text
int ExplicitWindow(const BackendJob &job, int w, int h, CropRect *win, std::string *err);
// 0 and *plan, or the exit code 1 and "Invalid argument: ..." in *err.  Needs no device, no session and no sink.
int SessionConfig(const BackendJob &job, const SourceFacts &src, const CropRect &window, SessionPlan *plan, std::string *err);

// one coded frame of a group: its temporal unit and what the stats file says about it (q: the session's records where the job measures;
// grain: the luma scaling at mid grey where it denoises)
struct FrameOut { std::vector<uint8_t> unit; av1mi_quality q[3]; int base_q_idx; int grain; int ar; int lr_filtered, lr_units; int cdef_moved, cdef_sbs; int lf_y, lf_uv; long ivtc_top, ivtc_bottom; };      // ar: the ar_coeff_lag coded (-av1mi_grain_lag)
// the layout of a group of frames over the session's segments: GOP s holds frames start[s] .. start[s] + len[s] - 1 of the group; cut
// (analysed jobs) flags the frames the scene analysis found.  At field rate the frames of a group are OUTPUT frames (two per source frame).
struct Group {
  std::vector<int32_t> start, len;
  std::vector<uint8_t> cut;
  long frames = 0;
  int T() const { int t = 0; for (int32_t l : len) t = l > t ? l : t; return t; }      // batches: the longest GOP
  bool exists(int s, int t) const { return t < len[(size_t)s]; }
  int32_t index(int s, int t) const { return exists(s, t) ? start[(size_t)s] + t : -1; }      // -1: a flat slot, its output dropped
  std::vector<int32_t> slots(int t) const { std::vector<int32_t> v(len.size()); for (size_t s = 0; s < v.size(); s++) v[s] = index((int)s, t); return v; }      // batch t: per segment
};
// The stats file: the line of frame n in presentation order, and the summary line.  tags: what a line says beyond the
// figures — the window, the colour record and the depth reduction " depth:10>8" (frame 0 only; w == 0 / null / depth_from 0 = none), q: (a job with a target), grain: (a job that denoises)
struct StatsTags { CropRect win; const av1mi_colour *colour = nullptr; int depth_from = 0, depth_to = 0; bool q = false, grain = false, ar = false, lr = false, cdef = false, lf = false, ivtc = false; int denoise_auto = -1, peak_auto = -1; };      // denoise_auto: " denoise:auto>N", the planned strength (frame 0 only; -1 = the job did not ask); peak_auto: " peak:auto>N", the planned source peak in cd/m2, the same way; ivtc: " ivtc:<top source>/<bottom source>", file-wide source frame numbers
std::string StatsFrameLine(long n, bool key, const FrameOut &f, int bit_depth, const StatsTags &tags, bool cut);
std::string StatsSummaryLine(const av1mi::quality::Summary &sum, long long bytes, int bit_depth);

// session_unit.cpp:
// the bitstream writer's frame description for segment `seg` of a collected session batch (pointers into the batch)
// visible_*: the true frame size when width x height is it rounded up to 8 (0 = the coded size)
void DescribeSessionFrame(const av1mi_gop_frame &fr, int seg, int width, int height, int bit_depth, SessionFrameDesc *d, int visible_width = 0,
                          int visible_height = 0);
// the temporal unit of segment `seg` of a collected batch: GPU-coded tiles wrapped, or the symbols coded on `threads` host threads
bool SessionTemporalUnit(const av1mi_gop_frame &fr, int seg, int width, int height, int bit_depth, int visible_width, int visible_height,
                         bool with_sequence_header, int threads, std::vector<uint8_t> *out, std::string *err, bool film_grain_present = false,
                         const av1mi_film_grain *film_grain = nullptr, const av1mi_colour *colour = nullptr);
}
