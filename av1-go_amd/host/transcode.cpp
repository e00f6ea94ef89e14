// transcode.cpp — see transcode.hpp.  Argument vector and error strings follow internal/ffmpeg/transcode.go.
#include "transcode.hpp"
#include "backend.hpp"
#include <sys/stat.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>

namespace av1mi_host {

int DetermineQuality(int height) {   // transcode.go:157-165
  if (height >= 1440) return 23;
  if (height >= 1080) return 24;
  return 25;
}
std::string determineSurfaceFormat(int bitDepth) { return bitDepth >= 10 ? "p010" : "nv12"; }
std::string joinFilterParts(const std::vector<std::string> &parts) {
  std::string out;
  for (size_t i = 0; i < parts.size(); i++) out += (i ? "," : "") + parts[i];
  return out;
}

bool TranscodeArgs(const std::string &ffmpegPath, const std::string &inputPath, const std::string &outputPath,
                   const ProbeResult &probeResult, bool isWebRipLike, std::vector<std::string> *args, std::string *err) {
  (void)ffmpegPath;   // unused upstream as well
  if (!probeResult.has_video_stream) {
    if (err) *err = "no video stream found in probe result";   // transcode.go:19
    return false;
  }
  std::vector<std::string> &a = *args;
  a = { "-hide_banner", "-analyzeduration", "50M", "-probesize", "50M",                        // :40-44
        "-init_hw_device", "vaapi=va", "-hwaccel", "vaapi", "-hwaccel_output_format", "vaapi",   // :48-52
        "-filter_hw_device", "va" };
  if (isWebRipLike) for (const char *s : { "-fflags", "+genpts", "-copyts", "-start_at_zero" }) a.push_back(s);   // :59-65
  a.push_back("-i"); a.push_back(inputPath);                                                   // :68
  for (const char *s : { "-map", "0", "-map", "-0:v", "-map", "-0:t" }) a.push_back(s);         // :71-75
  a.push_back("-map"); a.push_back("0:v:" + std::to_string(probeResult.VideoStream.Index));     // :76
  for (const char *s : { "-map", "0:a?", "-map", "-0:a:m:language:rus", "-map", "-0:a:m:language:ru", "-map", "0:s?",
                         "-map", "-0:s:m:language:rus", "-map", "-0:s:m:language:ru", "-map_chapters", "0" })
    a.push_back(s);                                                                              // :77-83
  const int quality = DetermineQuality(probeResult.VideoStream.Height);                          // :86
  std::vector<std::string> vf;
  if (isWebRipLike) vf.push_back("scale_vaapi=w='if(gt(iw,iw*sar),iw,iw*sar)':h='if(gt(iw,iw*sar),iw/sar,ih)'");   // :96
  for (const char *s : { "scale_vaapi=w=ceil(iw/2)*2:h=ceil(ih/2)*2", "hwdownload,format=nv12", "setsar=1", "format=nv12", "hwupload" })
    vf.push_back(s);                                                                             // :97-112
  a.push_back("-vf:v:0"); a.push_back(joinFilterParts(vf));                                      // :115
  a.push_back("-c:v:0"); a.push_back("av1_vaapi");                                               // :120
  a.push_back("-global_quality:v:0"); a.push_back(std::to_string(quality));                      // :121
  a.push_back("-compression_level"); a.push_back("2");                                           // :122
  if (isWebRipLike) for (const char *s : { "-vsync", "0", "-avoid_negative_ts", "make_zero" }) a.push_back(s);     // :126-131
  for (const char *s : { "-c:a", "copy", "-c:s", "copy", "-max_muxing_queue_size", "2048", "-map_metadata", "0", "-f", "matroska",
                         "-movflags", "+faststart" })
    a.push_back(s);                                                                              // :134-145
  a.push_back(outputPath);                                                                       // :148
  return true;
}

static const char kSarScale[] = "scale_vaapi=w='if(gt(iw,iw*sar),iw,iw*sar)':h='if(gt(iw,iw*sar),iw/sar,ih)'";   // :97
static const char kEvenScale[] = "scale_vaapi=w=ceil(iw/2)*2:h=ceil(ih/2)*2";                                        // :98, :107

static bool plain_int(const std::string &t, int *v) {
  if (t.empty() || t.size() > 6) return false;
  for (char c : t) if (c < '0' || c > '9') return false;
  *v = std::atoi(t.c_str());
  return true;
}

// crop=...: the four values (-1 = not given) of FFmpeg's option order out_w, out_h, x, y, keep_aspect, exact; false + *why for what is not honoured
static bool crop_arguments(const std::string &arg, int v[4], std::string *why) {
  v[0] = v[1] = v[2] = v[3] = -1;
  int pos = 0;
  size_t p = 0;
  while (p <= arg.size()) {
    size_t q = arg.find(':', p);
    if (q == std::string::npos) q = arg.size();
    const std::string tok = arg.substr(p, q - p);
    p = q + 1;
    const size_t eq = tok.find('=');
    std::string key = eq == std::string::npos ? "" : tok.substr(0, eq);
    const std::string val = eq == std::string::npos ? tok : tok.substr(eq + 1);
    if (key.empty()) {
      static const char *const order[6] = { "w", "h", "x", "y", "keep_aspect", "exact" };
      if (pos >= 6) { *why = "too many values"; return false; }
      key = order[pos++];
    }
    int n = 0;
    const int slot = key == "w" || key == "out_w" ? 0 : key == "h" || key == "out_h" ? 1 : key == "x" ? 2 : key == "y" ? 3 : -1;
    if (slot >= 0) {
      if (!plain_int(val, &n)) { *why = "plain integers only, no expressions"; return false; }
      v[slot] = n;
    } else if (key == "exact") {
      if (val != "0") { *why = "exact=1 is not built: the window is rounded down to even"; return false; }
    } else if (key == "keep_aspect") {
      if (val != "0") { *why = "keep_aspect is not built"; return false; }
    } else { *why = "unknown option " + key; return false; }
  }
  if (v[0] < 0 || v[1] < 0) { *why = "give the window's width and height"; return false; }
  return true;
}

bool ScaleTarget(int iw, int ih, int sar_n, int sar_d, const std::string &chain, int *w, int *h, bool *square, std::string *err, bool *to_420, bool *deint) {
  return ChainTarget(iw, ih, sar_n, sar_d, chain, w, h, square, err, to_420, deint, nullptr);
}

bool ChainTarget(int iw, int ih, int sar_n, int sar_d, const std::string &chain, int *w, int *h, bool *square, std::string *err, bool *to_420, bool *deint,
                 CropRect *crop, bool geometry, bool *tonemap) {
  if (sar_n <= 0 || sar_d <= 0) sar_n = sar_d = 1;
  long cw = iw, ch = ih;
  bool sq = sar_n == sar_d, scaled = false;
  if (crop) *crop = CropRect();
  // split at commas outside quotes
  std::vector<std::string> parts;
  std::string cur;
  bool quoted = false;
  for (char c : chain) {
    if (c == '\'') quoted = !quoted;
    if (c == ',' && !quoted) { parts.push_back(cur); cur.clear(); } else cur.push_back(c);
  }
  parts.push_back(cur);
  for (const std::string &f : parts) {
    int a = 0, b = 0;
    if (crop && f.compare(0, 5, "crop=") == 0) {
      int v[4];
      std::string why;
      bool ok = crop_arguments(f.substr(5), v, &why);
      if (ok && scaled) { ok = false; why = "a crop after a scale filter is not built: the window is cut from the source"; }
      if (ok && geometry) {
        const long W = v[0] & ~1, H = v[1] & ~1;
        const long X = (v[2] >= 0 ? v[2] : (cw - W) / 2) & ~1L, Y = (v[3] >= 0 ? v[3] : (ch - H) / 2) & ~1L;
        if (W < 16 || H < 16) { ok = false; why = "a window of at least 16x16"; }
        else if (W > cw || H > ch || X < 0 || Y < 0 || X > cw - W || Y > ch - H) { ok = false; why = "the window lies outside the " + std::to_string(cw) + "x" + std::to_string(ch) + " picture"; }
        else { crop->x += (int)X; crop->y += (int)Y; crop->w = (int)W; crop->h = (int)H; cw = W; ch = H; }
      }
      if (!ok) { if (err) *err = "Invalid argument: unsupported filter argument " + f + " (" + why + ")"; return false; }
    } else if (f == kSarScale) {
      scaled = true;
      if (sar_n < sar_d) ch = cw * sar_d / sar_n;      // gt(iw, iw * sar), i.e. sar < 1: (iw, iw / sar) — iw, as the expression is written
      else cw = cw * sar_n / sar_d;                    // else (iw * sar, ih)
      sar_n = sar_d = 1; sq = true;
    } else if (f == kEvenScale) {
      scaled = true;
      cw = (cw + 1) / 2 * 2; ch = (ch + 1) / 2 * 2;
    } else if (f.empty() || f == "hwdownload" || f == "hwupload" || f == "setsar=1") {
    } else if (f.compare(0, 7, "format=") == 0) {      // the encoder is handed 4:2:0 whatever the decoder produced (transcode.go:99-110); nothing else can be honoured
      const std::string name = f.substr(7);
      if (name != "nv12" && name != "p010" && name != "p010le" && name != "yuv420p" && name != "yuv420p10le") { if (err) *err = "Invalid argument: unsupported filter " + f; return false; }
      if (to_420) *to_420 = true;
    } else if (f == "tonemap_vaapi" || f.compare(0, 14, "tonemap_vaapi=") == 0) {
      // BT.2390 to BT.709 is what is built (include/av1mi.h "tone mapping"); the output's depth is -av1mi_depth's business, not this filter's format=
      std::string rest = f.size() > 14 ? f.substr(14) : "";
      while (!rest.empty()) {
        const size_t c = rest.find(':');
        const std::string tok = rest.substr(0, c);
        rest = c == std::string::npos ? "" : rest.substr(c + 1);
        if (tok != "format=nv12" && tok != "format=p010" && tok != "t=bt709" && tok != "m=bt709" && tok != "p=bt709") {
          if (err) *err = "Invalid argument: unsupported filter argument " + f + " (only format=nv12|p010 and t / m / p = bt709: the output is BT.709 SDR)";
          return false;
        }
      }
      if (tonemap) *tonemap = true;
    } else if (f == "yadif" || f == "bwdif" || f == "deinterlace_vaapi" || f.compare(0, 6, "yadif=") == 0 || f.compare(0, 6, "bwdif=") == 0 ||
               f.compare(0, 18, "deinterlace_vaapi=") == 0) {
      // same-rate deinterlacing is what is built (include/av1mi.h "deinterlacing"): one frame per frame.  Field-rate modes, a forced
      // parity or a deint= selection cannot be honoured from here and are not skipped
      const size_t eq = f.find('=');
      const std::string arg = eq == std::string::npos ? "" : f.substr(eq + 1);
      if (!arg.empty() && arg != "mode=0" && arg != "mode=send_frame") {
        if (err) *err = "Invalid argument: unsupported filter argument " + f + " (only mode=0 / mode=send_frame: one frame per frame)";
        return false;
      }
      if (deint) *deint = true;
    } else if (f.compare(0, 6, "scale=") == 0 && f.find(':') != std::string::npos && plain_int(f.substr(6, f.find(':') - 6), &a) &&
               plain_int(f.substr(f.find(':') + 1), &b)) {
      cw = a; ch = b; sar_n = sar_d = 1; sq = true; scaled = true;
    } else if (f.compare(0, 14, "scale_vaapi=w=") == 0 && f.find(":h=") != std::string::npos && plain_int(f.substr(14, f.find(":h=") - 14), &a) &&
               plain_int(f.substr(f.find(":h=") + 3), &b)) {
      cw = a; ch = b; sar_n = sar_d = 1; sq = true; scaled = true;
    } else {
      if (err) *err = "Invalid argument: unsupported filter " + f.substr(0, f.find('='));
      return false;
    }
    if (cw < 1 || ch < 1 || cw > 65535 || ch > 65535) { if (err) *err = "Invalid argument: filter " + f.substr(0, f.find('=')) + " yields an impossible size"; return false; }
  }
  *w = (int)cw; *h = (int)ch;
  if (square) *square = sq;
  return true;
}

// FFmpeg's names of the H.273 code points it lets a job set (libavutil/pixdesc.c), or a plain number 0 .. 255
static bool code_point(const std::string &v, const char *const (*names)[2], int *out) {
  for (; (*names)[0]; names++) if (v == (*names)[0]) { *out = std::atoi((*names)[1]); return true; }
  return plain_int(v, out) && *out <= 255;
}
static const char *const kPrimaries[][2] = { { "bt709", "1" }, { "unknown", "2" }, { "unspecified", "2" }, { "bt470m", "4" }, { "bt470bg", "5" }, { "smpte170m", "6" }, { "smpte240m", "7" }, { "film", "8" },
                                             { "bt2020", "9" }, { "smpte428", "10" }, { "smpte431", "11" }, { "smpte432", "12" }, { nullptr, nullptr } };
static const char *const kTransfer[][2] = { { "bt709", "1" }, { "unknown", "2" }, { "unspecified", "2" }, { "gamma22", "4" }, { "bt470m", "4" }, { "gamma28", "5" }, { "bt470bg", "5" }, { "smpte170m", "6" },
                                            { "smpte240m", "7" }, { "linear", "8" }, { "iec61966-2-4", "11" }, { "bt1361e", "12" }, { "iec61966-2-1", "13" }, { "bt2020-10", "14" },
                                            { "bt2020-12", "15" }, { "smpte2084", "16" }, { "smpte428", "17" }, { "arib-std-b67", "18" }, { nullptr, nullptr } };
static const char *const kMatrix[][2] = { { "rgb", "0" }, { "gbr", "0" }, { "bt709", "1" }, { "unknown", "2" }, { "unspecified", "2" }, { "fcc", "4" }, { "bt470bg", "5" }, { "smpte170m", "6" },
                                          { "smpte240m", "7" }, { "ycgco", "8" }, { "bt2020nc", "9" }, { "bt2020c", "10" }, { "smpte2085", "11" }, { nullptr, nullptr } };
static const char *const kRange[][2] = { { "tv", "0" }, { "mpeg", "0" }, { "limited", "0" }, { "pc", "1" }, { "jpeg", "1" }, { "full", "1" }, { nullptr, nullptr } };

// n numbers separated by commas between `open` and ')' at *p (which moves past them); each 0 .. limit
static bool numbers(const std::string &s, size_t *p, const char *open, int n, long long limit, long long *out) {
  if (s.compare(*p, strlen(open), open)) return false;
  *p += strlen(open);
  for (int i = 0; i < n; i++) {
    size_t d = 0;
    long long v = 0;
    while (*p + d < s.size() && d < 12 && s[*p + d] >= '0' && s[*p + d] <= '9') v = v * 10 + (s[*p + d++] - '0');
    if (!d || v > limit || *p + d >= s.size() || s[*p + d] != (i + 1 < n ? ',' : ')')) return false;
    out[i] = v; *p += d + 1;
  }
  return true;
}

// one of the colour options (true: args[i] was one; *why is set where its value is refused)
static bool colour_option(const std::string &name, const std::string &v, BackendJob *job, std::string *why) {
  std::string base = name;
  for (const char *suffix : { ":v:0", ":v" }) if (base.size() > strlen(suffix) && !base.compare(base.size() - strlen(suffix), strlen(suffix), suffix)) { base.resize(base.size() - strlen(suffix)); break; }
  auto take = [&](const char *const (*names)[2], int *out) { if (!code_point(v, names, out)) *why = "Invalid argument: " + name + " takes one of FFmpeg's names or a number 0 .. 255, not " + v; };
  if (base == "-color_primaries") take(kPrimaries, &job->color_primaries);
  else if (base == "-color_trc") take(kTransfer, &job->color_trc);
  else if (base == "-colorspace") {
    take(kMatrix, &job->colorspace);
    if (why->empty() && job->colorspace == 0) *why = "Invalid argument: " + name + " " + v + ": matrix 0 (identity / RGB) implies 4:4:4, which is not coded";
  }
  else if (base == "-color_range") { if (!code_point(v, kRange, &job->color_range) || job->color_range > 1) *why = "Invalid argument: " + name + " takes tv / mpeg / limited (0) or pc / jpeg / full (1), not " + v; }
  else if (name == "-av1mi_master_display") {
    long long g[2], b[2], r[2], wp[2], l[2];
    size_t p = 0;
    if (!numbers(v, &p, "G(", 2, 50000, g) || !numbers(v, &p, "B(", 2, 50000, b) || !numbers(v, &p, "R(", 2, 50000, r) || !numbers(v, &p, "WP(", 2, 50000, wp) ||
        !numbers(v, &p, "L(", 2, 100000000, l) || p != v.size() || l[0] <= l[1]) {
      *why = "Invalid argument: -av1mi_master_display takes G(x,y)B(x,y)R(x,y)WP(x,y)L(max,min): chromaticities 0 .. 50000 (units of 0.00002), luminance in 0.0001 cd/m2 up to 10000 cd/m2, max above min; not " + v;
      return true;
    }
    av1mi_colour &c = job->hdr;
    auto chroma = [](long long n) { return (uint16_t)std::min<long long>((n * 65536 + 25000) / 50000, 65535); };      // 0.00002 units -> 0.16, to nearest
    c.have_mdcv = 1;
    c.primary_x[0] = chroma(r[0]); c.primary_y[0] = chroma(r[1]); c.primary_x[1] = chroma(g[0]); c.primary_y[1] = chroma(g[1]); c.primary_x[2] = chroma(b[0]); c.primary_y[2] = chroma(b[1]);
    c.white_x = chroma(wp[0]); c.white_y = chroma(wp[1]);
    c.luminance_max = (uint32_t)((l[0] * 256 + 5000) / 10000); c.luminance_min = (uint32_t)((l[1] * 16384 + 5000) / 10000);      // 0.0001 cd/m2 -> 24.8 / 18.14
  }
  else if (name == "-av1mi_max_cll") {
    long long n[2];
    size_t p = 0;
    const std::string wrapped = "(" + v + ")";
    if (!numbers(wrapped, &p, "(", 2, 65535, n) || p != wrapped.size()) { *why = "Invalid argument: -av1mi_max_cll takes \"cll,fall\" in cd/m2 (0 .. 65535 each), not " + v; return true; }
    job->hdr.have_cll = 1; job->hdr.max_cll = (uint16_t)n[0]; job->hdr.max_fall = (uint16_t)n[1];
  }
  else return false;
  return true;
}

av1mi_colour JobColour(const BackendJob &job, int y4m_range) {
  av1mi_colour c = job.hdr;
  if (job.tonemap) {      // what the kernel makes: BT.709 limited, the display-referred metadata of the source no longer applies
    c = av1mi_colour();
    c.primaries = c.transfer = c.matrix = 1;
    return c;
  }
  c.primaries = job.color_primaries < 0 ? 2 : job.color_primaries; c.transfer = job.color_trc < 0 ? 2 : job.color_trc; c.matrix = job.colorspace < 0 ? 2 : job.colorspace;
  c.full_range = job.color_range >= 0 ? job.color_range : y4m_range > 0 ? 1 : 0;
  return c;
}

bool ParseBackendJob(const std::vector<std::string> &args, BackendJob *job, std::string *err) {
  if (args.size() < 3) { if (err) *err = "Invalid argument: too few arguments"; return false; }
  job->output = args.back();
  bool have_in = false, deint_given = false, grain_lag_given = false, depth_given = false;
  std::string colour_err;
  for (size_t i = 0; i + 1 < args.size(); i++) {
    if (args[i] == "-i") { job->input = args[i + 1]; have_in = true; }
    else if (args[i] == "-global_quality:v:0") job->quality = std::atoi(args[i + 1].c_str());
    else if (args[i] == "-g") job->gop = std::atoi(args[i + 1].c_str());
    else if (args[i] == "-av1mi_device") job->device = std::atoi(args[i + 1].c_str());
    else if (args[i] == "-av1mi_segments") job->segments = std::atoi(args[i + 1].c_str());
    else if (args[i] == "-threads") job->threads = std::atoi(args[i + 1].c_str());
    else if (args[i] == "-av1mi_gpu_entropy") job->gpu_entropy = std::atoi(args[i + 1].c_str()) != 0;
    else if (args[i] == "-av1mi_tracks") job->tracks.push_back(args[i + 1]);
    else if (args[i] == "-av1mi_key_block_size") job->key_block_size = std::atoi(args[i + 1].c_str());
    else if (args[i] == "-av1mi_pack10") job->pack10 = std::atoi(args[i + 1].c_str());
    else if (args[i] == "-av1mi_stats") job->stats_path = args[i + 1];
    else if (args[i] == "-av1mi_format") {
      if (args[i + 1] != "420") { if (err) *err = "Invalid argument: -av1mi_format takes 420 (the only layout that is coded), not " + args[i + 1]; return false; }
      job->to_420 = true;
    }
    else if (args[i] == "-av1mi_lr_search") {
      if (!plain_int(args[i + 1], &job->lr_search) || job->lr_search > 1) { if (err) *err = "Invalid argument: -av1mi_lr_search takes 0 or 1, not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-av1mi_cdef_search") {
      if (!plain_int(args[i + 1], &job->cdef_search) || job->cdef_search > 3) { if (err) *err = "Invalid argument: -av1mi_cdef_search takes 0, 1, 2 or 3, not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-av1mi_lf_search") {
      if (!plain_int(args[i + 1], &job->lf_search) || job->lf_search > 1) { if (err) *err = "Invalid argument: -av1mi_lf_search takes 0 or 1, not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-av1mi_me_range") {
      if (!plain_int(args[i + 1], &job->me_range) || job->me_range > 64 || (job->me_range & 3)) { if (err) *err = "Invalid argument: -av1mi_me_range takes 0 or a multiple of 4 up to 64, not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-av1mi_scenecut") {
      if (!plain_int(args[i + 1], &job->scenecut) || job->scenecut > 99) { if (err) *err = "Invalid argument: -av1mi_scenecut takes a sensitivity 1 .. 99 (0 = off), not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-av1mi_deinterlace") {
      const std::string &v = args[i + 1];
      if (v == "off") job->deinterlace = 0; else if (v == "auto") job->deinterlace = 1; else if (v == "tff") job->deinterlace = 2; else if (v == "bff") job->deinterlace = 3;
      else { if (err) *err = "Invalid argument: -av1mi_deinterlace takes off, auto, tff or bff, not " + v; return false; }
      deint_given = true;
    }
    else if (args[i] == "-av1mi_deinterlace_rate") {
      const std::string &v = args[i + 1];
      if (v == "frame") job->deint_rate = 0; else if (v == "field") job->deint_rate = 1;
      else { if (err) *err = "Invalid argument: -av1mi_deinterlace_rate takes frame or field, not " + v; return false; }
    }
    else if (args[i] == "-av1mi_ivtc") {
      if (args[i + 1] != "0" && args[i + 1] != "1") { if (err) *err = "Invalid argument: -av1mi_ivtc takes 0 or 1, not " + args[i + 1]; return false; }
      job->ivtc = args[i + 1] == "1";
    }
    else if (args[i] == "-av1mi_denoise") {
      job->denoise_auto = args[i + 1] == "auto";
      if (job->denoise_auto) job->denoise = 0;
      else if (!plain_int(args[i + 1], &job->denoise) || job->denoise > 16) { if (err) *err = "Invalid argument: -av1mi_denoise takes a strength 1 .. 16 (0 = off) or auto, not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-av1mi_denoise_range") {
      if (!plain_int(args[i + 1], &job->denoise_range) || (job->denoise_range != 0 && job->denoise_range != 4 && job->denoise_range != 8)) {
        if (err) *err = "Invalid argument: -av1mi_denoise_range takes 0 (off), 4 or 8, not " + args[i + 1];
        return false;
      }
    }
    else if (args[i] == "-av1mi_grain_lag") {
      if (!plain_int(args[i + 1], &job->grain_lag) || job->grain_lag > 3) { if (err) *err = "Invalid argument: -av1mi_grain_lag takes 0 (white grain) .. 3, not " + args[i + 1]; return false; }
      grain_lag_given = true;
    }
    else if (args[i] == "-av1mi_crop") {
      const std::string &v = args[i + 1];
      int n[4];
      std::string why;
      if (v == "off") job->crop_mode = 0; else if (v == "auto") job->crop_mode = 1;
      else if (crop_arguments(v, n, &why) && n[2] >= 0 && n[3] >= 0 && v.find('=') == std::string::npos && (n[0] & ~1) >= 16 && (n[1] & ~1) >= 16) {
        job->crop_mode = 2; job->crop.w = n[0] & ~1; job->crop.h = n[1] & ~1; job->crop.x = n[2] & ~1; job->crop.y = n[3] & ~1;
      } else { if (err) *err = "Invalid argument: -av1mi_crop takes off, auto or W:H:X:Y (plain integers, at least 16x16), not " + v; return false; }
    }
    else if (args[i] == "-av1mi_crop_limit") {
      if (!plain_int(args[i + 1], &job->crop_limit) || job->crop_limit > 255) { if (err) *err = "Invalid argument: -av1mi_crop_limit takes a mean 8-bit level 0 .. 255, not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-av1mi_film_grain") {
      if (args[i + 1] != "0" && args[i + 1] != "1") { if (err) *err = "Invalid argument: -av1mi_film_grain takes 0 or 1, not " + args[i + 1]; return false; }
      job->film_grain = args[i + 1] == "1";
    }
    else if (args[i] == "-av1mi_min_gop") {
      if (!plain_int(args[i + 1], &job->min_gop) || job->min_gop < 1 || job->min_gop > 256) { if (err) *err = "Invalid argument: -av1mi_min_gop takes a length in frames (1 .. gop - gop / 2), not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-av1mi_min_psnr") {
      char *end = nullptr;
      job->min_psnr = std::strtod(args[i + 1].c_str(), &end);
      // a finite bound: nan fails the first comparison, inf (which every lossy file would miss) the second
      if (args[i + 1].empty() || *end || !(job->min_psnr >= 0) || !(job->min_psnr <= 1e308)) { if (err) *err = "Invalid argument: -av1mi_min_psnr takes a finite bound in dB (0 = off), not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-b:v:0" || args[i] == "-b:v") {
      const std::string &v = args[i + 1];
      size_t n = 0;
      long long bits = 0;
      while (n < v.size() && n < 13 && v[n] >= '0' && v[n] <= '9') bits = bits * 10 + (v[n++] - '0');
      const std::string suffix = v.substr(n);
      if (suffix == "k" || suffix == "K") bits *= 1000; else if (suffix == "M") bits *= 1000000;
      if (n == 0 || n > 12 || (!suffix.empty() && suffix != "k" && suffix != "K" && suffix != "M") || bits < 1 || bits > 1000000000000ll) {
        if (err) *err = "Invalid argument: " + args[i] + " takes bits per second (a positive integer, suffix k or M), not " + v;
        return false;
      }
      job->bitrate = bits;
    }
    else if (args[i] == "-av1mi_target_bpp") {
      char *end = nullptr;
      const double x = std::strtod(args[i + 1].c_str(), &end);
      if (args[i + 1].empty() || *end || !(x >= 0.000001) || !(x <= 64)) { if (err) *err = "Invalid argument: -av1mi_target_bpp takes bits per pixel per frame (0.000001 .. 64), not " + args[i + 1]; return false; }
      job->target_bpp_u = std::llround(x * 1e6);
    }
    else if (args[i] == "-qmin" || args[i] == "-qmax") {
      int v = 0;
      if (!plain_int(args[i + 1], &v) || v < 1 || v > 255) { if (err) *err = "Invalid argument: " + args[i] + " takes a quantiser index 1 .. 255, not " + args[i + 1]; return false; }
      (args[i] == "-qmin" ? job->qmin : job->qmax) = v;
    }
    else if (colour_option(args[i], args[i + 1], job, &colour_err)) { if (!colour_err.empty()) { if (err) *err = colour_err; return false; } }
    else if (args[i] == "-av1mi_tonemap") {
      if (args[i + 1] == "off") job->tonemap = 0; else if (args[i + 1] == "bt2390") job->tonemap = 1;
      else { if (err) *err = "Invalid argument: -av1mi_tonemap takes off or bt2390, not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-av1mi_depth") {
      const std::string &v = args[i + 1];
      if (v == "8") job->depth = 8; else if (v == "10") job->depth = 10; else if (v == "source") job->depth = 0; else if (v == "chain") job->depth = -1;
      else { if (err) *err = "Invalid argument: -av1mi_depth takes 8, 10, source or chain, not " + v; return false; }
      depth_given = true;
    }
    else if (args[i] == "-av1mi_dither") {
      if (args[i + 1] == "ordered") job->dither = 1; else if (args[i + 1] == "round") job->dither = 0;
      else { if (err) *err = "Invalid argument: -av1mi_dither takes ordered or round, not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-av1mi_tonemap_peak") {
      job->tonemap_peak_auto = args[i + 1] == "auto";
      if (job->tonemap_peak_auto) job->tonemap_peak = 0;
      else if (!plain_int(args[i + 1], &job->tonemap_peak) || job->tonemap_peak < 100 || job->tonemap_peak > 10000) { if (err) *err = "Invalid argument: -av1mi_tonemap_peak takes cd/m2, 100 .. 10000, or auto, not " + args[i + 1]; return false; }
    }
    else if (args[i] == "-vf:v:0" || args[i] == "-vf") { job->vf = args[i + 1]; job->have_vf = true; }
    else if (args[i] == "-av1mi_scale") {
      const std::string &v = args[i + 1];
      const size_t x = v.find('x');
      if (x == std::string::npos || !plain_int(v.substr(0, x), &job->scale_w) || !plain_int(v.substr(x + 1), &job->scale_h) || job->scale_w < 16 || job->scale_h < 16 ||
          job->scale_w > 4096 || job->scale_h > 4096) {
        if (err) *err = "Invalid argument: -av1mi_scale takes WxH with 16 .. 4096 each, not " + v;
        return false;
      }
    }
  }
  if (job->have_vf) {      // a filter that cannot be applied must not be skipped silently: the chain is checked before anything runs
    int w, h;
    bool to_420 = false, deint = false;
    CropRect chain_crop;
    bool tonemap = false;
    if (!ChainTarget(16, 16, 1, 1, job->vf, &w, &h, nullptr, err, &to_420, &deint, &chain_crop, false, &tonemap)) return false;
    if (tonemap) job->tonemap = 1;
    if (job->crop_mode && job->vf.find("crop=") != std::string::npos) {
      if (err) *err = "Invalid argument: -av1mi_crop together with a crop= filter in the chain: give one";
      return false;
    }
    if (to_420) job->to_420 = true;
    if (deint && !deint_given) job->deinterlace = 1;      // a deinterlacer in the chain means auto; an explicit option keeps its say
    // what the chain's LAST format= names (ChainTarget has refused every name but these five): -av1mi_depth chain reads it
    std::string part;
    bool quoted = false;
    for (size_t k = 0; k <= job->vf.size(); k++) {
      const char c = k < job->vf.size() ? job->vf[k] : ',';
      if (c == '\'') quoted = !quoted;
      if (c != ',' || quoted) { part.push_back(c); continue; }
      if (part.compare(0, 7, "format=") == 0) job->chain_depth = part == "format=nv12" || part == "format=yuv420p" ? 8 : 10;
      part.clear();
    }
  }
  const bool denoises = job->denoise || job->denoise_auto;      // (auto: every refusal of -av1mi_denoise N holds whatever is planned later)
  if (job->dither >= 0 && !depth_given) { if (err) *err = "Invalid argument: -av1mi_dither needs -av1mi_depth: it is the rounding of the depth reduction"; return false; }
  if ((job->tonemap_peak || job->tonemap_peak_auto) && !job->tonemap) { if (err) *err = "Invalid argument: -av1mi_tonemap_peak needs -av1mi_tonemap bt2390 (or tonemap_vaapi in the chain)"; return false; }
  if (job->tonemap) {
    if (denoises) { if (err) *err = "Invalid argument: tone mapping together with -av1mi_denoise is not built: the grain would be measured in the source's light"; return false; }
    const bool src_ok = (job->color_primaries < 0 || job->color_primaries == 2 || job->color_primaries == 9) && (job->color_trc < 0 || job->color_trc == 2 || job->color_trc == 16) &&
                        (job->colorspace < 0 || job->colorspace == 2 || job->colorspace == 9) && job->color_range <= 0;
    if (!src_ok) { if (err) *err = "Invalid argument: tone mapping takes a bt2020 / smpte2084 / bt2020nc / tv source: with it -color_* describe the source, and they say otherwise"; return false; }
  }
  if (job->bitrate && job->target_bpp_u) { if (err) *err = "Invalid argument: -b:v:0 and -av1mi_target_bpp are two forms of one target: give one"; return false; }
  if ((job->qmin || job->qmax) && !job->bitrate && !job->target_bpp_u) { if (err) *err = "Invalid argument: -qmin / -qmax need a target (-b:v:0 or -av1mi_target_bpp)"; return false; }
  if (job->qmin && job->qmax && job->qmin > job->qmax) { if (err) *err = "Invalid argument: -qmin " + std::to_string(job->qmin) + " above -qmax " + std::to_string(job->qmax); return false; }
  if (job->scenecut && job->pack10) { if (err) *err = "Invalid argument: -av1mi_scenecut keeps the group's frames in a planar store on the GPU: not together with -av1mi_pack10 1"; return false; }
  if (job->deinterlace && job->pack10) { if (err) *err = "Invalid argument: -av1mi_deinterlace keeps the group's frames in a planar store on the GPU: not together with -av1mi_pack10 1"; return false; }
  if (job->deint_rate && job->deinterlace && job->gop >= 1 && (job->gop & 1)) {
    if (err) *err = "Invalid argument: with -av1mi_deinterlace_rate field -g counts output frames, two per source frame, and must be even: not -g " + std::to_string(job->gop);
    return false;
  }
  if (job->ivtc) {
    if (job->deinterlace) { if (err) *err = "Invalid argument: -av1mi_ivtc weaves the film frames of a telecined source back together, -av1mi_deinterlace (or a deinterlacer in the chain) filters them: give one"; return false; }
    if (denoises) { if (err) *err = "Invalid argument: -av1mi_ivtc together with -av1mi_denoise is not built: the denoiser's neighbours would be video frames, not the woven film frames"; return false; }
    if (job->pack10) { if (err) *err = "Invalid argument: -av1mi_ivtc keeps the group's frames in a planar store on the GPU: not together with -av1mi_pack10 1"; return false; }
    if (job->scenecut) { if (err) *err = "Invalid argument: -av1mi_ivtc together with -av1mi_scenecut is not built: the cuts of the source frames would have to be mapped through the dropped frames"; return false; }
    if (job->gop >= 1 && (job->gop & 3)) {
      if (err) *err = "Invalid argument: with -av1mi_ivtc -g counts output frames, four per five source frames, and must be a multiple of 4: not -g " + std::to_string(job->gop);
      return false;
    }
  }
  if ((job->crop_mode || (job->have_vf && job->vf.find("crop=") != std::string::npos)) && job->pack10) { if (err) *err = "Invalid argument: a crop window is cut from planar planes on the GPU: not together with -av1mi_pack10 1"; return false; }
  if (job->crop_mode == 1) {      // (a regular file whose frames cannot be addressed is refused when it is opened: backend.cpp)
    struct stat st;
    if (job->input == "-" || job->input == "pipe:0" || (!stat(job->input.c_str(), &st) && !S_ISREG(st.st_mode))) {
      if (err) *err = "Invalid argument: -av1mi_crop auto needs a seekable file: it samples frames from all over the input, not from a pipe or FIFO";
      return false;
    }
  }
  if (job->tonemap_peak_auto) {      // the same rule: a stream's first frames say nothing about its brightest scene
    struct stat st;
    if (job->input == "-" || job->input == "pipe:0" || (!stat(job->input.c_str(), &st) && !S_ISREG(st.st_mode))) {
      if (err) *err = "Invalid argument: -av1mi_tonemap_peak auto needs a seekable file: it samples frames from all over the input, not from a pipe or FIFO";
      return false;
    }
  }
  if (job->denoise_auto) {      // the same rule, for the same reason: a stream's first frames are its opening credits
    struct stat st;
    if (job->input == "-" || job->input == "pipe:0" || (!stat(job->input.c_str(), &st) && !S_ISREG(st.st_mode))) {
      if (err) *err = "Invalid argument: -av1mi_denoise auto needs a seekable file: it samples frame pairs from all over the input, not from a pipe or FIFO";
      return false;
    }
  }
  if (denoises && job->pack10) { if (err) *err = "Invalid argument: -av1mi_denoise keeps the group's frames in a planar store on the GPU: not together with -av1mi_pack10 1"; return false; }
  if (denoises && job->deinterlace) { if (err) *err = "Invalid argument: -av1mi_denoise filters the group's frames on their way from the store, as -av1mi_deinterlace does: not together with -av1mi_deinterlace"; return false; }
  if (job->denoise_range && !denoises) { if (err) *err = "Invalid argument: -av1mi_denoise_range needs -av1mi_denoise"; return false; }
  if (job->film_grain >= 0 && !denoises) { if (err) *err = "Invalid argument: -av1mi_film_grain needs -av1mi_denoise"; return false; }
  if (grain_lag_given && !denoises) { if (err) *err = "Invalid argument: -av1mi_grain_lag needs -av1mi_denoise"; return false; }
  if (grain_lag_given && job->film_grain == 0) { if (err) *err = "Invalid argument: -av1mi_grain_lag shapes the film grain: not together with -av1mi_film_grain 0"; return false; }
  if (job->min_gop && !job->scenecut) { if (err) *err = "Invalid argument: -av1mi_min_gop needs -av1mi_scenecut"; return false; }
  if (job->min_gop && job->gop >= 1 && job->min_gop > job->gop - job->gop / 2) { if (err) *err = "Invalid argument: -av1mi_min_gop " + std::to_string(job->min_gop) + " above gop - gop / 2 = " + std::to_string(job->gop - job->gop / 2); return false; }
  if (!have_in) { if (err) *err = "Invalid argument: no input (-i) given"; return false; }
  if (job->quality < 0 || job->quality > 255 || job->gop < 1 || job->gop > 256 || job->segments < 1 || job->segments > 256 || job->threads < 0 || (job->key_block_size != 8 && job->key_block_size != 32) || (job->pack10 != 0 && job->pack10 != 1)) { if (err) *err = "Invalid argument: quality/gop/key block size/pack10 out of range"; return false; }
  return true;
}

RunResult RunTranscode(const std::string &backendPath, const std::vector<std::string> &args) {
  (void)backendPath;   // the library is linked, there is no child process to locate
  BackendJob job;
  std::string err;
  if (!ParseBackendJob(args, &job, &err)) return { 1, "av1mi failed with exit code 1: " + err };
  BackendReport report;
  const int code = RunBackend(job, &err, &report);
  if (code == 0) return { 0, "", report.denoise };
  if (err.size() > 800) err = err.substr(0, 800) + "...";      // transcode.go:295-297
  if (code < 0) return { -1, "av1mi execution failed: " + err, report.denoise };   // transcode.go:311 (could not run)
  if (code == 3) return { 3, err, report.denoise };                // the quality gate: "quality gate: psnr_y ..." as it is
  return { code, "av1mi failed with exit code " + std::to_string(code) + ": " + err, report.denoise };   // transcode.go:299
}

}  // namespace av1mi_host
