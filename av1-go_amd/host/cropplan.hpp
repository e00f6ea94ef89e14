// cropplan.hpp — from the margins of a sample of frames (include/av1mi.h "bar detection", av1mi_crop_analyse) to the crop window of the
// job (av1mi_gop_config.crop_*): the sibling of sceneplan.hpp.  A pure function in plain C++, exported by libav1mi_host.so as
// av1mi_host_crop_plan; the reference has no counterpart (its filter chain never crops, internal/ffmpeg/transcode.go:92-115).
#pragma once
#include <stdint.h>
#include "../../include/av1mi.h"

namespace av1mi_host {

// -av1mi_crop auto without -av1mi_crop_limit: FFmpeg cropdetect's default limit (a mean 8-bit level)
constexpr int kCropLimitDefault = 24;
constexpr int kCropSampleFrames = 32;      // frames of the file that -av1mi_crop auto analyses, spread evenly (all of a shorter file)

struct CropRect {      // w == 0: no window
  int x = 0, y = 0, w = 0, h = 0;
  bool trims(int fw, int fh) const { return w > 0 && (x || y || w < (fw & ~1) || h < (fh & ~1)); }      // does it cut a margin of a fw x fh picture?
};

// n records of frames of TRUE size w x h -> the window, or none (returns false, *out = {}):
//   1. frames that are dark all over (top == h) say nothing about the bars and are dropped;
//   2. fewer than 2 frames left: no window;
//   3. T, B, L, R = the minima of the four margins over the frames left: a subtitle or a logo inside a bar of ANY sampled frame keeps
//      that part of the bar;
//   4. each is rounded down to even (4:2:0);
//   5. T + B < 8 -> T = B = 0, L + R < 8 -> L = R = 0: less than a row of blocks gains nothing;
//   6. the window is (L, T, w - L - R, h - T - B) with its width and height rounded down to even;
//   7. a result smaller than 16 x 16: no window.
// Without bars the result is the whole picture (its odd last column / row aside): CropRect::trims() tells the caller whether the window
// cuts a margin at all; -av1mi_crop auto takes the path without a window where it does not.
inline bool PlanCrop(const av1mi_crop_record *rec, int n, int w, int h, CropRect *out) {
  *out = CropRect();
  if (!rec || w < 1 || h < 1) return false;
  uint32_t T = 0xFFFFFFFFu, B = T, L = T, R = T;
  int used = 0;
  for (int i = 0; i < n; i++) {
    if (rec[i].top == (uint32_t)h) continue;
    used++;
    if (rec[i].top < T) T = rec[i].top;
    if (rec[i].bottom < B) B = rec[i].bottom;
    if (rec[i].left < L) L = rec[i].left;
    if (rec[i].right < R) R = rec[i].right;
  }
  if (used < 2) return false;
  T &= ~1u; B &= ~1u; L &= ~1u; R &= ~1u;
  if (T + B < 8) T = B = 0;
  if (L + R < 8) L = R = 0;
  const long cw = ((long)w - (long)L - (long)R) & ~1L, ch = ((long)h - (long)T - (long)B) & ~1L;
  if (cw < 16 || ch < 16) return false;
  out->x = (int)L; out->y = (int)T; out->w = (int)cw; out->h = (int)ch;
  return true;
}

}  // namespace av1mi_host
