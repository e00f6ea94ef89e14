// peakplan.hpp — from the peak records of a sample of frames (include/av1mi.h "peak records", av1mi_peak_analyse) to the source peak of
// the job's tone map (-av1mi_tonemap_peak auto): the sibling of cropplan.hpp and noiseplan.hpp.  Pure functions in plain C++, exported by
// libav1mi_host.so as av1mi_plan_peak; the reference has no counterpart (its encoder child takes the peak from the container's metadata).
// The rules are the header's "the plan"; restated in numpy by tests/peak_ref.py.
#pragma once
#include <stdint.h>
#include <algorithm>
#include "../../include/av1mi.h"

namespace av1mi_host {

constexpr int kPeakSampleFrames = 32;      // frames of the file that -av1mi_tonemap_peak auto analyses: the crop sampler's number and slots
constexpr int kPeakBins = 1024;            // of a record's histogram: the 10-bit PQ codes of max(R', G', B')
// POLICY, not measurements (tuning on real footage: DESIGN section 7, item 0):
constexpr int kPeakSkipShift = 14;         // a frame's brightest pixels >> 14 of it (0.006 %) are let go: specular glints, hot pixels
constexpr int kPeakFloor = 400;            // cd/m2: no peak is planned below it (the low end of the range "tone mapping" bounds gain[] over)
constexpr int kPeakCap = 10000;            // cd/m2: PQ's own

// the frames of the sample in a file of n frames: P = min(32, n) of them, frame i of the sample is floor(i n / P)
inline int PeakSampleFrames(long n) { return (int)std::min<long>(kPeakSampleFrames, n < 0 ? 0 : n); }
inline long PeakSampleSlot(int i, long n) { return (long)i * n / std::max(PeakSampleFrames(n), 1); }

// a frame's code: the largest c with hist[c] + .. + hist[1023] > pixels >> 14, or 0 if there is none
inline int PeakFrameCode(const av1mi_peak_record &r) {
  const uint64_t skip = r.pixels >> kPeakSkipShift;
  uint64_t above = 0;
  for (int c = kPeakBins - 1; c > 0; c--)
    if ((above += r.hist[c]) > skip) return c;
  return 0;
}

// cd/m2 from a code: lin[] is in 2^-8 cd/m2, rounded up, then the floor and the cap
inline int PeakOfCode(int code, const uint32_t lin[1024]) { return (int)std::min<uint64_t>(std::max<uint64_t>(((uint64_t)lin[code] + 255) >> 8, kPeakFloor), kPeakCap); }

// n records -> the peak in cd/m2 (400 .. 10000), or -1 for arguments outside these rules (n < 1, no records or table, a record without
// pixels).  frame_code (may be null): n entries, every frame's code.
inline int PlanPeak(const av1mi_peak_record *rec, int n, const uint32_t lin[1024], int32_t *frame_code) {
  if (n < 1 || !rec || !lin) return -1;
  int C = 0;
  for (int i = 0; i < n; i++) {
    if (!rec[i].pixels) return -1;
    const int c = PeakFrameCode(rec[i]);
    if (frame_code) frame_code[i] = c;
    C = std::max(C, c);      // the brightest scene's: a maximum, not a quantile over frames
  }
  return PeakOfCode(C, lin);
}

}  // namespace av1mi_host
