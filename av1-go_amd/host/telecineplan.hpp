// telecineplan.hpp — from the field-match records of a run of frames (include/av1mi.h "inverse telecine", av1mi_telecine_analyse /
// av1mi_gop_store_telecine) to the woven output: which frames are dropped and which two frames every kept one is woven from.  Pure
// functions, exported for the CPU tests by capi_host.cpp (av1mi_plan_telecine); the reference has no counterpart (its encoder child
// deinterlaces or not, internal/ffmpeg/transcode.go:120).  The rules are the header's "the plan"; restated in numpy by tests/telecine_ref.py.
#pragma once
#include <stdint.h>
#include "../../include/av1mi.h"

namespace av1mi_host {

// the cadence: of every 5 source frames 4 are output
constexpr int kTelecineCycle = 5;

// outputs of n source frames: n - floor(n / 5); a negative n (unknown) stays negative
inline long TelecineOutputs(long n) { return n < 0 ? n : n - n / kTelecineCycle; }

// the match of a frame: 0 = p (the frame before), 1 = c, 2 = n: the smallest comb, ties to the earlier in the order c, p, n
inline int TelecineMatch(const av1mi_telecine_record &r) {
  int best = 1;
  if (r.comb[0] < r.comb[best]) best = 0;
  if (r.comb[2] < r.comb[best]) best = 2;
  return best;
}

// The plan of a run of `frames` records whose first `front` and last `back` (0 or 1 each) are context.  The n = frames - front - back own
// frames give n - n / 5 outputs: top[k] / bottom[k] = the positions IN THE RUN (context included) of output k's top and bottom source.
// Returns the number of outputs, or -1 for arguments outside these rules.  top and bottom hold n - n / 5 entries.
inline int PlanTelecine(const av1mi_telecine_record *rec, int frames, int front, int back, int32_t *top, int32_t *bottom) {
  if (!rec || !top || !bottom || front < 0 || front > 1 || back < 0 || back > 1 || frames < front + back) return -1;
  const int n = frames - front - back;
  int out = 0;
  for (int c0 = 0; c0 < n; c0 += kTelecineCycle) {
    const int len = n - c0 < kTelecineCycle ? n - c0 : kTelecineCycle;
    int drop = -1;
    if (len == kTelecineCycle) {
      drop = 0;
      for (int i = 1; i < len; i++)
        if (rec[front + c0 + i].bdiff < rec[front + c0 + drop].bdiff) drop = i;
    }
    for (int i = 0; i < len; i++) {
      if (i == drop) continue;
      const int f = front + c0 + i;
      int t = f + TelecineMatch(rec[f]) - 1;
      t = t < 0 ? 0 : t > frames - 1 ? frames - 1 : t;
      top[out] = t; bottom[out] = f;
      out++;
    }
  }
  return out;
}

}  // namespace av1mi_host
