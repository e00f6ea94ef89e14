// fieldrate.hpp — what -av1mi_deinterlace_rate field and -av1mi_ivtc change on the host, as pure functions: how many output frames a
// source frame becomes, the output's frame rate and frame count, and where the scene cuts of the source lie among the output frames.
// EVERY place that needs the job's output rate or count (the sink's header and timecodes, the rate controller's bytes per frame, the
// report's bits per pixel, the number of segments, the size of the store) asks JobOutputOf; nothing else doubles a rate or drops a fifth
// of a count.  Exported for the CPU tests by capi_host.cpp.
#pragma once
#include <stdint.h>
#include "telecineplan.hpp"
#include "transcode.hpp"

namespace av1mi_host {

// output frames per source frame: 2 where the job asks for field rate AND deinterlaces this source (interlace: the Y4M header's I
// parameter as Y4mSource keeps it, 0 progressive, 1 It, 2 Ib, 3 Im), else 1.  `field` has no meaning where nothing is deinterlaced:
// -av1mi_deinterlace off, or auto on a progressive source, run as they always have.
inline int OutputPerSource(const BackendJob &job, int interlace) {
  const bool deinterlaces = job.deinterlace >= 2 || (job.deinterlace == 1 && (interlace == 1 || interlace == 2));
  return job.deint_rate == 1 && deinterlaces ? 2 : 1;
}

// the job's output: its frame rate and its frame count (-1 = a stream, unknown), from the source's, and the RATIO num output frames per
// den source frames that both follow.  Field rate: 2 / 1, the rate not reduced (30000/1001 becomes 60000/1001, as a file written at
// twice the rate says it), per_source 2.  Inverse telecine (-av1mi_ivtc 1, whatever the header's I parameter says): 4 / 5, the rate
// fps_n * 4 / (fps_d * 5) REDUCED (30000/1001 becomes 24000/1001), the count n - floor(n / 5) (telecineplan.hpp: a tail of fewer than 5
// frames drops none), per_source 1.  Else 1 / 1.
struct JobOutput { int per_source, fps_n, fps_d; long frames; int num, den; };
inline JobOutput JobOutputOf(const BackendJob &job, int interlace, int fps_n, int fps_d, long source_frames) {
  if (job.ivtc) {
    long long n = (long long)fps_n * (kTelecineCycle - 1), d = (long long)fps_d * kTelecineCycle, a = n, b = d;
    while (b) { const long long t = a % b; a = b; b = t; }
    if (a > 1) { n /= a; d /= a; }
    return { 1, (int)n, (int)d, TelecineOutputs(source_frames), kTelecineCycle - 1, kTelecineCycle };
  }
  const int k = OutputPerSource(job, interlace);
  return { k, fps_n * k, fps_d, source_frames < 0 ? -1 : source_frames * k, k, 1 };
}

// n source frames' cut flags -> 2 n output frames': output 2 f is a cut iff source f is; output 2 f + 1 (the second field of the same
// frame) never is
inline void FieldRateCuts(const uint8_t *cut, long n, uint8_t *out) {
  for (long f = 0; f < n; f++) { out[2 * f] = cut[f] ? 1 : 0; out[2 * f + 1] = 0; }
}

}  // namespace av1mi_host
