// fieldrate.hpp — what -av1mi_deinterlace_rate field changes on the host, as pure functions: how many output frames a source frame
// becomes, the output's frame rate and frame count, and where the scene cuts of the source lie among the output frames.  EVERY place that
// needs the job's output rate or count (the sink's header and timecodes, the rate controller's bytes per frame, the report's bits per
// pixel, the number of segments) asks JobOutputOf; nothing else doubles a rate.  Exported for the CPU tests by capi_host.cpp.
#pragma once
#include <stdint.h>
#include "transcode.hpp"

namespace av1mi_host {

// output frames per source frame: 2 where the job asks for field rate AND deinterlaces this source (interlace: the Y4M header's I
// parameter as Y4mSource keeps it, 0 progressive, 1 It, 2 Ib, 3 Im), else 1.  `field` has no meaning where nothing is deinterlaced:
// -av1mi_deinterlace off, or auto on a progressive source, run as they always have.
inline int OutputPerSource(const BackendJob &job, int interlace) {
  const bool deinterlaces = job.deinterlace >= 2 || (job.deinterlace == 1 && (interlace == 1 || interlace == 2));
  return job.deint_rate == 1 && deinterlaces ? 2 : 1;
}

// the job's output: its frame rate (not reduced: 30000/1001 becomes 60000/1001, as a file written at twice the rate says it) and its
// frame count (-1 = a stream, unknown), from the source's
struct JobOutput { int per_source, fps_n, fps_d; long frames; };
inline JobOutput JobOutputOf(const BackendJob &job, int interlace, int fps_n, int fps_d, long source_frames) {
  const int k = OutputPerSource(job, interlace);
  return { k, fps_n * k, fps_d, source_frames < 0 ? -1 : source_frames * k };
}

// n source frames' cut flags -> 2 n output frames': output 2 f is a cut iff source f is; output 2 f + 1 (the second field of the same
// frame) never is
inline void FieldRateCuts(const uint8_t *cut, long n, uint8_t *out) {
  for (long f = 0; f < n; f++) { out[2 * f] = cut[f] ? 1 : 0; out[2 * f + 1] = 0; }
}

}  // namespace av1mi_host
