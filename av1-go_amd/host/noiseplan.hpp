// noiseplan.hpp — from the noise records of a sample of frame pairs (include/av1mi.h "noise records", av1mi_noise_analyse) to the strength
// of the job's denoiser (-av1mi_denoise auto): the sibling of cropplan.hpp.  Pure functions in plain C++, exported by libav1mi_host.so as
// av1mi_plan_denoise; the reference has no counterpart (its encoder child never denoises, internal/ffmpeg/transcode.go:120).  The rules
// are the header's "the plan"; restated in numpy by tests/noise_ref.py.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/av1mi.h"

namespace av1mi_host {

constexpr int kNoiseSamplePairs = 16;      // pairs of consecutive frames that -av1mi_denoise auto analyses, spread evenly (all of a shorter file)
constexpr int kNoiseBins = 256;            // of a record's histogram; the last one holds "16 codes or more": motion, never counted
// The floor, in 1/16 of an 8-bit code: a sigma under half a code plans no denoiser.  A decision, not a derivation: rounding to 8 bits alone
// gives a sigma of 0.29, and a filter (with its frame store and its grain synthesis) that chases that gains nothing.
constexpr int kNoiseFloorS16 = 8;

// the pair slots of the sample in a file of n frames: P = min(16, floor(n / 2)) pairs; pair i is frames 2 s, 2 s + 1 with
// s = floor(i (floor(n / 2) - 1) / max(P - 1, 1))
inline int NoiseSamplePairs(long n) { return (int)std::min<long>(kNoiseSamplePairs, n < 0 ? 0 : n / 2); }
inline long NoisePairSlot(int i, long n) {
  const int P = NoiseSamplePairs(n);
  return (long)i * (n / 2 - 1) / std::max(P - 1, 1);
}

// a pair's level: the lower quartile of its counted blocks' bins, or -1 for a pair that is not valid
inline int NoisePairLevel(const av1mi_noise_record &r) {
  uint64_t counted = 0;
  for (int b = 0; b < kNoiseBins - 1; b++) counted += r.hist[b];
  if (counted < 1 || 4 * counted < r.eligible || r.eligible < r.blocks / 16) return -1;
  const uint64_t want = (counted + 3) / 4;
  uint64_t seen = 0;
  for (int b = 0; b < kNoiseBins - 1; b++)
    if ((seen += r.hist[b]) >= want) return b;
  return kNoiseBins - 2;      // (not reached: the bins sum to counted)
}

// sigma in 1/16 code from a level: the mean |difference| of two independent noises of sigma is 2 sigma / sqrt(pi) = 1.128 sigma, and
// 227 / 256 = 1 / 1.128
inline int NoiseSigma16(int q) { return (227 * q + 128) >> 8; }

// The strength for a sigma: ceil(1.5 sigma), 0 under the floor, 16 at most.  The 1.5 is derived from the filter (include/av1mi.h
// "denoising"), not tuned: a neighbour's weight is w_F = 16 - floor(16 MAD / (3 T)), and the filter counts a sample as grain iff
// w_P + w_N >= 24, that is w >= 12 per neighbour, that is 16 MAD / (3 T) <= 4.  A still sample under noise of sigma has MAD = 1.128 sigma:
// T >= 1.5 sigma.  So this is the smallest strength at which a still, noisy sample is on average counted as grain.
inline int NoiseStrength(int s16) { return s16 < kNoiseFloorS16 ? 0 : std::min(16, (3 * s16 + 31) >> 5); }

// n records -> the strength 0 .. 16 (no valid pair: 0), or -1 for arguments outside these rules.  pair_q (may be null): n entries, each
// pair's level or -1; s16 (may be null): the file's sigma in 1/16 code, -1 without a valid pair.
inline int PlanDenoise(const av1mi_noise_record *rec, int n, int32_t *pair_q, int32_t *s16) {
  if (n < 0 || (n > 0 && !rec)) return -1;
  std::vector<int> q;
  for (int i = 0; i < n; i++) {
    const int l = NoisePairLevel(rec[i]);
    if (pair_q) pair_q[i] = l;
    if (l >= 0) q.push_back(l);
  }
  if (s16) *s16 = -1;
  if (q.empty()) return 0;
  std::sort(q.begin(), q.end());
  const int s = NoiseSigma16(q[(q.size() - 1) / 4]);      // noise is the file's; motion in some pairs only adds to it
  if (s16) *s16 = s;
  return NoiseStrength(s);
}

}  // namespace av1mi_host
