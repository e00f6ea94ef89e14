// filmgrain.hpp — from grain records to film grain parameters (include/av1mi_filmgrain.h av1mi_film_grain_from_records): plain host code.
//
// The denoising gather (include/av1mi.h "denoising") leaves, per frame and plane, 16 bins by output intensity of the squared residual
// r = C - out over the samples that stood still.  This turns one frame's three records into the film_grain_params a decoder needs to put
// statistically equal grain back (AV1 spec 5.9.30 / 7.18.3).
//
//   model     with both weights at 16, out = (C + P + N) / 3 and r = (2 C - P - N) / 3: for independent grain of variance s^2 per frame
//             the residual holds (4 + 1 + 1) / 9 = 2/3 of it, so s = rms(r) * sqrt(3 / 2) (kResidualToGrain).  Counted samples with
//             smaller weights hold less (weights 12, 12: 0.54): the estimate leans low; the closed loop of tests/test_filmgrain_stream.py
//             measures by how much.
//   gain      a decoder adds noise = (scaling x grain) >> (8 + grain_scaling_minus_8) with its own Gaussian table.  MEASURED with dav1d
//             1.5.3 on a flat grey 256x256 key frame with a constant scaling function (white grain, overlap on), standard deviation of
//             (grain on - grain off): luma 19.81 at scaling 160, shift 8, 8 bit; 9.906 at shift 9; 79.25 and 39.63 at 10 bit; chroma
//             10.39 / 10.15 at shift 9.  So at grain_scaling_minus_8 = 1, which this file always codes (scaling 255 reaches s = 15.8
//             in 8-bit terms, one step is 0.062), s_out = kGainLuma x scaling x 2^(bit_depth - 8) with kGainLuma = 0.0619, and
//             kGainChroma = 0.0650 (mean of the two planes).
//   luma      a point per bin that holds at least kMinCount samples, at the bin's centre (16 i + 8 in the 8-bit terms of point_y_value),
//             scaling = round(rms * sqrt(3/2) / (gain * 2^(bit_depth - 8))), clamped to 255.  The decoder interpolates between points and
//             holds the first and last value outside them: an empty bin takes its neighbours' values that way.  More than 14 such bins:
//             the ones with the fewest samples are dropped.
//   chroma    one constant function per plane from the plane's total (two points, 0 and 255), where the total holds kMinCount samples;
//             cb_mult = cr_mult = 192, luma_mult = 128, offset = 256: the index of the scaling function is the chroma sample itself
//             (spec 7.18.3.5: (luma x (128 - 128) + chroma x (192 - 128)) >> 6, + (256 - 256)) — immaterial for a constant function.
//   fixed     ar_coeff_lag 0 (white grain; the one chroma coefficient, the luma grain's share, 0), ar_coeff_shift_minus_6 0,
//             grain_scale_shift 0, overlap_flag 1, chroma_scaling_from_luma 0, clip_to_restricted_range 0.
//   seed      grain_seed = ((frame_index + 1) x 40503) mod 65536: an odd multiplier, so 65536 consecutive frames get distinct seeds.
//   no grain  no luma point (an end of a run, a flat slot, a moving picture): apply_grain = 0; 4:2:0 allows no chroma points without luma.
#pragma once
#include "../../include/av1mi_filmgrain.h"

namespace av1mi_host {
constexpr double kResidualToGrain = 1.224744871391589;      // sqrt(3 / 2)
constexpr double kGainLuma = 0.0619, kGainChroma = 0.0650;   // per unit of scaling at grain_scaling_minus_8 = 1, in 8-bit code values
constexpr unsigned kMinCount = 256;                          // samples a bin (luma) or a plane (chroma) must hold
// records: the frame's three records [plane]; false for a null pointer or a bit depth other than 8 or 10
bool FilmGrainFromRecords(const av1mi_grain_record *records, int bit_depth, int frame_index, av1mi_film_grain *out);
// the luma scaling function at mid grey (8-bit value 128), 0 when the frame gets no grain: the stats file's grain: field
int FilmGrainMidGrey(const av1mi_film_grain &g);
}  // namespace av1mi_host
