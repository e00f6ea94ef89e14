// filmgrain.hpp — from grain records to film grain parameters (include/av1mi_filmgrain.h av1mi_film_grain_from_records, and
// av1mi_film_grain_from_records_ar for coloured grain): plain host code.
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
//
// Coloured grain (FilmGrainFromRecordsAr, lag 1 .. 3): everything above, plus the autoregressive filter a decoder runs over its unit-variance
// template (spec 7.18.3.3), so that the synthesised grain has the SIZE of the removed one.  From the plane's grain covariance
// (include/av1mi.h "grain covariance": cov[dy][dx + 6], the residual's products with its neighbours), per plane:
//   rho       rho(d) = cov(d) / cov(0), rho(-d) = rho(d).  Only ratios: samples filtered with part of the weight scale both alike.  (The
//             sum at offset d runs over (w - |dx|)(h - dy) pairs where cov(0) runs over w h: below 1 % at 640 x 360, not corrected.)
//   equations the neighbours n_0 .. n_(N-1) in the spec's order for the lag l: rows -l .. 0, columns -l .. l, stopping before (0, 0); N =
//             2 l (l + 1).  Yule-Walker: sum_j a_j rho(n_i - n_j) = rho(n_i), differences up to (+-2 l, +-l): what the covariance holds for
//             l <= 3.  Solved in doubles by elimination with partial pivoting, with the ridge kArRidge = 1e-3 on the diagonal (a measured
//             rho is noisy, and 24 near-dependent neighbours of smooth grain make the plain system ill-conditioned).
//   shift     ONE ar_coeff_shift_minus_6 for the three planes: the largest shift in 6 .. 9 at which every round(a 2^shift) lies in
//             -128 .. 127; coded as that + 128.  A plane whose coefficients do not fit at shift 6 falls back (below).
//   gain      G = the sum of h^2 over the impulse response of the QUANTISED filter, h(0, 0) = 1, h(x, y) = sum_i c_i 2^-shift h((x, y) + n_i),
//             run in raster order over y = 0 .. 32, x = -32 .. 32 (rows above reach to BOTH sides, so it is a half plane, 33 x 65).  The
//             decoder filters a unit-variance template: AR filtering raises its variance by G, so the plane's scaling values are divided
//             by sqrt(G) and the total variance stays what the records say.
//   template  G is the gain of the ideal filter.  The decoder does not run that: it fills a template of 73 x 82 values (38 x 44 for
//             subsampled chroma) with white Gaussian values of standard deviation 31.7 in 8-bit terms (kTemplateSigma = kGainLuma x 512),
//             runs the recursion over it in place from row 3 and column 3 on, with the sum rounded at the shift, and CLIPS every value
//             to -128 .. 127 (4 deviations of the white template, 4 / sqrt(G) of the filtered one's) before the next value reads it;
//             blocks are then cut from row and column 9 (6 for chroma) on.  A Gaussian estimate of the clip alone left the regenerated
//             deviation 6.5 % short at G = 4.45, because clipped values re-enter the recursion.  So ArTemplateGain RUNS that procedure:
//             kTemplateRuns = 16 templates (48 of the chroma size) from a fixed xorshift / Box-Muller source, made once, the variance of the
//             region blocks are cut from after the recursion over the variance before it.  Deterministic; the estimate's standard
//             error is about 1 % of the gain (some 70 000 correlated samples), half of that in the deviation.  At G = 4.45 it gives
//             3.7; the divisor of the scaling values is its square root.  10 bits scale template and clip alike: the same number.
//   scaling   a value divided by 2 is a number of 30 where the white one was 60, and its step twice the share.  Where every value of the
//             three planes stays below 255 when doubled, grain_scaling_minus_8 is 2 and the values are doubled (the decoder's gain
//             halves exactly with every step of that shift: "gain" at the top); else it stays 1.
//   fall back plane by plane to the next smaller lag, finally to white grain (lag 0, G = 1), where cov(0) is 0, the plane's records hold
//             fewer than kMinCount samples, a coefficient does not fit, G is not finite, exceeds kArMaxGain = 8 (the clip then sits
//             at 1.4 deviations and takes more than a quarter of the variance), or more than 1e-3 of it lies outside |x| <= 16, y <= 16 (it does not converge).
//             The coded ar_coeff_lag is the largest of the planes' lags; a plane of a smaller lag has zeros outside its own neighbourhood.
//   chroma    its own covariance and coefficients; the extra coefficient, the luma grain's share, stays 0 (coded 128).
//   limit     what the covariance holds beside grain (a slow change of the picture that the filter half removes) colours the result.
#pragma once
#include "../../include/av1mi_filmgrain.h"

namespace av1mi_host {
constexpr double kResidualToGrain = 1.224744871391589;      // sqrt(3 / 2)
constexpr double kGainLuma = 0.0619, kGainChroma = 0.0650;   // per unit of scaling at grain_scaling_minus_8 = 1, in 8-bit code values
constexpr unsigned kMinCount = 256;                          // samples a bin (luma) or a plane (chroma) must hold
// records: the frame's three records [plane]; false for a null pointer or a bit depth other than 8 or 10
bool FilmGrainFromRecords(const av1mi_grain_record *records, int bit_depth, int frame_index, av1mi_film_grain *out);
// the same with coloured grain: cov = the frame's three covariance records [plane], lag 0 .. 3 the largest lag coded (0 = the function
// above, byte for byte); false also for a null cov or a lag outside 0 .. 3
constexpr double kArRidge = 1e-3, kArMaxGain = 8.0, kTemplateSigma = 31.7;
constexpr int kTemplateRuns = 16;
bool FilmGrainFromRecordsAr(const av1mi_grain_record *records, const av1mi_grain_cov_record *cov, int bit_depth, int frame_index, int lag, av1mi_film_grain *out);
// the pieces, for the tests: the real-valued coefficients of one plane at one lag in the spec's order (false: cov(0) is 0 or the system is
// singular), and the gain of quantised coefficients (c_i, not + 128) at a shift (a negative value: it does not converge)
bool ArSolve(const av1mi_grain_cov_record &cov, int lag, double *a);
double ArGain(const int *c, int lag, int shift);
// the variance gain of the decoder's own template procedure ("template" above); chroma: the template of a subsampled plane
double ArTemplateGain(const int *c, int lag, int shift, bool chroma);
// the luma scaling function at mid grey (8-bit value 128), 0 when the frame gets no grain: the stats file's grain: field
int FilmGrainMidGrey(const av1mi_film_grain &g);
}  // namespace av1mi_host
