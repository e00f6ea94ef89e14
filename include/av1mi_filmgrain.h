/* av1mi_filmgrain.h — film grain on the host side of libav1mi_host.so: grain records (include/av1mi.h "grain records") -> the
 * av1mi_film_grain of include/av1mi_host.h, and the session's temporal unit with such parameters in its frame header.  Plain C. */
#ifndef AV1MI_FILMGRAIN_H
#define AV1MI_FILMGRAIN_H
#include "av1mi_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* av1mi_session_temporal_unit (include/av1mi_host.h) with film grain: film_grain_present = what the stream's sequence header says (it is written from it when with_sequence_header
 * is set), film_grain = this frame's parameters or NULL (apply_grain = 0), as av1mi_obu_frame's fields of those names.  0 / NULL gives
 * av1mi_session_temporal_unit's bytes. */
long long av1mi_session_temporal_unit_grain(const av1mi_gop_frame *fr, int seg, int width, int height, int bit_depth, int visible_width,
                                            int visible_height, int with_sequence_header, int threads, int film_grain_present,
                                            const av1mi_film_grain *film_grain, uint8_t *out, long long cap, char *err, int errcap);

/* Film grain parameters from the grain records of ONE frame (include/av1mi.h "grain records": records[plane], e.g. av1mi_gop_frame.grain +
 * segment * 3): luma scaling points from the bins that hold enough samples, a constant function per chroma plane, white grain, a seed
 * derived from frame_index; apply_grain = 0 where the luma record gives no point.  The model and the measured decoder gain are in
 * av1-go_amd/host/filmgrain.hpp.  bit_depth 8 or 10.  0 = OK, -1 = bad argument. */
int av1mi_film_grain_from_records(const av1mi_grain_record *records, int bit_depth, int frame_index, av1mi_film_grain *out);
/* The same with COLOURED grain: cov = the frame's three covariance records (include/av1mi.h "grain covariance": cov[plane], e.g.
 * av1mi_gop_frame.grain_cov + segment * 3); lag 0 .. 3 = the largest ar_coeff_lag coded.  Per plane the autoregressive coefficients that
 * give the synthesised grain the removed grain's normalised covariance (Yule-Walker over the spec's neighbour order), one
 * ar_coeff_shift_minus_6 for the three planes, and the scaling points divided by the square root of the quantised filter's variance gain,
 * so that the total variance stays what the records say; a plane falls back to a smaller lag and finally to white grain where its
 * covariance is empty or the filter would be unstable.  lag 0 gives av1mi_film_grain_from_records' bytes.  The model is in
 * av1-go_amd/host/filmgrain.hpp.  0 = OK, -1 = bad argument. */
int av1mi_film_grain_from_records_ar(const av1mi_grain_record *records, const av1mi_grain_cov_record *cov, int bit_depth, int frame_index, int lag,
                                     av1mi_film_grain *out);
/* the luma scaling value at mid grey of a set of parameters (0 = no grain): the stats file's grain: field */
int av1mi_film_grain_mid_grey(const av1mi_film_grain *g);

#ifdef __cplusplus
}
#endif
#endif /* AV1MI_FILMGRAIN_H */
