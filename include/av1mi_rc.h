/*
 * av1mi_rc.h — the one-pass rate controller of libav1mi_host.so (part of the C ABI of include/av1mi_host.h, which includes this
 * file).  Feedback only: it is told which batch comes next and how many bytes the oldest batch in flight turned out to have, and
 * answers with the quantiser of the next batch (av1mi.h av1mi_gop_set_base_q_idx: one quantiser per batch, all segments share it).
 * No GPU, no floating point, no clock: the q sequence is a function of the calls alone.
 *
 * Arithmetic (normative: tests/ratecontrol_ref.py restates it from this text and must give the same q sequence).  Every quantity is
 * an exact integer (the inputs are 64-bit); fdiv(a, b) = floor(a / b) for b > 0, also for negative a; clamp(v, lo, hi) = lo where v < lo, hi
 * where v > hi, else v.  Frame types: 0 key, 1 P.
 *   step(q)   = av1mi_rc_qstep(q, bit_depth): the AC quantiser step of q (csrc/qtables.hpp, av1mi.h av1mi_ac_q).
 *   target    = num / den bytes per frame, reduced by their greatest common divisor at open.
 *   State     X[0], X[1] (complexity: bytes x step per frame) and seen[0], seen[1] (false); debt (0; in units of 1 / den bytes:
 *             bytes x den - frames x num); last_q (start_q); a queue of the batches in flight, oldest first, each (type, frames, q, share).
 *   av1mi_rc_next_q(type k, frames n):
 *     window = window_gops x G x n                                 (frames; G = gop_length)
 *     if not seen[0], or G > 1 and not seen[1]:  q = start_q
 *     else
 *       debt    = clamp(debt, -window x num, window x num)         (no wind-up beyond one window of the target)
 *       allowed = clamp(num - fdiv(debt, window), fdiv(num x band_low_pct, 100), fdiv(num x band_high_pct, 100))
 *       bytes   = fdiv(allowed, den)                               (the allowed average bytes per frame over the coming window)
 *       q       = the smallest c in qmin .. qmax with  X[0] + (G - 1) x X[1] <= bytes x G x step(c);  qmax if there is none
 *       q       = clamp(clamp(q, last_q - max_step, last_q + max_step), qmin, qmax)
 *     share = seen[k] ? fdiv(X[k] x n, step(q)) x den - n x num : 0   (the batch counts with its PREDICTED bytes while in flight)
 *     debt += share;  the batch (k, n, q, share) joins the queue;  last_q = q;  q is returned.
 *   av1mi_rc_collected(bytes b): the oldest batch (k, n, q, share) leaves the queue;
 *     debt += b x den - n x num - share                            (the prediction is replaced by the truth)
 *     obs   = fdiv(b x step(q), n)
 *     X[k]  = seen[k] ? fdiv(X[k] x (weight_den - weight_num) + obs x weight_num, weight_den) : obs;   seen[k] = true.
 * Ranges checked at open (products of these stay far inside the 128-bit integers host/ratecontrol.cpp computes in): num, den >= 1, after reduction den <= 2^24 and num < 2^31 x den;
 * 1 <= gop_length <= 4096; 1 <= qmin <= start_q <= qmax <= 255; bit_depth 8 or 10; 1 <= weight_num <= weight_den <= 256;
 * 1 <= window_gops <= 64; 1 <= band_low_pct <= 100 <= band_high_pct <= 400; 1 <= max_step <= 255.  Per call: 1 <= frames <= 4096,
 * 0 <= bytes < 2^36, at most 64 batches in flight.
 */
#ifndef AV1MI_RC_H
#define AV1MI_RC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct av1mi_rc_params {
  int64_t target_num, target_den;   /* the target in bytes per frame as an exact rational: bits per second / 8 / frames per second */
  int32_t gop_length;               /* frames per closed GOP (one key frame, gop_length - 1 P frames) */
  int32_t start_q;                  /* returned until both frame types have been observed (the job's -global_quality) */
  int32_t qmin, qmax;               /* defaults 1 / 255 */
  int32_t bit_depth;                /* 8 or 10: selects the step table */
  /* tuning (av1mi_rc_defaults; chosen with tools/bench_ratecontrol.py) */
  int32_t weight_num, weight_den;   /* the moving average's weight of a new observation */
  int32_t window_gops;              /* the window over which a debt is to be repaid, in GOPs of the batch's width */
  int32_t band_low_pct, band_high_pct;   /* the allowed average stays within these percentages of the target */
  int32_t max_step;                 /* largest change of q from one batch to the next */
} av1mi_rc_params;

typedef struct av1mi_rc av1mi_rc;

/* fills qmin / qmax and the tuning values with their defaults; the target, gop_length, start_q and bit_depth are the caller's */
void av1mi_rc_defaults(av1mi_rc_params *p);
/* the AC quantiser step the model uses; 0 for q outside 0..255 or a bit depth other than 8 / 10 */
int av1mi_rc_qstep(int q, int bit_depth);
/* 0 and *out, or -1 (invalid parameters: see "Ranges") with the reason in err (when given; at most errcap bytes) */
int av1mi_rc_open(const av1mi_rc_params *p, av1mi_rc **out, char *err, int errcap);
/* before each submit: the quantiser of the next batch (frame_type 0 key / 1 P, frames_in_batch = the segments that exist); the batch
 * is in flight from here on.  -1 on a bad argument or a full queue */
int av1mi_rc_next_q(av1mi_rc *rc, int frame_type, int frames_in_batch);
/* the oldest batch in flight has been collected: bytes = the sum of its temporal units over the segments that exist.  0, or -1 */
int av1mi_rc_collected(av1mi_rc *rc, int64_t bytes);
void av1mi_rc_close(av1mi_rc *rc);

#ifdef __cplusplus
}
#endif
#endif
