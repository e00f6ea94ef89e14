// ratecontrol.cpp — see ratecontrol.hpp; every line of NextQ / Collected is a line of "Arithmetic" in include/av1mi_rc.h.
#include "ratecontrol.hpp"
#include <cstdio>
#include <cstring>
#include <new>
#include <numeric>
#include "../csrc/qtables.hpp"

namespace av1mi_host {

static int qstep(int q, int bd) {
  if (q < 0 || q > 255 || (bd != 8 && bd != 10)) return 0;
  return bd == 8 ? av1mi::k_ac_q8[q] : av1mi::k_ac_q10[q];
}

const char *RateControl::ParamError(const av1mi_rc_params &p) {
  if (p.target_num < 1 || p.target_den < 1) return "the target must be positive";
  const long long g = std::gcd((long long)p.target_num, (long long)p.target_den), num = p.target_num / g, den = p.target_den / g;
  if (den > (1ll << 24) || (I)num >= ((I)1 << 31) * den) return "the target (bytes per frame) needs a denominator up to 2^24 and a value below 2^31";
  if (p.gop_length < 1 || p.gop_length > 4096) return "gop_length must lie in 1..4096";
  if (p.bit_depth != 8 && p.bit_depth != 10) return "bit_depth must be 8 or 10";
  if (p.qmin < 1 || p.qmax > 255 || p.qmin > p.qmax) return "qmin / qmax must satisfy 1 <= qmin <= qmax <= 255";
  if (p.start_q < p.qmin || p.start_q > p.qmax) return "start_q must lie in qmin..qmax";
  if (p.weight_num < 1 || p.weight_num > p.weight_den || p.weight_den > 256) return "the averaging weight must satisfy 1 <= weight_num <= weight_den <= 256";
  if (p.window_gops < 1 || p.window_gops > 64) return "window_gops must lie in 1..64";
  if (p.band_low_pct < 1 || p.band_low_pct > 100 || p.band_high_pct < 100 || p.band_high_pct > 400) return "the band must satisfy 1 <= band_low_pct <= 100 <= band_high_pct <= 400";
  if (p.max_step < 1 || p.max_step > 255) return "max_step must lie in 1..255";
  return nullptr;
}

RateControl::RateControl(const av1mi_rc_params &p) : p_(p), last_q_(p.start_q) {
  const long long g = std::gcd((long long)p.target_num, (long long)p.target_den);
  num_ = p.target_num / g; den_ = p.target_den / g;
}

int RateControl::NextQ(int k, int n) {
  if (k < 0 || k > 1 || n < 1 || n > 4096 || flight_.size() >= 64) return -1;
  const I G = p_.gop_length, window = (I)p_.window_gops * G * n;
  int q;
  if (!seen_[0] || (G > 1 && !seen_[1])) {
    q = p_.start_q;
  } else {
    debt_ = clamp(debt_, -window * num_, window * num_);
    const I allowed = clamp(num_ - fdiv(debt_, window), fdiv(num_ * p_.band_low_pct, 100), fdiv(num_ * p_.band_high_pct, 100));
    const I bytes = fdiv(allowed, den_), need = X_[0] + (G - 1) * X_[1];
    q = p_.qmax;
    for (int c = p_.qmin; c <= p_.qmax; c++)
      if (need <= bytes * G * qstep(c, p_.bit_depth)) { q = c; break; }
    q = (int)clamp(clamp(q, last_q_ - p_.max_step, last_q_ + p_.max_step), p_.qmin, p_.qmax);
  }
  const I share = seen_[k] ? fdiv(X_[k] * n, qstep(q, p_.bit_depth)) * den_ - (I)n * num_ : 0;
  debt_ += share;
  flight_.push_back({ k, n, q, share });
  last_q_ = q;
  return q;
}

int RateControl::Collected(long long b) {
  if (flight_.empty() || b < 0 || b >= (1ll << 36)) return -1;
  const Flight f = flight_.front();
  flight_.pop_front();
  debt_ += (I)b * den_ - (I)f.frames * num_ - f.share;
  const I obs = fdiv((I)b * qstep(f.q, p_.bit_depth), f.frames);
  X_[f.type] = seen_[f.type] ? fdiv(X_[f.type] * (p_.weight_den - p_.weight_num) + obs * p_.weight_num, p_.weight_den) : obs;
  seen_[f.type] = true;
  return 0;
}

}  // namespace av1mi_host

struct av1mi_rc { av1mi_host::RateControl rc; explicit av1mi_rc(const av1mi_rc_params &p) : rc(p) {} };

extern "C" {

void av1mi_rc_defaults(av1mi_rc_params *p) {
  if (!p) return;
  p->qmin = 1; p->qmax = 255;
  // chosen with tools/bench_ratecontrol.py: the one place these numbers live
  p->weight_num = 1; p->weight_den = 4; p->window_gops = 4; p->band_low_pct = 50; p->band_high_pct = 150; p->max_step = 8;
}
int av1mi_rc_qstep(int q, int bit_depth) { return av1mi_host::qstep(q, bit_depth); }
int av1mi_rc_open(const av1mi_rc_params *p, av1mi_rc **out, char *err, int errcap) {
  if (out) *out = nullptr;
  const char *why = !p || !out ? "null argument" : av1mi_host::RateControl::ParamError(*p);
  if (!why) { *out = new (std::nothrow) av1mi_rc(*p); if (!*out) why = "out of memory"; }
  if (why && err && errcap > 0) { strncpy(err, why, (size_t)errcap - 1); err[errcap - 1] = 0; }
  return why ? -1 : 0;
}
int av1mi_rc_next_q(av1mi_rc *rc, int frame_type, int frames_in_batch) { return rc ? rc->rc.NextQ(frame_type, frames_in_batch) : -1; }
int av1mi_rc_collected(av1mi_rc *rc, int64_t bytes) { return rc ? rc->rc.Collected(bytes) : -1; }
void av1mi_rc_close(av1mi_rc *rc) { delete rc; }

}  // extern "C"
