// ratecontrol.hpp — the one-pass, feedback-only rate controller behind -b:v:0 / -av1mi_target_bpp (include/av1mi_rc.h states its
// arithmetic normatively; tests/ratecontrol_ref.py is its twin).  One quantiser per batch; integers only, so the q sequence — and with
// it the output file — is a function of the input alone.
#pragma once
#include <deque>
#include <string>
#include "../../include/av1mi_rc.h"

namespace av1mi_host {

class RateControl {
 public:
  // null = fine, else the reason the parameters are refused
  static const char *ParamError(const av1mi_rc_params &p);
  explicit RateControl(const av1mi_rc_params &p);
  int NextQ(int frame_type, int frames);       // -1: bad argument / queue full
  int Collected(long long bytes);              // -1: bad argument / nothing in flight
  const av1mi_rc_params &params() const { return p_; }

 private:
  typedef __int128 I;
  struct Flight { int type, frames, q; I share; };
  static I fdiv(I a, I b) { I q = a / b; return (a % b != 0 && (a < 0)) ? q - 1 : q; }
  static I clamp(I v, I lo, I hi) { return v < lo ? lo : v > hi ? hi : v; }
  av1mi_rc_params p_;
  I num_, den_, X_[2] = { 0, 0 }, debt_ = 0;
  bool seen_[2] = { false, false };
  int last_q_;
  std::deque<Flight> flight_;
};

}  // namespace av1mi_host
