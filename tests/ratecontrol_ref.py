"""The one-pass rate controller of include/av1mi_rc.h restated in Python integers from the header's text ("Arithmetic").  Nothing here
is taken from host/ratecontrol.cpp: the step table comes through av1mi_rc_qstep and the tuning defaults through av1mi_rc_defaults, so
the two can only agree on a q sequence if both do what the header says.  `predict=False` switches the in-flight prediction off (such a
batch then weighs nothing until it is collected): the negative control of the lag test, not a mode of the library."""
from math import gcd

KEY, INTER = 0, 1


def fdiv(a, b):
    """floor(a / b) for b > 0 — Python's // already floors; named so that the reader finds the header's fdiv"""
    return a // b


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


class Twin:
    def __init__(self, qstep, target_num, target_den, gop_length, start_q, qmin, qmax, bit_depth, weight_num, weight_den, window_gops,
                 band_low_pct, band_high_pct, max_step, predict=True):
        g = gcd(target_num, target_den)
        self.num, self.den = target_num // g, target_den // g
        self.G, self.start_q, self.qmin, self.qmax = gop_length, start_q, qmin, qmax
        self.wn, self.wd, self.window_gops, self.lo, self.hi, self.max_step = weight_num, weight_den, window_gops, band_low_pct, band_high_pct, max_step
        self.step = [0] + [qstep(q, bit_depth) for q in range(1, 256)]
        self.X, self.seen = [0, 0], [False, False]
        self.debt = 0                  # in units of 1 / den bytes
        self.flight = []               # oldest first: (frame type, frames, q, the share of the debt it was given)
        self.last_q = start_q
        self.predict = predict

    def _bound(self, window):
        self.debt = clamp(self.debt, -window * self.num, window * self.num)

    def next_q(self, frame_type, frames):
        window = self.window_gops * self.G * frames
        if not self.seen[KEY] or (self.G > 1 and not self.seen[INTER]):
            q = self.start_q
        else:
            self._bound(window)
            allowed = clamp(self.num - fdiv(self.debt, window), fdiv(self.num * self.lo, 100), fdiv(self.num * self.hi, 100))
            allowed_bytes = fdiv(allowed, self.den)
            need = self.X[KEY] + (self.G - 1) * self.X[INTER]
            q = self.qmax
            for c in range(self.qmin, self.qmax + 1):
                if need <= allowed_bytes * self.G * self.step[c]:
                    q = c
                    break
            q = clamp(clamp(q, self.last_q - self.max_step, self.last_q + self.max_step), self.qmin, self.qmax)
        share = 0
        if self.predict and self.seen[frame_type]:
            share = fdiv(self.X[frame_type] * frames, self.step[q]) * self.den - frames * self.num
        self.debt += share
        self.flight.append((frame_type, frames, q, share))
        self.last_q = q
        return q

    def collected(self, nbytes):
        frame_type, frames, q, share = self.flight.pop(0)
        self.debt += nbytes * self.den - frames * self.num - share
        obs = fdiv(nbytes * self.step[q], frames)
        if self.seen[frame_type]:
            self.X[frame_type] = fdiv(self.X[frame_type] * (self.wd - self.wn) + obs * self.wn, self.wd)
        else:
            self.X[frame_type], self.seen[frame_type] = obs, True
