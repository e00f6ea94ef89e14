"""The one-pass rate controller (include/av1mi_rc.h, host/ratecontrol.cpp) against its Python twin (tests/ratecontrol_ref.py, written
from the header's text) on simulated plants, and the properties the header's arithmetic is meant to have.  No GPU."""
import ctypes as C
from fractions import Fraction

import pytest

import av1stream
from ratecontrol_ref import INTER, KEY, Twin


class Params(C.Structure):
    _fields_ = [("target_num", C.c_int64), ("target_den", C.c_int64), ("gop_length", C.c_int32), ("start_q", C.c_int32), ("qmin", C.c_int32),
                ("qmax", C.c_int32), ("bit_depth", C.c_int32), ("weight_num", C.c_int32), ("weight_den", C.c_int32), ("window_gops", C.c_int32),
                ("band_low_pct", C.c_int32), ("band_high_pct", C.c_int32), ("max_step", C.c_int32)]


@pytest.fixture(scope="module")
def host():
    lib = av1stream.lib()
    lib.av1mi_rc_defaults.restype = None
    lib.av1mi_rc_defaults.argtypes = [C.POINTER(Params)]
    lib.av1mi_rc_open.argtypes = [C.POINTER(Params), C.POINTER(C.c_void_p), C.c_char_p, C.c_int]
    lib.av1mi_rc_next_q.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.av1mi_rc_collected.argtypes = [C.c_void_p, C.c_int64]
    lib.av1mi_rc_close.argtypes = [C.c_void_p]
    lib.av1mi_rc_close.restype = None
    lib.av1mi_rc_qstep.argtypes = [C.c_int, C.c_int]
    return lib


def params(host, num, den, gop, start_q, bd=8, **over):
    p = Params()
    host.av1mi_rc_defaults(C.byref(p))
    p.target_num, p.target_den, p.gop_length, p.start_q, p.bit_depth = num, den, gop, start_q, bd
    for k, v in over.items():
        setattr(p, k, v)
    return p


def twin_of(host, p, predict=True):
    return Twin(host.av1mi_rc_qstep, p.target_num, p.target_den, p.gop_length, p.start_q, p.qmin, p.qmax, p.bit_depth, p.weight_num, p.weight_den,
                p.window_gops, p.band_low_pct, p.band_high_pct, p.max_step, predict=predict)


class Library:
    def __init__(self, host, p):
        self.host, self.h = host, C.c_void_p()
        err = C.create_string_buffer(256)
        assert host.av1mi_rc_open(C.byref(p), C.byref(self.h), err, 256) == 0, err.value

    def next_q(self, k, n):
        q = self.host.av1mi_rc_next_q(self.h, k, n)
        assert q >= 1
        return q

    def collected(self, b):
        assert self.host.av1mi_rc_collected(self.h, b) == 0

    def close(self):
        self.host.av1mi_rc_close(self.h)


def iroot(x, n):
    """floor of the n-th root of the non-negative integer x"""
    lo, hi = 0, 1
    while hi ** n <= x:
        hi *= 2
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if mid ** n <= x else (lo, mid)
    return lo


def plant_bytes(c, n, step, a):
    """floor(c * n / step ^ a) for a = a_num / a_den, in integers: step ^ (a_num / a_den) is taken as the floor of the a_den-th root of
    step ^ a_num scaled by 10^6 (exact for a = 1)"""
    a = Fraction(a).limit_denominator(10)
    scaled = iroot(step ** a.numerator * 10 ** (6 * a.denominator), a.denominator)      # 10^6 * step ^ a
    return c * n * 10 ** 6 // scaled


def drive(ctl, qstep, bd, gop, frames, lag, batches, c_key, c_p, a, change_at=None, tail_frames=None):
    """`batches` batches through a controller and a plant with `lag` batches in flight when the next is asked for: the q sequence, and the
    (bytes, frames) of every batch in submission order"""
    qs, flight, out = [], [], []
    for t in range(batches):
        k = KEY if t % gop == 0 else INTER
        n = tail_frames if tail_frames and t >= batches - gop else frames
        c = (c_key if k == KEY else c_p) * (2 if change_at is not None and t >= change_at else 1)
        q = ctl.next_q(k, n)
        qs.append(q)
        flight.append((c, n, q))
        if len(flight) > lag:
            c, n, q = flight.pop(0)
            b = plant_bytes(c, n, qstep(q, bd), a)
            ctl.collected(b)
            out.append((b, n))
    for c, n, q in flight:
        b = plant_bytes(c, n, qstep(q, bd), a)
        ctl.collected(b)
        out.append((b, n))
    return qs, out


CASES = [(a, gop, frames, lag) for a in (0.8, 1, 1.3) for gop in (4, 30) for frames in (1, 12) for lag in (0, 2)]


@pytest.mark.parametrize("a,gop,frames,lag", CASES)
def test_the_library_and_the_twin_give_the_same_q_sequence(host, a, gop, frames, lag):
    bd = 8 if gop == 4 else 10
    # targets between the plant's output at coarse and fine quantisers; start away from where it settles
    for num, den, start, change, tail in ((4000, 1, 60, None, None), (30000 * 1001, 8 * 30000, 140, 5 * gop + 1, None), (9000, 7, 100, None, 5 if frames > 1 else None)):
        p = params(host, num, den, gop, start, bd)
        lib, twin = Library(host, p), twin_of(host, p)
        try:
            args = (host.av1mi_rc_qstep, bd, gop, frames, lag, 10 * gop, 2400000, 300000, a)
            got, _ = drive(lib, *args, change_at=change, tail_frames=tail)
            exp, _ = drive(twin, *args, change_at=change, tail_frames=tail)
        finally:
            lib.close()
        assert got == exp, (num, den, start)
        assert len(set(got)) > 3, "the plant never moved the controller: the case checks nothing"


@pytest.mark.parametrize("num,qmin,qmax,pinned", [(1, 20, 200, 200), (10 ** 9, 20, 200, 20), (1, 1, 255, 255), (10 ** 9, 1, 255, 1)])
def test_unreachable_targets_pin_the_quantiser_at_its_bound(host, num, qmin, qmax, pinned):
    p = params(host, num, 1, 4, 100, 8, qmin=qmin, qmax=qmax)
    lib, twin = Library(host, p), twin_of(host, p)
    try:
        args = (host.av1mi_rc_qstep, 8, 4, 3, 2, 80, 2400000, 300000, 1)
        got, _ = drive(lib, *args)
        exp, _ = drive(twin, *args)
    finally:
        lib.close()
    assert got == exp and set(got[-20:]) == {pinned} and qmin <= min(got) and max(got) <= qmax
    steps = [abs(b - a) for a, b in zip(got, got[1:])]
    assert max(steps) <= p.max_step


@pytest.mark.parametrize("gop,frames,lag", [(4, 1, 0), (4, 12, 2), (30, 1, 2), (30, 12, 0), (30, 12, 2)])
def test_a_constant_plant_settles_at_the_target(host, gop, frames, lag):
    """a = 1, constant c, after the first two GOPs: q stays within one step (the step limit) of a fixed point, and the average bytes per
    frame from there on lies within the largest ratio of successive steps inside the range of q visited of the target.  The twin alone is
    asked: the first test ties the library to it."""
    bd, target = 8, 4000
    p = params(host, target, 1, gop, 120, bd)
    qs, out = drive(twin_of(host, p), host.av1mi_rc_qstep, bd, gop, frames, lag, 60 * gop, 2400000, 300000, 1)
    tail_q, tail = qs[2 * gop:], out[2 * gop:]
    assert max(tail_q) - min(tail_q) <= 2 * p.max_step, (min(tail_q), max(tail_q))
    lo, hi = min(tail_q), max(tail_q)
    ratio = max(Fraction(host.av1mi_rc_qstep(q + 1, bd), host.av1mi_rc_qstep(q, bd)) for q in range(max(lo - 1, 1), min(hi + 1, 255)))
    avg = Fraction(sum(b for b, _ in tail), sum(n for _, n in tail))
    print("GOP %d, %d frames per batch, lag %d: q %d..%d, average / target %.5f, bound %.5f" % (gop, frames, lag, lo, hi, float(avg / target), float(ratio)))
    assert Fraction(target) / ratio <= avg <= target * ratio, (float(avg), float(ratio))


def test_in_flight_prediction_keeps_the_lag_from_overshooting(host):
    """lag 2 on the a = 1 plant whose c doubles: with the batches in flight counted at their predicted bytes, q passes the new fixed
    point by no more than the step limit; the twin without the prediction (the negative control) passes it by more"""
    bd, gop, frames, lag, change = 8, 4, 2, 2, 4 * 30 + 1
    p = params(host, 4000, 1, gop, 110, bd)
    over = {}
    for predict in (True, False):
        qs, _ = drive(twin_of(host, p, predict=predict), host.av1mi_rc_qstep, bd, gop, frames, lag, 60 * gop, 1600000, 400000, 1, change_at=change)
        settled = sorted(qs[50 * gop:])
        fixed = settled[len(settled) // 2]
        over[predict] = max(qs[change:]) - fixed
        print("prediction %s: fixed point %d, highest q after the change %d" % (predict, fixed, max(qs[change:])))
    assert over[True] <= p.max_step < over[False], over


def test_invalid_parameters_are_refused(host):
    good = dict(num=4000, den=1, gop=30, start_q=100)
    for bad in (dict(num=0), dict(num=-5), dict(den=0), dict(gop=0), dict(start_q=0), dict(start_q=256), dict(qmin=120), dict(qmax=90),
                dict(qmin=90, qmax=80), dict(bd=9), dict(max_step=0), dict(weight_num=5, weight_den=4), dict(window_gops=0)):
        kw = dict(good)
        over = {k: v for k, v in bad.items() if k not in ("num", "den", "gop", "start_q", "bd")}
        kw.update({k: v for k, v in bad.items() if k in kw})
        p = params(host, kw["num"], kw["den"], kw["gop"], kw["start_q"], bad.get("bd", 8), **over)
        h, err = C.c_void_p(), C.create_string_buffer(256)
        assert host.av1mi_rc_open(C.byref(p), C.byref(h), err, 256) == -1 and not h.value and err.value, bad
    p = params(host, 4000, 1, 30, 100)
    lib = Library(host, p)
    assert host.av1mi_rc_collected(lib.h, 10) == -1                      # nothing in flight
    assert host.av1mi_rc_next_q(lib.h, 2, 1) == -1 and host.av1mi_rc_next_q(lib.h, 0, 0) == -1
    assert host.av1mi_rc_next_q(lib.h, 0, 4) == 100
    lib.close()
    assert host.av1mi_rc_qstep(256, 8) == 0 and host.av1mi_rc_qstep(10, 12) == 0


def test_the_step_table_is_the_quantisers(host, av1mi):
    lib = av1mi.load()
    for bd in (8, 10):
        for q in range(256):
            assert host.av1mi_rc_qstep(q, bd) == lib.av1mi_ac_q(q, bd)
