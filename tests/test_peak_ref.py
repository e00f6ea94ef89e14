"""The numpy twin of the peak records and the peak plan (tests/peak_ref.py) against cases computed by hand from include/av1mi.h "peak
records", and the host's planner (av1mi_plan_peak through av1stream.plan_peak) against the twin.  No GPU."""
import numpy as np
import pytest

import peak_ref as R
import tonemap_ref as T


def _frame(y, u, v, w=16, h=8):
    return np.full((1, h, w), y, np.uint16), np.full((1, h // 2, w // 2), u, np.uint16), np.full((1, h // 2, w // 2), v, np.uint16)


def _only_bin(rec):
    assert int(rec["hist"].sum()) == int(rec["pixels"])
    (b,) = np.nonzero(rec["hist"])[0]
    return int(b)


def test_neutral_frames():
    """Y = 940 neutral: y = 19133 * 876 + 8192 = 16768700, >> 14 = 1023 in all three; Y = 64: 8192 >> 14 = 0"""
    assert T.constants()["to_rgb"] == [19133, 27584, 10688, 3078, 35194]
    r = R.records(*_frame(940, 512, 512), 16, 8)[0]
    assert _only_bin(r) == 1023 and int(r["pixels"]) == 128
    assert _only_bin(R.records(*_frame(64, 512, 512), 16, 8)[0]) == 0
    assert _only_bin(R.records(*_frame(0, 512, 512), 16, 8)[0]) == 0            # below black: clamped at 0
    assert _only_bin(R.records(*_frame(0xFFFF, 0xFFFF, 0xFFFF), 16, 8)[0]) == 1023      # samples above 1023 count as 1023


def test_saturated_chroma_each_component_the_maximum():
    """Y = 300: y = 19133 * 236 + 8192 = 4523580.
    V = 700 (v = 188): R' = (4523580 + 27584 * 188) >> 14 = 9709372 >> 14 = 592; G' = 2514236 >> 14 = 153; B' = 276.
    U = 700 (u = 188): B' = (4523580 + 35194 * 188) >> 14 = 11140052 >> 14 = 679; G' = 3944916 >> 14 = 240; R' = 276.
    U = V = 300 (u = v = -212): G' = (4523580 + 10688 * 212 + 3078 * 212) >> 14 = 7441972 >> 14 = 454; R' and B' negative: clamped at 0."""
    assert _only_bin(R.records(*_frame(300, 512, 700), 16, 8)[0]) == 592
    assert _only_bin(R.records(*_frame(300, 700, 512), 16, 8)[0]) == 679
    assert _only_bin(R.records(*_frame(300, 300, 300), 16, 8)[0]) == 454
    assert R.max_rgb(np.array([[300]]), np.array([[512]]), np.array([[700]])).tolist() == [[592]]
    # the clamp at 1023: Y = 500, V = 960: R' = (19133 * 436 + 8192 + 27584 * 448) >> 14 = 1263 -> 1023
    assert _only_bin(R.records(*_frame(500, 512, 960), 16, 8)[0]) == 1023


def test_true_size_and_chroma_sharing():
    """a 9 x 7 picture in a 16 x 8 buffer: 63 pixels; the last column shares its chroma sample (x >> 1 = 4) with nothing else"""
    Y, U, V = _frame(300, 512, 512)
    U[0, :, 4] = 700      # column 8 alone sees it
    Y[:, 7:, :] = 0xFFFF
    Y[:, :, 9:] = 0xFFFF
    U[:, :, 5:] = 0xFFFF
    V[:, :, 5:] = 0xFFFF
    r = R.records(Y, U, V, 9, 7)[0]
    assert int(r["pixels"]) == 63 and int(r["hist"][276]) == 56 and int(r["hist"][679]) == 7 and int(r["hist"].sum()) == 63


def _rec(bins, pixels=None):
    r = np.zeros(1, R.PEAK_DTYPE)
    for b, n in bins.items():
        r[0]["hist"][b] = n
    r[0]["pixels"] = sum(bins.values()) if pixels is None else pixels
    return r


def test_skip_on_both_sides():
    """128 x 128 = 16384 pixels: skip = 1.  One bright pixel is let go, two are not; under 16384 pixels nothing is let go"""
    Y, U, V = _frame(300, 512, 512, 128, 128)
    Y[0, 5, 5] = 900
    assert (int(R.records(Y, U, V, 128, 128)[0]["pixels"]) >> 14) == 1
    assert R.plan(R.records(Y, U, V, 128, 128))[1] == [276]
    Y[0, 99, 77] = 800      # M = (19133 * 736 + 8192) >> 14 = 859
    assert R.plan(R.records(Y, U, V, 128, 128))[1] == [859]
    Y[0, 98, 77] = 800
    assert R.plan(R.records(Y, U, V, 128, 128))[1] == [859]
    assert R.plan(R.records(Y[:, :127], U, V, 128, 127))[1] == [(19133 * 836 + 8192) >> 14]      # 16256 pixels: skip = 0, the pixel of 900 counts
    assert R.frame_code(_rec({300: 3840 * 2160 - 506, 1000: 506})[0]) == 300 and R.frame_code(_rec({300: 3840 * 2160 - 507, 1000: 507})[0]) == 1000


def test_floor_cap_and_the_maximum_over_frames():
    lin = T.tables(1000)["lin"]
    assert int(lin[1023]) == 2560000 and (lin == T.tables(4000)["lin"]).all()
    assert R.plan(_rec({0: 4096})) == (400, [0])                       # an all-black frame: the floor
    assert R.plan(_rec({1023: 4096})) == (10000, [1023])               # the cap
    c400 = int(np.nonzero((lin + 255) >> 8 > 400)[0][0])               # the first code above the floor
    assert R.plan(_rec({c400 - 1: 10}))[0] == 400 and R.plan(_rec({c400: 10}))[0] == (int(lin[c400]) + 255) >> 8 > 400
    recs = np.concatenate([_rec({200: 4096}), _rec({700: 4096}), _rec({500: 4096})])
    assert R.plan(recs) == ((int(lin[700]) + 255) >> 8, [200, 700, 500]) and 400 < R.plan(recs)[0] < 10000
    with pytest.raises(ValueError):
        R.plan(recs[:0])
    with pytest.raises(ValueError):
        R.plan(np.concatenate([recs, _rec({})]))


def test_host_plan_is_the_twin():
    import av1mi
    import av1stream
    assert av1mi.PEAK_DTYPE == R.PEAK_DTYPE and R.PEAK_DTYPE.itemsize == 4100
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = int(rng.integers(1, 9))
        recs = np.zeros(n, R.PEAK_DTYPE)
        for r in recs:
            top = int(rng.integers(1, 1024))
            pixels = int(rng.choice([4096, 16384, 40000, 3840 * 2160]))
            body = rng.multinomial(pixels - min(pixels >> 14, 40) - int(rng.integers(0, 3)), np.ones(top) / top)
            r["hist"][:top] = body
            tail = pixels - int(body.sum())      # a few pixels above the body: on either side of skip
            r["hist"][rng.integers(top, 1024, tail) if top < 1024 else [1023] * tail] += 1 if tail else 0
            r["pixels"] = int(r["hist"].sum())
        peak, codes = av1stream.plan_peak(recs)
        assert (peak, codes.tolist()) == R.plan(recs), trial
    for bad in (recs[:0], np.concatenate([recs, np.zeros(1, R.PEAK_DTYPE)])):
        with pytest.raises(ValueError):
            av1stream.plan_peak(bad)
    assert av1stream.peak_sample_slots(8) == list(range(8)) and av1stream.peak_sample_slots(1000) == [i * 1000 // 32 for i in range(32)] and av1stream.peak_sample_slots(0) == []
