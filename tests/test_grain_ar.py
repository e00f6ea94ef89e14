"""Coloured film grain on the CPU: the grain covariance's numpy restatement (tests/grain_cov_ref.py) into av1mi_film_grain_from_records_ar
(host/filmgrain.hpp "coloured grain"): the coefficients it recovers, its fallbacks, the closed loop through dav1d, and -av1mi_grain_lag
through the transcode job's argument parser.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import grain_ar_loop as L
import grain_cov_ref as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "av1-go_amd", "host", "libav1mi_host.so")
GAIN = 0.0619      # host/filmgrain.hpp kGainLuma


def _neighbours(lag):
    return [(dx, dy) for dy in range(-lag, 1) for dx in range(-lag, lag + 1) if (dy, dx) < (0, 0)]


def _response(coeffs, lag, shift, K=32):
    """the impulse response of quantised coefficients over y = 0 .. K, x = -K .. K (the half plane of filmgrain.hpp), [K + 1, 2 K + 1]"""
    h = np.zeros((K + 1 + 3, 2 * K + 1 + 6))
    nb = _neighbours(lag)
    for y in range(K + 1):
        for x in range(-K, K + 1):
            v = 1.0 if (x, y) == (0, 0) else 0.0
            for c, (dx, dy) in zip(coeffs, nb):
                if c:
                    v += c / (1 << shift) * h[y + dy + 3, x + dx + K + 3]
            h[y + 3, x + K + 3] = v
    return h[3:, 3:-3]


def _template_gain(coeffs, lag, shift, chroma, runs=64, seed=1):
    """the decoder's template procedure (spec 7.18.3.3 as dav1d runs it) on `runs` templates at once: white values of deviation 31.7, the
    recursion in place from (3, 3) with the sum rounded at the shift and every value clipped to -128 .. 127; the variance of the part
    blocks are cut from, after over before"""
    H, W, start = (38, 44, 6) if chroma else (73, 82, 9)
    t = np.rint(np.random.default_rng(seed).normal(0, 31.7, (runs, H, W))).astype(np.int64)
    before = float((t[:, start:, start:W - 3] ** 2).sum())
    nb = _neighbours(lag)
    for y in range(3, H):
        for x in range(3, W - 3):
            s = sum(c * t[:, y + dy, x + dx] for c, (dx, dy) in zip(coeffs, nb) if c)
            t[:, y, x] = np.clip(t[:, y, x] + ((s + (1 << (shift - 1))) >> shift), -128, 127)
    return float((t[:, start:, start:W - 3] ** 2).sum()) / before


def _implied_rho(h, dx, dy):
    """the normalised covariance of white noise through the response h at offset (dx, dy), dx, dy >= 0"""
    a = h[:h.shape[0] - dy, :h.shape[1] - dx]
    b = h[dy:, dx:]
    return float((a * b).sum() / (h * h).sum())


def _records(sum_sq, count, chroma_count=None):
    import av1mi
    rec = np.zeros((3, 16), av1mi.GRAIN_DTYPE)
    for p in range(3):
        rec[p, 8]["sum_sq"], rec[p, 8]["count"] = sum_sq, count if p == 0 or chroma_count is None else chroma_count
    return rec


@pytest.fixture(scope="module")
def coloured():
    """a residual with the injected covariance, its covariance record and grain records that hold it in bin 8"""
    r = np.rint(L.coloured(np.random.default_rng(3), (384, 384), 6.0)).astype(np.int64)
    return r, GC.of_residual(r), _records(int((r * r).sum()), r.size)


def _coeffs(g, plane=0):
    n = 2 * g.ar_coeff_lag * (g.ar_coeff_lag + 1)
    src = (g.ar_coeffs_y_plus_128, g.ar_coeffs_cb_plus_128, g.ar_coeffs_cr_plus_128)[plane]
    return [int(src[i]) - 128 for i in range(n)]


def test_known_covariance_gives_its_coefficients_back(coloured):
    import av1stream
    r, cov, rec = coloured
    g = av1stream.film_grain_from_records_ar(rec, np.stack([cov] * 3), 8, 1, 2)
    white = av1stream.film_grain_from_records(rec, 8, 1)
    assert g.apply_grain == 1 and g.ar_coeff_lag == 2
    # the expected shift, from a solution of the same equations in numpy (the ridge of filmgrain.hpp)
    f, nb = GC.rho(cov), _neighbours(2)
    A = np.array([[f(a[0] - b[0], a[1] - b[1]) for b in nb] for a in nb]) + 1e-3 * np.eye(len(nb))
    a = np.linalg.solve(A, np.array([f(*n) for n in nb]))
    shift = max(s for s in (6, 7, 8, 9) if np.all(np.abs(np.floor(a * (1 << s) + 0.5) + 0.5) <= 128))
    assert g.ar_coeff_shift_minus_6 + 6 == shift
    c = _coeffs(g)
    assert c == [int(v) for v in np.floor(a * (1 << shift) + 0.5)]
    assert _coeffs(g, 1) == c and _coeffs(g, 2) == c and g.ar_coeffs_cb_plus_128[len(c)] == 128 and g.ar_coeffs_cr_plus_128[len(c)] == 128
    # the filter's own covariance against the input's: 12 coefficients, each within half a step 2^-(shift + 1) of the solution, move a
    # normalised covariance by at most their sum; 0.02 for the ridge and for what a causal model of this size cannot follow
    h = _response(c, 2, shift)
    bound = len(c) * 2.0 ** -(shift + 1) + 0.02
    for dx, dy in L.OFFSETS:
        got, want = _implied_rho(h, dx, dy), f(dx, dy)
        print("rho(%d, %d): the filter's %.4f, the input's %.4f (injected %.4f)" % (dx, dy, got, want, L.INJECTED[(dx, dy)]))
        assert abs(got - want) <= bound
    # (the gain of the decoder's template procedure, filmgrain.hpp "template") x (scaled point)^2 is the white function's variance.  The
    # gain is measured here on templates of this file's own (numpy's generator, 64 of them); the margin is the rounding of the two 8-bit
    # values plus 2.5 % of the white value: three standard errors of the two estimates together (0.65 % and 0.33 % of the deviation, from
    # 16 and 64 templates of some 750 independent samples each)
    G = float((h * h).sum())
    assert G > 1.2
    amp = {chroma: np.sqrt(_template_gain(c, 2, shift, chroma)) for chroma in (False, True)}
    print("G %.3f, the template's gain %.3f (luma) %.3f (chroma)" % (G, amp[False] ** 2, amp[True] ** 2))
    assert amp[False] ** 2 < G
    unit = 2.0 ** (white.grain_scaling_minus_8 - g.grain_scaling_minus_8)      # of a scaling value, in the white function's (filmgrain.hpp "scaling")
    assert g.grain_scaling_minus_8 == 2 and white.grain_scaling_minus_8 == 1       # (values near 120 / 2: doubled, they fit)
    for i in range(g.num_y_points):
        assert g.point_y_value[i] == white.point_y_value[i]
        assert abs(g.point_y_scaling[i] * unit * amp[False] - white.point_y_scaling[i]) <= 0.5 * unit * amp[False] + 0.5 + 0.025 * white.point_y_scaling[i]
    assert g.point_y_scaling[0] * unit < white.point_y_scaling[0]
    assert abs(g.point_cb_scaling[0] * unit * amp[True] - white.point_cb_scaling[0]) <= 0.5 * unit * amp[True] + 0.5 + 0.025 * white.point_cb_scaling[0]
    assert (g.grain_seed, g.num_y_points, g.num_cb_points, g.num_cr_points) == (white.grain_seed, white.num_y_points, white.num_cb_points, white.num_cr_points)


def test_lag_0_is_the_white_function(coloured):
    import av1stream
    _, cov, rec = coloured
    assert bytes(av1stream.film_grain_from_records_ar(rec, np.stack([cov] * 3), 8, 7, 0)) == bytes(av1stream.film_grain_from_records(rec, 8, 7))
    for lag in (-1, 4):
        with pytest.raises(ValueError):
            av1stream.film_grain_from_records_ar(rec, np.stack([cov] * 3), 8, 7, lag)


@pytest.mark.parametrize("lag", [1, 2, 3])
def test_fallbacks(coloured, lag):
    import av1stream
    _, cov, rec = coloured
    white = bytes(av1stream.film_grain_from_records(rec, 8, 1))
    # an all-zero covariance: cov(0) is 0
    assert bytes(av1stream.film_grain_from_records_ar(rec, np.zeros((3, 4, 13), np.int64), 8, 1, lag)) == white
    # rho = 1 at every offset: the filter that reproduces it has a pole at 1, its gain does not converge at any lag
    flat = np.full((4, 13), 1000000, np.int64)
    assert bytes(av1stream.film_grain_from_records_ar(rec, np.stack([flat] * 3), 8, 1, lag)) == white
    # a checkerboard (rho = (-1)^(dx + dy)) likewise, with the pole at -1
    dy, dx = np.mgrid[0:4, -6:7]
    board = (1000000 * (1 - 2 * ((dx + dy) & 1))).astype(np.int64)
    assert bytes(av1stream.film_grain_from_records_ar(rec, np.stack([board] * 3), 8, 1, lag)) == white
    # a chroma plane under kMinCount (256 samples): no points and no coefficients for it; the others keep theirs
    few = _records(int(rec[0, 8]["sum_sq"]), int(rec[0, 8]["count"]))
    few[1, 8]["count"], few[1, 8]["sum_sq"] = 255, 255 * 36
    g = av1stream.film_grain_from_records_ar(few, np.stack([cov] * 3), 8, 1, lag)
    assert g.ar_coeff_lag == lag and g.num_cb_points == 0 and g.num_cr_points == 2
    assert all(v == 0 for v in _coeffs(g, 1)) and any(_coeffs(g, 0)) and _coeffs(g, 2) == _coeffs(g, 0)
    # the luma plane under it: no grain at all
    none = _records(255 * 36, 255)
    g = av1stream.film_grain_from_records_ar(none, np.stack([cov] * 3), 8, 1, lag)
    assert g.apply_grain == 0 and bytes(g) == bytes(av1stream.film_grain_from_records(none, 8, 1))
    # luma white (its covariance empty), chroma coloured: the coded lag is the chroma planes', the luma coefficients are zeros
    mixed = np.stack([np.zeros((4, 13), np.int64), cov, cov])
    g = av1stream.film_grain_from_records_ar(rec, mixed, 8, 1, lag)
    w = av1stream.film_grain_from_records(rec, 8, 1)
    assert g.ar_coeff_lag == lag and all(v == 0 for v in _coeffs(g, 0)) and any(_coeffs(g, 1))
    unit = 2.0 ** (w.grain_scaling_minus_8 - g.grain_scaling_minus_8)      # (one more bit of scaling where the doubled values fit)
    assert abs(g.point_y_scaling[0] * unit - w.point_y_scaling[0]) <= 0.5 and g.point_cb_scaling[0] * unit < w.point_cb_scaling[0]


def test_closed_loop_regenerates_the_grain_size(O):
    """coloured grain of sigma 4 at 8 bits -> denoise_ref -> records + covariance -> parameters -> stream -> dav1d.  White parameters
    (lag 0, the parent's) synthesise grain without a size: this leg shows the defect.  At lag 2 the synthesised grain's normalised
    covariance is closer to the injected one than white grain's by a factor of two wherever the injected one is at least 0.2, and the
    standard deviation stays within one step of the scaling value (plus three standard errors of a standard deviation over a region, the
    band of tests/test_filmgrain_stream.py) of the lag-0 leg's of the same seed: the division by sqrt(G).
    OBSERVED (tests/golden/grain_ar_observed.json): rho at (1,0) (0,1) (1,1) (2,0): -0.002 -0.011 -0.001 0.020 at lag
    0, 0.618 0.605 0.379 0.101 at lag 2 against the injected 0.667 0.667 0.444 0.167; the ratio per region 0.999 0.979 0.987 at lag 0 and
    0.976 0.959 0.966 at lag 2, band 0.030.  (The decoder cuts every block of a frame from ONE template, that of the frame's grain seed,
    and a filtered template's realised deviation scatters by some 2 % around its expectation: over five seeds the difference between
    the legs ran from -0.032 to +0.022 with a mean of -0.007.  The case here is the one tests/test_filmgrain_stream.py uses.)
    """
    import dav1d_grain as DG
    import pipeline as P
    if not DG.available():
        pytest.skip("dav1d is not in this image")
    sigma, bd, seed = 4, 8, 11
    legs = {lag: L.loop(O, P, sigma, bd, seed, lag) for lag in (0, 2)}
    observed = json.load(open(os.path.join(ROOT, "tests", "golden", "grain_ar_observed.json")))
    for lag, r in legs.items():
        g = r["grain"]
        print("lag %d: coded lag %d shift %d, ratio per region %s, rho %s, the residual's rho %s" % (
            lag, g.ar_coeff_lag, g.ar_coeff_shift_minus_6 + 6, np.round(r["ratio"], 4), {k: round(v, 4) for k, v in r["rho"].items()},
            {k: round(v, 4) for k, v in r["residual_rho"].items()}))
    assert legs[0]["grain"].ar_coeff_lag == 0 and legs[2]["grain"].ar_coeff_lag == 2
    n = (L.F.ROWS[0][1] - L.F.ROWS[0][0]) * L.F.W
    for o in L.OFFSETS:
        assert abs(legs[0]["rho"][o]) < 0.1, "white grain with a covariance at %s: %.4f" % (o, legs[0]["rho"][o])
        if L.INJECTED[o] >= 0.2:
            e0, e2 = abs(legs[0]["rho"][o] - L.INJECTED[o]), abs(legs[2]["rho"][o] - L.INJECTED[o])
            assert e2 < e0 / 2, "offset %s: error %.4f at lag 2, %.4f at lag 0" % (o, e2, e0)
        # the recorded observation is this run's (the loop is deterministic), to the rounding of the file
        assert abs(observed["lag2"]["rho"]["%d,%d" % o] - legs[2]["rho"][o]) < 5e-4 and abs(observed["lag0"]["rho"]["%d,%d" % o] - legs[0]["rho"][o]) < 5e-4
    band = GAIN / sigma + 3 / np.sqrt(2 * n)
    for region, (a, b) in enumerate(zip(legs[0]["ratio"], legs[2]["ratio"])):
        assert abs(a - b) <= band, "region %d: ratio %.4f at lag 2, %.4f at lag 0, band %.4f" % (region, b, a, band)


def _transcode(argv):
    host = C.CDLL(HOST)
    host.av1mi_host_run_transcode.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(2048)
    return host.av1mi_host_run_transcode("\n".join(str(a) for a in argv).encode(), buf, 2048), buf.value.decode()


@pytest.mark.parametrize("bad,why", [(["-av1mi_denoise", "4", "-av1mi_grain_lag", "4"], "Invalid argument: -av1mi_grain_lag takes 0 (white grain) .. 3, not 4"),
                                     (["-av1mi_denoise", "4", "-av1mi_grain_lag", "-1"], "Invalid argument: -av1mi_grain_lag takes"),
                                     (["-av1mi_denoise", "4", "-av1mi_grain_lag", "x"], "Invalid argument: -av1mi_grain_lag takes"),
                                     (["-av1mi_grain_lag", "2"], "Invalid argument: -av1mi_grain_lag needs -av1mi_denoise"),
                                     (["-av1mi_grain_lag", "0"], "Invalid argument: -av1mi_grain_lag needs -av1mi_denoise"),
                                     (["-av1mi_denoise", "4", "-av1mi_film_grain", "0", "-av1mi_grain_lag", "2"], "Invalid argument: -av1mi_grain_lag shapes the film grain: not together with -av1mi_film_grain 0"),
                                     (["-av1mi_grain_lag", "2", "-av1mi_film_grain", "0", "-av1mi_denoise", "4"], "not together with -av1mi_film_grain 0")])
def test_grain_lag_is_refused_where_it_cannot_apply(bad, why):
    code, err = _transcode(["-i", "in.y4m"] + bad + ["out.obu"])
    assert code == 1 and why in err, err


def test_session_config_follows_the_grain_lag(tmp_path):
    """-av1mi_grain_lag N > 0 opens the session with grain_cov = 1; 0 and no option leave it 0 (host/backend.cpp SessionConfig)"""
    import av1mi
    host = C.CDLL(HOST)
    host.av1mi_host_session_config.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(av1mi.GopConfig), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    src = str(tmp_path / "a.y4m")
    open(src, "wb").write(b"YUV4MPEG2 W64 H48 F30:1 Ip A1:1 C420jpeg\n" + (b"FRAME\n" + bytes(64 * 48 * 3 // 2)) * 8)
    got = {}
    for name, extra in (("none", []), ("lag0", ["-av1mi_grain_lag", "0"]), ("lag3", ["-av1mi_grain_lag", "3"])):
        cfg, target, switches, err = av1mi.GopConfig(), (C.c_int * 3)(), (C.c_int * 5)(), C.create_string_buffer(1024)
        argv = ["av1mi", "-i", src, "-av1mi_denoise", "4", "-g", "4", "-av1mi_segments", "2"] + extra + [src + ".mkv"]
        assert host.av1mi_host_session_config("\n".join(argv).encode(), None, C.byref(cfg), target, switches, err, 1024) == 0, err.value
        got[name] = {k: getattr(cfg, k) for k, _ in av1mi.GopConfig._fields_}
    assert got["none"]["grain_cov"] == 0 and got["lag0"] == got["none"] and got["lag3"] == dict(got["none"], grain_cov=1)
