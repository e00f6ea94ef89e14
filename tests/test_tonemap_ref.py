"""CPU tests of tone mapping (include/av1mi.h "tone mapping"): av1mi_tone_map_tables against the formulas in numpy doubles, the constants against
fractions, and the integer chain's properties and accuracy (tests/tonemap_ref.py).  No GPU."""
import numpy as np
import pytest

import tonemap_ref as R

PEAKS = [400, 1000, 4000, 10000]
# the integer chain against the chain in doubles, worst absolute difference in codes as MEASURED here over all Y x a 9 x 9 grid of (U, V) and 1e5
# random triples (the worst of the four peaks): everything, and luma over every colour inside the BT.709 gamut.  Outside the gamut a component
# that the matrix brings close to 0 carries the rounding of the other two's 10-bit PQ codes, which the steep foot of the OETF magnifies.
WORST_ALL = {"y": 4.17, "u": 2.77, "v": 9.54}
WORST_IN_GAMUT_Y = 3.59


@pytest.fixture(scope="module")
def lib_tables(av1mi):
    return {p: av1mi.tone_map_tables(p) for p in PEAKS}


@pytest.mark.parametrize("peak", PEAKS)
def test_tables_are_the_formulas(lib_tables, peak):
    t, T = lib_tables[peak], R.tables(peak)
    for k, want in T.items():
        got = np.array(getattr(t, k), np.int64)[:len(want)]
        assert np.abs(got - want).max() <= 1, k
    assert t.peak == peak
    assert t.lin[0] == 0 and t.lin[1023] == 10000 * 256 and t.gain[0] == 65536 and t.oetf_lo[0] == 0
    light = np.minimum((np.array(t.lin, np.int64) * np.array(t.gain, np.int64) + 32768) >> 16, R.SDR_PEAK)
    assert (np.diff(light) >= 0).all() and light[-1] == R.SDR_PEAK


def test_peak_out_of_range_is_refused(av1mi):
    for peak in (99, 10001, 0, -5):
        with pytest.raises(ValueError):
            av1mi.tone_map_tables(peak)


def test_constants_are_the_fractions(lib_tables):
    t, K = lib_tables[1000], R.constants()
    assert list(t.to_rgb) == K["to_rgb"] and [list(r) for r in t.gamut] == K["gamut"] and [list(r) for r in t.to_yuv] == K["to_yuv"]
    assert all(sum(r) == 16384 for r in K["gamut"]) and sum(K["to_yuv"][1]) == 0 and sum(K["to_yuv"][2]) == 0


@pytest.mark.parametrize("source", ["library", "formulas"])
@pytest.mark.parametrize("peak", PEAKS)
def test_neutral_axis(lib_tables, peak, source):
    """U = V = 512 stays 512 for all 1024 Y codes, and Y out never falls as Y in rises: with the library's tables and constants, and with the reference's"""
    if source == "library":
        t = lib_tables[peak]
        T = {k: np.array(getattr(t, k), np.int64) for k in ("lin", "gain", "oetf_lo", "oetf_hi")}
        K = {"to_rgb": list(t.to_rgb), "gamut": [list(r) for r in t.gamut], "to_yuv": [list(r) for r in t.to_yuv]}
    else:
        T, K = R.tables(peak), R.constants()
    Y = np.repeat(np.arange(1024), 2)[None, :].repeat(2, 0)
    U = np.full((1, 1024), 512)
    yo, uo, vo = R.tone_map(Y, U, U, T, K)
    assert (uo == 512).all() and (vo == 512).all()
    assert (np.diff(yo[0].astype(int)) >= 0).all() and yo[0, 0] == 64 and yo[0, -1] == 940


def _in_gamut(Y, U, V):
    """legal R'G'B' whose three BT.709 linear components, before the clamp at 0, are not negative"""
    e = (Y - 64) / 876.0
    u = (np.repeat(np.repeat(U, 2, 0), 2, 1) - 512) / 896.0
    v = (np.repeat(np.repeat(V, 2, 0), 2, 1) - 512) / 896.0
    r, b = e + 2 * (1 - 0.2627) * v, e + 2 * (1 - 0.0593) * u
    g = (e - 0.2627 * r - 0.0593 * b) / 0.678
    ok = (np.minimum(np.minimum(r, g), b) >= 0) & (np.maximum(np.maximum(r, g), b) <= 1)
    lin = [R.pq_eotf(np.clip(c, 0, 1)) for c in (r, g, b)]
    out = [sum(float(m) * l for m, l in zip(row, lin)) for row in R.gamut_matrix()]
    return ok & (np.minimum(np.minimum(out[0], out[1]), out[2]) >= 0)


@pytest.mark.parametrize("peak", PEAKS)
def test_accuracy_against_the_float_model(lib_tables, peak):
    """the integer chain WITH THE LIBRARY'S TABLES against the chain in doubles"""
    t = lib_tables[peak]
    T = {k: np.array(getattr(t, k), np.int64) for k in ("lin", "gain", "oetf_lo", "oetf_hi")}
    g = np.linspace(0, 1023, 9).round().astype(np.int64)
    uv = np.array([(a, b) for a in g for b in g])
    Yg = np.tile(np.repeat(np.arange(1024), 2), (2 * 81, 1))
    Ug, Vg = np.repeat(uv[:, 0:1], 1024, 1), np.repeat(uv[:, 1:2], 1024, 1)
    rng = np.random.default_rng(peak)
    Yr = np.repeat(np.repeat(rng.integers(0, 1024, (250, 400)), 2, 0), 2, 1)      # 1e5 triples, the quad's four pixels alike
    Ur, Vr = rng.integers(0, 1024, (250, 400)), rng.integers(0, 1024, (250, 400))
    worst = {"y": 0.0, "u": 0.0, "v": 0.0, "in": 0.0}
    for Y, U, V in ((Yg, Ug, Vg), (Yr, Ur, Vr)):
        got, want = R.tone_map(Y, U, V, T), R.float_model(Y, U, V, peak)
        for k, a, b in zip("yuv", got, want):
            worst[k] = max(worst[k], float(np.abs(a - b).max()))
        m = _in_gamut(Y.astype(np.float64), U.astype(np.float64), V.astype(np.float64))
        worst["in"] = max(worst["in"], float(np.abs(got[0] - want[0])[m].max()))
    print("peak %d: worst |integer - float| Y %.2f U %.2f V %.2f; Y inside the BT.709 gamut %.2f" % (peak, worst["y"], worst["u"], worst["v"], worst["in"]))
    for k in "yuv":
        assert worst[k] <= WORST_ALL[k] + 1, (k, worst)
    assert worst["in"] <= WORST_IN_GAMUT_Y + 1, worst
