"""Tone mapping PQ / BT.2020 -> SDR / BT.709: the arithmetic of include/av1mi.h "tone mapping", restated in numpy.

constants()      the Q14 constants, derived with fractions from the formulas
tables(peak)     the four tables from the formulas in numpy doubles (what av1mi_tone_map_tables builds on the host)
tone_map(...)    the integer chain over planar 4:2:0 10-bit planes, per 2x2 luma quad: what k_tone_map computes, bit for bit
float_model(...) the same chain in doubles without tables or roundings between the steps: the accuracy yardstick
"""
from fractions import Fraction as F

import numpy as np

LO = 512                 # the OETF's direct entries: linear values 0 .. 511
HI_OCTAVES = 6           # then octaves 2^9 .. 2^15 of 64 intervals each, nodes in Q6
HI_NODES = HI_OCTAVES * 64 + 1
SDR_PEAK = 100 << 8      # 100 cd/m2 in 2^-8 cd/m2


def _rnd(x):
    """nearest integer of a Fraction, halves away from zero"""
    x = F(x)
    return int(x + F(1, 2)) if x >= 0 else -int(-x + F(1, 2))


def _inv3(m):
    (a, b, c), (d, e, f), (g, h, i) = m
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    return [[(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det],
            [(f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det],
            [(d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det]]


def _mul3(a, b):
    return [[sum(a[r][k] * b[k][c] for k in range(3)) for c in range(3)] for r in range(3)]


def _rgb_to_xyz(prim, white):
    """the matrix of a set of primaries ((xr, yr), (xg, yg), (xb, yb)) with the white point (xw, yw): columns scaled so that RGB = 1 gives white"""
    cols = [[x / y, F(1), (1 - x - y) / y] for x, y in prim]
    m = [[cols[c][r] for c in range(3)] for r in range(3)]
    xw, yw = white
    s = [sum(row[k] * v for k, v in enumerate([xw / yw, F(1), (1 - xw - yw) / yw])) for row in _inv3(m)]
    return [[m[r][c] * s[c] for c in range(3)] for r in range(3)]


def _to_sum(row, total):
    """Q14 row whose rounded entries are made to sum to `total`: the remainder goes to the entry of largest magnitude (the first of equals)"""
    q = [_rnd(v * 16384) for v in row]
    big = max(range(3), key=lambda k: (abs(q[k]), -k))
    q[big] += total - sum(q)
    return q


D65 = (F(3127, 10000), F(3290, 10000))
P2020 = ((F(708, 1000), F(292, 1000)), (F(170, 1000), F(797, 1000)), (F(131, 1000), F(46, 1000)))
P709 = ((F(64, 100), F(33, 100)), (F(30, 100), F(60, 100)), (F(15, 100), F(6, 100)))


def gamut_matrix():
    """BT.2020 -> BT.709 linear RGB, exact"""
    return _mul3(_inv3(_rgb_to_xyz(P709, D65)), _rgb_to_xyz(P2020, D65))


def constants():
    kr, kb = F(2627, 10000), F(593, 10000)
    kg = 1 - kr - kb
    c = {}
    # 1. Y'CbCr (limited, 10 bit) -> R'G'B' codes 0 .. 1023: E = (Y - 64) / 876, Cb = (U - 512) / 896
    c["to_rgb"] = [_rnd(F(16384 * 1023, 876)), _rnd(F(16384 * 1023, 896) * 2 * (1 - kr)), _rnd(F(16384 * 1023, 896) * 2 * kr * (1 - kr) / kg),
                   _rnd(F(16384 * 1023, 896) * 2 * kb * (1 - kb) / kg), _rnd(F(16384 * 1023, 896) * 2 * (1 - kb))]      # y, rv, gv, gu, bu
    # 4. gamut: rows sum to 16384
    c["gamut"] = [_to_sum(row, 16384) for row in gamut_matrix()]
    # 7. R'G'B' codes -> BT.709 Y'CbCr limited: the Cb and Cr rows sum to 0
    kr, kb = F(2126, 10000), F(722, 10000)
    kg = 1 - kr - kb
    sy, sc = F(876, 1023), F(896, 1023)
    c["to_yuv"] = [[_rnd(v * sy * 16384) for v in (kr, kg, kb)],
                   _to_sum([v * sc for v in (-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), F(1, 2))], 0),
                   _to_sum([v * sc for v in (F(1, 2), -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr)))], 0)]
    return c


M1, M2 = 2610.0 / 16384, 2523.0 / 4096 * 128
C1, C2, C3 = 3424.0 / 4096, 2413.0 / 4096 * 32, 2392.0 / 4096 * 32


def pq_eotf(e):
    """PQ signal 0 .. 1 -> cd/m2 (SMPTE ST 2084)"""
    p = np.power(np.asarray(e, np.float64), 1.0 / M2)
    return 10000.0 * np.power(np.maximum(p - C1, 0.0) / (C2 - C3 * p), 1.0 / M1)


def pq_inv(l):
    """cd/m2 -> PQ signal"""
    y = np.power(np.asarray(l, np.float64) / 10000.0, M1)
    return np.power((C1 + C2 * y) / (1.0 + C3 * y), M2)


def eetf(e, peak):
    """BT.2390 EETF on PQ signals: a source of 0 .. peak cd/m2 to a display of 0 .. 100 cd/m2 (black level 0 on both sides)"""
    src = pq_inv(peak)
    e1 = np.minimum(np.asarray(e, np.float64) / src, 1.0)
    mx = pq_inv(100.0) / src
    ks = 1.5 * mx - 0.5
    t = np.clip((e1 - ks) / (1.0 - ks), 0.0, 1.0)
    p = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1 - ks) + (-2 * t ** 3 + 3 * t ** 2) * mx
    return np.where(e1 < ks, e1, p) * src


def oetf709(l):
    """linear light 0 .. 1 (and beyond) -> BT.709 signal"""
    l = np.asarray(l, np.float64)
    return np.where(l < 0.018, 4.5 * l, 1.099 * np.power(np.maximum(l, 0.018), 0.45) - 0.099)


def gain_curve(m, peak):
    """linear gain for the PQ signal m (0 .. 1): what the EETF does to the largest component, as a ratio of light"""
    m = np.asarray(m, np.float64)
    lin = pq_eotf(m)
    return np.where(lin > 0, pq_eotf(eetf(m, peak)) / np.where(lin > 0, lin, 1.0), 1.0)


def tables(peak):
    code = np.arange(1024) / 1023.0
    lin = np.floor(pq_eotf(code) * 256.0 + 0.5).astype(np.int64)
    gain = np.floor(gain_curve(code, peak) * 65536.0 + 0.5).astype(np.int64)
    out = lambda m: min((int(lin[m]) * int(gain[m]) + 32768) >> 16, SDR_PEAK)
    for m in range(1, 1024):      # the neutral axis never loses light: step 5's result is made non-decreasing, a step of one where the rounding broke it
        while out(m) < out(m - 1):
            gain[m] += 1
    lo = np.floor(oetf709(np.arange(LO) / float(SDR_PEAK)) * 1023.0 + 0.5).astype(np.int64)
    x = np.concatenate([(64 + np.arange(64)) << (k - 6) for k in range(9, 9 + HI_OCTAVES)] + [np.array([1 << (9 + HI_OCTAVES)])])
    hi = np.floor(oetf709(x / float(SDR_PEAK)) * 1023.0 * 64.0 + 0.5).astype(np.int64)
    return {"lin": lin, "gain": gain, "oetf_lo": lo, "oetf_hi": hi}


def _oetf(c, T):
    """linear 0 .. SDR_PEAK -> code 0 .. 1023: direct below LO, else the octave's nodes and linear interpolation"""
    c = np.asarray(c, np.int64)
    big = np.maximum(c, LO)
    k = np.floor(np.log2(big)).astype(np.int64)      # exact for integers below 2^53
    sh = k - 6
    idx = (k - 9) * 64 + (big >> sh) - 64
    frac = big & ((1 << sh) - 1)
    v = T["oetf_hi"][idx] * ((1 << sh) - frac) + T["oetf_hi"][idx + 1] * frac
    hi = np.minimum((v + (1 << (sh + 5))) >> (sh + 6), 1023)
    return np.where(c < LO, T["oetf_lo"][np.minimum(c, LO - 1)], hi)


def tone_map(Y, U, V, T, K=None):
    """planar 4:2:0 10-bit planes (Y: rows x w, U / V: rows / 2 x w / 2; any number of stacked frames of even height) -> the same, tone-mapped"""
    K = K or constants()
    Y = np.asarray(Y, np.int64); U = np.asarray(U, np.int64); V = np.asarray(V, np.int64)
    u = np.repeat(np.repeat(U, 2, 0), 2, 1) - 512
    v = np.repeat(np.repeat(V, 2, 0), 2, 1) - 512
    cy, rv, gv, gu, bu = K["to_rgb"]
    y = cy * (Y - 64) + 8192
    rgb = [np.clip((y + rv * v) >> 14, 0, 1023), np.clip((y - gv * v - gu * u) >> 14, 0, 1023), np.clip((y + bu * u) >> 14, 0, 1023)]
    m = np.maximum(np.maximum(rgb[0], rgb[1]), rgb[2])
    lin = [T["lin"][c] for c in rgb]
    g = T["gain"][m]
    out = []
    for row in K["gamut"]:
        c = np.maximum((row[0] * lin[0] + row[1] * lin[1] + row[2] * lin[2] + 8192) >> 14, 0)
        c = np.minimum((c * g + 32768) >> 16, SDR_PEAK)
        out.append(_oetf(c, T))
    ky, ku, kv = K["to_yuv"]
    dot = lambda k: k[0] * out[0] + k[1] * out[1] + k[2] * out[2]
    Yo = np.clip(64 + ((dot(ky) + 8192) >> 14), 0, 1023)
    quad = lambda a: a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    Uo = np.clip(512 + ((quad(dot(ku)) + 32768) >> 16), 0, 1023)
    Vo = np.clip(512 + ((quad(dot(kv)) + 32768) >> 16), 0, 1023)
    return Yo.astype(np.uint16), Uo.astype(np.uint16), Vo.astype(np.uint16)


def float_model(Y, U, V, peak):
    """the chain in doubles: no tables, no rounding until the end (Y per pixel, U / V the mean of the quad).  Returns doubles"""
    Y = np.asarray(Y, np.float64); U = np.asarray(U, np.float64); V = np.asarray(V, np.float64)
    u = (np.repeat(np.repeat(U, 2, 0), 2, 1) - 512) / 896.0
    v = (np.repeat(np.repeat(V, 2, 0), 2, 1) - 512) / 896.0
    e = (Y - 64) / 876.0
    kr, kb = 0.2627, 0.0593
    kg = 1 - kr - kb
    # (the codes are not quantised here, but the clamp to the PQ signal range is part of the definition)
    r = np.clip(e + 2 * (1 - kr) * v, 0, 1); b = np.clip(e + 2 * (1 - kb) * u, 0, 1)
    g = np.clip(e - 2 * kr * (1 - kr) / kg * v - 2 * kb * (1 - kb) / kg * u, 0, 1)
    gn = gain_curve(np.maximum(np.maximum(r, g), b), peak)
    lin = [pq_eotf(c) for c in (r, g, b)]
    M = [[float(x) for x in row] for row in gamut_matrix()]
    out = [oetf709(np.minimum(np.maximum(row[0] * lin[0] + row[1] * lin[1] + row[2] * lin[2], 0) * gn, 100.0) / 100.0) for row in M]
    kr, kb = 0.2126, 0.0722
    kg = 1 - kr - kb
    yy = kr * out[0] + kg * out[1] + kb * out[2]
    quad = lambda a: (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) / 4.0
    return 64 + 876 * yy, 512 + 896 * quad((out[2] - yy) / (2 * (1 - kb))), 512 + 896 * quad((out[0] - yy) / (2 * (1 - kr)))
