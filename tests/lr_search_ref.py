"""The restoration search restated (include/av1mi.h "restoration search"): the candidates, the exact bits of a record, lambda, the
cost table and the pick, from the oracle's restoration of a whole plane per candidate.  Nothing here reads the library."""
import numpy as np

UNIT = 64
CANDIDATES = 9
# the 1-D filters per plane class as (tap0, tap1, tap2): I (identity), D (the policy's), L (a low-pass)
FILTERS = (((0, 0, 0), (3, -7, 15), (0, 2, 14)),        # luma
           ((0, 0, 0), (0, -7, 15), (0, 2, 14)))        # chroma: tap0 is not coded, so it is 0
POLICY = 4                                               # (D, D): the record of av1mi_frame_params
# the Wiener taps' syntax (spec 5.11.58): range, subexponential parameter k and the default reference per tap
TAP_MIN, TAP_MAX, TAP_K, TAP_REF = (-5, -23, -17), (10, 8, 46), (1, 2, 3), (3, -7, 15)


def record(chroma, c):
    """candidate c's 8-byte unit record: 0 is "none", c >= 1 the Wiener record with vertical filter c // 3 and horizontal filter c % 3"""
    if c == 0:
        return [0] * 8
    assert 1 <= c < CANDIDATES
    f = FILTERS[1 if chroma else 0]
    return [1, *f[c // 3], *f[c % 3], 0]


def _subexp_bits(num_syms, k, v):
    """literal bits of decode_subexp_bool (spec 4.10.10 structure) for the value v of num_syms"""
    i, mk, bits = 0, 0, 0
    while True:
        b2 = k + i - 1 if i else k
        a = 1 << b2
        if num_syms <= mk + 3 * a:
            n, x = num_syms - mk, v - mk                  # NS(n)
            w = n.bit_length()
            m = (1 << w) - n
            return bits + (w - 1 if x < m else w)
        bits += 1                                         # subexp_more_bools
        if v < mk + a:
            return bits + b2
        i, mk = i + 1, mk + a


def _recenter(r, v):
    return v if v > 2 * r else 2 * (v - r) if v >= r else 2 * (r - v) - 1


def tap_bits(v, j):
    """decode_signed_subexp_with_ref_bool of tap j's value v against the default reference"""
    mx = TAP_MAX[j] + 1 - TAP_MIN[j]
    v, r = v - TAP_MIN[j], TAP_REF[j] - TAP_MIN[j]
    return _subexp_bits(mx, TAP_K[j], _recenter(r, v) if (r << 1) <= mx else _recenter(mx - 1 - r, mx - 1 - v))


def bits(chroma, c):
    """bits_c: 1 for use_wiener, plus the literals of the record's taps (vertical, then horizontal; chroma codes no tap0)"""
    rec = record(chroma, c)
    if rec[0] != 1:
        return 1
    return 1 + sum(tap_bits(rec[1 + 3 * ps + j], j) for ps in range(2) for j in range(1 if chroma else 0, 3))


def lam(O, q, bd):
    return (3 * O.dc_q(q, bd) ** 2) >> 7


def unit_map(O, h, w, ss):
    """[h, w] -> the unit (raster index) a plane's sample is restored with (spec 7.17: the unit rows start 8 luma rows above the
    multiples of the unit size, the last unit of a row / column takes what is left)"""
    rows, cols = O.lr_units(UNIT, h), O.lr_units(UNIT, w)
    ur = np.minimum((np.arange(h) + (8 >> ss)) // UNIT, rows - 1)
    uc = np.minimum(np.arange(w) // UNIT, cols - 1)
    return ur[:, None] * cols + uc[None, :], rows * cols


def sse_table(O, cdef, dbl, src, bd, ss):
    """[unit, candidate] int64: the squared error against src of the plane restored with candidate c in every unit, per unit"""
    h, w = cdef.shape
    umap, n = unit_map(O, h, w, ss)
    rows, cols = O.lr_units(UNIT, h), O.lr_units(UNIT, w)
    out = np.zeros((n, CANDIDATES), np.int64)
    for c in range(CANDIDATES):
        units = np.tile(np.array(record(ss, c), np.int8), (rows, cols, 1))
        lr = O.lr_plane(cdef, dbl, bd, ss, UNIT, units)
        e = (lr.astype(np.int64) - src.astype(np.int64)) ** 2
        out[:, c] = [e[umap == u].sum() for u in range(n)]
    return out


def pick(table, chroma, lmb):
    """the arg-min of J = SSE + lambda * bits per unit, the lowest index on a tie; returns (indices, J [unit, candidate])"""
    j = table + lmb * np.array([bits(chroma, c) for c in range(CANDIDATES)], np.int64)[None, :]
    return np.argmin(j, axis=1), j                      # (numpy's argmin returns the first minimum)


def frame_tables(O, cdef, dbl, src, bd):
    """the three planes' tables of a 4:2:0 frame end to end, in the library's order: Y's units, U's, V's"""
    return np.concatenate([sse_table(O, cdef[p], dbl[p], src[p], bd, int(p > 0)) for p in range(3)])
