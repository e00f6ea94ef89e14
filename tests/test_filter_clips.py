"""The clips of tests/filter_clips.py do what they are there for, and the oracle's filters are the decoder's on them — CPU only.

First the pin: every clip is coded as a key frame at q index 1 (the reconstruction keeps the extremes), the stream carries the filter
parameters of filter_clips (deblocking level sets and sharpness, CDEF strength sets per superblock at damping 3 and 6 with skipped
blocks, Wiener units with every tap at an end of its range, the self-guided sets 0, 9, 10, 14, 15 with their weights at the ends), and
dav1d's planes after deblocking, after CDEF and after restoration equal O.deblock_plane / O.cdef_frame / O.lr_plane bit for bit.

Then the content: the deblocking masks, the narrow filter, the CDEF filter and the horizontal Wiener pass are restated in numpy on exact
integers (and held against the oracle where they overlap), and what the clips are built for is counted: edge lines at and one above
every threshold, lines the narrow filter's clamps change, blocks of variance 0 and at the cap, samples the min / max clamp decides,
Wiener units whose intermediate leaves its range, samples at both ends after every stage.  Every count must be at least 1 at each
depth; the counts observed are in the docstrings (`python tests/test_filter_clips.py` prints them)."""
import functools
import os
import sys

import numpy as np
import pytest

import dav1d_ref as D
import filter_clips as FC

DEPTHS = (8, 10)
CONTENT_SIZE = (136, 72)      # (w, h) the counts are taken at


def _oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from oracle import oracle
    oracle.build()
    return oracle


def _uniform_maps(O, w, h, lv):
    return (np.full((h // 4, w // 4), int(O.lf_mi(3, 3, lv[0], lv[1])), np.uint32), np.full((h // 8, w // 8), int(O.lf_mi(2, 2, lv[2], lv[2])), np.uint32),
            np.full((h // 8, w // 8), int(O.lf_mi(2, 2, lv[3], lv[3])), np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against dav1d on this content
def _recipe(O, k, w, h):
    """filter parameters number k of a w x h stream: (levels, sharpness, damping, the strength sets, an index per superblock, lr types,
    units per plane).  Over k in 0 .. 4 every level set, both dampings, every strength set in every superblock position, Wiener planes,
    self-guided planes and switchable ones occur."""
    lv, sharp = FC.LF_SETS[k % len(FC.LF_SETS)]
    damping = (3, 6)[k % 2]
    nsb = ((h + 63) // 64) * ((w + 63) // 64)
    sets = np.array(FC.CDEF_SETS + ((7, 1, 6, 2),), np.uint8)
    idx = ((np.arange(nsb) + k) % 4).astype(np.uint8)
    lrt = ((1, 1, 2), (2, 2, 1), (3, 3, 3), (1, 2, 3), (2, 1, 1))[k % 5]
    kind = {1: "wiener", 2: "sgr", 3: "mixed"}
    units = [FC.lr_unit_map(O, w >> int(p > 0), h >> int(p > 0), 64 >> int(p > 0), kind[lrt[p]], chroma=p > 0, shift=k + p) for p in range(3)]
    return lv, sharp, damping, sets, idx, lrt, units


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("w,h", FC.SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_oracle_filters_equal_dav1d_on_the_clips(bd, w, h, k):
    """per clip: key frame at q index 1 -> stream with recipe k -> dav1d with inloop_filters = deblock, deblock + CDEF, all"""
    if D.load() is None:
        pytest.skip("no dav1d in this image (pillow.libs/libavif)")
    import av1stream
    O = _oracle()
    rng = np.random.default_rng([bd, w, h, k])
    skipped = 0
    for name in FC.NAMES:
        Y, U, V = FC.clip(name, w, h, bd)
        r = O.intra_encode_frame(Y, U, V, bd, 8, 1)
        rec = [r["rec_y"], r["rec_u"], r["rec_v"]]
        nb = (w // 8) * (h // 8)
        allz = (np.abs(r["lev_y"]).reshape(nb, -1).sum(1) + np.abs(r["lev_u"]).reshape(nb, -1).sum(1) + np.abs(r["lev_v"]).reshape(nb, -1).sum(1)) == 0
        skip = (allz & (rng.random(nb) < 0.7)).astype(np.uint8)
        skipped += int(skip.sum())
        lv, sharp, damping, sets, idx, lrt, units = _recipe(O, k, w, h)
        mi = _uniform_maps(O, w, h, lv)
        dbl = [O.deblock_plane(rec[p], bd, int(p > 0), mi[p], sharp) for p in range(3)]
        cdef = O.cdef_frame(dbl[0], dbl[1], dbl[2], bd, damping, sets[idx], skip.reshape(h // 8, w // 8))
        out = [O.lr_plane(cdef[p], dbl[p], bd, int(p > 0), 64 >> int(p > 0), units[p]) for p in range(3)]
        tu = av1stream.temporal_unit(w, h, bd, 1, y_mode=r["modes_y"], uv_mode=r["modes_uv"], lev_y=r["lev_y"], lev_u=r["lev_u"], lev_v=r["lev_v"],
                                     skip=skip, lf_level=lv, lf_sharpness=sharp, cdef_damping=damping, cdef_bits=2,
                                     cdef_y=[int(a) << 2 | int(b) for a, b in sets[:, :2]], cdef_uv=[int(a) << 2 | int(b) for a, b in sets[:, 2:]],
                                     cdef_idx=idx, lr_type=lrt, lr_unit_shift=0, lr_uv_shift=1, lr_units=units)
        for stage, flt, ref in (("deblocked", D.INLOOP_DEBLOCK, dbl), ("cdef", D.INLOOP_DEBLOCK | D.INLOOP_CDEF, cdef), ("restored", D.INLOOP_ALL, out)):
            got = D.decode(tu, inloop_filters=flt)[0]
            for p in range(3):
                assert (got[p] == ref[p]).all(), ("clip %s, %dx%d, %d bit, recipe %d (levels %s sharpness %d, damping %d, lr %s): %s plane %d differs from dav1d at %s"
                                                  % (name, w, h, bd, k, lv, sharp, damping, lrt, stage, p, np.argwhere(got[p] != ref[p])[:4].tolist()))
        if name in ("binary", "checker1", "full_swing_blocks"):      # q index 1 keeps the extremes
            assert all(int((a == 0).sum()) > 0 and int((a == FC.top_of(bd)).sum()) > 0 for a in rec), name
    assert skipped > 0      # (the flat clips' blocks after the first have no levels)


# ---------------------------------------------------------------------------------------------------------------------
# the deblocking masks and the narrow filter, restated for a uniform map of 8x8 luma / 4x4 chroma transforms
def edge_lines(X, bs):
    """per vertical block edge and row the samples p3 .. p0 / q0 .. q3 (p1, p0 / q0, q1 for 4x4 blocks): two lists of [rows, edges]"""
    X = X.astype(np.int64)
    xs = np.arange(bs, X.shape[1], bs)
    n = 4 if bs == 8 else 2
    return [X[:, xs - 1 - i] for i in range(n)], [X[:, xs + i] for i in range(n)]


def masks(X, bs, lvl, sharp, bd):
    """the decisions of lf_filter on every line of edge_lines: what each comparison compares, and what comes of them"""
    sh = bd - 8
    lim, blim, hev = (v << sh for v in FC.lf_limits(lvl, sharp))
    P, Q = edge_lines(X, bs)
    ad = lambda a, b: np.abs(a - b)
    d10 = np.maximum(ad(P[1], P[0]), ad(Q[1], Q[0]))
    m, fl = d10, d10
    for i in range(2, len(P)):
        m = np.maximum(m, np.maximum(ad(P[i], P[i - 1]), ad(Q[i], Q[i - 1])))
        fl = np.maximum(fl, np.maximum(ad(P[i], P[0]), ad(Q[i], Q[0])))
    bl = 2 * ad(P[0], Q[0]) + ad(P[1], Q[1]) // 2
    mask = (m <= lim) & (bl <= blim)
    flat = (fl <= (1 << sh)) if len(P) == 4 else np.zeros_like(mask)
    return dict(P=P, Q=Q, d10=d10, m=m, fl=fl, bl=bl, lim=lim, blim=blim, hev=hev, mask=mask, flat=mask & flat, narrow=mask & ~flat)


def narrow_filter(P, Q, hev_t, bd, clamped=True):
    """filter4 of the spec (7.14.6.2) on arrays of lines, mask passed; clamped=False: every clamp to [-128, 127] << (bd - 8) left out"""
    sh = bd - 8
    lo, hi, t80 = -(128 << sh), (128 << sh) - 1, 128 << sh
    c = (lambda v: np.clip(v, lo, hi)) if clamped else (lambda v: v)
    ps1, ps0, qs0, qs1 = P[1] - t80, P[0] - t80, Q[0] - t80, Q[1] - t80
    hev = np.maximum(np.abs(P[1] - P[0]), np.abs(Q[1] - Q[0])) > hev_t
    f = c(np.where(hev, c(ps1 - qs1), 0) + 3 * (qs0 - ps0))
    f1, f2 = c(f + 4) >> 3, c(f + 3) >> 3
    f3 = np.where(hev, 0, (f1 + 1) >> 1)
    return [c(ps1 + f3) + t80, c(ps0 + f2) + t80, c(qs0 - f1) + t80, c(qs1 - f3) + t80]      # p1, p0, q0, q1


_LF_KEYS = ("m_at", "m_above", "blim_at", "blim_above", "hev_at", "hev_above", "flat_0", "flat_at", "flat_above", "narrow_lines", "clamp_changed")


def _count_pass(o, X, after, bs, lvl, sharp, bd):
    """adds one pass over plane X (edges vertical; `after`: the oracle's plane after this pass) to the counts o — each comparison counted
    where the others let it decide — and holds the restatement against the oracle on the way"""
    if lvl == 0:
        assert (after == X).all()
        return
    k = masks(X, bs, lvl, sharp, bd)
    one = 1 << (bd - 8)
    other_m, other_bl = k["bl"] <= k["blim"], k["m"] <= k["lim"]
    o["m_at"] += int(((k["m"] == k["lim"]) & other_m).sum())
    o["m_above"] += int(((k["m"] == k["lim"] + 1) & other_m).sum())
    o["blim_at"] += int(((k["bl"] == k["blim"]) & other_bl).sum())
    o["blim_above"] += int(((k["bl"] == k["blim"] + 1) & other_bl).sum())
    o["hev_at"] += int((k["narrow"] & (k["d10"] == k["hev"])).sum())
    o["hev_above"] += int((k["narrow"] & (k["d10"] == k["hev"] + 1)).sum())
    if bs == 8:
        o["flat_0"] += int((k["mask"] & (k["fl"] == 0)).sum())
        o["flat_at"] += int((k["mask"] & (k["fl"] == one)).sum())
        o["flat_above"] += int((k["mask"] & (k["fl"] == one + 1)).sum())
    with_c, without = narrow_filter(k["P"], k["Q"], k["hev"], bd), narrow_filter(k["P"], k["Q"], k["hev"], bd, clamped=False)
    o["narrow_lines"] += int(k["narrow"].sum())
    o["clamp_changed"] += int((k["narrow"] & np.any([a != b for a, b in zip(with_c, without)], axis=0)).sum())
    # the oracle agrees: a line the mask stops is unchanged, a line of the narrow filter is the restated one
    Pa, Qa = edge_lines(after, bs)
    for i in range(len(Pa)):
        assert (Pa[i][~k["mask"]] == k["P"][i][~k["mask"]]).all() and (Qa[i][~k["mask"]] == k["Q"][i][~k["mask"]]).all()
    n = k["narrow"]
    for got, want in zip((Pa[1], Pa[0], Qa[0], Qa[1]), with_c):
        assert (got[n] == want[n]).all()


@functools.lru_cache(maxsize=None)
def observe_deblock(bd):
    """the counts over every clip, level set and plane at CONTENT_SIZE; and, for the key map's 32x32 luma transforms (filter length 14),
    how many lines have the outer samples p4 .. p6 / q4 .. q6 exactly 0, 1 << (bd - 8) and one more away from p0 / q0"""
    O = _oracle()
    w, h = CONTENT_SIZE
    o = dict.fromkeys(_LF_KEYS + ("flat2_0", "flat2_at", "flat2_above"), 0)
    one = 1 << (bd - 8)
    for name in FC.NAMES:
        planes = FC.clip(name, w, h, bd)
        for lv, sharp in FC.LF_SETS:
            mi = _uniform_maps(O, w, h, lv)
            for p in range(3):
                bs, lvl = (8, lv[:2]) if p == 0 else (4, (lv[1 + p], lv[1 + p]))
                first = O.deblock_plane(planes[p], bd, int(p > 0), mi[p], sharp, pass_mask=1)
                both = O.deblock_plane(planes[p], bd, int(p > 0), mi[p], sharp)
                _count_pass(o, planes[p], first, bs, lvl[0], sharp, bd)
                _count_pass(o, first.T, both.T, bs, lvl[1], sharp, bd)
        X = planes[0].astype(np.int64)[:h // 64 * 64]
        xs = np.arange(32, w, 32)
        v = np.max([np.abs(X[:, xs - 1 - i] - X[:, xs - 1]) for i in (4, 5, 6)] + [np.abs(X[:, xs + i] - X[:, xs]) for i in (4, 5, 6)], axis=0)
        near = np.max([np.abs(X[:, xs - 1 - i] - X[:, xs - 1]) for i in (1, 2, 3)] + [np.abs(X[:, xs + i] - X[:, xs]) for i in (1, 2, 3)], axis=0) <= one
        for key, d in (("flat2_0", 0), ("flat2_at", one), ("flat2_above", one + 1)):
            o[key] += int((near & (v == d)).sum())
    return o


@pytest.mark.parametrize("bd", DEPTHS)
def test_deblocking_edges_sit_at_and_one_above_every_threshold(bd):
    """edge lines (a row of a vertical edge, a column of a horizontal one) over the 12 clips, the 5 level sets and the 3 planes at 136x72,
    each counted where the other comparisons let this one decide.  Observed, 8 bits / 10 bits:
    m == lim 942 / 347, lim + 1 525 / 320; 2 |p0 - q0| + |p1 - q1| / 2 == mblim 104 / 105, mblim + 1 80 / 56;
    d10 == hev under the narrow filter 24946 / 24287, hev + 1 1907 / 936; flat's largest difference 0: 35520 / 35941, at 1 << (bd - 8)
    1642 / 571, one more 666 / 397; flat2's (32x32 transforms) 0: 1020 / 1020, at 48 / 24, one more 8 / 8."""
    o = observe_deblock(bd)
    for k in ("m_at", "m_above", "blim_at", "blim_above", "hev_at", "hev_above", "flat_0", "flat_at", "flat_above", "flat2_0", "flat2_at", "flat2_above"):
        assert o[k] >= 1, (k, o)


@pytest.mark.parametrize("bd", DEPTHS)
def test_the_narrow_filters_clamps_change_lines(bd):
    """lines that take the narrow filter and come out differently when its clamps to [-128, 127] << (bd - 8) are left out (big_steps'
    steps of 45 .. 75 at level 63 are most of them).  Observed: 8 bits 3378 of 49983 narrow-filter lines, 10 bits 3482 of 49784."""
    o = observe_deblock(bd)
    assert o["clamp_changed"] >= 1 and o["narrow_lines"] > o["clamp_changed"], o


# ---------------------------------------------------------------------------------------------------------------------
# CDEF: the direction search's by-products and the filter of the luma plane, restated
_DIRS = (((-1, 1), (-2, 2)), ((0, 1), (-1, 2)), ((0, 1), (0, 2)), ((0, 1), (1, 2)), ((1, 1), (2, 2)), ((1, 0), (2, 1)), ((1, 0), (2, 0)), ((1, 0), (2, -1)))


def _msb(v):
    return int(v).bit_length() - 1


def _constrain(diff, thr, damping):
    if thr == 0:
        return np.zeros_like(diff)
    shift = max(0, damping - _msb(thr))
    mag = np.abs(diff)
    return np.sign(diff) * np.minimum(mag, np.maximum(0, thr - (mag >> shift)))


def cdef_luma(O, Y, bd, damping, st):
    """spec 7.15 on the luma plane with one strength set everywhere: (the filtered plane, the same before the min / max clamp, per 8x8 block
    the direction search's variance, per block whether it is flat)"""
    h, w = Y.shape
    cs = bd - 8
    X = np.full((h + 4, w + 4), -1, np.int64)
    X[2:-2, 2:-2] = Y
    out, raw = Y.astype(np.int64).copy(), Y.astype(np.int64).copy()
    var_of, flat_of = np.zeros((h // 8, w // 8), np.int64), np.zeros((h // 8, w // 8), bool)
    for by in range(h // 8):
        for bx in range(w // 8):
            blk = Y[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]
            d, var = O.cdef_find_dir(blk, bd)
            var_of[by, bx], flat_of[by, bx] = var, int(blk.min()) == int(blk.max())
            pri0, sec = st[0] << cs, (4 if st[1] == 3 else st[1]) << cs
            vs = min(_msb(var >> 6), 12) if var >> 6 else 0
            pri = (pri0 * (4 + vs) + 8) >> 4 if var else 0
            dirn = d if pri0 else 0
            pt = ((4, 2), (3, 3))[(pri >> cs) & 1]
            x = blk.astype(np.int64)
            total, mx, mn = np.zeros_like(x), x.copy(), x.copy()
            for k in range(2):
                for sgn in (-1, 1):
                    for dd, thr, wgt in ((dirn, pri, pt[k]), ((dirn + 2) & 7, sec, (2, 1)[k]), ((dirn + 6) & 7, sec, (2, 1)[k])):
                        dy, dx = sgn * _DIRS[dd][k][0], sgn * _DIRS[dd][k][1]
                        t = X[2 + by * 8 + dy:2 + by * 8 + dy + 8, 2 + bx * 8 + dx:2 + bx * 8 + dx + 8]
                        ok = t >= 0
                        total += np.where(ok, wgt * _constrain(t - x, thr, damping + cs), 0)
                        mx, mn = np.where(ok, np.maximum(mx, t), mx), np.where(ok, np.minimum(mn, t), mn)
            y = x + ((8 + total - (total < 0)) >> 4)
            raw[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = y
            out[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = np.clip(y, mn, mx)
    return out, raw, var_of, flat_of


@functools.lru_cache(maxsize=None)
def observe_cdef(bd):
    O = _oracle()
    w, h = CONTENT_SIZE
    o = dict(var0_not_flat=0, var0_flat=0, var_capped=0, clamp_decides=0)
    for name in FC.NAMES:
        Y, U, V = FC.clip(name, w, h, bd)
        for st, damping in ((FC.CDEF_SETS[0], 3), (FC.CDEF_SETS[1], 6)):
            out, raw, var_of, flat_of = cdef_luma(O, Y, bd, damping, st)
            ref = O.cdef_frame(Y, U, V, bd, damping, np.tile(np.array(st, np.uint8), (6, 1)), np.zeros((h // 8, w // 8), np.uint8))[0]
            assert (out == ref).all(), (name, st, damping, np.argwhere(out != ref)[:4])      # the restatement is the oracle's filter
            o["clamp_decides"] += int((out != raw).sum())
        o["var0_not_flat"] += int(((var_of == 0) & ~flat_of).sum())
        o["var0_flat"] += int(((var_of == 0) & flat_of).sum())
        o["var_capped"] += int(((var_of >> 6) >= (1 << 12)).sum())
    return o


@pytest.mark.parametrize("bd", DEPTHS)
def test_cdef_variance_is_zero_and_at_its_cap_and_the_clamp_decides(bd):
    """8x8 luma blocks over the 12 clips at 136x72: variance 0 on a block that is not flat (every direction ties, or the best and its
    opposite do: checkers, the plus, the X), variance >> 6 at or beyond 1 << 12 (the cap of the primary strength's adjustment), and
    output samples that the clamp to the taps' min / max changed, under (15, 3) at damping 3 and (1, 0) at damping 6.
    Observed, 8 bits / 10 bits: variance 0 not flat 335 / 355 (flat: 478 / 489), capped 524 / 524, clamp decides 8 / 8 samples (full_swing_blocks'
    samples 3 << (bd - 8) off their field: a difference of the full range gets the weight 0 and never reaches the clamp)."""
    o = observe_cdef(bd)
    assert o["var0_not_flat"] >= 1 and o["var0_flat"] >= 1 and o["var_capped"] >= 1 and o["clamp_decides"] >= 1, o


# ---------------------------------------------------------------------------------------------------------------------
# restoration: the horizontal Wiener pass, and the ends of the range after every stage
def wiener_rows(X, hf, bd):
    """the horizontal pass of spec 7.17.4 on every row of a plane (columns clamped to the plane), before its clip: Round2(sum, 3)"""
    X = np.pad(X.astype(np.int64), ((0, 0), (3, 3)), mode="edge")
    taps = [hf[0], hf[1], hf[2], 128 - 2 * (hf[0] + hf[1] + hf[2]), hf[2], hf[1], hf[0]]
    s = sum(t * X[:, i:X.shape[1] - 6 + i] for i, t in enumerate(taps))
    return (s + 4) >> 3


@functools.lru_cache(maxsize=None)
def observe_lr(bd):
    O = _oracle()
    w, h = CONTENT_SIZE
    offset, limit = 1 << (bd + 3), (1 << (bd + 5)) - 1
    o = dict(units_low=0, units_high=0, units=0)
    for f, name in enumerate(FC.NAMES):
        units = FC.lr_unit_map(O, w, h, 64, "wiener", shift=FC.lr_shift(f))
        X = FC.clip(name, w, h, bd)[0]
        for r in range(units.shape[0]):
            for c in range(units.shape[1]):
                rows = slice(max(0, r * 64 - 8), h if r == units.shape[0] - 1 else (r + 1) * 64 - 8)
                cols = slice(c * 64, w if c == units.shape[1] - 1 else (c + 1) * 64)
                v = wiener_rows(X, [int(t) for t in units[r, c, 4:7]], bd)[rows, cols]
                o["units"] += 1
                o["units_low"] += int((v < -offset).any())
                o["units_high"] += int((v > limit - offset).any())
    return o


@pytest.mark.parametrize("bd", DEPTHS)
def test_wiener_intermediate_hits_both_clamps(bd):
    """Wiener units (64x64, taps at the ends of their ranges) with a horizontal intermediate below -(1 << (bd + 3)) / above
    (1 << (bd + 5)) - 1 - (1 << (bd + 3)) before the clip.  Observed: 3 low and 3 high of 24 units at either depth (noise's and binary's units with the horizontal taps (-5, -23, -17) and
    (10, -23, -17), the only ones whose centre tap is large enough)."""
    o = observe_lr(bd)
    assert o["units_low"] >= 1 and o["units_high"] >= 1, o


@functools.lru_cache(maxsize=None)
def observe_stages(bd):
    """per stage: samples at 0 and at the top value over the clips, and the clips the stage changes nothing in"""
    O = _oracle()
    w, h = CONTENT_SIZE
    top = FC.top_of(bd)
    o = {s: dict(at_0=0, at_top=0, unchanged=[]) for s in ("deblocked", "cdef", "restored")}
    lv, sharp = FC.LF_SETS[1]
    mi = _uniform_maps(O, w, h, lv)
    for i, name in enumerate(FC.NAMES):
        rec = FC.clip(name, w, h, bd)
        dbl = [O.deblock_plane(rec[p], bd, int(p > 0), mi[p], sharp) for p in range(3)]
        cdef = O.cdef_frame(dbl[0], dbl[1], dbl[2], bd, 3, np.tile(np.array(FC.CDEF_SETS[0], np.uint8), (6, 1)), np.zeros((h // 8, w // 8), np.uint8))
        lr = [O.lr_plane(cdef[p], dbl[p], bd, int(p > 0), 64 >> int(p > 0), FC.lr_unit_map(O, w >> int(p > 0), h >> int(p > 0), 64 >> int(p > 0), "wiener", shift=i))
              for p in range(3)]
        for stage, before, after in (("deblocked", rec, dbl), ("cdef", dbl, cdef), ("restored", cdef, lr)):
            o[stage]["at_0"] += sum(int((a == 0).sum()) for a in after)
            o[stage]["at_top"] += sum(int((a == top).sum()) for a in after)
            if all((a == b).all() for a, b in zip(before, after)):
                o[stage]["unchanged"].append(name)
    return o


# A picture of 0 and the top value only cannot be changed by deblocking or CDEF, whatever the parameters: a deblocking mask passes only
# where neighbouring samples differ by at most lim <= 63, which leaves lines of equal samples, and CDEF's constrain() gives a difference
# of the full range the weight 0.  Those clips are there for the ties, the marks and the sums; restoration does change them.
_TWO_LEVEL = ("binary", "checker1", "checker2", "stripes", "stripes_across", "diag")
UNCHANGED = dict(deblocked=_TWO_LEVEL + FC.FLAT + ("full_swing_blocks",), cdef=_TWO_LEVEL + FC.FLAT, restored=FC.FLAT)


@pytest.mark.parametrize("bd", DEPTHS)
def test_every_stage_reaches_both_ends_and_changes_every_clip_it_can(bd):
    """the chain deblocking (level 63) -> CDEF (15, 3, damping 3) -> restoration (Wiener units, taps at their ends) at 136x72: samples at
    0 / at the top value after each stage, and the clips a stage leaves unchanged are exactly the flat ones and — for deblocking and CDEF —
    those of two levels (UNCHANGED above says why; full_swing_blocks' samples just off their field are what CDEF changes in it).
    Observed (at 0 / at top), 8 bits: deblocked 66012 / 65147, CDEF 65906 / 65068, restored 28870 / 28606; 10 bits: 66102 / 64882,
    65956 / 64796, 28977 / 28590."""
    o = observe_stages(bd)
    for stage, k in o.items():
        assert k["at_0"] >= 1 and k["at_top"] >= 1, (stage, k)
        assert sorted(k["unchanged"]) == sorted(UNCHANGED[stage]), (stage, k["unchanged"])


# ---------------------------------------------------------------------------------------------------------------------
# the clips themselves, and the error sums' room
@pytest.mark.parametrize("bd", DEPTHS)
def test_shapes_types_and_range(bd):
    top = FC.top_of(bd)
    for w, h in FC.SIZES:
        for name in FC.NAMES:
            c = FC.clip(name, w, h, bd)
            assert [a.shape for a in c] == [(h, w), (h // 2, w // 2), (h // 2, w // 2)], name
            assert all(a.dtype == (np.uint8 if bd == 8 else np.uint16) and int(a.max()) <= top for a in c), name
        for name in ("binary", "checker1", "full_swing_blocks", "big_steps"):      # both ends of the range in every plane
            assert all(int(a.min()) == 0 and int(a.max()) == top for a in FC.clip(name, w, h, bd)), name
        inv = FC.inverse_of(FC.clip("binary", w, h, bd), bd)
        assert all((a.astype(int) + b == top).all() for a, b in zip(inv, FC.clip("binary", w, h, bd)))
    for w, h in FC.LR_SIZES:
        assert FC.plane("binary", w, h, bd).shape == (h, w)
    # one superblock of SIZES' last is interior by the CDEF kernels' rule, none of the others
    interior = lambda w, h: [(x, y) for y in range((h + 63) // 64) for x in range((w + 63) // 64) if x > 0 and y > 0 and x * 64 + 66 <= w and y * 64 + 66 <= h]
    assert [interior(w, h) for w, h in FC.SIZES] == [[], [], [(1, 1)]]


def superblock_sums(rec, src, true_size):
    """per 64x64 superblock the squared error of the three planes inside the true size: exact Python ints"""
    tw, th = true_size
    h, w = rec[0].shape
    out = []
    for sy in range((h + 63) // 64):
        for sx in range((w + 63) // 64):
            e = 0
            for p in range(3):
                n, pw, ph = (64, tw, th) if p == 0 else (32, (tw + 1) // 2, (th + 1) // 2)
                d = (rec[p].astype(np.int64) - src[p].astype(np.int64))[:ph, :pw][sy * n:(sy + 1) * n, sx * n:(sx + 1) * n]
                e += int((d * d).sum())
            out.append(e)
    return out


def test_full_swing_sums_need_64_bits():
    """the unfiltered candidate of the searches on a binary reconstruction against its inverse: every sample errs by the top value.  At 10
    bits a whole superblock sums to 6144 x 1023^2 = 6 429 874 176, beyond 2^32; at 8 bits to 6144 x 255^2 = 399 513 600.  By the lane layout
    of search_sse.hpp (16 luma + 8 chroma samples a lane, 64 lanes a wave) the partial sums at 10 bits are 24 x 1023^2 = 25 116 696 a lane
    (the header's bound: below 2^25 = 33 554 432) and 1 607 468 544 a wave (below 2^31 = 2 147 483 648): three quarters of the room."""
    worst = {}
    for bd in DEPTHS:
        for (w, h), true_size in (((136, 72), (130, 70)), ((64, 64), (64, 64))):
            rec = FC.clip("binary", w, h, bd)
            sums = superblock_sums(rec, FC.inverse_of(rec, bd), true_size)
            worst[bd, w] = max(sums)
            assert max(sums) == 6144 * FC.top_of(bd) ** 2      # the first superblock is whole at both sizes
    assert worst[10, 136] > 1 << 31 and worst[10, 64] > 1 << 31 and max(worst.values()) > 1 << 32
    lane, wave = 24 * 1023 ** 2, 64 * 24 * 1023 ** 2
    assert lane == 25116696 and lane < 1 << 25 and wave == 1607468544 and wave < 1 << 31
    # restoration's decision sums (lr_filter.hpp): 16 samples a lane in 32 bits
    assert 16 * 1023 ** 2 == 16744464 and 16 * 1023 ** 2 < 16 << 20


if __name__ == "__main__":
    import time
    for bd in DEPTHS:
        for f in (observe_deblock, observe_cdef, observe_lr, observe_stages):
            t = time.time()
            print(bd, f.__name__, f(bd), "%.1f s" % (time.time() - t), flush=True)
