"""Hard content for the in-loop filters (deblock_filter.hpp, cdef_filter.hpp, lr_filter.hpp, search_sse.hpp): one 4:2:0 frame per clip at
8 and 10 bits, built so that what lf_util.test_image and the searches' mild generators never do happens on many edge lines and blocks —
deblocking edges that sit exactly at and one above each mask threshold, steps that drive the narrow filter into its clamps next to
samples at 0 and at the top value, 8x8 blocks whose CDEF directions tie or whose variance is 0 or at its cap, taps that the min / max
clamp decides, Wiener rows whose intermediate leaves its range, error sums of full-swing differences.  Plain numpy, seeded, nothing read
from disk; test infrastructure only.

Every generator returns (Y, U, V): [h, w] / [h / 2, w / 2] arrays of the depth's sample type.  What each clip is there for is checked
with the oracle and dav1d alone in tests/test_filter_clips.py; the GPU is held to them in tests/test_gpu_filter_content.py.  The filter
parameters both files run (level sets, strength sets, restoration units at the ends of their ranges) stand here as well."""
import numpy as np

import intra_clips as IC

# (w, h).  64x64: one superblock, every side a picture border.  136x72: partial superblocks right and bottom, a chroma block narrower than
# 32, two luma restoration stripes.  136x136: superblock (1, 1) is interior by the CDEF kernels' own rule (cdef_kernel.hip: sbx > 0,
# sby > 0, sb * 64 + 66 <= size — two samples of the next superblock are enough), with partial superblocks around it.
SIZES = ((64, 64), (136, 72), (136, 136))
# planes for restoration, (w, h): the first of SIZES' partial ones, and the two of tests/test_gpu_lr.py that take the scalar Wiener route
LR_SIZES = ((136, 72), (70, 72), (23, 40))

top_of = IC.top_of


def _dt(bd):
    return np.uint8 if bd == 8 else np.uint16


# ---- the parameters under test
def lf_limits(lvl, sharp):
    """(lim, mblim, hev) of a filter level (AV1 spec 7.14.4), in 8-bit units"""
    shift = 2 if sharp > 4 else (1 if sharp > 0 else 0)
    inside = lvl >> shift
    if sharp > 0:
        inside = min(inside, 9 - sharp)
    inside = max(inside, 1)
    return inside, 2 * (lvl + 2) + inside, lvl >> 4


# ((luma vertical, luma horizontal, U, V), sharpness); the last: no horizontal luma edge is filtered
LF_SETS = (((4, 3, 5, 5), 0), ((63, 63, 63, 63), 0), ((4, 3, 5, 5), 5), ((63, 63, 63, 63), 5), ((20, 0, 12, 12), 0))


def lf_thresholds():
    """the distinct (lim, mblim, hev) of every level and sharpness in LF_SETS"""
    return sorted({lf_limits(l, s) for lv, s in LF_SETS for l in lv if l})


CDEF_SETS = ((15, 3, 15, 3), (1, 0, 1, 0), (0, 2, 0, 1))      # (y primary, y secondary code, uv primary, uv secondary code)
CDEF_OFF = (255, 0, 0, 0)
WIENER_RANGES = ((-5, 10), (-23, 8), (-17, 46))
SGR_SETS = (0, 9, 10, 14, 15)


def wiener_end_records(chroma=False):
    """eight (vertical taps, horizontal taps): every tap at an end of its range, each of the 8 end combinations once as the vertical and
    once as the horizontal filter; chroma: the outer tap 0 (five taps, as a stream codes them)"""
    ends = [[WIENER_RANGES[i][(k >> i) & 1] for i in range(3)] for k in range(8)]
    if chroma:
        ends = [[0, e[1], e[2]] for e in ends]
    return [(ends[k], ends[7 - k]) for k in range(8)]


def sgr_end_records():
    """(set, xqd0, xqd1) for the sets 0, 9, 10, 14, 15 with the weights at the ends of their ranges, as a stream can code them: sets 10 .. 13
    have no first pass (xqd0 = 0), sets 14 and 15 no second (xqd1 follows from xqd0)"""
    out = []
    for s in SGR_SETS:
        for x0 in (-96, 31):
            for x1 in (-32, 95):
                if s >= 14:
                    x1 = min(max(128 - x0, -32), 95)
                elif s >= 10:
                    x0 = 0
                if (s, x0, x1) not in out:
                    out.append((s, x0, x1))
    return out


def lr_shift(f):
    """the turn frame f of a job starts at: frames 0 and 1 of NAMES (noise, binary) meet the horizontal filter (-5, -23, -17), the one
    whose intermediate leaves its range on isolated samples"""
    return 5 + f


def lr_unit_map(O, w, h, unit, kind, chroma=False, shift=0):
    """[rows, cols, 8] restoration units for a w x h plane: kind 'wiener' = wiener_end_records in turn, 'sgr' = sgr_end_records in turn,
    'mixed' = Wiener, self-guided and none in turn; shift moves the turn (frames of one job get different units)"""
    wr = [O.lr_unit_wiener(v, hz) for v, hz in wiener_end_records(chroma)]
    sr = [O.lr_unit_sgr(*r) for r in sgr_end_records()]
    u = np.zeros((O.lr_units(unit, h), O.lr_units(unit, w), 8), np.int8)
    for r in range(u.shape[0]):
        for c in range(u.shape[1]):
            k = shift + r * u.shape[1] + c
            if kind == "wiener":
                u[r, c] = wr[k % len(wr)]
            elif kind == "sgr":
                u[r, c] = sr[k % len(sr)]
            else:
                u[r, c] = (wr[(k // 3) % len(wr)], sr[(k // 3) % len(sr)], O.lr_unit_none())[k % 3]
    return u


# ---- deblocking: edges at the thresholds
def _blim_pair(target, lim):
    """(A, C) = (|p0 - q0|, |p1 - q1|) with 2 A + C / 2 == target and |A - C| smallest (it must not exceed lim: q0 - q1 is A - C)"""
    best = None
    for A in range(target // 2 + 1):
        for C in (2 * (target - 2 * A), 2 * (target - 2 * A) + 1):
            if best is None or abs(A - C) < abs(best[0] - best[1]):
                best = (A, C)
    return best if abs(best[0] - best[1]) <= lim else None


def edge_recipes(bd):
    """(dp, dq, A, C): the offset of the sample next to the edge against its flat block on either side, |p0 - q0|, and |p1 - q1| where the
    recipe sets it (else None: it follows).  Per threshold set: |p1 - p0| and |q1 - q0| at lim and lim + 1 under a small step;
    2 |p0 - q0| + |p1 - q1| / 2 at mblim and mblim + 1 with flat sides; |p1 - p0| at hev and hev + 1 under a step the mask passes; and
    for flat / flat2 (|p_i - p0| for every i the filter length reads) 0, 1 << (bd - 8) and one more."""
    sh = bd - 8
    one = 1 << sh
    out = []
    for lim, blim, hev in lf_thresholds():
        L, B, H = lim << sh, blim << sh, hev << sh
        for d in (L, L + 1):
            out += [(d, 0, one, None), (0, d, 0, None)]
        for target in (B, B + 1):
            pair = _blim_pair(target, L)
            if pair:
                out.append((0, 0, pair[0], pair[1]))
        for d in (H, H + 1):
            out += [(d, 0, 3 * one, None), (0, d, 2 * one, None)]
    for d in (0, one, one + 1):
        out += [(d, 0, 2 * one, None), (d, d, one, None), (0, d, 0, None)]
    return out


def _walk(n_along, n_rows, bs, bd, recipes):
    """[n_rows * bs, n_along]: per block row a walk along the row, flat blocks of bs samples whose first and last sample carry the
    recipes' offsets (every fourth block row: whose first and second half do); the rows of a block row are equal"""
    top, mid = top_of(bd), top_of(bd) // 2
    out = np.zeros((n_rows * bs, n_along), np.int64)
    nb = n_along // bs
    for r in range(n_rows):
        row = np.zeros(n_along, np.int64)
        B = (37 * (r + 1) << (bd - 8)) % (top - 2 * (40 << (bd - 8))) + (40 << (bd - 8))
        q0 = B
        for c in range(nb + 1):
            dp, dq, A, C = recipes[(c + 7 * r) % len(recipes)]      # the edge between block c and block c + 1
            s = 1 if B < mid else -1
            p0 = B + s * dp
            if c < nb and r % 4 == 3:      # the offsets on half a block each: p1 .. p3 follow p0, and p4 .. p6 are what differs (flat2)
                row[c * bs:c * bs + bs // 2] = q0
                row[c * bs + bs // 2:(c + 1) * bs] = p0
            elif c < nb:
                row[c * bs:(c + 1) * bs] = B
                row[c * bs] = q0
                row[(c + 1) * bs - 1] = p0
            if C is None:
                q0 = p0 + s * A
                B = q0 - s * dq
            else:
                B = B + s * C
                q0 = B + s * (A - C)
        out[r * bs:(r + 1) * bs] = row
    assert out.min() >= 0 and out.max() <= top
    return out


def steps_at_threshold(w, h, bd):
    """flat 8x8 luma / 4x4 chroma blocks whose samples next to a block edge are offset by the recipes of edge_recipes.  The upper half
    walks along the rows (vertical edges, which the first pass sees as they are), the lower half down the columns (horizontal edges)."""
    rec = edge_recipes(bd)
    out = []
    for i, (ph, pw) in enumerate(((h, w), (h // 2, w // 2), (h // 2, w // 2))):
        bs = 8 if i == 0 else 4
        rows_top = (ph // 2) // bs
        a = np.zeros((ph, pw), np.int64)
        a[:rows_top * bs] = _walk(pw, rows_top, bs, bd, rec[i:] + rec[:i])
        a[rows_top * bs:] = _walk(ph - rows_top * bs, pw // bs, bs, bd, rec[3 + i:] + rec[:3 + i]).T
        out.append(a.astype(_dt(bd)))
    return tuple(out)


def big_steps(w, h, bd, seed=21):
    """8x8 luma / 4x4 chroma blocks whose levels step by 45 .. 75 (8-bit units) between neighbours both ways: 3 |q0 - p0| leaves the
    narrow filter's [-128, 127] while 2 |p0 - q0| + |p1 - q1| / 2 still passes the mask of level 63; every fifth level is 0 or the top
    value, so the clamps of the filtered samples engage as well.  A texture of up to 6 keeps the blocks from being flat (the flat
    filters would take the edge) and switches high edge variance on in most lines."""
    rng = np.random.default_rng([seed, bd, w, h])
    sh, top = bd - 8, top_of(bd)
    levels = np.array([0, 50, 120, 190, 255, 185, 110, 45], np.int64) << sh
    levels[4] = top
    out = []
    for i, (ph, pw) in enumerate(((h, w), (h // 2, w // 2), (h // 2, w // 2))):
        bs = 8 if i == 0 else 4
        y, x = np.mgrid[0:ph, 0:pw]
        base = levels[(x // bs + y // bs + i) % 8]
        tex = rng.integers(0, (6 << sh) + 1, (ph, pw))
        tex[(y // bs) % 3 == 2] = 0      # every third block row: no texture, the flat filters take over
        out.append(np.clip(np.where(base < top // 2, base + tex, base - tex), 0, top).astype(_dt(bd)))
    return tuple(out)


# ---- CDEF: full-swing blocks
def _line_index(d, i, j):
    """the line of direction d that sample (i, j) of an 8x8 block lies on (AV1 spec 7.15.2)"""
    return (i + j, i + j // 2, i, 3 + i - j // 2, 7 + i - j, 3 - i // 2 + j, j, i // 2 + j)[d]


def block_patterns():
    """0 / 1 patterns of 8x8 samples, by name: checkers, stripes of one and of two samples along each of the eight CDEF directions, a
    plus and an X (two directions tie for the best), single samples and a single dark sample on a bright field, and two with a sample
    just off its field (value 2)"""
    i, j = np.mgrid[0:8, 0:8]
    pats = {"checker1": (i + j) & 1, "checker2": (i // 2 + j // 2) & 1}
    for d in range(8):
        pats["stripe1_d%d" % d] = _line_index(d, i, j) & 1
        pats["stripe2_d%d" % d] = (_line_index(d, i, j) // 2) & 1
    pats["plus"] = ((i == 3) | (j == 3)).astype(int)
    pats["x"] = ((i == j) | (i + j == 7)).astype(int)
    pats["dot"] = ((i == 3) & (j == 4)).astype(int)
    pats["dots"] = ((i % 4 == 1) & (j % 4 == 2)).astype(int)
    pats["hole"] = 1 - pats["dot"]
    # 2 = a sample 3 << (bd - 8) off the field it stands on, all of its taps on the field: differences small enough for the filter to
    # use them in full, so the sum overshoots the field and the min / max clamp decides; the stripe in column 0 gives the block the
    # variance that keeps the primary strength up
    pats["low_dot"] = np.where(j == 0, 1, np.where((i == 3) & (j == 5), 2, 0))
    pats["low_hole"] = np.where(j == 0, 0, np.where((i == 4) & (j == 5), 2, 1))
    return pats


def full_swing_blocks(w, h, bd):
    """8x8 luma blocks of block_patterns at 0 / top, every third block exactly flat (0, mid-grey or top) so that patterns and flat blocks
    are neighbours; chroma: the same patterns on its 4x4 blocks (the top-left quarter of each)"""
    top = top_of(bd)
    pats = list(block_patterns().values())
    flats = (0, 128 << (bd - 8), top)
    out = []
    for i, (ph, pw) in enumerate(((h, w), (h // 2, w // 2), (h // 2, w // 2))):
        bs = 8 if i == 0 else 4
        a = np.zeros((ph, pw), np.int64)
        k = i
        for by in range(ph // bs):
            for bx in range(pw // bs):
                if (bx + 2 * by) % 3 == 0:
                    blk = np.full((bs, bs), flats[(bx + by) % 3])
                else:
                    pat = pats[k % len(pats)][:bs, :bs]
                    field = top * (pat[2, 3] == 1)      # what a sample of value 2 stands on
                    blk = np.where(pat == 2, abs(field - (3 << (bd - 8))), top * (pat == 1))
                    k += 1
                a[by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs] = blk
        out.append(a.astype(_dt(bd)))
    return tuple(out)


def inverse_of(planes, bd):
    """top - sample: the source against which every sample of a 0 / top picture errs by the full range"""
    return tuple((top_of(bd) - a.astype(np.int64)).astype(_dt(bd)) for a in planes)


NAMES = ("noise", "binary", "checker1", "checker2", "stripes", "stripes_across", "diag", "flat0", "flat_top", "steps_at_threshold",
         "big_steps", "full_swing_blocks")
FLAT = ("flat0", "flat_top")


def clip(name, w, h, bd):
    """a clip by name: this module's generators, and those of intra_clips"""
    if name in globals():
        return globals()[name](w, h, bd)
    return IC.clip(name, w, h, bd)


def plane(name, w, h, bd):
    """one w x h plane of a clip, any size: the luma plane of the clip at the size rounded up to 8, cropped"""
    return clip(name, (w + 7) // 8 * 8, (h + 7) // 8 * 8, bd)[0][:h, :w]


stack = IC.stack
