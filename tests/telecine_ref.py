"""Inverse telecine restated in numpy (include/av1mi.h "inverse telecine"): the field-match records, the plan, the weave; and a synthetic
film with its 3:2 pulldown for the tests.  The GPU kernels (av1-go_amd/csrc/telecine_kernels.hip) and the host's planner
(av1-go_amd/host/telecineplan.hpp) are bit exact against this file."""
import numpy as np

TELECINE_DTYPE = np.dtype([("comb", "<u8", 3), ("bdiff", "<u8")])      # av1mi_telecine_record: comb of p, c, n; bdiff
NO_PREDECESSOR = 2 ** 64 - 1
CYCLE = 5


# ---------------------------------------------------------------------------------------------- records
def records(Y, bd, w, h):
    """the records of the run Y [frames, H8, W8] (luma buffers) whose true size is w x h: nothing at or beyond the true size is read"""
    m = np.asarray(Y)[:, :h, :w].astype(np.int64) >> (bd - 8)
    n = len(m)
    out = np.zeros(n, TELECINE_DTYPE)
    ys = np.arange(2, h - 1, 2)                    # even y with 2 <= y <= h - 2
    for f in range(n):
        B = m[f]
        up, dn = B[ys - 1], B[ys + 1]
        for j, g in enumerate((max(f - 1, 0), f, min(f + 1, n - 1))):
            out["comb"][f, j] = int(np.maximum(0, np.abs(2 * m[g][ys] - up - dn) - np.abs(up - dn) - 8).sum())
        out["bdiff"][f] = int(np.abs(B[1::2] - m[f - 1][1::2]).sum()) if f else NO_PREDECESSOR
    return out


# ---------------------------------------------------------------------------------------------- the plan
def match(rec):
    """0 = p, 1 = c, 2 = n: the smallest comb, ties to the earlier in the order c, p, n"""
    p, c, n = (int(v) for v in rec["comb"])
    best, val = 1, c
    if p < val:
        best, val = 0, p
    if n < val:
        best = 2
    return best


def plan(rec, front=0, back=0):
    """the run's records, its first `front` and last `back` frames context -> (top, bottom): positions in the run, one pair per output"""
    N = len(rec)
    n = N - front - back
    assert front in (0, 1) and back in (0, 1) and n >= 0
    top, bottom = [], []
    for c0 in range(0, n, CYCLE):
        ln = min(CYCLE, n - c0)
        drop = -1
        if ln == CYCLE:
            drop = int(np.argmin(rec["bdiff"][front + c0: front + c0 + CYCLE]))      # the first on ties
        for i in range(ln):
            if i == drop:
                continue
            f = front + c0 + i
            top.append(min(max(f + match(rec[f]) - 1, 0), N - 1))
            bottom.append(f)
    return np.array(top, np.int32), np.array(bottom, np.int32)


def outputs(n):
    return n - n // CYCLE


# ---------------------------------------------------------------------------------------------- the weave
def weave_plane(top, bottom, w, h):
    """one plane's buffers (PH, PW) of true size w x h -> the woven buffer: row y from row min(y, h - 1) of top where that is even, else
    of bottom; columns at or beyond w repeat column w - 1.  top None = zeros"""
    if top is None:
        return np.zeros_like(bottom)
    out = np.empty_like(top)
    for y in range(top.shape[0]):
        r = min(y, h - 1)
        row = (bottom if r & 1 else top)[r]
        out[y, :w] = row[:w]
        out[y, w:] = row[w - 1]
    return out


# ---------------------------------------------------------------------------------------------- synthetic film and pulldown
def film_frame(k, w, h, bd=8):
    """film frame k as (Y, U, V) of true size: a texture that translates 3 samples a frame and an edge that moves 5, so every frame
    differs from the last everywhere; smooth down the columns, so that a frame's own top lines lie between its bottom lines (comb 0)
    while another frame's do not"""
    def plane(pw, ph, a, speed):
        x, y = np.meshgrid(np.arange(pw, dtype=np.float64), np.arange(ph, dtype=np.float64))
        xs = x - speed * k
        v = 118 + a * np.sin(2 * np.pi * xs / 13.0 + y / 40.0) + 0.6 * a * np.sin(2 * np.pi * xs / 7.3 + 1.0) + 0.25 * y
        v = v + 40.0 * (x < 6 + 5 * k * speed / 3.0)
        return np.clip(np.rint(v), 4, 250)
    Y = plane(w, h, 44.0, 3.0)
    U = plane((w + 1) // 2, (h + 1) // 2, 30.0, 1.5)
    V = plane((w + 1) // 2, (h + 1) // 2, 24.0, 1.5)[:, ::-1]
    dt = np.uint8 if bd == 8 else np.uint16
    return tuple((p * (1 << (bd - 8)) + (k % (1 << (bd - 8)))).astype(dt) for p in (Y, U, V))


# the film frame (relative to the cycle's first) whose top / bottom field video frame r of a cycle carries: 4 film frames -> 5 video frames
PULLDOWN = {"tff": ((0, 1, 1, 2, 3), (0, 1, 2, 3, 3)), "bff": ((0, 1, 2, 3, 3), (0, 1, 1, 2, 3))}


def video_sources(v, order):
    """video frame v of an endless pulldown -> (film frame of its top field, film frame of its bottom field)"""
    pt, pb = PULLDOWN[order]
    return 4 * (v // CYCLE) + pt[v % CYCLE], 4 * (v // CYCLE) + pb[v % CYCLE]


def interleave(top, bottom):
    out = bottom.copy()
    out[0::2] = top[0::2]
    return out


def video_frame(v, order, w, h, bd=8):
    """video frame v as (Y, U, V): every plane woven by its own row parity from the two film frames (what a telecine of planar 4:2:0 gives)"""
    t, b = video_sources(v, order)
    return tuple(interleave(a, c) for a, c in zip(film_frame(t, w, h, bd), film_frame(b, w, h, bd)))


def pad8(p, luma):
    """a true-size plane in its buffer: the luma buffer is the true size rounded up to 8, a chroma buffer half of that; edge replicated"""
    h, w = p.shape
    if luma:
        ph, pw = (h + 7) & ~7, (w + 7) & ~7
    else:
        ph, pw = ((2 * h + 7) & ~7) // 2, ((2 * w + 7) & ~7) // 2
    return np.pad(p, ((0, ph - h), (0, pw - w)), mode="edge")
