"""Bar detection and the crop plan, restated in numpy from include/av1mi.h "bar detection" and av1-go_amd/host/cropplan.hpp: the margins
of a frame, the window a sample of frames yields, and the window as numpy slices of a 4:2:0 frame."""
import numpy as np

CROP_DTYPE = np.dtype([("top", "<u4"), ("bottom", "<u4"), ("left", "<u4"), ("right", "<u4")])


def _run(dark):
    """the number of leading True entries"""
    n = 0
    for d in dark:
        if not d:
            break
        n += 1
    return n


def margins(luma, bit_depth, w, h, limit):
    """the record (top, bottom, left, right) of one luma plane (a buffer at least h x w; only [:h, :w] is looked at)"""
    m8 = luma[:h, :w].astype(np.int64) >> (bit_depth - 8)
    rows, cols = m8.sum(axis=1), m8.sum(axis=0)
    dr, dc = rows <= limit * w, cols <= limit * h
    return _run(dr), _run(dr[::-1]), _run(dc), _run(dc[::-1])


def records(Y, bit_depth, w, h, limit):
    """CROP_DTYPE [frames] of stacked luma planes Y [frames, H8, W8]"""
    out = np.zeros(len(Y), CROP_DTYPE)
    for f, plane in enumerate(Y):
        out[f] = margins(plane, bit_depth, w, h, limit)
    return out


def plan(rec, w, h):
    """(x, y, width, height) or None"""
    use = [r for r in rec if int(r["top"]) != h]
    if len(use) < 2:
        return None
    T, B, L, R = (min(int(r[k]) for r in use) & ~1 for k in ("top", "bottom", "left", "right"))
    if T + B < 8:
        T = B = 0
    if L + R < 8:
        L = R = 0
    cw, ch = (w - L - R) & ~1, (h - T - B) & ~1
    if cw < 16 or ch < 16:
        return None
    return L, T, cw, ch


def window(planes, x, y, cw, ch):
    """the window of one 4:2:0 frame (Y, U, V arrays at least as large as the true size): three arrays of cw x ch and its half"""
    return [planes[0][y:y + ch, x:x + cw], planes[1][y // 2:(y + ch) // 2, x // 2:(x + cw) // 2], planes[2][y // 2:(y + ch) // 2, x // 2:(x + cw) // 2]]
