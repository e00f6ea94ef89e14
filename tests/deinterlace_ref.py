"""The deinterlacer of include/av1mi.h ("deinterlacing") in numpy, written from the header's text: the reference the kernel
(av1-go_amd/csrc/deint_kernels.hip) is compared with bit for bit.  Plain array code, one plane at a time; no GPU."""
import numpy as np

ORDER = (0, -1, 1, -2, 2)      # the directions, in the order they are tried


def _parts(P, C, N, w, h, k):
    """the pieces of the filter over the MISSING lines of one plane (true size w x h, parity k): dict of int64 arrays [lines, w] and
    `rows`, the missing lines' numbers; None when the plane has no missing line"""
    P, C, N = (np.asarray(a)[:h, :w].astype(np.int64) for a in (P, C, N))
    rows = np.array([y for y in range(h) if y % 2 != k], np.int64)
    if h == 1 or rows.size == 0:
        return None
    up = np.where(rows >= 1, rows - 1, rows + 1)
    dn = np.where(rows + 1 <= h - 1, rows + 1, rows - 1)
    x = np.arange(w)
    col = lambda a, r, j: a[r][:, np.clip(x + j, 0, w - 1)]      # a[r][x + j], x clamped
    a = lambda j: col(C, up, j)
    b = lambda j: col(C, dn, j)
    best, s, dirs, scores = None, None, None, {}
    for d in ORDER:
        score = scores[d] = sum(np.abs(a(j + d) - b(j - d)) for j in (-1, 0, 1))
        cand = (a(d) + b(-d) + 1) >> 1
        if best is None:
            best, s, dirs = score, cand, np.zeros_like(score)
        else:
            win = score < best          # strictly smaller than every earlier one
            best, s, dirs = np.where(win, score, best), np.where(win, cand, s), np.where(win, d, dirs)
    t0, t1 = P[rows], C[rows]
    t = (t0 + t1 + 1) >> 1
    m = (np.abs(t0 - t1) + 1) >> 1
    for F in (P, N):
        m = np.maximum(m, (np.abs(F[up] - a(0)) + np.abs(F[dn] - b(0)) + 1) >> 1)
    out = np.minimum(np.maximum(s, t - m), t + m)
    return dict(rows=rows, s=s, t=t, m=m, d=dirs, out=out, scores=scores)


def plane(P, C, N, w, h, k):
    """one plane of frame C deinterlaced: arrays of the BUFFER's size (at least w x h; only the true size is read) -> the buffer's size,
    the padding replicating the output's own edge"""
    C = np.asarray(C)
    out = C[:h, :w].copy()
    parts = _parts(P, C, N, w, h, k)
    if parts is not None:
        out[parts["rows"]] = parts["out"].astype(C.dtype)
    H, W = C.shape
    return np.pad(out, ((0, H - h), (0, W - w)), mode="edge")


def run(frames, w, h, k):
    """a run of frames [n, H, W] of one plane -> the same shape: frame f with P = frame max(f - 1, 0), N = frame min(f + 1, n - 1)"""
    frames = np.asarray(frames)
    n = frames.shape[0]
    return np.stack([plane(frames[max(f - 1, 0)], frames[f], frames[min(f + 1, n - 1)], w, h, k) for f in range(n)])


def shares(frames, w, h, k):
    """over the missing samples of the run's MIDDLE frames (1 .. n - 2): the shares whose output differs from t, that pick a direction
    d != 0, and that are clamped at t - m or t + m (the edge-directed value lies outside the bound)"""
    frames = np.asarray(frames)
    n, tot, off_t, dirs, clamped = frames.shape[0], 0, 0, 0, 0
    for f in range(1, n - 1):
        p = _parts(frames[f - 1], frames[f], frames[f + 1], w, h, k)
        tot += p["out"].size
        off_t += int((p["out"] != p["t"]).sum())
        dirs += int((p["d"] != 0).sum())
        clamped += int(((p["s"] < p["t"] - p["m"]) | (p["s"] > p["t"] + p["m"])).sum())
    return off_t / tot, dirs / tot, clamped / tot
