"""Field-rate deinterlacing of include/av1mi.h ("FIELD-RATE OUTPUT" under "deinterlacing") in numpy, written from the header's text: the
reference the field-rate instantiation of the kernel (av1-go_amd/csrc/deint_kernels.hip) is compared with bit for bit.  Plain array
code, one plane at a time; no GPU, nothing of the library."""
import numpy as np

ORDER = (0, -1, 1, -2, 2)      # the directions, in the order they are tried


def field(P, C, N, w, h, k, phi):
    """one plane of output 2 f + phi of frame C (P, N: the frames before and after it, the run's clamping applied by the caller): arrays of
    the BUFFER's size (only the true size w x h is read) -> the buffer's size, the padding replicating the output's own edge.  k: the
    source's parity (0 = top field first)"""
    C = np.asarray(C)
    p, c, n = (np.asarray(a)[:h, :w].astype(np.int64) for a in (P, C, N))
    keep = k if phi == 0 else 1 - k                      # the lines with y mod 2 == keep are copied
    out = c.copy()
    rows = np.array([y for y in range(h) if y % 2 != keep], np.int64)
    if h > 1 and rows.size:
        up = np.where(rows >= 1, rows - 1, rows + 1)
        dn = np.where(rows + 1 <= h - 1, rows + 1, rows - 1)
        x = np.arange(w)
        a = lambda j: c[up][:, np.clip(x + j, 0, w - 1)]
        b = lambda j: c[dn][:, np.clip(x + j, 0, w - 1)]
        best = s = None
        for d in ORDER:
            score = sum(np.abs(a(j + d) - b(j - d)) for j in (-1, 0, 1))
            cand = (a(d) + b(-d) + 1) >> 1
            if best is None:
                best, s = score, cand
            else:
                win = score < best                       # strictly smaller than every earlier one
                best, s = np.where(win, score, best), np.where(win, cand, s)
        t0, t1 = (p[rows], c[rows]) if phi == 0 else (c[rows], n[rows])      # one field before and one field after the missing one
        t = (t0 + t1 + 1) >> 1
        m = (np.abs(t0 - t1) + 1) >> 1
        for F in (p, n):                                 # the fields of the kept parity before and after: the same in both phases
            m = np.maximum(m, (np.abs(F[up] - a(0)) + np.abs(F[dn] - b(0)) + 1) >> 1)
        out[rows] = np.minimum(np.maximum(s, t - m), t + m)
    H, W = C.shape
    return np.pad(out.astype(C.dtype), ((0, H - h), (0, W - w)), mode="edge")


def fields(frames, w, h, k):
    """a run of frames [n, H, W] of one plane -> [2 n, H, W]: output 2 f + phi from frame f with P = frame max(f - 1, 0) and N = frame
    min(f + 1, n - 1)"""
    frames = np.asarray(frames)
    n = frames.shape[0]
    return np.stack([field(frames[max(f - 1, 0)], frames[f], frames[min(f + 1, n - 1)], w, h, k, phi) for f in range(n) for phi in (0, 1)])
