"""numpy restatement of the resampler defined in include/av1mi.h ("scaling"), shared by test_scale.py and test_gpu_scale.py.  Written
from the header's text; nothing here calls the library: these are the definitions the library is checked against."""
import numpy as np


def taps(n, m):
    """T = 2 * ceil(3 * max(n, m) / m), in integers"""
    return 2 * -((-3 * max(n, m)) // m)


def filter_table(n, m):
    """(T, first [m] int64, coef [m, T] int64) for n source -> m output samples: Lanczos-3 in float64, rows normalised, scaled by
    16384, rounded to nearest, the remainder on the tap of largest magnitude"""
    T = taps(n, m)
    s = max(n, m) / m
    j = np.arange(m, dtype=np.int64)
    num = (2 * j + 1) * n - m                         # centre c = num / (2 m)
    first = num // (2 * m) - T // 2 + 1               # floor division
    c = num / (2 * m)
    x = np.abs(((first[:, None] + np.arange(T)[None, :]) - c[:, None]) / s)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.pi * x
        w = np.where(x == 0, 1.0, (np.sin(a) / a) * (np.sin(a / 3) / (a / 3)))
    w = np.where(x >= 3, 0.0, w)
    q = np.floor(w / w.sum(axis=1, keepdims=True) * 16384.0 + 0.5).astype(np.int64)
    big = np.argmax(np.abs(q), axis=1)                # the first of equals
    q[j, big] += 16384 - q.sum(axis=1)
    return T, first, q


def _pass(x, n, first, coef):
    """sum over the taps of coef * x[..., clamp(first + k, 0, n - 1)] along the last axis (int64)"""
    idx = np.clip(first[:, None] + np.arange(coef.shape[1])[None, :], 0, n - 1)      # [m, T]
    out = np.zeros(x.shape[:-1] + (len(first),), np.int64)
    for k in range(coef.shape[1]):
        out += x[..., idx[:, k]] * coef[:, k]
    return out


def scale_plane(p, m_w, m_h, bd, table=filter_table):
    """one plane [n_h, n_w] (true size) -> [m_h, m_w]: horizontally into the 16-bit intermediate, then vertically"""
    p = np.asarray(p).astype(np.int64)
    n_h, n_w = p.shape
    _, fh, ch = table(n_w, m_w)
    _, fv, cv = table(n_h, m_h)
    fh, ch, fv, cv = (np.asarray(a).astype(np.int64) for a in (fh, ch, fv, cv))
    t = (_pass(p, n_w, fh, ch) + (1 << 9)) >> 10
    assert np.abs(t).max() < 1 << 15
    o = (_pass(np.ascontiguousarray(t.T), n_h, fv, cv).T + (1 << 17)) >> 18
    return np.clip(o, 0, (1 << bd) - 1).astype(np.uint8 if bd == 8 else np.uint16)


def scale_frame(y, u, v, dst_w, dst_h, bd, table=filter_table):
    """planes of one frame at their true sizes (chroma (n + 1) // 2) -> the planes of the CODED size (dst rounded up to 8; chroma
    target dst // 2), the last true column / row replicated into the padding"""
    cw, ch = (dst_w + 7) & ~7, (dst_h + 7) & ~7
    out = []
    for i, p in enumerate((y, u, v)):
        mw, mh, pw, ph = (dst_w, dst_h, cw, ch) if i == 0 else (dst_w // 2, dst_h // 2, cw // 2, ch // 2)
        s = scale_plane(p, mw, mh, bd, table)
        out.append(np.pad(s, ((0, ph - mh), (0, pw - mw)), mode="edge"))
    return out
