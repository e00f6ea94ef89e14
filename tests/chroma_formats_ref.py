"""numpy reference of include/av1mi.h "chroma formats", written from the header's text alone: a source with a chroma layout (4:2:0,
4:2:2, 4:4:4, grey) and a depth (8, 10, 12) -> the 4:2:0 planes at the coded depth (8 -> 8, 10 -> 10, 12 -> 10).  Plus the layouts'
buffer shapes and a content generator for the tests."""
import numpy as np

C420, C422, C444, C400 = 0, 1, 2, 3      # enum av1mi_source_chroma
LAYOUTS = (C420, C422, C444, C400)
DEPTHS = ((8, 8), (10, 10), (12, 10))    # (source_bit_depth, bit_depth): the valid pairs
KINDS = ("noise", "max", "zero", "checker", "ramp")


def up8(n):
    return (n + 7) & ~7


def dtype(bits):
    return np.uint8 if bits == 8 else np.uint16


def true_chroma_size(chroma, w, h):
    """w_p x h_p of a chroma plane of a w x h frame; None for grey"""
    return {C420: ((w + 1) // 2, (h + 1) // 2), C422: ((w + 1) // 2, h), C444: (w, h), C400: None}[chroma]


def buffer_shapes(chroma, w, h):
    """[rows, columns] of the three source buffers of ONE frame of true size w x h (the size rounded up to 8); None = no such plane"""
    W8, H8 = up8(w), up8(h)
    c = {C420: (H8 // 2, W8 // 2), C422: (H8, W8 // 2), C444: (H8, W8), C400: None}[chroma]
    return [(H8, W8), c, c]


def _rule(S, s, mx):
    """out = min((S + (1 << (s - 1))) >> s, max), out = S where s = 0"""
    S = S.astype(np.int64)
    return S if s == 0 else np.minimum((S + (1 << (s - 1))) >> s, mx)


def _clamped(plane, wp, hp):
    """in(x, y) = plane[min(y, h_p - 1)][min(max(x, 0), w_p - 1)] as a function of index arrays; only the true size is touched"""
    true = plane[:hp, :wp].astype(np.int64)
    return lambda x, y: true[np.minimum(y, hp - 1)[:, None], np.clip(x, 0, wp - 1)[None, :]]


def convert(chroma, src_bd, bd, w, h, planes):
    """planes: the three source buffers of ONE frame (buffer_shapes; entries of a grey source's chroma ignored) -> [Y, U, V] of
    up8(w) x up8(h) luma and half-size chroma at bd, every sample written"""
    assert (src_bd, bd) in DEPTHS and chroma in LAYOUTS
    d, mx, dt = src_bd - bd, (1 << bd) - 1, dtype(bd)
    W8, H8 = up8(w), up8(h)
    x, y = np.arange(W8), np.arange(H8)
    out = [_rule(_clamped(planes[0], w, h)(x, y), d, mx).astype(dt)]
    xc, yc = np.arange(W8 // 2), np.arange(H8 // 2)
    for p in (1, 2):
        if chroma == C400:
            out.append(np.full((H8 // 2, W8 // 2), 1 << (bd - 1), dt))
            continue
        wp, hp = true_chroma_size(chroma, w, h)
        f = _clamped(planes[p], wp, hp)
        if chroma == C420:
            S, s = f(xc, yc), d
        elif chroma == C422:
            S, s = f(xc, 2 * yc) + f(xc, 2 * yc + 1), 1 + d
        else:
            S = sum(f(2 * xc - 1, r) + 2 * f(2 * xc, r) + f(2 * xc + 1, r) for r in (2 * yc, 2 * yc + 1))
            s = 3 + d
        out.append(_rule(S, s, mx).astype(dt))
    return out


def convert_stack(chroma, src_bd, bd, w, h, frames, planes):
    """`frames` frames stacked vertically in each buffer -> the stacked 4:2:0 planes"""
    shapes = buffer_shapes(chroma, w, h)
    outs = [convert(chroma, src_bd, bd, w, h, [planes[p][f * shapes[p][0]:(f + 1) * shapes[p][0]] if shapes[p] else None for p in range(3)])
            for f in range(frames)]
    return [np.concatenate([o[p] for o in outs]) for p in range(3)]


def content(kind, chroma, src_bd, w, h, frames=1, seed=0, padding=None):
    """the stacked source buffers of `frames` frames of true size w x h; padding: None = the content continues into the buffers'
    padding, else that value (e.g. all ones) fills everything beyond the true size of every plane"""
    rng = np.random.default_rng(seed)
    dt, mx = dtype(src_bd), (1 << src_bd) - 1
    out = []
    for p, shp in enumerate(buffer_shapes(chroma, w, h)):
        if shp is None:
            out.append(None)
            continue
        R, C = shp
        if kind == "noise":
            a = rng.integers(0, mx + 1, (frames, R, C))
        elif kind == "max":
            a = np.full((frames, R, C), mx)
        elif kind == "zero":
            a = np.zeros((frames, R, C), np.int64)
        elif kind == "checker":      # one-sample checkerboard in chroma (full swing), a flat luma
            yy, xx = np.mgrid[0:R, 0:C]
            a = np.broadcast_to(((yy + xx) & 1) * mx if p else np.full((R, C), mx // 2), (frames, R, C)).copy()
        elif kind == "ramp":
            yy, xx = np.mgrid[0:R, 0:C]
            a = np.stack([(xx * 3 + yy * 5 + f * 7 + p * 11) % (mx + 1) for f in range(frames)])
        else:
            raise ValueError(kind)
        a = a.astype(dt)
        if padding is not None:
            tw, th = (w, h) if p == 0 else true_chroma_size(chroma, w, h)
            a[:, th:, :] = padding
            a[:, :, tw:] = padding
        out.append(a.reshape(frames * R, C))
    return out
