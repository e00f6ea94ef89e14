"""Interlaced clips for the deinterlacing tests: a textured shot that pans (3, 1) samples per FIELD.  The motion is sampled at field
times — the first field of frame t at time 2 t, the second at 2 t + 1 — and the two fields are woven into one frame, so the combing
is real.  Deterministic; nothing is read from disk."""
import numpy as np

PAN = (3, 1)      # samples per field: x, y


def _canvas(w, h, fields, bd, seed):
    """a texture large enough for every field's window: diagonal gratings at several angles (edges that the direction search follows)
    over blocks of few levels (steps that the temporal average smears)"""
    rng = np.random.default_rng(seed)
    H, W = h + PAN[1] * fields + 8, w + PAN[0] * fields + 8
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    t = np.zeros((H, W))
    for fx, fy, amp in ((0.21, 0.13, 0.22), (-0.17, 0.19, 0.2), (0.09, -0.05, 0.18), (0.31, 0.02, 0.12)):
        t += amp * np.sin(2 * np.pi * (fx * x + fy * y) + rng.uniform(0, 6.28))
    blocks = rng.integers(0, 5, ((H + 11) // 12, (W + 11) // 12)) / 4.0 - 0.5
    t += 0.5 * np.repeat(np.repeat(blocks, 12, axis=0), 12, axis=1)[:H, :W]
    t += rng.normal(0, 0.02, (H, W))
    hi = (1 << bd) - 1
    return np.clip(np.rint((0.5 + 0.45 * t) * hi), 0, hi).astype(np.uint8 if bd == 8 else np.uint16)


def pan_plane(w, h, n, bd, parity, seed):
    """[n, h, w]: n frames of one plane; parity 0 = top field first (the even lines are the earlier field)"""
    tex = _canvas(w, h, 2 * n, bd, seed)
    out = np.empty((n, h, w), tex.dtype)
    for t in range(n):
        for field in (0, 1):
            f = 2 * t + field
            win = tex[PAN[1] * f:PAN[1] * f + h, PAN[0] * f:PAN[0] * f + w]
            first_lines = parity if field == 0 else 1 - parity
            out[t, first_lines::2] = win[first_lines::2]
    return out


def pan_clip(w, h, n, bd, parity, seed=7, chroma=(1, 1)):
    """(Y, U, V) of n frames, w x h luma; chroma = the (horizontal, vertical) subsampling shifts ((1, 1) 4:2:0, (1, 0) 4:2:2)"""
    cw, ch = w >> chroma[0], h >> chroma[1]
    return (pan_plane(w, h, n, bd, parity, seed), pan_plane(cw, ch, n, bd, parity, seed + 1), pan_plane(cw, ch, n, bd, parity, seed + 2))


def write_y4m(path, clip, bd, interlace="t", fps=30):
    """the clip as Y4M 4:2:0 with the header's I parameter (None = absent)"""
    Y, U, V = clip
    h, w = Y.shape[1:]
    tag = "" if interlace is None else " I%s" % interlace
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F%d:1%s A1:1 C%s\n" % (w, h, fps, tag, "420jpeg" if bd == 8 else "420p10")).encode())
        for t in range(Y.shape[0]):
            f.write(b"FRAME\n")
            for p in (Y[t], U[t], V[t]):
                f.write(np.ascontiguousarray(p).astype("<u2" if bd == 10 else np.uint8).tobytes())


# The shapes of the kernel tests (tests/test_gpu_deinterlace.py), the smallest at which the kernel can go wrong: name -> luma buffer size,
# true luma size, chroma subsampling shifts, frames, seed.  tests/test_deinterlace.py checks that the reference exercises the spatial
# and the temporal path on each of them.
CASES = {
    "8x8": dict(size=(8, 8), true=(8, 8), chroma=(1, 1), n=3, seed=1),            # every missing chroma line has a mirrored neighbour
    "40x24": dict(size=(40, 24), true=(40, 24), chroma=(1, 1), n=3, seed=7),      # chroma rows of 20 bytes: a dword tail
    "38x22": dict(size=(40, 24), true=(38, 22), chroma=(1, 1), n=3, seed=7),      # the padding rule, clamps at the true edge
    "272x16": dict(size=(272, 16), true=(272, 16), chroma=(1, 1), n=3, seed=7),   # more than 16 cells a row
    "1040x8": dict(size=(1040, 8), true=(1040, 8), chroma=(1, 1), n=3, seed=7),   # 65 (8 bit) / 130 (16 bit) cells a row: a neighbour in the next wave
    "422": dict(size=(32, 16), true=(32, 16), chroma=(1, 0), n=3, seed=7),        # a 4:2:2 fed layout: chroma as high as luma
}


def case_clip(name, bd, parity, n=None):
    """the clip of a case at the BUFFER's size (the samples beyond the true size are part of the texture: the filter must not use them)"""
    c = CASES[name]
    return pan_clip(c["size"][0], c["size"][1], n or c["n"], bd, parity, c["seed"], c["chroma"])


def case_true_sizes(name):
    """[(w, h)] per plane: the true size of the case's planes"""
    c = CASES[name]
    (tw, th), (sx, sy) = c["true"], c["chroma"]
    cw, ch = (tw + (1 << sx) - 1) >> sx, (th + (1 << sy) - 1) >> sy
    return [(tw, th), (cw, ch), (cw, ch)]
