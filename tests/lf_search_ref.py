"""The deblocking search (include/av1mi.h "deblocking search") restated with numpy: the candidate levels, the patched map, the cost
per candidate by the oracle's deblocking of the WHOLE plane (no tiles: the kernel's structure is not repeated here), the pick, and
the content and base maps the tests share."""
import numpy as np

M = (4, 0, 2, 3, 5, 6, 8, 12)
HOLD = np.uint32(1 << 24)


def level(L, c, chroma):
    return L if c == 0 else min(63, max(0 if chroma else 1, (L * M[c] + 2) >> 2))


def levels(P, c):
    """the four header levels of candidate c for policy levels P; ValueError for what the search refuses"""
    P = [int(x) for x in P]
    if P[2] != P[3] or (P[0] == 0 and P[1] == 0 and P[2] != 0) or not 0 <= c < 8 or min(P) < 0 or max(P) > 63:
        raise ValueError("refused")
    return [level(P[0], c, False), level(P[1], c, False), level(P[2], c, True), level(P[3], c, True)]


def patched(mi, vertical, horizontal):
    """the map with the two level bytes replaced in every word that does not carry bit 24"""
    mi = np.asarray(mi, np.uint32)
    new = (mi & np.uint32(0xFF0000FF)) | np.uint32(vertical << 8) | np.uint32(horizontal << 16)
    return np.where(mi & HOLD, mi, new).astype(np.uint32)


def base_maps(w, h, true_size=None, key32=False, level_bytes=0):
    """the session's maps (gop_session.hip side_information): 8x8 luma / 4x4 chroma transforms, every block edge a prediction edge;
    units at or beyond the true size held; key32: 32x32 / 16x16 transforms over the complete superblock rows.  level_bytes: what the
    level fields hold (the search must not read them)"""
    tw, th = true_size if true_size else (w, h)
    lv = np.uint32(level_bytes << 8 | level_bytes << 16)
    y = np.full((h // 4, w // 4), 3 | 3 << 4 | 3 << 25, np.uint32) | lv
    c = np.full((h // 8, w // 8), 2 | 2 << 4 | 3 << 25, np.uint32) | lv
    ry, cy = np.meshgrid(np.arange(h // 4), np.arange(w // 4), indexing="ij")
    y[(4 * ry >= th) | (4 * cy >= tw)] = 3 | 3 << 4 | 1 << 24
    rc, cc = np.meshgrid(np.arange(h // 8), np.arange(w // 8), indexing="ij")
    c[(8 * rc >= th) | (8 * cc >= tw)] = 2 | 2 << 4 | 1 << 24
    if key32:
        rows = h // 64 * 64
        y[:rows // 4] = (y[:rows // 4] & ~np.uint32(0xFF)) | np.uint32(5 | 5 << 4)
        c[:rows // 8] = (c[:rows // 8] & ~np.uint32(0xFF)) | np.uint32(4 | 4 << 4)
    return y, c


def content(kind, rng, w, h, bd):
    """(source planes, reconstruction planes) of one 4:2:0 frame.  kind 0: a smooth source, the reconstruction with an offset per 8x8 (4x4
    chroma) block: blocking that strong levels remove; kind 1: a source of flat blocks on that grid with small steps between them and a
    near-exact reconstruction: every filtered edge is a loss, weak levels win; kind 2: noise"""
    sh, top = bd - 8, (1 << bd) - 1
    src, rec = [], []
    for p in range(3):
        ph, pw, b = (h, w, 8) if p == 0 else (h // 2, w // 2, 4)
        yy, xx = np.meshgrid(np.arange(ph), np.arange(pw), indexing="ij")
        if kind == 0:
            s = (60 + 0.35 * xx + 0.2 * yy + 6 * np.sin(xx / 23.0) * np.cos(yy / 17.0)) * (1 << sh)
            off = rng.integers(-9, 10, (ph // b + 1, pw // b + 1)) * (1 << sh)
            r = s + np.kron(off, np.ones((b, b)))[:ph, :pw]
        elif kind == 1:
            steps = rng.integers(0, 4, (ph // b + 1, pw // b + 1)) * 3 * (1 << sh)
            s = 100 * (1 << sh) + np.kron(steps, np.ones((b, b)))[:ph, :pw]
            r = s + rng.integers(-1, 2, (ph, pw)) * (rng.random((ph, pw)) < 0.05)
        else:
            s = (120 + rng.integers(-14, 15, (ph, pw))) * (1 << sh)      # (small enough for the masks to let the filters in)
            r = s + rng.integers(-6, 7, (ph, pw)) * (1 << sh)
        dt = np.uint8 if bd == 8 else np.uint16
        src.append(np.clip(np.rint(s), 0, top).astype(dt))
        rec.append(np.clip(np.rint(r), 0, top).astype(dt))
    return src, rec


def _sse(a, b, th, tw):
    d = a[:th, :tw].astype(np.int64) - b[:th, :tw].astype(np.int64)
    return int((d * d).sum())


def search(O, rec, src, bd, P, sharpness, mi_y, mi_c, true_size=None):
    """one frame: (sse uint64 [2][8], choice [2], header levels [4], the three planes deblocked at the chosen candidates)"""
    h, w = rec[0].shape
    tw, th = true_size if true_size else (w, h)
    cw, ch = (tw + 1) // 2, (th + 1) // 2
    sse = np.zeros((2, 8), np.uint64)
    planes = [[None] * 8 for _ in range(3)]
    for c in range(8):
        lv = levels(P, c)
        planes[0][c] = O.deblock_plane(rec[0], bd, 0, patched(mi_y, lv[0], lv[1]), sharpness)
        sse[0, c] = _sse(planes[0][c], src[0], th, tw)
        for p in (1, 2):
            planes[p][c] = O.deblock_plane(rec[p], bd, 1, patched(mi_c, lv[2], lv[2]), sharpness)
            sse[1, c] += np.uint64(_sse(planes[p][c], src[p], ch, cw))
    choice = [int(np.argmin(sse[0])), int(np.argmin(sse[1]))]      # (argmin: the first of equal minima)
    ly, lc = levels(P, choice[0]), levels(P, choice[1])
    return sse, choice, [ly[0], ly[1], lc[2], lc[3]], [planes[0][choice[0]], planes[1][choice[1]], planes[2][choice[1]]]


# the GPU test's inputs, shared with the CPU test that checks they make the reference choose differently: (w, h, true size)
SIZES = [(64, 64, None), (136, 72, None), (136, 72, (130, 70))]
POLICY = (20, 14, 12, 12)      # vertical and horizontal levels differ, so that a swap of the two shows


def frames(w, h, bd, seed=0):
    """three frames of content kinds 0, 1, 2, stacked per plane: (src[3], rec[3]), each [3, rows, cols]"""
    rng = np.random.default_rng(1000 * bd + w + h + seed)
    fr = [content(k, rng, w, h, bd) for k in range(3)]
    return [np.stack([f[0][p] for f in fr]) for p in range(3)], [np.stack([f[1][p] for f in fr]) for p in range(3)]
