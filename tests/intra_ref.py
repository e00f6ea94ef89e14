"""The key-frame mode decision restated in numpy on top of O.intra_predict, the dav1d-pinned predictor (tests/test_oracle_intra.py):
which blocks see which neighbours, the edge filter type, the 13 SADs (chroma: U + V), the first minimum.  It shares no code with the
loop of oracle/av1o_pipeline.c or with av1-go_amd/csrc; given a frame's source and the closed-loop reconstruction it says what every
block must have chosen, whether the choice was a tie, and whether a candidate's upsampled edge (AV1 spec 7.11.2.11) overshot the
sample range before the clip.  Test infrastructure only."""
import numpy as np

# the candidates in the order they are compared (the first minimum wins): DC V H D45 D135 D113 D157 D203 D67 SMOOTH PAETH SMOOTH_V SMOOTH_H
CANDIDATES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 10, 11)
DC, SMOOTH_MODES = 0, (9, 10, 11)
TILE = 64


def morton(x, y):
    m = 0
    for i in range(4):
        m |= ((x >> i) & 1) << (2 * i) | ((y >> i) & 1) << (2 * i + 1)
    return m


def blocks_in_coding_order(w, h, bs):
    """(fx, fy, top, top_right, left, bottom_left) of every bs x bs block: tile by tile, z-order inside the 64x64 tile; a neighbour is
    available when it lies inside the tile and the frame and was coded before"""
    n, bw, bh = TILE // bs, w // bs, h // bs
    for sby in range((h + TILE - 1) // TILE):
        for sbx in range((w + TILE - 1) // TILE):
            for k in range(n * n):
                bx = sum(((k >> (2 * i)) & 1) << i for i in range(4))
                by = sum(((k >> (2 * i + 1)) & 1) << i for i in range(4))
                fx, fy = sbx * n + bx, sby * n + by
                if fx >= bw or fy >= bh:
                    continue
                top, left = by > 0, bx > 0
                tr = top and bx + 1 < n and fx + 1 < bw and morton(bx + 1, by - 1) < k
                bl = left and by + 1 < n and fy + 1 < bh and morton(bx - 1, by + 1) < k
                yield fx, fy, top, tr, left, bl


def upsamples(b, delta, filter_type):
    """spec 7.11.2.10: is the edge of a b x b block upsampled at this angle delta from the edge's axis"""
    d = abs(delta)
    return 0 < d < 40 and 2 * b <= (8 if filter_type else 16)


# the directional candidates whose angle is within 40 degrees of an axis: (mode, edge, angle delta, does it read the edge's extension)
_UPSAMPLED = ((8, "above", 67 - 90, True), (5, "above", 113 - 90, False), (6, "left", 157 - 180, False), (7, "left", 203 - 180, True))


def raw_edge(P, bd, x, y, b, along, have, have_ext, other, ext):
    """spec 7.11.2: the edge above (along = 'above') or left of the b x b block at (x, y) of plane P, entries -1 .. n - 1 as a list
    whose first entry is the corner; n = 2 b with the extension (top-right / bottom-left).  Unavailable parts repeat the last
    available sample, an unavailable edge is the other edge's first sample or base -/+ 1."""
    base = 128 << (bd - 8)
    n = 2 * b if ext else b
    ref = (lambda i: int(P[y - 1, x + i])) if along == "above" else (lambda i: int(P[y + i, x - 1]))
    first_of_other = (lambda: int(P[y, x - 1])) if along == "above" else (lambda: int(P[y - 1, x]))
    if have:
        avail = b + (b if ext and have_ext else 0)
        e = [ref(min(i, avail - 1)) for i in range(n)]
    elif other:
        e = [first_of_other()] * n
    else:
        e = [base - 1 if along == "above" else base + 1] * n
    if have and other:
        corner = int(P[y - 1, x - 1])
    elif have:
        corner = ref(0)
    elif other:
        corner = first_of_other()
    else:
        corner = base
    return [corner] + e


def upsampled_unclipped(edge):
    """spec 7.11.2.11 without its Clip1: the new half-sample entries of an edge [corner, p0 .. p(n-1)]"""
    buf = [edge[0]] + edge + [edge[-1]]
    return [(-buf[i] + 9 * buf[i + 1] + 9 * buf[i + 2] - buf[i + 3] + 8) >> 4 for i in range(len(edge) - 1)]


def overshoot(P, bd, x, y, b, top, tr, left, bl, filter_type):
    """(below 0, above the top value): does an upsampled edge value of a candidate that upsamples leave the range before the clip"""
    lo = hi = False
    for _, along, delta, ext in _UPSAMPLED:
        if not upsamples(b, delta, filter_type):
            continue
        e = raw_edge(P, bd, x, y, b, along, top if along == "above" else left, tr if along == "above" else bl,
                     left if along == "above" else top, ext)
        v = upsampled_unclipped(e)
        lo, hi = lo or min(v) < 0, hi or max(v) > (1 << bd) - 1
    return lo, hi


def decide(O, src, nb, bd, b, x, y, top, tr, left, bl, filter_type):
    """one decision over the planes that share it (luma: one; chroma: U and V): the 13 SADs in candidate order"""
    sads = []
    for mode in CANDIDATES:
        sad = 0
        for S, P in zip(src, nb):
            pred = O.intra_predict(P, x, y, b, b, mode, 0, bd, b if top else 0, b if tr else 0, b if left else 0, b if bl else 0,
                                   filter_type=filter_type)
            sad += int(np.abs(S[y:y + b, x:x + b].astype(np.int64) - pred).sum())
        sads.append(sad)
    return sads


def frame_decisions(O, src, rec, bd, bs, open_loop=False):
    """src, rec = (Y, U, V) of one frame; rec the closed-loop reconstruction (with open_loop the candidates are predicted from the
    source's own neighbours with filter type 0, and rec is not read).  Returns per plane kind ('y', 'uv') a dict of arrays over the
    blocks in raster order: mode (the first minimum), tied (the minimum is reached more than once), dc_tied (DC is among them),
    ft (the filter type), lo / hi (a candidate's unclipped upsampled edge value lies below 0 / above top)."""
    h, w = src[0].shape
    bw, nblk = w // bs, (w // bs) * (h // bs)
    out = {k: dict(mode=np.zeros(nblk, np.uint8), tied=np.zeros(nblk, bool), dc_tied=np.zeros(nblk, bool), ft=np.zeros(nblk, np.uint8),
                   lo=np.zeros(nblk, bool), hi=np.zeros(nblk, bool)) for k in ("y", "uv")}
    nbp = src if open_loop else rec
    for fx, fy, top, tr, left, bl in blocks_in_coding_order(w, h, bs):
        blk = fy * bw + fx
        for kind, planes, b in (("y", (0,), bs), ("uv", (1, 2), bs // 2)):
            o = out[kind]
            ft = 0
            if not open_loop:      # a smooth-predicted neighbour inside the tile, per plane kind
                ft = int((top and o["mode"][blk - bw] in SMOOTH_MODES) or (left and o["mode"][blk - 1] in SMOOTH_MODES))
            sads = decide(O, [src[p] for p in planes], [nbp[p] for p in planes], bd, b, fx * b, fy * b, top, tr, left, bl, ft)
            best = min(sads)
            o["mode"][blk] = CANDIDATES[sads.index(best)]
            o["tied"][blk] = sads.count(best) > 1
            o["dc_tied"][blk] = sads.count(best) > 1 and sads[0] == best
            o["ft"][blk] = ft
            for p in planes:
                lo, hi = overshoot(nbp[p], bd, fx * b, fy * b, b, top, tr, left, bl, ft)
                o["lo"][blk] |= lo
                o["hi"][blk] |= hi
    return out
