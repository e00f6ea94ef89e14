"""The CDEF search (include/av1mi.h "CDEF search") restated on top of the oracle's CDEF: the candidate strength sets, the per-superblock
squared error of every candidate (the whole frame filtered once per candidate with a uniform set, then summed per superblock over the
true size), the pick.  Shared by the CPU and the GPU tests."""
import numpy as np


def dbl(x):
    return min(15, max(1, 2 * x))


def up(x):
    return min(3, x + 1)


def sets_of(v, bits):
    """the 8 candidate bytes ((primary << 2) | secondary code) from a policy byte v; entries from 1 << bits on are 0"""
    P, S = v >> 2, v & 3
    cand = [(P, S), (0, 0), (P >> 1, S), (dbl(P), S), (P, up(S)), (P, 0), (dbl(P), up(S)), (dbl(dbl(P)), up(S))]
    return [(p << 2) | s if c < (1 << bits) else 0 for c, (p, s) in enumerate(cand)]


def sets(params, bits):
    return sets_of(params.cdef_y, bits), sets_of(params.cdef_uv, bits)


def strength(y, uv, c):
    """candidate c as the four strength bytes the CDEF entry points take"""
    return [y[c] >> 2, y[c] & 3, uv[c] >> 2, uv[c] & 3]


def cdef_with(O, dbl_planes, bd, damping, records, skip8):
    """the oracle's CDEF with one strength record per superblock ([nsb, 4])"""
    return O.cdef_frame(dbl_planes[0], dbl_planes[1], dbl_planes[2], bd, damping, np.asarray(records, np.uint8), skip8)


def table(O, dbl_planes, src, bd, damping, y, uv, bits, skip8, true_size=None):
    """uint64 [sb, 8]: SSE_c per superblock over the three planes inside the true size; columns from 1 << bits on hold 0"""
    h, w = dbl_planes[0].shape
    tw, th = true_size if true_size is not None else (w, h)
    sbh, sbw = (h + 63) // 64, (w + 63) // 64
    t = np.zeros((sbh * sbw, 8), np.uint64)
    for c in range(1 << bits):
        out = cdef_with(O, dbl_planes, bd, damping, np.tile(np.array(strength(y, uv, c), np.uint8), (sbh * sbw, 1)), skip8)
        for p in range(3):
            ph, pw, n = (th, tw, 64) if p == 0 else ((th + 1) // 2, (tw + 1) // 2, 32)
            d = (out[p].astype(np.int64) - np.asarray(src[p]).astype(np.int64))[:ph, :pw] ** 2
            for r in range(sbh):
                for q in range(sbw):
                    t[r * sbw + q, c] += np.uint64(d[r * n:(r + 1) * n, q * n:(q + 1) * n].sum())
    return t


def pick(t, bits):
    """the lowest sum wins, on a tie the lowest index (numpy's argmin takes the first)"""
    return np.argmin(t[:, :1 << bits], axis=1).astype(np.uint8)


def records(y, uv, idx):
    return np.array([strength(y, uv, int(c)) for c in idx], np.uint8)


def content(rng, w, h, bd, shift=0):
    """(source planes, "deblocked" planes) on which the candidates differ per superblock.  By superblock column c % 3: 0 = straight
    edges, with ringing added to the deblocked planes (filtering pays); 1 = fine texture that the deblocked planes reproduce exactly
    (filtering costs); 2 = flat, the deblocked planes equal to the source in the first superblock row (every candidate ties: index
    0) and with faint noise below (a filter pays).  shift moves the edges: frames of different content."""
    mx, sh = (1 << bd) - 1, bd - 8
    src_planes, dbl_planes = [], []
    for p in range(3):
        ph, pw, n = (h, w, 64) if p == 0 else (h // 2, w // 2, 32)
        yy, xx = np.mgrid[0:ph, 0:pw]
        kind = (xx // n) % 3
        edges = (((xx + yy // 2 + shift) // 11) % 2) * (90 << sh) + (40 << sh)
        tex = rng.integers(0, 60 << sh, (ph, pw)) + (80 << sh)
        src = np.where(kind == 0, edges, np.where(kind == 1, tex, 110 << sh)).astype(np.int64)
        ring = rng.integers(-(14 << sh), (14 << sh) + 1, (ph, pw))
        faint = rng.integers(-(3 << sh), (3 << sh) + 1, (ph, pw))
        d = src + np.where(kind == 0, ring, 0) + np.where((kind == 2) & (yy >= n), faint, 0)
        dt = np.uint8 if bd == 8 else np.uint16
        src_planes.append(np.clip(src, 0, mx).astype(dt))
        dbl_planes.append(np.clip(d, 0, mx).astype(dt))
    return src_planes, dbl_planes
