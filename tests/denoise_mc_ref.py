"""Motion-compensated denoising (include/av1mi.h "motion-compensated denoising") in numpy, written from the header's text: the reference
the kernels (av1-go_amd/csrc/grain_kernels.hip) are compared with bit for bit.  The weights, K, the output and the records are
tests/denoise_ref.py's; this file adds the block search and the displaced comparison.  Integers only; no GPU."""
import numpy as np

import denoise_ref as R

BLOCK = 16
VEC_DTYPE = np.dtype([("dx_p", "i1"), ("dy_p", "i1"), ("dx_n", "i1"), ("dy_n", "i1")])      # av1mi_denoise_vec


def grid(w0, h0):
    """(blocks across, blocks down) of a luma plane of true size w0 x h0"""
    return (w0 + BLOCK - 1) // BLOCK, (h0 + BLOCK - 1) // BLOCK


def candidates(rng):
    """the candidates (dx, dy) by rank: (0, 0) first, the others in raster order of (dy, dx) from (-rng, -rng)"""
    assert rng in (4, 8)
    return [(0, 0)] + [(dx, dy) for dy in range(-rng, rng + 1) for dx in range(-rng, rng + 1) if (dx, dy) != (0, 0)]


def _displaced(F, w, h, X, Y, vx, vy):
    """F(clamp(X + vx), clamp(Y + vy)) over the true size"""
    return np.asarray(F)[np.clip(Y + vy, 0, h - 1), np.clip(X + vx, 0, w - 1)].astype(np.int64)


def block_sums(a):
    """[h, w] -> [blocks down, blocks across]: the sum over every 16x16 block (the last ones may be partial)"""
    h, w = a.shape
    return np.add.reduceat(np.add.reduceat(a, np.arange(0, h, BLOCK), axis=0), np.arange(0, w, BLOCK), axis=1)


def search(C, F, w0, h0, bd, strength, rng, bias=True):
    """the vector of every block towards F: int [blocks down, blocks across, 2] = (dx, dy), and the winning cost"""
    T = R.threshold(strength, bd)
    Y, X = np.mgrid[0:h0, 0:w0]
    c = np.asarray(C)[:h0, :w0].astype(np.int64)
    n = block_sums(np.ones((h0, w0), np.int64))
    best = None
    cand = candidates(rng)
    for rank, (dx, dy) in enumerate(cand):
        cost = block_sums(np.abs(c - _displaced(F, w0, h0, X, Y, dx, dy))) + ((n * T) >> 2 if rank and bias else 0)
        assert cost.max() < 1 << 19
        key = (cost << 11) | rank
        best = key if best is None else np.minimum(best, key)
    vec = np.array(cand, np.int64)[best & 2047]
    return vec, best >> 11


def vectors(P, C, N, w0, h0, bd, strength, rng):
    """the records of a middle frame's blocks, VEC_DTYPE [blocks] in raster order"""
    vp, vn = search(C, P, w0, h0, bd, strength, rng)[0], search(C, N, w0, h0, bd, strength, rng)[0]
    out = np.zeros(vp.shape[:2], VEC_DTYPE)
    out["dx_p"], out["dy_p"], out["dx_n"], out["dy_n"] = vp[..., 0], vp[..., 1], vn[..., 0], vn[..., 1]
    return out.reshape(-1)


def sad3(C, F, w, h, vx, vy):
    """D_F: the 3x3 sum of |C(cx, cy) - F(clamp(cx + vx), clamp(cy + vy))|, (cx, cy) clamped, (vx, vy) the vector of the block that holds
    the CENTRE sample: int64 arrays [h, w]"""
    Y, X = np.mgrid[0:h, 0:w]
    c = np.asarray(C)
    d = np.zeros((h, w), np.int64)
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            cx, cy = np.clip(X + i, 0, w - 1), np.clip(Y + j, 0, h - 1)
            d += np.abs(c[cy, cx].astype(np.int64) - _displaced(F, w, h, cx, cy, vx, vy))
    return d


def plane(P, C, N, w, h, bd, strength, vec, nbx, ss=(0, 0), end=False):
    """one plane of frame C, subsampled by ss = (ssx, ssy) against luma; vec: the frame's VEC_DTYPE [blocks], nbx blocks across -> (the
    buffer's size, the padding replicating the output's own edge; the record)"""
    C = np.asarray(C)
    rec = R.empty_record()
    if end:
        out = C[:h, :w].copy()
    else:
        T = R.threshold(strength, bd)
        Y, X = np.mgrid[0:h, 0:w]
        blk = ((Y << ss[1]) >> 4) * nbx + ((X << ss[0]) >> 4)
        v = np.asarray(vec).reshape(-1)[blk]
        vxp, vyp, vxn, vyn = (v[k].astype(np.int64) >> s for k, s in (("dx_p", ss[0]), ("dy_p", ss[1]), ("dx_n", ss[0]), ("dy_n", ss[1])))      # (>>: floor)
        wp, wn = R.weight(sad3(C, P, w, h, vxp, vyp), T), R.weight(sad3(C, N, w, h, vxn, vyn), T)
        c = C[:h, :w].astype(np.int64)
        num = 16 * c + wp * _displaced(P, w, h, X, Y, vxp, vyp) + wn * _displaced(N, w, h, X, Y, vxn, vyn)
        o = (num * np.asarray(R.K, np.int64)[wp + wn] + (1 << 15)) >> 16
        out = o.astype(C.dtype)
        ok = (wp + wn) >= R.COUNTED_FROM
        b, r = (o >> (bd - 4))[ok], (c - o)[ok]
        rec["sum_sq"] = [int((r[b == i] ** 2).sum()) for i in range(R.BINS)]
        rec["count"] = np.bincount(b, minlength=R.BINS)
    H, W = C.shape
    return np.pad(out, ((0, H - h), (0, W - w)), mode="edge"), rec


def run(planes, true_sizes, bd, strength, rng, force=None):
    """a run of frames: planes = up to three arrays [n, H, W] (luma first; None or an empty one = no such plane), true_sizes their (w, h)
    -> (outputs per plane, records [n, BINS] per plane, vectors VEC_DTYPE [n, blocks]).  The ends of the run pass through, are not
    searched and have zero vectors.  force: vectors [n, blocks] to filter with in place of the search's"""
    Y = np.asarray(planes[0])
    n = Y.shape[0]
    w0, h0 = true_sizes[0]
    nbx, nby = grid(w0, h0)
    vec = np.zeros((n, nbx * nby), VEC_DTYPE)
    for f in range(1, n - 1):
        vec[f] = force[f] if force is not None else vectors(Y[f - 1], Y[f], Y[f + 1], w0, h0, bd, strength, rng)
    outs, recs = [], []
    for a, (w, h) in zip(planes, true_sizes):
        if a is None or not np.asarray(a).size:
            outs.append(None); recs.append(None)
            continue
        a = np.asarray(a)
        ss = (int(a.shape[2] < Y.shape[2]), int(a.shape[1] < Y.shape[1]))
        res = [plane(a[max(f - 1, 0)], a[f], a[min(f + 1, n - 1)], w, h, bd, strength, vec[f], nbx, ss, end=f == 0 or f == n - 1) for f in range(n)]
        outs.append(np.stack([o for o, _ in res])); recs.append(np.stack([r for _, r in res]))
    return outs, recs, vec
