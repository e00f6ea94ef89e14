"""Clips for the tests of motion-compensated denoising: a textured picture that translates by a whole number of luma samples per frame
under independent Gaussian grain, in any chroma layout."""
import numpy as np

STEP = (3, -2)      # luma samples per frame, (x, y): block vectors are (-3, 2) towards P and (3, -2) towards N


def texture(w, h, seed, margin):
    """[h + 2 margin, w + 2 margin] in 8-bit code values: coarse patches under per-sample detail, so that every 16x16 block has ONE best match"""
    rng = np.random.default_rng(seed)
    H, W = h + 2 * margin, w + 2 * margin
    coarse = np.kron(rng.integers(-40, 41, ((H + 7) // 8, (W + 7) // 8)), np.ones((8, 8), np.int64))[:H, :W]
    return 128 + coarse + rng.integers(-24, 25, (H, W))


def translating(sizes, n, bd, seed, sigma, step=STEP, true=None):
    """per plane [n, H, W] (sizes = (W, H) per plane, luma first, (0, 0) = none -> None): frame f shows the texture displaced by f * step;
    chroma planes sample their own texture at the luma positions they cover.  true: the luma true size, beyond which the buffers hold junk"""
    W0, H0 = sizes[0]
    margin = n * max(abs(step[0]), abs(step[1])) + 1
    rng = np.random.default_rng(seed + 1000)
    dt = np.uint8 if bd == 8 else np.uint16
    out = []
    for p, (W, H) in enumerate(sizes):
        if not W or not H:
            out.append(None)
            continue
        ssx, ssy = int(W < W0), int(H < H0)
        tex = texture(W0, H0, seed + p, margin)
        fr = []
        for f in range(n):
            ox, oy = margin - f * step[0], margin - f * step[1]
            a = tex[oy:oy + H0:1 << ssy, ox:ox + W0:1 << ssx][:H, :W]
            a = (a << (bd - 8)) + np.rint(rng.normal(0, sigma * (1 << (bd - 8)), a.shape)).astype(np.int64)
            fr.append(np.clip(a, 0, (1 << bd) - 1))
        a = np.stack(fr).astype(dt)
        if true is not None:      # the input's padding must not matter
            tw, th = (true[0] + ssx) >> ssx, (true[1] + ssy) >> ssy
            a[:, th:, :] = (1 << bd) - 1
            a[:, :, tw:] = 0
        out.append(a)
    return out


def true_sizes(sizes, true):
    """the planes' true sizes for a luma true size: halved upwards where the plane is subsampled"""
    return [(((true[0] + int(W < sizes[0][0])) >> int(W < sizes[0][0])), ((true[1] + int(H < sizes[0][1])) >> int(H < sizes[0][1]))) if W and H else (0, 0) for (W, H) in sizes]
