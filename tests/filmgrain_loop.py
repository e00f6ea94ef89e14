"""The closed loop of the film grain feature on the CPU: a clean picture with three flat regions + Gaussian grain -> tests/denoise_ref.py
-> grain records -> av1mi_film_grain_from_records -> a stream (the oracle codes the denoised frame) -> dav1d with the grain on and off.
TEST INFRASTRUCTURE; no GPU."""
import numpy as np

import denoise_ref as R

W = H = 256
LEVELS = (56, 136, 200)                      # 8-bit values at the centres of bins 3, 8 and 12
ROWS = ((0, 80), (88, 168), (176, 256))      # the regions: bands of 80 rows, 8 rows apart (N = 20 480 samples each)
STRENGTH, Q = 16, 60


def clean(bd):
    Y = np.zeros((H, W), np.int64)
    for v, (r0, r1) in zip(LEVELS, ((0, 84), (84, 172), (172, 256))):
        Y[r0:r1] = v << (bd - 8)
    return Y, np.full((H // 2, W // 2), 128 << (bd - 8), np.int64)


def loop(O, P, sigma8, bd, seed, frame_index=1):
    """-> dict(ratio: per region std(grain on - grain off) / the injected sigma, chroma_ratio: per plane, grain: the FilmGrain,
    off: the decoded planes with the grain off)"""
    import av1stream
    import dav1d_grain as DG
    import test_av1_conformance as TC
    rng = np.random.default_rng(seed)
    sigma = sigma8 * (1 << (bd - 8))
    dt = np.uint8 if bd == 8 else np.uint16
    Y, Cc = clean(bd)
    noisy = [np.clip(np.rint(a[None] + rng.normal(0, sigma, (3,) + a.shape)), 0, (1 << bd) - 1).astype(dt) for a in (Y, Cc, Cc)]
    runs = [R.run(a, a.shape[2], a.shape[1], bd, STRENGTH) for a in noisy]
    rec = np.stack([r[1][1] for r in runs])                                   # the middle frame's records [plane, bin]
    g = av1stream.film_grain_from_records(rec, bd, frame_index)
    src = [r[0][1] for r in runs]                                             # the denoised middle frame
    r = O.intra_encode_frame(src[0], src[1], src[2], bd, 8, Q)
    hdr, _ = TC._filters(O, P, r, bd, Q, 0, W, H, np.zeros((H // 8, W // 8), np.uint8), src)
    stream = av1stream.temporal_unit(W, H, bd, Q, y_mode=r["modes_y"], uv_mode=r["modes_uv"], lev_y=r["lev_y"], lev_u=r["lev_u"], lev_v=r["lev_v"],
                                     film_grain=g, **hdr)
    off, on = DG.decode(stream, False)[0], DG.decode(stream, True)[0]
    d = [on[i].astype(np.float64) - off[i] for i in range(3)]
    return dict(ratio=[d[0][r0:r1].std() / sigma for r0, r1 in ROWS], chroma_ratio=[d[i].std() / sigma for i in (1, 2)], grain=g, off=off, records=rec)
