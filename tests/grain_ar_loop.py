"""The closed loop of coloured film grain on the CPU, tests/filmgrain_loop.py's with a grain that has a size: the clean picture of that
file + Gaussian grain smoothed by [1 2 1] x [1 2 1] -> tests/denoise_ref.py -> grain records and tests/grain_cov_ref.py ->
av1mi_film_grain_from_records_ar -> a stream (the oracle codes the denoised frame) -> dav1d with the grain on and off.
TEST INFRASTRUCTURE; no GPU."""
import numpy as np

import denoise_ref as R
import filmgrain_loop as F
import grain_cov_ref as GC

OFFSETS = ((1, 0), (0, 1), (1, 1), (2, 0))      # (dx, dy)
TAPS = np.array([1.0, 2.0, 1.0]) / 4.0
# rho of white noise through TAPS in both directions: the taps' autocorrelation [6, 4, 1] / 16, normalised, per axis
INJECTED = {(1, 0): 4 / 6, (0, 1): 4 / 6, (1, 1): 16 / 36, (2, 0): 1 / 6}


def coloured(rng, shape, sigma):
    """Gaussian noise of standard deviation sigma whose normalised covariance is INJECTED (smoothed cyclically: no edge is special)"""
    a = rng.normal(0, 1, shape)
    for axis in (len(shape) - 2, len(shape) - 1):
        a = sum(t * np.roll(a, k - 1, axis) for k, t in enumerate(TAPS))
    return a * (sigma / (6 / 16))      # the taps' energy per axis is 6 / 16


def rho_of(d):
    """the normalised covariance of a plane at OFFSETS, its mean removed"""
    d = np.asarray(d, np.float64)
    d = d - d.mean()
    h, w = d.shape
    c0 = (d * d).mean()
    return {(dx, dy): float((d[:h - dy, :w - dx] * d[dy:, dx:]).mean() / c0) for dx, dy in OFFSETS}


def loop(O, P, sigma8, bd, seed, lag, frame_index=1):
    """-> dict(ratio: per region std(grain on - grain off) / the injected sigma, rho: {offset: mean over the regions of the synthesised
    grain's}, residual_rho: the luma covariance's, grain: the FilmGrain)"""
    import av1stream
    import dav1d_grain as DG
    import test_av1_conformance as TC
    rng = np.random.default_rng(seed)
    sigma = sigma8 * (1 << (bd - 8))
    dt = np.uint8 if bd == 8 else np.uint16
    Y, Cc = F.clean(bd)
    noisy = [np.clip(np.rint(a[None] + coloured(rng, (3,) + a.shape, sigma)), 0, (1 << bd) - 1).astype(dt) for a in (Y, Cc, Cc)]
    runs = [R.run(a, a.shape[2], a.shape[1], bd, F.STRENGTH) for a in noisy]
    rec = np.stack([r[1][1] for r in runs])                                   # the middle frame's records [plane, bin]
    cov = np.stack([GC.plane(a[1], r[0][1], a.shape[2], a.shape[1]) for a, r in zip(noisy, runs)])
    g = av1stream.film_grain_from_records_ar(rec, cov, bd, frame_index, lag)
    src = [r[0][1] for r in runs]                                             # the denoised middle frame
    r = O.intra_encode_frame(src[0], src[1], src[2], bd, 8, F.Q)
    hdr, _ = TC._filters(O, P, r, bd, F.Q, 0, F.W, F.H, np.zeros((F.H // 8, F.W // 8), np.uint8), src)
    stream = av1stream.temporal_unit(F.W, F.H, bd, F.Q, y_mode=r["modes_y"], uv_mode=r["modes_uv"], lev_y=r["lev_y"], lev_u=r["lev_u"], lev_v=r["lev_v"],
                                     film_grain=g, **hdr)
    off, on = DG.decode(stream, False)[0], DG.decode(stream, True)[0]
    d = on[0].astype(np.float64) - off[0]
    per = [rho_of(d[r0:r1]) for r0, r1 in F.ROWS]
    f = GC.rho(cov[0])
    return dict(ratio=[d[r0:r1].std() / sigma for r0, r1 in F.ROWS], rho={o: float(np.mean([p[o] for p in per])) for o in OFFSETS},
                residual_rho={o: f(*o) for o in OFFSETS}, grain=g, records=rec, cov=cov)
