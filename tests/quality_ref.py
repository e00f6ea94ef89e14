"""The quality records of include/av1mi.h ("quality") restated in numpy from the header's text: per plane the exact squared error and
the sum of the 8x8-window, step-4 SSIM values (the x264 / FFmpeg `ssim` form).  Test infrastructure: the host twin
(av1mi_quality_planes_host) and the kernel (av1mi_quality_planes) are compared against it."""
import math

import numpy as np

DTYPE = np.dtype([("sse", "<u8"), ("ssim_sum", "<f8"), ("samples", "<u4"), ("windows", "<u4")])      # av1mi_quality


def constants(bd):
    L = (1 << bd) - 1
    return int(math.floor(0.01 ** 2 * L * L * 64 + 0.5)), int(math.floor(0.03 ** 2 * L * L * 64 * 63 + 0.5))


def window_values(a, b, bd):
    """the SSIM value of every window of one plane, [floor(H / 4) - 1, floor(W / 4) - 1] doubles"""
    H, W = a.shape
    nby, nbx = H // 4, W // 4
    a = a[:nby * 4, :nbx * 4].astype(np.int64)
    b = b[:nby * 4, :nbx * 4].astype(np.int64)
    blk = lambda x: x.reshape(nby, 4, nbx, 4).sum(axis=(1, 3))
    win = lambda x: x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:]
    s1, s2, ss, s12 = win(blk(a)), win(blk(b)), win(blk(a * a + b * b)), win(blk(a * b))
    c1, c2 = constants(bd)
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    f = lambda x: x.astype(np.float64)      # each factor is below 2^35: exact
    return (f(2 * s1 * s2 + c1) * f(2 * covar + c2)) / (f(s1 * s1 + s2 * s2 + c1) * f(vars_ + c2))


def plane(a, b, bd):
    """one record for a (source) against b (decoded), arrays [H, W] at the plane's TRUE size"""
    assert a.shape == b.shape
    d = a.astype(np.int64) - b.astype(np.int64)
    v = window_values(a, b, bd)
    r = np.zeros((), DTYPE)
    r["sse"] = int((d * d).sum())
    r["ssim_sum"] = math.fsum(v.ravel().tolist())      # the correctly rounded sum: the implementations' orders are compared against it
    r["samples"] = a.size
    r["windows"] = v.size
    return r


def frame(src, dec, bd):
    """records [3] of one frame: src / dec = (Y, U, V) at the true sizes"""
    return np.array([plane(s, d, bd) for s, d in zip(src, dec)], DTYPE)


def psnr(records, bd):
    """PSNR of one record, or of several taken together (summed squared error over summed sample counts)"""
    rec = np.atleast_1d(records)
    sse, n = sum(int(x) for x in rec["sse"].ravel()), sum(int(x) for x in rec["samples"].ravel())
    L = (1 << bd) - 1
    return math.inf if sse == 0 else 10.0 * math.log10(L * L * n / sse)


def ssim(record):
    return float(record["ssim_sum"]) / float(record["windows"])


def figures(rec3, bd):
    """the eight figures of one frame from its records [3]: psnr y, u, v, all; ssim y, u, v, all"""
    p = [psnr(rec3[i], bd) for i in range(3)] + [psnr(rec3, bd)]
    s = [ssim(rec3[i]) for i in range(3)]
    return p + s + [(4 * s[0] + s[1] + s[2]) / 6]


def summary(recs, bd):
    """recs [frames, 3] -> the summary's eight figures: PSNR from the squared error summed over all frames, SSIM the mean of the frame
    values"""
    recs = np.asarray(recs)
    p = [psnr(recs[:, i], bd) for i in range(3)] + [psnr(recs, bd)]
    per = np.array([figures(r, bd)[4:] for r in recs])
    return p + per.mean(axis=0).tolist()


def fmt(values):
    names = ["psnr_y", "psnr_u", "psnr_v", "psnr_all", "ssim_y", "ssim_u", "ssim_v", "ssim_all"]
    return " ".join("%s:%s" % (n, "inf" if math.isinf(v) else "%.6f" % v) for n, v in zip(names, values))
