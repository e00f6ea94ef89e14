"""The grain covariance of include/av1mi.h ("grain covariance") in numpy, written from the header's text: the reference the kernels
(av1-go_amd/csrc/grain_cov_kernels.hip) are compared with bit for bit, and what the CPU tests of the AR model feed it with.  Integers
only, one plane at a time; no GPU."""
import numpy as np

DY, DX = 4, 13      # sum[dy][dx + 6], dy = 0 .. 3, dx = -6 .. 6
COV_DTYPE = np.dtype([("sum", "<i8", (DY, DX))])      # av1mi_grain_cov_record


def empty():
    return np.zeros((DY, DX), np.int64)


def of_residual(r):
    """sum[dy][dx + 6] of a residual plane r [h, w] (any integer type): the products of every pair inside the plane"""
    r = np.asarray(r).astype(np.int64)
    h, w = r.shape
    out = empty()
    for dy in range(DY):
        for dx in range(-6, 7):
            if dy >= h or abs(dx) >= w:
                continue      # no such pair
            a = r[:h - dy, max(0, -dx):w - max(0, dx)]
            b = r[dy:, max(0, dx):w - max(0, -dx)]
            out[dy, dx + 6] = int((a * b).sum())
    return out


def plane(C, out, w, h):
    """C (the fed plane, or None = zeros) and out (what the gather wrote), arrays of the BUFFER's size: only the true size w x h is read"""
    o = np.asarray(out)[:h, :w].astype(np.int64)
    c = np.zeros_like(o) if C is None else np.asarray(C)[:h, :w].astype(np.int64)
    return of_residual(c - o)


def rho(cov):
    """the normalised covariance as a function (dx, dy) -> cov(d) / cov(0), with rho(-d) = rho(d); 0 where cov(0) is 0"""
    cov = np.asarray(cov, np.float64)
    c0 = cov[0, 6]

    def f(dx, dy):
        if dy < 0:
            dx, dy = -dx, -dy
        return 0.0 if c0 == 0 else cov[dy, dx + 6] / c0
    return f
