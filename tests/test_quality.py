"""The quality records on the CPU (include/av1mi.h "quality"; av1-go_amd/csrc/quality.hpp): the host twin av1mi_quality_planes_host
against the numpy restatement (quality_ref.py), the constants, the argument rules, the two command line options and the stats file's
summary line.  Integers are compared for equality.

ssim_sum: the per-window values are the same bits by construction (integers, one product above, one below, one IEEE division); only
the order of the additions differs from the reference's correctly rounded sum.  With at most 2.6e5 windows per plane here the bound is
2.6e5 * 2^-53 = 3e-11 of the sum of magnitudes; the tolerance is the issue's relative 1e-12.  Measured: noise and codec-like content
stay below 2e-14 (the rounding errors of a running sum accumulate like a random walk, sqrt(n) * 2^-53); the worst case is the host
twin's running sum over equal values (all 0 against all L, where every addition rounds the same way): 4.8e-13 at 1366x768."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import quality_ref as R

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "av1-go_amd", "host", "libav1mi_host.so")
RTOL = 1e-12


def _r8(n):
    return (n + 7) & ~7


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(HOST)
    lib.av1mi_quality_planes_host.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5
    lib.av1mi_quality_psnr.argtypes = [C.c_void_p, C.c_int]
    lib.av1mi_quality_psnr.restype = C.c_double
    lib.av1mi_quality_ssim.argtypes = [C.c_void_p]
    lib.av1mi_quality_ssim.restype = C.c_double
    return lib


def planes_of(w, h):
    return [(w, h), ((w + 1) // 2, (h + 1) // 2), ((w + 1) // 2, (h + 1) // 2)]


def content(kind, bd, w, h, frames, seed):
    """(src, dec): per frame (Y, U, V) at the TRUE sizes"""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bd == 8 else np.uint16
    L = (1 << bd) - 1
    src, dec = [], []
    for f in range(frames):
        a, b = [], []
        for pw, ph in planes_of(w, h):
            if kind == "noise":
                x, y = rng.integers(0, L + 1, (ph, pw)), rng.integers(0, L + 1, (ph, pw))
            elif kind == "near":       # what a codec leaves: the source plus a small error
                x = rng.integers(0, L + 1, (ph, pw))
                y = np.clip(x + rng.integers(-3, 4, (ph, pw)), 0, L)
            elif kind == "identical":
                x = rng.integers(0, L + 1, (ph, pw))
                y = x.copy()
            elif kind == "extremes":
                x, y = np.zeros((ph, pw), np.int64), np.full((ph, pw), L)
            elif kind == "last_column":      # one differing sample in the last column
                x = rng.integers(0, L + 1, (ph, pw))
                y = x.copy()
                y[ph // 2, pw - 1] = (int(x[ph // 2, pw - 1]) + L // 2 + 1) % (L + 1)
            else:
                raise ValueError(kind)
            a.append(x.astype(dt)); b.append(y.astype(dt))
        src.append(a); dec.append(b)
    return src, dec


def stack(frames, w, h, fill):
    """the frames in buffers of the true size rounded up to 8, stacked; the padding holds `fill`, which must not count"""
    dt = frames[0][0].dtype
    out = []
    for i in range(3):
        pw, ph = (_r8(w), _r8(h)) if i == 0 else (_r8(w) // 2, _r8(h) // 2)
        buf = np.full((len(frames), ph, pw), fill, dt)
        for f, planes in enumerate(frames):
            th, tw = planes[i].shape
            buf[f, :th, :tw] = planes[i]
        out.append(np.ascontiguousarray(buf.reshape(len(frames) * ph, pw)))
    return out


def reference(src, dec0, dec1, select, bd):
    frames = len(src)
    out = np.zeros((frames, 3), R.DTYPE)
    for f in range(frames):
        for p in range(3):
            d = dec0[f][p] if select is None or select[f * 3 + p] else dec1[f][p]
            out[f, p] = R.plane(src[f][p], d, bd)
    return out


def host_records(host, bd, w, h, frames, src, dec0, dec1=None, select=None):
    ptrs = lambda planes: (C.c_void_p * 3)(*[a.ctypes.data for a in planes]) if planes is not None else None
    out = np.zeros((frames, 3), R.DTYPE)
    sel = np.ascontiguousarray(select, np.uint8) if select is not None else None
    rc = host.av1mi_quality_planes_host(bd, w, h, frames, ptrs(src), ptrs(dec0), ptrs(dec1), sel.ctypes.data if sel is not None else None, out.ctypes.data)
    assert rc == 0
    return out


def compare(got, want, what, rtol=RTOL):
    worst = 0.0
    for k in ("sse", "samples", "windows"):
        assert np.array_equal(got[k], want[k]), "%s: %s differs: %s vs %s" % (what, k, got[k].tolist(), want[k].tolist())
    for g, r in zip(got["ssim_sum"].ravel(), want["ssim_sum"].ravel()):
        err = abs(g - r) / abs(r) if r else abs(g)
        worst = max(worst, err)
    print("%s: worst relative error of ssim_sum %.3g" % (what, worst))
    assert worst <= rtol, "%s: ssim_sum off by %.3g relative" % (what, worst)
    return worst


SIZES = [(16, 16, 1), (24, 40, 1), (854, 480, 1), (1366, 768, 1), (192, 128, 3)]
KINDS = ["noise", "near", "identical", "extremes", "last_column"]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h,frames", SIZES)
def test_host_twin_matches_numpy(host, w, h, frames, bd):
    L = (1 << bd) - 1
    for kind in KINDS:
        src, dec = content(kind, bd, w, h, frames, 3)
        alt, select = None, None
        if frames > 1:      # a select array that mixes both candidates
            _, alt = content("noise", bd, w, h, frames, 4)
            select = [(f + p) % 2 for f in range(frames) for p in range(3)]
        got = host_records(host, bd, w, h, frames, stack(src, w, h, L), stack(dec, w, h, 0), stack(alt, w, h, L) if alt else None, select)
        want = reference(src, dec, alt, select, bd)
        compare(got, want, "%dx%d x%d, %d bit, %s" % (w, h, frames, bd, kind))
        for f in range(frames):
            for p, (pw, ph) in enumerate(planes_of(w, h)):
                assert got[f, p]["samples"] == pw * ph and got[f, p]["windows"] == (pw // 4 - 1) * (ph // 4 - 1)
        first = [(f, p) for f in range(frames) for p in range(3) if select is None or select[f * 3 + p]]
        if kind == "identical":
            for f, p in first:
                rec = got[f, p:p + 1]
                assert rec["sse"][0] == 0 and rec["ssim_sum"][0] == float(rec["windows"][0])      # every window exactly 1.0
                assert math.isinf(host.av1mi_quality_psnr(rec.ctypes.data, bd)) and host.av1mi_quality_ssim(rec.ctypes.data) == 1.0
                assert (R.window_values(src[f][p], dec[f][p], bd) == 1.0).all()
        if kind == "extremes":
            for f, p in first:
                assert got[f, p]["sse"] == L * L * int(got[f, p]["samples"])
                assert host.av1mi_quality_psnr(got[f, p:p + 1].ctypes.data, bd) == 0.0
        if kind == "last_column":
            # outside the whole blocks wherever the plane's width is not a multiple of 4: counts in sse, not in ssim
            for f, p in first:
                pw = planes_of(w, h)[p][0]
                assert got[f, p]["sse"] == (L // 2 + 1) ** 2
                assert (got[f, p]["ssim_sum"] == float(got[f, p]["windows"])) == (pw % 4 != 0)


def test_derived_figures(host):
    src, dec = content("near", 10, 854, 480, 1, 9)
    got = host_records(host, 10, 854, 480, 1, stack(src, 854, 480, 0), stack(dec, 854, 480, 0))
    for p in range(3):
        rec = got[0, p:p + 1]
        assert host.av1mi_quality_psnr(rec.ctypes.data, 10) == pytest.approx(R.psnr(rec[0], 10), rel=1e-14)
        assert host.av1mi_quality_ssim(rec.ctypes.data) == R.ssim(rec[0])


def test_constants(host):
    host.av1mi_host_quality_constants.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    for bd, want in ((8, (416, 235963)), (10, (6698, 3797644))):
        c1, c2 = C.c_longlong(), C.c_longlong()
        host.av1mi_host_quality_constants(bd, C.byref(c1), C.byref(c2))
        assert (c1.value, c2.value) == want == R.constants(bd)


def test_small_sizes_are_refused(host):
    a = np.zeros((64, 64), np.uint8)
    out = np.zeros((1, 3), R.DTYPE)
    p = (C.c_void_p * 3)(a.ctypes.data, a.ctypes.data, a.ctypes.data)
    for w, h in ((15, 16), (16, 15), (8, 8), (0, 0), (15, 64)):
        assert host.av1mi_quality_planes_host(8, w, h, 1, p, p, None, None, out.ctypes.data) == -1      # AV1MI_E_INVAL
    assert host.av1mi_quality_planes_host(8, 16, 16, 1, p, p, None, None, out.ctypes.data) == 0
    assert host.av1mi_quality_planes_host(9, 16, 16, 1, p, p, None, None, out.ctypes.data) == -1
    sel = np.ones(3, np.uint8)
    assert host.av1mi_quality_planes_host(8, 16, 16, 1, p, p, None, sel.ctypes.data, out.ctypes.data) == -1     # a select array needs the second candidate


def _parse(host, argv):
    host.av1mi_host_parse_quality_options.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_int]
    path, err, bound = C.create_string_buffer(512), C.create_string_buffer(512), C.c_double(-1)
    rc = host.av1mi_host_parse_quality_options("\n".join(argv).encode(), path, 512, C.byref(bound), err, 512)
    return rc, path.value.decode(), bound.value, err.value.decode()


def test_parse_backend_job_accepts_the_options(host):
    assert _parse(host, ["-i", "in.y4m", "out.obu"]) == (0, "", 0.0, "")
    assert _parse(host, ["-i", "in.y4m", "-av1mi_stats", "/tmp/s.log", "-av1mi_min_psnr", "38.5", "out.obu"]) == (0, "/tmp/s.log", 38.5, "")
    for bad in ("abc", "-1", "", "nan", "inf", "-inf", "1e999"):      # a bound is finite: no lossy file reaches inf
        rc, _, _, err = _parse(host, ["-i", "in.y4m", "-av1mi_min_psnr", bad, "out.obu"])
        assert rc == -1 and "-av1mi_min_psnr" in err


def test_summary_line_from_hand_made_records(host):
    host.av1mi_host_quality_summary_line.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    recs = np.zeros((3, 3), R.DTYPE)
    # (sse, ssim_sum, samples, windows); frame 1's U plane is lossless
    rows = [[(5000, 90.0, 10000, 100), (700, 23.5, 2500, 25), (900, 24.0, 2500, 25)],
            [(8000, 80.0, 10000, 100), (0, 25.0, 2500, 25), (1100, 22.0, 2500, 25)],
            [(2000, 99.0, 10000, 100), (300, 24.5, 2500, 25), (100, 24.75, 2500, 25)]]
    for f in range(3):
        for p in range(3):
            recs[f, p] = rows[f][p]
    sizes = np.array([1200, 340, 355], np.int64)
    buf = C.create_string_buffer(1024)
    n = host.av1mi_host_quality_summary_line(recs.ctypes.data, sizes.ctypes.data, 3, 8, buf, 1024)
    line = buf.value.decode()
    assert n == len(line)
    assert line == "summary frames:3 bytes:1895 " + R.fmt(R.summary(recs, 8))
    # by hand: luma sse 15000 over 30000 samples; ssim_y the mean of 0.90, 0.80, 0.99
    f = dict(kv.split(":") for kv in line.split()[1:])
    assert float(f["psnr_y"]) == pytest.approx(10 * math.log10(255 * 255 * 30000 / 15000), abs=1e-6)
    assert float(f["ssim_y"]) == pytest.approx((0.90 + 0.80 + 0.99) / 3, abs=1e-6)
    assert float(f["psnr_all"]) == pytest.approx(10 * math.log10(255 * 255 * 45000 / 18100), abs=1e-6)
    # a lossless clip prints inf
    recs["sse"] = 0
    host.av1mi_host_quality_summary_line(recs.ctypes.data, sizes.ctypes.data, 3, 8, buf, 1024)
    assert " psnr_y:inf psnr_u:inf psnr_v:inf psnr_all:inf " in buf.value.decode()
