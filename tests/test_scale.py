"""Scaling without a GPU: the resampler's coefficient table (av1mi_scale_filter) against the numpy restatement of the definition in
include/av1mi.h (scale_ref.py), the sanity of that restatement, and the product's argument handling: the `-vf` chain and
`-av1mi_scale`, the Y4M sample aspect ratio, the display size of the Matroska video track."""
import ctypes as C
import os

import numpy as np
import pytest

import scale_ref as R

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "av1-go_amd", "host", "libav1mi_host.so")

PAIRS = [(1440, 1920), (3840, 1920), (4096, 1024), (1024, 4096), (853, 854), (1919, 1920), (1080, 1080), (2160, 1080), (96, 136), (80, 72),
         (720, 768), (427, 427), (8, 32), (512, 128)]

SAR_CHAIN = "scale_vaapi=w='if(gt(iw,iw*sar),iw,iw*sar)':h='if(gt(iw,iw*sar),iw/sar,ih)'"
PLAIN_CHAIN = "scale_vaapi=w=ceil(iw/2)*2:h=ceil(ih/2)*2,hwdownload,format=nv12,setsar=1,format=nv12,hwupload"
WEBRIP_CHAIN = SAR_CHAIN + "," + PLAIN_CHAIN


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(HOST):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(HOST)])
    lib = C.CDLL(HOST)
    lib.av1mi_run_transcode.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t]
    lib.av1mi_host_scale_target.argtypes = [C.c_int] * 4 + [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.av1mi_host_y4m_sar.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    lib.av1mi_host_transcode_args.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int] * 4 + [C.c_char_p, C.c_int]
    return lib


# ---- the table ----------------------------------------------------------------------------------------------------------------

def _pairs():
    rng = np.random.default_rng(1)
    extra = []
    while len(extra) < 8:
        n, m = (int(v) for v in rng.integers(8, 4097, 2))
        if n <= 4 * m and m <= 4 * n:
            extra.append((n, m))
    return PAIRS + extra


def test_filter_table_matches_numpy(av1mi):
    for n, m in _pairs():
        T, first, coef = av1mi.scale_filter(n, m)
        T2, first2, coef2 = R.filter_table(n, m)
        assert T == T2 == R.taps(n, m) and coef.shape == (m, T), (n, m)
        assert (first == first2).all(), (n, m)
        c = coef.astype(np.int64)
        assert (c.sum(axis=1) == 16384).all(), (n, m)
        # the sine of two maths libraries may round one coefficient the other way and the remainder rule then moves a second unit:
        # a bound on rounding, not a quality tolerance
        assert np.abs(c - coef2).max() <= 2, (n, m)
        assert np.abs(c).sum(axis=1).max() < 1.6 * 16384      # the header's bound: the intermediate fits int16 at 10 bits
        if n == m:
            want = np.zeros((m, T), np.int64)
            want[:, T // 2 - 1] = 16384
            assert (c == want).all() and (first == np.arange(m) - T // 2 + 1).all()
    assert av1mi.scale_filter(3840, 1920)[0] == 12 and av1mi.scale_filter(1440, 1920)[0] == 6 and av1mi.scale_filter(4096, 1024)[0] == 24


def test_filter_refuses_bad_sizes_and_ratios(av1mi):
    for n, m in ((7, 8), (8, 7), (4097, 4096), (2048, 4097), (1000, 249), (249, 1000), (0, 8), (-5, 8)):
        with pytest.raises(av1mi.Av1miError):
            av1mi.scale_filter(n, m)
    t = C.c_int()
    assert av1mi.load().av1mi_scale_filter(100, 50, None, None, None) != 0
    assert av1mi.load().av1mi_scale_filter(100, 50, C.byref(t), None, None) == 0 and t.value == 12      # first == NULL: only T


# ---- the numpy restatement is itself sane ---------------------------------------------------------------------------------------

def test_reference_keeps_a_constant_plane_constant():
    for bd, value in ((8, 77), (8, 255), (10, 1023), (10, 0), (10, 513)):
        p = np.full((40, 56), value)
        for mw, mh in ((56, 40), (75, 53), (28, 20), (14, 10), (224, 160), (57, 39)):
            out = R.scale_plane(p, mw, mh, bd)
            assert out.shape == (mh, mw) and (out == value).all(), (bd, value, mw, mh)


def test_reference_keeps_a_ramp_monotone_and_the_identity_exact():
    ramp = np.tile(np.arange(96) * 2, (16, 1))
    out = R.scale_plane(ramp, 128, 16, 8).astype(int)
    assert (np.diff(out[:, 4:-4], axis=1) >= 0).all() and (out == out[0]).all()
    rng = np.random.default_rng(2)
    for bd in (8, 10):
        p = rng.integers(0, 1 << bd, (24, 40))
        assert (R.scale_plane(p, 40, 24, bd) == p).all()
    y, u, v = rng.integers(0, 256, (70, 134)), rng.integers(0, 256, (35, 67)), rng.integers(0, 256, (35, 67))
    oy, ou, ov = R.scale_frame(y, u, v, 134, 70, 8)      # identity into the coded size: the edge is replicated into the padding
    assert oy.shape == (72, 136) and ou.shape == ov.shape == (36, 68)
    assert (oy[:70, :134] == y).all() and (oy[:, 135] == oy[:, 133]).all() and (oy[71] == oy[69]).all()
    assert (ou[:35, :67] == u).all() and (ou[:, 67] == ou[:, 66]).all() and (ov[35] == ov[34]).all()


# ---- argument handling ----------------------------------------------------------------------------------------------------------

def _run(host, tmp_path, extra):
    err = C.create_string_buffer(1024)
    argv = ["-i", str(tmp_path / "missing.y4m")] + extra + [str(tmp_path / "out.obu")]
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    return host.av1mi_run_transcode(len(argv), arr, err, 1024), err.value


def test_filter_chain_and_scale_option_are_parsed_without_a_gpu(host, av1mi, tmp_path):
    """the reference's two chains pass parsing, which without a GPU shows as the later `no usable HIP device` result (code -1); a filter
    that cannot be applied and a malformed -av1mi_scale are ParseBackendJob's `Invalid argument` (exit code 1)"""
    buf = C.create_string_buffer(8192)
    for webrip in (0, 1):      # the argv TranscodeArgs builds carries exactly these chains
        assert host.av1mi_host_transcode_args(b"a", b"b", 1, 0, 1080, webrip, buf, 8192) > 0
        argv = buf.value.decode().split("\n")
        assert argv[argv.index("-vf:v:0") + 1] == (WEBRIP_CHAIN if webrip else PLAIN_CHAIN)
    for good in (["-vf:v:0", PLAIN_CHAIN], ["-vf:v:0", WEBRIP_CHAIN], ["-vf", "scale=1280:720"], ["-av1mi_scale", "1280x720"],
                 ["-vf:v:0", "scale_vaapi=w=640:h=360,setsar=1"]):
        code, text = _run(host, tmp_path, good)
        assert b"Invalid argument" not in text and code != 0, (good, text)
        if av1mi.load().av1mi_device_count() == 0:
            assert code == -1 and b"no usable HIP device" in text
    code, text = _run(host, tmp_path, ["-vf:v:0", "hflip"])
    assert code == 1 and text == b"av1mi failed with exit code 1: Invalid argument: unsupported filter hflip", text
    for bad in (["-vf:v:0", PLAIN_CHAIN + ",crop=16:16"], ["-vf", "scale=iw/2:ih/2"], ["-vf:v:0", "setsar=2"], ["-av1mi_scale", "10x10"],
                ["-av1mi_scale", "0x0"], ["-av1mi_scale", "1920"], ["-av1mi_scale", "5000x100"], ["-av1mi_scale", "64x-64"]):
        code, text = _run(host, tmp_path, bad)
        assert code == 1 and text.startswith(b"av1mi failed with exit code 1: Invalid argument"), (bad, code, text)


def test_scale_target_of_the_reference_chains(host):
    def target(iw, ih, sar, chain):
        w, h = C.c_int(), C.c_int()
        rc = host.av1mi_host_scale_target(iw, ih, sar[0], sar[1], chain.encode(), C.byref(w), C.byref(h))
        return (w.value, h.value) if rc == 0 else None
    assert target(1440, 1080, (4, 3), WEBRIP_CHAIN) == (1920, 1080)
    assert target(720, 576, (16, 15), WEBRIP_CHAIN) == (768, 576)
    assert target(853, 480, (1, 1), PLAIN_CHAIN) == (854, 480)
    assert target(853, 479, (1, 1), WEBRIP_CHAIN) == (854, 480)
    assert target(1920, 1080, (1, 1), PLAIN_CHAIN) == (1920, 1080) and target(1920, 1080, (1, 1), WEBRIP_CHAIN) == (1920, 1080)
    assert target(1440, 1080, (4, 3), PLAIN_CHAIN) == (1440, 1080)            # not a web rip: the pixels stay as they are
    # sar < 1: the expression's second branch divides iw (as written upstream), truncated
    assert target(720, 480, (8, 9), WEBRIP_CHAIN) == (720, 810)
    assert target(1920, 1080, (1, 1), "scale=1280:720") == (1280, 720)
    assert target(1920, 1080, (1, 1), "scale_vaapi=w=641:h=361," + PLAIN_CHAIN) == (642, 362)
    assert target(1920, 1080, (0, 0), WEBRIP_CHAIN) == (1920, 1080)           # unknown aspect ratio = square
    assert target(1920, 1080, (1, 1), "hflip") is None and target(64, 64, (1, 1), "scale=a:b") is None


def test_y4m_sample_aspect_ratio_is_kept(host, tmp_path):
    def sar(field):
        path = tmp_path / "a.y4m"
        path.write_bytes(("YUV4MPEG2 W16 H16 F30:1 Ip %sC420jpeg\n" % field).encode() + b"FRAME\n" + bytes(16 * 16 * 3 // 2))
        out = (C.c_int * 2)()
        assert host.av1mi_host_y4m_sar(str(path).encode(), out) == 0
        return out[0], out[1]
    assert sar("A16:15 ") == (16, 15) and sar("A4:3 ") == (4, 3) and sar("A1:1 ") == (1, 1)
    assert sar("") == (1, 1) and sar("A0:0 ") == (1, 1) and sar("Ax ") == (1, 1) and sar("A4 ") == (1, 1) and sar("A-4:3 ") == (1, 1)


def test_display_size_of_the_matroska_video_track(host, tmp_path):
    units = [b"\x12\x00" + bytes([i] * 20) for i in range(3)]
    data = b"".join(units)
    sizes = (C.c_longlong * 3)(*[len(u) for u in units])
    keys = (C.c_uint8 * 3)(1, 0, 0)
    outs = {}
    for name, dw, dh in (("none", 0, 0), ("wide", 384, 288)):
        path = tmp_path / (name + ".mkv")
        assert host.av1mi_host_mux_units_display(str(path).encode(), 360, 288, 8, 30, 1, data, sizes, keys, 3, dw, dh) == 0
        outs[name] = path.read_bytes()
    plain = tmp_path / "plain.mkv"
    assert host.av1mi_host_mux_units(str(plain).encode(), 360, 288, 8, 30, 1, data, sizes, keys, 3) == 0
    assert outs["none"] == plain.read_bytes()                              # tracks of 1:1 sources are written exactly as before
    assert b"\x54\xb0" not in outs["none"] and b"\x54\xba" not in outs["none"]
    w = outs["wide"]
    assert b"\xb0\x82\x01\x68" in w and b"\xba\x82\x01\x20" in w           # PixelWidth 360, PixelHeight 288
    assert b"\x54\xb0\x82\x01\x80" in w and b"\x54\xba\x82\x01\x20" in w   # DisplayWidth 384, DisplayHeight 288
    assert len(w) == len(outs["none"]) + 10
