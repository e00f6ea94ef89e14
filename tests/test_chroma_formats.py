"""Chroma formats without a GPU (include/av1mi.h "chroma formats"): the numpy reference's own properties, Y4mSource with and without
the job's opt-in, the argument parsing that sets it, and the buffer sizes of every layout."""
import ctypes as C
import os

import numpy as np
import pytest

import chroma_formats_ref as R

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "av1-go_amd", "host", "libav1mi_host.so")
REFERENCE_CHAIN = "scale_vaapi=w=ceil(iw/2)*2:h=ceil(ih/2)*2,hwdownload,format=nv12,setsar=1,format=nv12,hwupload"      # transcode.go:97-112


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(HOST)
    lib.av1mi_host_y4m_layout.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    lib.av1mi_host_parse_format_option.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.av1mi_host_transcode_args.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int] * 4 + [C.c_char_p, C.c_int]
    return lib


# ---- the reference's own properties -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src_bd,bd", R.DEPTHS)
@pytest.mark.parametrize("chroma", R.LAYOUTS)
def test_a_constant_plane_stays_constant(chroma, src_bd, bd):
    w, h, d = 22, 14, src_bd - bd
    for value in (0, 1, 37 << (src_bd - 8), (1 << src_bd) - 4):      # (values that round down: every filter then gives value >> d)
        planes = [None if s is None else np.full(s, value, R.dtype(src_bd)) for s in R.buffer_shapes(chroma, w, h)]
        out = R.convert(chroma, src_bd, bd, w, h, planes)
        assert out[0].shape == (16, 24) and out[1].shape == out[2].shape == (8, 12) and out[0].dtype == R.dtype(bd)
        assert (out[0] == value >> d).all()
        for p in (1, 2):
            assert (out[p] == (1 << (bd - 1) if chroma == R.C400 else value >> d)).all()


@pytest.mark.parametrize("chroma", R.LAYOUTS)
def test_all_max_12_bit_gives_max(chroma):
    """(4095 + 2) >> 2 = 1024: the sum rounds past the 10-bit maximum, so the clamp matters — in every filter"""
    planes = R.content("max", chroma, 12, 22, 14)
    out = R.convert(chroma, 12, 10, 22, 14, planes)
    assert (out[0] == 1023).all()
    for p in (1, 2):
        assert (out[p] == (512 if chroma == R.C400 else 1023)).all()


@pytest.mark.parametrize("bd", [8, 10])
def test_420_at_equal_depths_is_the_identity(bd):
    planes = R.content("noise", R.C420, bd, 24, 16, seed=3)
    out = R.convert(R.C420, bd, bd, 24, 16, planes)
    for p in range(3):
        assert out[p].dtype == planes[p].dtype and (out[p] == planes[p]).all()
    # a cropped size: the true samples unchanged, the padding the clamped edge (never the buffer's padding)
    planes = R.content("noise", R.C420, bd, 21, 13, seed=4, padding=(1 << bd) - 1)
    out = R.convert(R.C420, bd, bd, 21, 13, planes)
    assert (out[0][:13, :21] == planes[0][:13, :21]).all() and (out[0][:, 21:] == out[0][:, 20:21]).all() and (out[0][13:] == out[0][12:13]).all()
    assert (out[1][:7, :11] == planes[1][:7, :11]).all() and (out[1][:, 11:] == out[1][:, 10:11]).all() and (out[1][7:] == out[1][6:7]).all()


def test_filters_on_known_samples():
    """hand-computed: the 4:2:2 pair average, the 4:4:4 [1 2 1] x [1 1] filter with its left clamp, one rounding each"""
    u = np.zeros((8, 4), np.uint8)
    u[0, 0], u[1, 0], u[2, 1], u[3, 1] = 10, 13, 255, 255
    out = R.convert(R.C422, 8, 8, 8, 8, [np.zeros((8, 8), np.uint8), u, u])
    assert out[1][0, 0] == 12 and out[1][1, 1] == 255 and out[1][0, 1] == 0      # (10 + 13 + 1) >> 1
    u = np.zeros((8, 8), np.uint8)
    u[0, 0:3] = (8, 16, 40)
    u[1, 0:3] = (8, 16, 40)
    out = R.convert(R.C444, 8, 8, 8, 8, [np.zeros((8, 8), np.uint8), u, u])
    assert out[1][0, 0] == (2 * (8 + 2 * 8 + 16) + 4) >> 3      # in(-1) = in(0)
    assert out[1][0, 1] == (2 * (16 + 2 * 40 + 0) + 4) >> 3
    chk = R.content("checker", R.C444, 10, 16, 16)
    out = R.convert(R.C444, 10, 10, 16, 16, chk)
    assert (out[1][:, 1:] == 512).all()      # a one-sample checkerboard averages out: (4 * 1023 + 4) >> 3, away from the left clamp


def test_nothing_beyond_the_true_size_is_read():
    for chroma in R.LAYOUTS:
        for src_bd, bd in R.DEPTHS:
            a = R.content("noise", chroma, src_bd, 21, 13, seed=5, padding=0)
            b = R.content("noise", chroma, src_bd, 21, 13, seed=5, padding=(1 << src_bd) - 1)
            for x, y in zip(R.convert(chroma, src_bd, bd, 21, 13, a), R.convert(chroma, src_bd, bd, 21, 13, b)):
                assert (x == y).all()


# ---- Y4mSource ------------------------------------------------------------------------------------------------------------------

ACCEPTED = {      # tag: (chroma, source depth, coded depth)
    "420jpeg": (0, 8, 8), "420mpeg2": (0, 8, 8), "420paldv": (0, 8, 8), "420": (0, 8, 8), "422": (1, 8, 8), "444": (2, 8, 8), "mono": (3, 8, 8),
    "420p10": (0, 10, 10), "422p10": (1, 10, 10), "444p10": (2, 10, 10), "mono10": (3, 10, 10),
    "420p12": (0, 12, 10), "422p12": (1, 12, 10), "444p12": (2, 12, 10), "mono12": (3, 12, 10),
}
REFUSED = ["411", "420p9", "420p14", "420p16", "422p9", "422p16", "444p14", "444p16", "444alpha", "mono9", "mono16", "rgb"]


def _layout(host, path, any_layout):
    geo, fb, n, err = (C.c_int * 5)(), C.c_ulonglong(), C.c_longlong(), C.create_string_buffer(512)
    rc = host.av1mi_host_y4m_layout(str(path).encode(), int(any_layout), geo, C.byref(fb), C.byref(n), err, 512)
    return rc, list(geo), fb.value, n.value, err.value.decode()


def _file(path, tag, w, h, frame_bytes, frames=2):
    path.write_bytes(("YUV4MPEG2 W%d H%d F25:1 C%s\n" % (w, h, tag)).encode() + (b"FRAME\n" + bytes(frame_bytes)) * frames)


def _frame_bytes(chroma, depth, w, h):
    c = R.true_chroma_size(chroma, w, h)
    return (w * h + (2 * c[0] * c[1] if c else 0)) * (1 if depth == 8 else 2)


@pytest.mark.parametrize("tag", sorted(ACCEPTED))
def test_accepted_tags_parse_to_the_right_geometry_and_frame_size(host, tmp_path, tag):
    chroma, depth, coded = ACCEPTED[tag]
    for w, h in ((64, 48), (35, 21)):
        fb = _frame_bytes(chroma, depth, w, h)
        _file(tmp_path / "a.y4m", tag, w, h, fb)
        rc, geo, got_fb, n, err = _layout(host, tmp_path / "a.y4m", True)
        assert rc == 0, err
        assert geo == [w, h, coded, chroma, depth] and got_fb == fb and n == 2


@pytest.mark.parametrize("tag", REFUSED)
def test_refused_tags_are_refused_by_name(host, tmp_path, tag):
    _file(tmp_path / "a.y4m", tag, 64, 48, 64 * 48 * 3)
    for any_layout in (True, False):
        if tag == "420p9" and not any_layout:      # (without the opt-in the header is read as it always was: "420p9" passes as 8-bit 4:2:0)
            continue
        rc, _, _, _, err = _layout(host, tmp_path / "a.y4m", any_layout)
        assert rc == -1 and "unsupported Y4M colourspace " + tag in err


def test_without_the_opt_in_only_420_at_8_and_10_bits(host, tmp_path):
    for tag, (chroma, depth, coded) in sorted(ACCEPTED.items()):
        _file(tmp_path / "a.y4m", tag, 64, 48, _frame_bytes(chroma, depth, 64, 48))
        rc, geo, _, _, err = _layout(host, tmp_path / "a.y4m", False)
        if chroma == 0 and depth != 12:
            assert rc == 0 and geo == [64, 48, coded, 0, depth]
        else:
            assert rc == -1 and err == "Invalid argument: unsupported Y4M colourspace %s (4:2:0 8/10-bit only)" % tag


# ---- argument parsing -----------------------------------------------------------------------------------------------------------

def _to_420(host, argv):
    err = C.create_string_buffer(512)
    return host.av1mi_host_parse_format_option("\n".join(argv).encode(), err, 512), err.value.decode()


def test_the_job_decides_the_conversion(host):
    buf = C.create_string_buffer(8192)
    for webrip in (0, 1):      # the argv the reference builds: its chain always ends in format=nv12
        assert host.av1mi_host_transcode_args(b"in.y4m", b"out.mkv", 1, 0, 1080, webrip, buf, 8192) > 0
        argv = buf.value.decode().split("\n")
        assert REFERENCE_CHAIN in argv[argv.index("-vf:v:0") + 1]
        assert _to_420(host, argv) == (1, "")
    assert _to_420(host, ["-i", "a.y4m", "out.obu"]) == (0, "")
    assert _to_420(host, ["-i", "a.y4m", "-vf:v:0", "scale=64:48", "out.obu"]) == (0, "")
    for name in ("nv12", "p010", "p010le", "yuv420p", "yuv420p10le"):
        assert _to_420(host, ["-i", "a.y4m", "-vf:v:0", "scale=64:48,format=" + name, "out.obu"]) == (1, "")
    for name in ("yuv444p", "yuv422p10le", "gray", "rgb24", ""):
        rc, err = _to_420(host, ["-i", "a.y4m", "-vf:v:0", "format=" + name, "out.obu"])
        assert rc == -1 and err == "Invalid argument: unsupported filter format=" + name
    assert _to_420(host, ["-i", "a.y4m", "-av1mi_format", "420", "out.obu"]) == (1, "")
    for bad in ("444", "422", "nv12", ""):
        rc, err = _to_420(host, ["-i", "a.y4m", "-av1mi_format", bad, "out.obu"])
        assert rc == -1 and "-av1mi_format takes 420" in err


# ---- buffer sizes ------------------------------------------------------------------------------------------------------------------

def test_source_plane_bytes_of_every_layout(av1mi):
    for chroma in R.LAYOUTS:
        for depth in (8, 10, 12):
            for w, rows in ((8, 8), (72, 40 * 3), (1368, 768)):
                shapes = R.buffer_shapes(chroma, w, rows)
                assert shapes == av1mi.source_plane_shapes(chroma, w, rows)
                for p in range(3):
                    want = 0 if shapes[p] is None else shapes[p][0] * shapes[p][1] * (1 if depth == 8 else 2)
                    assert av1mi.source_plane_bytes(chroma, depth, p, w, rows) == want
    assert av1mi.source_plane_bytes(R.C400, 8, 1, 64, 64) == 0 and av1mi.source_plane_bytes(R.C400, 8, 2, 64, 64) == 0
    for bad in ((4, 8, 0, 64, 64), (-1, 8, 0, 64, 64), (0, 9, 0, 64, 64), (0, 16, 0, 64, 64), (0, 8, 3, 64, 64), (0, 8, 0, 60, 64), (0, 8, 0, 64, 60), (0, 8, 0, 0, 64)):
        assert av1mi.source_plane_bytes(*bad) == 0
    # 4:2:0 at the coded depth is the planar input format
    for bd in (8, 10):
        for p in range(3):
            assert av1mi.source_plane_bytes(R.C420, bd, p, 136, 72 * 2) == av1mi.input_plane_bytes(av1mi.INPUT_PLANAR, bd, p, 136, 72 * 2)
