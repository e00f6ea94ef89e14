"""The session's input formats (include/av1mi.h enum av1mi_input_format) without a GPU: the sizes and the host-side packing of
libav1mi.so against the numpy restatement of the header's definitions (input_formats_ref.py), and the product's -av1mi_pack10
option as far as argument parsing goes.  Every comparison is equality."""
import ctypes as C
import os

import numpy as np
import pytest

import input_formats_ref as R

FORMATS = (R.PLANAR, R.PACKED10, R.P010, R.NV12)
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "av1-go_amd", "host", "libav1mi_host.so")


def _bd(fmt):
    return 8 if fmt == R.NV12 else 10


@pytest.mark.parametrize("width,rows", [(8, 8), (136, 72), (3840, 2160 * 12)])
def test_plane_bytes_for_every_combination(av1mi, width, rows):
    for fmt in (-1,) + FORMATS + (4,):
        for bd in (8, 10, 12):
            for plane in (-1, 0, 1, 2, 3):
                assert av1mi.input_plane_bytes(fmt, bd, plane, width, rows) == R.plane_bytes(fmt, bd, plane, width, rows), (fmt, bd, plane)
    # spelled out once, so that the restatement itself is pinned: a 10-bit sample costs 10 bits, a semi-planar chroma plane holds both
    ny, nc = width * rows, width * rows // 4
    assert [av1mi.input_plane_bytes(R.PACKED10, 10, p, width, rows) for p in range(3)] == [ny * 5 // 4, nc * 5 // 4, nc * 5 // 4]
    assert [av1mi.input_plane_bytes(R.P010, 10, p, width, rows) for p in range(3)] == [ny * 2, nc * 4, 0]
    assert [av1mi.input_plane_bytes(R.NV12, 8, p, width, rows) for p in range(3)] == [ny, nc * 2, 0]
    assert [av1mi.input_plane_bytes(R.PLANAR, 8, p, width, rows) for p in range(3)] == [ny, nc, nc]
    for fmt, bd in ((R.PACKED10, 8), (R.P010, 8), (R.NV12, 10)):
        assert [av1mi.input_plane_bytes(fmt, bd, p, width, rows) for p in range(3)] == [0, 0, 0]
    assert av1mi.input_plane_bytes(R.PACKED10, 10, 0, width + 4, rows) == 0 and av1mi.input_plane_bytes(R.PACKED10, 10, 0, width, 0) == 0


def test_the_two_statements_of_the_packed_layout_agree():
    """bit string (sample i in bits [10 i, 10 i + 10)) == the header's five-byte formula, on every content kind"""
    for kind in ("random", "zeros", "max", "ramp"):
        y = R.content(kind, 10, 136, 72, 5)[0]
        assert (R.pack10_bits(y) == R.pack10_bytes(y)).all()
    assert R.pack10_bits(np.array([1023, 0, 0, 0])).tolist() == [0xFF, 0x03, 0, 0, 0]
    assert R.pack10_bits(np.array([0, 1, 0, 0x200])).tolist() == [0, 0x04, 0, 0, 0x80]


@pytest.mark.parametrize("width,rows", [(8, 8), (136, 72 * 3), (1920, 1080)])
@pytest.mark.parametrize("kind", ["random", "zeros", "max", "ramp"])
@pytest.mark.parametrize("fmt", [R.PACKED10, R.P010, R.NV12])
def test_pack_matches_the_definition(av1mi, fmt, kind, width, rows):
    bd = _bd(fmt)
    y, u, v = R.content(kind, bd, width, rows, 11)
    got = av1mi.input_pack(fmt, bd, y, u, v)
    want = R.pack(fmt, bd, y, u, v, pack10=R.pack10_bits)      # PACKED10: the bit string itself, built with numpy integer arithmetic
    for p, w in enumerate(want):
        assert got[p].nbytes == w.nbytes == av1mi.input_plane_bytes(fmt, bd, p, width, rows)
        assert (got[p] == w).all(), "format %d plane %d differs from the definition" % (fmt, p)
    if len(want) == 2:
        assert got[2].nbytes == 0


def test_pack_planar_is_a_copy_and_bad_combinations_are_refused(av1mi):
    for bd in (8, 10):
        y, u, v = R.content("random", bd, 24, 16, 2)
        got = av1mi.input_pack(R.PLANAR, bd, y, u, v)
        assert all((g == a.ravel().view(np.uint8)).all() for g, a in zip(got, (y, u, v)))
    y, u, v = R.content("random", 8, 24, 16, 2)
    lib = av1mi.load()
    lib.av1mi_input_pack.argtypes = [C.c_int] * 4 + [C.c_void_p] * 6
    out = np.zeros(4096, np.uint8)
    p = lambda a: a.ctypes.data
    for fmt, bd in ((R.PACKED10, 8), (R.P010, 8), (R.NV12, 10), (7, 8)):
        assert lib.av1mi_input_pack(fmt, bd, 24, 16, p(y), p(u), p(v), p(out), p(out), p(out)) == -1
    assert lib.av1mi_input_pack(R.NV12, 8, 24, 16, None, p(u), p(v), p(out), p(out), None) == -1
    assert lib.av1mi_input_pack(R.NV12, 8, 24, 16, p(y), p(u), p(v), p(out), p(out), None) == 0      # no third plane to write


@pytest.mark.parametrize("width,height,segments", [(8, 8, 5), (136, 72, 3)])
def test_packing_segment_by_segment_equals_packing_the_stack(av1mi, width, height, segments):
    """what the product's reader threads rely on: every segment starts on a 4-byte boundary of the packed planes and packs on its own"""
    y, u, v = R.content("random", 10, width, height * segments, 21)
    whole = av1mi.input_pack(R.PACKED10, 10, y, u, v)
    n = [av1mi.input_plane_bytes(R.PACKED10, 10, p, width, height) for p in range(3)]
    assert all(k % 4 == 0 for k in n)
    bufs = [np.full(k * segments, 0xA5, np.uint8) for k in n]
    for s in reversed(range(segments)):      # any order
        av1mi.input_pack(R.PACKED10, 10, y[s * height:(s + 1) * height], u[s * height // 2:(s + 1) * height // 2], v[s * height // 2:(s + 1) * height // 2],
                         out=[(b, k * s) for b, k in zip(bufs, n)])
    for b, w in zip(bufs, whole):
        assert (b == w).all()
    # zero samples pack to zero bytes (absent segments of a batch are cleared with memset)
    z = av1mi.input_pack(R.PACKED10, 10, *R.content("zeros", 10, width, height))
    assert not any(p.any() for p in z)


def test_pack10_option_is_parsed_without_a_gpu(av1mi, tmp_path):
    """-av1mi_pack10 takes 0 or 1: anything else is ParseBackendJob's `Invalid argument` (exit code 1); 1 passes parsing, which
    without a GPU shows as the later `no usable HIP device` result (code -1)"""
    if not os.path.exists(HOST):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(HOST)])
    host = C.CDLL(HOST)
    host.av1mi_run_transcode.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t]
    err = C.create_string_buffer(1024)

    def run(value):
        argv = ["-i", str(tmp_path / "missing.y4m"), "-av1mi_pack10", value, str(tmp_path / "out.obu")]
        arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
        return host.av1mi_run_transcode(len(argv), arr, err, 1024), err.value

    for bad in ("2", "-1"):
        code, text = run(bad)
        assert code == 1 and text.startswith(b"av1mi failed with exit code 1: Invalid argument"), (bad, code, text)
    for good in ("0", "1"):
        code, text = run(good)
        assert b"Invalid argument" not in text and code != 0
        if av1mi.load().av1mi_device_count() == 0:
            assert code == -1 and b"no usable HIP device" in text
        else:      # with a GPU the run gets as far as the input file
            assert code == 1 and b"No such file" in text
