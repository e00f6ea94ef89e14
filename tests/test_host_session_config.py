"""What a transcode job opens its GOP session with (host/backend.cpp SessionConfig: a pure function of the job, the Y4M header's facts and
the settled crop window), field by field, without a GPU.  The expected values are read off RunBackend as it was before the policy became a
function of its own."""
import ctypes as C
import os
import subprocess

import pytest

import av1mi

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "av1-go_amd", "host", "libav1mi_host.so")
FIELDS = [name for name, _ in av1mi.GopConfig._fields_]
SWITCHES = ("packed", "stored", "analysed", "grainy", "measure")
PACKED10, CHROMA_422 = 1, 1      # include/av1mi.h enum av1mi_input_format / av1mi_source_chroma


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(HOST)])
    lib = C.CDLL(HOST)
    lib.av1mi_host_session_config.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(av1mi.GopConfig), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return lib


def _y4m(path, w, h, frames, tag="420jpeg", header="Ip A1:1", bytes_per_frame=None):
    """a header plus `frames` grey frames; bytes_per_frame for layouts other than 8-bit 4:2:0"""
    n = w * h * 3 // 2 if bytes_per_frame is None else bytes_per_frame
    path.write_bytes(("YUV4MPEG2 W%d H%d F30:1 %s C%s\n" % (w, h, header, tag)).encode() + (b"FRAME\n" + bytes(n)) * frames)
    return str(path)


def _config(host, src, *options, auto_win=None):
    """(exit code, {field: value}, target (width, height, square), {switch: bool}, error text) for `av1mi -i src <options> out.mkv`"""
    argv = ["av1mi", "-i", src] + list(options) + [src + ".mkv"]
    cfg, target, switches, err = av1mi.GopConfig(), (C.c_int * 3)(), (C.c_int * 5)(), C.create_string_buffer(1024)
    for name in FIELDS:
        setattr(cfg, name, -77)      # (whatever the hook leaves alone shows)
    win = (C.c_int * 4)(*auto_win) if auto_win else None
    code = host.av1mi_host_session_config("\n".join(argv).encode(), win, C.byref(cfg), target, switches, err, 1024)
    return code, {name: getattr(cfg, name) for name in FIELDS}, tuple(target), dict(zip(SWITCHES, map(bool, switches))), err.value.decode()


def _expect(got, **fields):
    """every field of the config: the ones named, 0 for the rest"""
    want = dict.fromkeys(FIELDS, 0)
    want.update(fields)
    assert got == want, {k: (got[k], want[k]) for k in FIELDS if got[k] != want[k]}


# the fields every job below shares: defaults of BackendJob and of RunBackend
BASE = dict(bit_depth=8, base_q_idx=25, gop_length=30, segments=1, search_range=8, gpu_entropy=1, key_block_size=32)


def test_defaults_on_a_plain_source(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 10)
    code, cfg, target, sw, err = _config(host, src, "-global_quality:v:0", "31")
    assert code == 0 and err == ""
    # (4 segments asked by default, clamped to the file's one GOP of 30)
    _expect(cfg, **dict(BASE, width=64, height=48, base_q_idx=31))
    assert target == (64, 48, 1) and sw == dict.fromkeys(SWITCHES, False)


def test_a_size_that_is_no_multiple_of_8(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 70, 50, 3)
    code, cfg, target, _, _ = _config(host, src)
    assert code == 0
    _expect(cfg, **dict(BASE, width=72, height=56, visible_width=70, visible_height=50, key_block_size=8))      # 72 is no multiple of 32
    assert target == (70, 50, 1)


def test_an_explicit_scale(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 3, header="Ip A4:3")
    code, cfg, target, _, _ = _config(host, src, "-av1mi_scale", "32x24")
    assert code == 0
    _expect(cfg, **dict(BASE, width=32, height=24, source_width=64, source_height=48))
    assert target == (32, 24, 1)      # an explicit size means square pixels, whatever the header's A says


def test_an_explicit_window(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 3)
    code, cfg, target, _, _ = _config(host, src, "-av1mi_crop", "32:32:16:8")
    assert code == 0
    _expect(cfg, **dict(BASE, width=32, height=32, source_width=64, source_height=48, crop_x=16, crop_y=8, crop_width=32, crop_height=32))
    assert target == (32, 32, 1)
    code, _, _, _, err = _config(host, src, "-av1mi_crop", "32:32:40:8")
    assert code == 1 and err == "Invalid argument: -av1mi_crop 32:32:40:8 lies outside the 64x48 picture"


def test_a_window_found_by_auto(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 3)
    code, cfg, target, _, _ = _config(host, src, "-av1mi_crop", "auto", auto_win=(0, 8, 64, 32))
    assert code == 0
    _expect(cfg, **dict(BASE, width=64, height=32, source_width=64, source_height=48, crop_x=0, crop_y=8, crop_width=64, crop_height=32))
    assert target == (64, 32, 1)
    code, cfg, _, _, _ = _config(host, src, "-av1mi_crop", "auto")      # no bars found: the job without a window
    assert code == 0
    _expect(cfg, **dict(BASE, width=64, height=48))


def test_a_chain_that_does_not_fit_the_source(host, tmp_path):
    """a chain's geometry is first checked against the source here (ParseBackendJob checks its syntax alone): exit code 1 and the text"""
    src = _y4m(tmp_path / "a.y4m", 64, 48, 3)
    code, _, _, _, err = _config(host, src, "-vf:v:0", "crop=200:200:0:0")
    assert code == 1 and err == "Invalid argument: unsupported filter argument crop=200:200:0:0 (the window lies outside the 64x48 picture)"
    code, _, _, _, err = _config(host, src, "-vf", "crop=32:32:40:8,scale=32:32")
    assert code == 1 and err == "Invalid argument: unsupported filter argument crop=32:32:40:8 (the window lies outside the 64x48 picture)"


def test_pack10_on_a_10_bit_source(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 3, tag="420p10", bytes_per_frame=64 * 48 * 3)
    code, cfg, _, sw, _ = _config(host, src, "-av1mi_pack10", "1")
    assert code == 0
    _expect(cfg, **dict(BASE, width=64, height=48, bit_depth=10, input_format=PACKED10))
    assert sw["packed"]


def test_pack10_is_ignored_for_a_source_that_is_converted(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 3, tag="422p10", bytes_per_frame=64 * 48 * 4)
    code, cfg, _, sw, _ = _config(host, src, "-av1mi_format", "420", "-av1mi_pack10", "1")
    assert code == 0
    _expect(cfg, **dict(BASE, width=64, height=48, bit_depth=10, input_format=0, source_chroma=CHROMA_422, source_bit_depth=10))
    assert not sw["packed"]


def test_deinterlace_auto_follows_the_header(host, tmp_path):
    G, S = 4, 2
    options = ("-av1mi_deinterlace", "auto", "-g", str(G), "-av1mi_segments", str(S))
    src = _y4m(tmp_path / "t.y4m", 64, 48, S * G, header="It A1:1")
    code, cfg, _, sw, _ = _config(host, src, *options)
    assert code == 0
    _expect(cfg, **dict(BASE, width=64, height=48, gop_length=G, segments=S, deinterlace=1, store_frames=S * G))
    assert sw["stored"] and not sw["analysed"]
    src = _y4m(tmp_path / "m.y4m", 64, 48, S * G, header="Im A1:1")
    code, _, _, _, err = _config(host, src, *options)
    assert code == 1
    assert err == "Invalid argument: -av1mi_deinterlace auto: the source is mixed-mode interlaced (Im); field-rate output and inverse telecine are not built"


def test_denoise_without_film_grain(host, tmp_path):
    G, S = 4, 2
    src = _y4m(tmp_path / "a.y4m", 64, 48, S * G)
    options = ("-av1mi_denoise", "4", "-g", str(G), "-av1mi_segments", str(S))
    code, cfg, _, sw, _ = _config(host, src, *options, "-av1mi_film_grain", "0")
    assert code == 0
    _expect(cfg, **dict(BASE, width=64, height=48, gop_length=G, segments=S, denoise=4, store_frames=S * G))
    assert sw["stored"] and not sw["grainy"]
    code, cfg2, _, sw, _ = _config(host, src, *options)      # film grain is on unless told otherwise: the same session, parameters in the headers
    assert code == 0 and cfg2 == cfg and sw["grainy"]


def test_tone_mapping_refuses_what_cannot_be_hdr10(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 3)
    code, _, _, _, err = _config(host, src, "-av1mi_tonemap", "bt2390")
    assert code == 1 and err == "Invalid argument: tone mapping needs a 10-bit source (an 8-bit HDR10 source does not exist)"
    src = _y4m(tmp_path / "b.y4m", 64, 48, 3, tag="420p10 XCOLORRANGE=FULL", bytes_per_frame=64 * 48 * 3)
    code, _, _, _, err = _config(host, src, "-av1mi_tonemap", "bt2390")
    assert code == 1 and err == "Invalid argument: tone mapping takes a limited-range source; the Y4M header says XCOLORRANGE=FULL"


def test_a_stats_file_makes_the_session_measure(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 3)
    code, cfg, _, sw, _ = _config(host, src, "-av1mi_stats", str(tmp_path / "stats.txt"))
    assert code == 0
    _expect(cfg, **dict(BASE, width=64, height=48, quality_stats=1))
    assert sw["measure"]
