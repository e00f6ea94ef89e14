"""-av1mi_tonemap_peak auto as an argument: what ParseBackendJob makes of it, that it needs the tone map, a seekable file and a source whose
frames are 4:2:0 at 10 bits, and that a number keeps working.  No GPU."""
import ctypes as C

import pytest

TM = ["-av1mi_tonemap", "bt2390"]


def _parse(extra, source="missing.y4m"):
    import av1stream
    return av1stream.parse_peak_options(["-i", source] + extra + ["out.mkv"])


def test_auto_parses():
    assert _parse(TM + ["-av1mi_tonemap_peak", "auto"]) == dict(tonemap=1, peak=0, auto=1)
    assert _parse(["-vf:v:0", "tonemap_vaapi", "-av1mi_tonemap_peak", "auto"]) == dict(tonemap=1, peak=0, auto=1)
    assert _parse(TM) == dict(tonemap=1, peak=0, auto=0) and _parse([]) == dict(tonemap=0, peak=0, auto=0)
    # the last one given has the say, as with every option
    assert _parse(TM + ["-av1mi_tonemap_peak", "auto", "-av1mi_tonemap_peak", "600"]) == dict(tonemap=1, peak=600, auto=0)
    assert _parse(TM + ["-av1mi_tonemap_peak", "600", "-av1mi_tonemap_peak", "auto"]) == dict(tonemap=1, peak=0, auto=1)


def test_a_number_keeps_working():
    for n in (100, 1000, 4000, 10000):
        assert _parse(TM + ["-av1mi_tonemap_peak", n]) == dict(tonemap=1, peak=n, auto=0)
    for bad in ("99", "10001", "Auto", "auto ", "automatic", "-1"):
        with pytest.raises(ValueError) as e:
            _parse(TM + ["-av1mi_tonemap_peak", bad])
        assert "-av1mi_tonemap_peak takes cd/m2, 100 .. 10000, or auto, not " + bad in str(e.value)
    with pytest.raises(ValueError) as e:
        _parse(["-av1mi_tonemap_peak", "1000"])
    assert "-av1mi_tonemap_peak needs -av1mi_tonemap bt2390" in str(e.value)


def test_auto_needs_the_tone_map(tmp_path):
    import av1stream
    for extra in ([], ["-av1mi_tonemap", "off"]):
        code, text = av1stream.run_transcode(["-i", tmp_path / "missing.y4m", "-av1mi_tonemap_peak", "auto"] + extra + [tmp_path / "out.mkv"])
        assert code == 1 and "Invalid argument: -av1mi_tonemap_peak needs -av1mi_tonemap bt2390 (or tonemap_vaapi in the chain)" in text, text


def test_auto_needs_a_seekable_file(tmp_path):
    import os
    import av1stream
    fifo = tmp_path / "in.fifo"
    os.mkfifo(fifo)
    for source in ("-", "pipe:0", fifo):
        code, text = av1stream.run_transcode(["-i", source] + TM + ["-av1mi_tonemap_peak", "auto", tmp_path / "out.mkv"])
        assert code == 1 and "Invalid argument: -av1mi_tonemap_peak auto needs a seekable file" in text and "not from a pipe or FIFO" in text, (source, text)
        assert av1stream.parse_peak_options(["-i", source] + TM + ["-av1mi_tonemap_peak", "4000", "out.mkv"])["peak"] == 4000      # a number reads the stream in order
    # the wording is -av1mi_crop auto's
    code, crop = av1stream.run_transcode(["-i", "-", "-av1mi_crop", "auto", tmp_path / "out.mkv"])
    assert text.split("auto needs", 1)[1] == crop.split("auto needs", 1)[1]


def _y4m(path, colourspace, samples, bytes_per, w=64, h=48, frames=2):
    path.write_bytes(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s\n" % (w, h, colourspace)).encode() + (b"FRAME\n" + bytes(w * h * samples // 2 * bytes_per)) * frames)
    return str(path)


def _plan(av1mi, argv):
    """SessionConfig for an argv (av1mi_host_session_config: the Y4M header is read, no device is opened): the session's config, or the text"""
    import av1stream
    host = av1stream.lib()
    host.av1mi_host_session_config.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(av1mi.GopConfig), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    cfg, target, switches, err = av1mi.GopConfig(), (C.c_int * 3)(), (C.c_int * 5)(), C.create_string_buffer(1024)
    code = host.av1mi_host_session_config("\n".join(["av1mi"] + [str(a) for a in argv]).encode(), None, C.byref(cfg), target, switches, err, 1024)
    return cfg if code == 0 else err.value.decode()


@pytest.mark.parametrize("colourspace,samples,bytes_per", [("422p10", 4, 2), ("444p10", 6, 2), ("mono10", 2, 2), ("420p12", 3, 2), ("420jpeg", 3, 1)])
def test_auto_is_refused_for_frames_that_are_not_420_at_10_bits(av1mi, tmp_path, colourspace, samples, bytes_per):
    """the refusal needs the file's header: the session's config refuses, before a frame is read; a number passes the same header (where
    the tone map takes the source at all)"""
    src = _y4m(tmp_path / "s.y4m", colourspace, samples, bytes_per)
    text = _plan(av1mi, ["-i", src, "-av1mi_format", "420"] + TM + ["-av1mi_tonemap_peak", "auto", src + ".obu"])
    assert isinstance(text, str) and "-av1mi_tonemap_peak auto measures 4:2:0 10-bit frames as the file holds them" in text, text
    number = _plan(av1mi, ["-i", src, "-av1mi_format", "420"] + TM + ["-av1mi_tonemap_peak", "4000", src + ".obu"])
    if colourspace == "420jpeg":
        assert isinstance(number, str) and "tone mapping needs a 10-bit source" in number
    else:
        assert not isinstance(number, str) and (number.tone_map, number.tone_map_peak) == (1, 4000)


def test_auto_passes_a_420_10_bit_header(av1mi, tmp_path):
    """until the plan is made the config is the one of the job without a peak"""
    src = _y4m(tmp_path / "s.y4m", "420p10", 3, 2)
    cfg = _plan(av1mi, ["-i", src] + TM + ["-av1mi_tonemap_peak", "auto", src + ".obu"])
    assert not isinstance(cfg, str) and (cfg.tone_map, cfg.tone_map_peak) == (1, 0)
