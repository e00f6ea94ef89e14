"""-av1mi_denoise auto as an argument: what ParseBackendJob makes of it, that every refusal of -av1mi_denoise N holds for auto before anything
runs (whatever strength would be planned), what it is accepted with, and that it needs a seekable file.  No GPU."""
import ctypes as C

import pytest

CHAIN = "scale_vaapi=w=ceil(iw/2)*2:h=ceil(ih/2)*2,hwdownload,format=nv12,setsar=1,format=nv12,hwupload"


def _parse(extra, source="missing.y4m"):
    import av1stream
    return av1stream.parse_denoise_options(["-i", source] + extra + ["out.mkv"])


def test_auto_parses():
    assert _parse(["-av1mi_denoise", "auto"]) == dict(denoise=0, auto=1, range=0, film_grain=-1, grain_lag=0)
    assert _parse(["-av1mi_denoise", "4"]) == dict(denoise=4, auto=0, range=0, film_grain=-1, grain_lag=0)
    assert _parse([])["auto"] == 0
    # the last one given has the say, as with every option
    assert _parse(["-av1mi_denoise", "auto", "-av1mi_denoise", "3"]) == dict(denoise=3, auto=0, range=0, film_grain=-1, grain_lag=0)
    assert _parse(["-av1mi_denoise", "3", "-av1mi_denoise", "auto"])["denoise"] == 0
    for bad in ("Auto", "auto ", "automatic", "-1", "17"):
        with pytest.raises(ValueError) as e:
            _parse(["-av1mi_denoise", bad])
        assert "-av1mi_denoise takes a strength 1 .. 16 (0 = off) or auto, not " + bad in str(e.value)


@pytest.mark.parametrize("extra,why", [(["-av1mi_pack10", "1"], "-av1mi_denoise keeps the group's frames in a planar store on the GPU: not together with -av1mi_pack10 1"),
                                       (["-av1mi_deinterlace", "auto"], "not together with -av1mi_deinterlace"),
                                       (["-vf:v:0", "yadif"], "not together with -av1mi_deinterlace"),
                                       (["-av1mi_ivtc", "1", "-g", "4"], "-av1mi_ivtc together with -av1mi_denoise is not built"),
                                       (["-av1mi_tonemap", "bt2390"], "tone mapping together with -av1mi_denoise is not built"),
                                       (["-vf:v:0", "tonemap_vaapi"], "tone mapping together with -av1mi_denoise is not built")])
def test_refusals_of_a_strength_hold_for_auto(tmp_path, extra, why):
    """through av1mi_run_transcode itself: the input does not even exist, and the refusal is the arguments'"""
    import av1stream
    for value in ("auto", "4"):
        code, text = av1stream.run_transcode(["-i", tmp_path / "missing.y4m", "-av1mi_denoise", value] + extra + [tmp_path / "out.mkv"])
        assert code == 1 and "Invalid argument: " in text and why in text, (value, extra, text)


def _y4m(path, bd, w=64, h=48, frames=2):
    n = w * h * 3 // 2 * (1 if bd == 8 else 2)
    path.write_bytes(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s\n" % (w, h, "420jpeg" if bd == 8 else "420p%d" % bd)).encode() + (b"FRAME\n" + bytes(n)) * frames)
    return str(path)


def _plan(av1mi, argv):
    """SessionConfig for an argv (av1mi_host_session_config: the Y4M header is read, no device is opened): the session's config, or the text"""
    import av1stream
    host = av1stream.lib()
    host.av1mi_host_session_config.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(av1mi.GopConfig), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    cfg, target, switches, err = av1mi.GopConfig(), (C.c_int * 3)(), (C.c_int * 5)(), C.create_string_buffer(1024)
    code = host.av1mi_host_session_config("\n".join(["av1mi"] + [str(a) for a in argv]).encode(), None, C.byref(cfg), target, switches, err, 1024)
    return (cfg, list(switches)) if code == 0 else err.value.decode()


def test_depth_reduction_is_refused_with_auto(av1mi, tmp_path):
    """the fifth refusal needs the source's depth: the session's config refuses it, with a strength and with auto alike"""
    s8, s10 = _y4m(tmp_path / "a8.y4m", 8), _y4m(tmp_path / "a10.y4m", 10)
    for value in ("auto", "4"):
        for extra in (["-av1mi_depth", "8"], ["-av1mi_depth", "chain", "-vf:v:0", CHAIN]):
            text = _plan(av1mi, ["-i", s10, "-av1mi_denoise", value] + extra + [s10 + ".obu"])
            assert isinstance(text, str) and "a depth reduction together with -av1mi_denoise is not built" in text, (value, extra, text)
        assert not isinstance(_plan(av1mi, ["-i", s8, "-av1mi_denoise", value, "-av1mi_depth", "8", s8 + ".obu"]), str)      # nothing is reduced


def test_before_the_plan_auto_opens_no_denoiser(av1mi, tmp_path):
    """until a strength is planned the config is the one of the job without the option: no store, no denoiser"""
    s8 = _y4m(tmp_path / "a8.y4m", 8)
    cfg, switches = _plan(av1mi, ["-i", s8, "-av1mi_denoise", "auto", "-av1mi_denoise_range", "4", s8 + ".obu"])
    base, base_switches = _plan(av1mi, ["-i", s8, s8 + ".obu"])
    assert (cfg.denoise, cfg.store_frames) == (0, 0) and switches == base_switches
    four, _ = _plan(av1mi, ["-i", s8, "-av1mi_denoise", "4", "-av1mi_denoise_range", "4", s8 + ".obu"])
    assert (four.denoise, four.denoise_range) == (4, 4) and four.store_frames > 0


@pytest.mark.parametrize("extra", [["-av1mi_denoise_range", "4"], ["-av1mi_denoise_range", "8", "-av1mi_film_grain", "0"], ["-av1mi_film_grain", "1", "-av1mi_grain_lag", "2"],
                                   ["-av1mi_scenecut", "15"], ["-av1mi_crop", "auto"], ["-av1mi_stats", "s.txt"]])
def test_accepted_with_auto(av1mi, tmp_path, extra):
    import av1stream
    code, text = av1stream.run_transcode(["-i", tmp_path / "missing.y4m", "-av1mi_denoise", "auto"] + extra + [tmp_path / "out.mkv"])
    assert "Invalid argument" not in text and code != 0, (extra, text)
    if av1mi.load().av1mi_device_count() == 0:
        assert code == -1 and "no usable HIP device" in text


def test_what_shapes_the_denoiser_still_needs_one():
    for extra, why in ((["-av1mi_denoise_range", "4"], "-av1mi_denoise_range needs -av1mi_denoise"), (["-av1mi_film_grain", "1"], "-av1mi_film_grain needs -av1mi_denoise"),
                       (["-av1mi_denoise", "auto", "-av1mi_grain_lag", "2", "-av1mi_film_grain", "0"], "not together with -av1mi_film_grain 0"),
                       (["-av1mi_denoise", "auto", "-av1mi_denoise_range", "3"], "-av1mi_denoise_range takes 0 (off), 4 or 8")):
        with pytest.raises(ValueError) as e:
            _parse(extra)
        assert why in str(e.value)


def test_auto_needs_a_seekable_file(tmp_path):
    import os
    import av1stream
    fifo = tmp_path / "in.fifo"
    os.mkfifo(fifo)
    for source in ("-", "pipe:0", fifo):
        code, text = av1stream.run_transcode(["-i", source, "-av1mi_denoise", "auto", tmp_path / "out.mkv"])
        assert code == 1 and "Invalid argument: -av1mi_denoise auto needs a seekable file" in text and "not from a pipe or FIFO" in text, (source, text)
        assert av1stream.parse_denoise_options(["-i", source, "-av1mi_denoise", "4", "out.mkv"])["denoise"] == 4      # a strength reads the stream in order


def test_the_daemon_config_carries_it():
    import av1stream
    host = av1stream.lib()
    host.av1mi_host_job_args_denoise.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    host.av1mi_host_job_args.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_char_p, C.c_int]
    buf, base = C.create_string_buffer(8192), C.create_string_buffer(8192)
    assert host.av1mi_host_job_args(b"in.mkv", b"out.mkv", 720, 0, 0.0, base, 8192) > 0
    n = host.av1mi_host_job_args_denoise(b"in.mkv", b"out.mkv", 720, b"", buf, 8192)
    assert n > 0 and buf.value == base.value      # a default config adds nothing
    assert host.av1mi_host_job_args_denoise(b"in.mkv", b"out.mkv", 720, b"auto", buf, 8192) == n + 2
    argv = buf.value.decode().split("\n")
    assert argv[-3:] == ["-av1mi_denoise", "auto", "out.mkv"] and argv[:-3] == base.value.decode().split("\n")[:-1]
    assert av1stream.parse_denoise_options(argv)["auto"] == 1
