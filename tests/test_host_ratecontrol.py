"""The rate options of the product path (host/transcode.cpp ParseBackendJob, host/daemon.cpp AppendConfigArgs): what is accepted, what
is refused and with which text, and that the reference's argv is unchanged unless a target is asked for.  No GPU."""
import ctypes as C

import pytest

import av1stream


@pytest.fixture(scope="module")
def host():
    lib = av1stream.lib()
    lib.av1mi_host_parse_rate_options.argtypes = [C.c_char_p, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    lib.av1mi_host_job_args.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_char_p, C.c_int]
    lib.av1mi_host_transcode_args.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int] * 4 + [C.c_char_p, C.c_int]
    return lib


def parse(host, *opts):
    out, err = (C.c_longlong * 5)(), C.create_string_buffer(512)
    rc = host.av1mi_host_parse_rate_options("\n".join(["-i", "in.y4m"] + list(opts) + ["out.mkv"]).encode(), out, err, 512)
    return rc, list(out), err.value.decode()


def test_targets_are_parsed(host):
    assert parse(host) == (0, [0, 0, 0, 0, 25], "")
    assert parse(host, "-b:v:0", "4M")[:2] == (0, [4000000, 0, 0, 0, 25])
    assert parse(host, "-b:v", "800k")[:2] == (0, [800000, 0, 0, 0, 25])
    assert parse(host, "-b:v:0", "123456", "-global_quality:v:0", "60")[:2] == (0, [123456, 0, 0, 0, 60])
    assert parse(host, "-av1mi_target_bpp", "0.15")[:2] == (0, [0, 150000, 0, 0, 25])
    assert parse(host, "-av1mi_target_bpp", "0.12", "-qmin", "40", "-qmax", "200")[:2] == (0, [0, 120000, 40, 200, 25])
    assert parse(host, "-b:v:0", "2M", "-qmax", "70")[:2] == (0, [2000000, 0, 0, 70, 25])


@pytest.mark.parametrize("opts,text", [
    (("-b:v:0", "4M", "-av1mi_target_bpp", "0.15"), "Invalid argument: -b:v:0 and -av1mi_target_bpp are two forms of one target: give one"),
    (("-qmin", "10"), "Invalid argument: -qmin / -qmax need a target (-b:v:0 or -av1mi_target_bpp)"),
    (("-qmax", "100"), "Invalid argument: -qmin / -qmax need a target (-b:v:0 or -av1mi_target_bpp)"),
    (("-b:v:0", "1M", "-qmin", "90", "-qmax", "80"), "Invalid argument: -qmin 90 above -qmax 80"),
    (("-b:v:0", "0"), "Invalid argument: -b:v:0 takes bits per second (a positive integer, suffix k or M), not 0"),
    (("-b:v:0", "4G"), "Invalid argument: -b:v:0 takes bits per second (a positive integer, suffix k or M), not 4G"),
    (("-b:v", "-5"), "Invalid argument: -b:v takes bits per second (a positive integer, suffix k or M), not -5"),
    (("-b:v:0", "1.5M"), "Invalid argument: -b:v:0 takes bits per second (a positive integer, suffix k or M), not 1.5M"),
    (("-b:v:0", "M"), "Invalid argument: -b:v:0 takes bits per second (a positive integer, suffix k or M), not M"),
    (("-av1mi_target_bpp", "0"), "Invalid argument: -av1mi_target_bpp takes bits per pixel per frame (0.000001 .. 64), not 0"),
    (("-av1mi_target_bpp", "nan"), "Invalid argument: -av1mi_target_bpp takes bits per pixel per frame (0.000001 .. 64), not nan"),
    (("-av1mi_target_bpp", "0.1x"), "Invalid argument: -av1mi_target_bpp takes bits per pixel per frame (0.000001 .. 64), not 0.1x"),
    (("-av1mi_target_bpp", "100"), "Invalid argument: -av1mi_target_bpp takes bits per pixel per frame (0.000001 .. 64), not 100"),
    (("-b:v:0", "1M", "-qmin", "0"), "Invalid argument: -qmin takes a quantiser index 1 .. 255, not 0"),
    (("-b:v:0", "1M", "-qmax", "256"), "Invalid argument: -qmax takes a quantiser index 1 .. 255, not 256"),
])
def test_bad_rate_options_are_refused(host, opts, text):
    rc, _, err = parse(host, *opts)
    assert rc == -1 and err == text
    buf = C.create_string_buffer(1024)      # ... and through RunTranscode, before anything runs
    code = host.av1mi_host_run_transcode("\n".join(["-i", "in.y4m"] + list(opts) + ["out.mkv"]).encode(), buf, 1024)
    assert code == 1 and buf.value.decode() == "av1mi failed with exit code 1: " + text


@pytest.mark.parametrize("webrip", [0, 1])
def test_the_job_argv_gains_the_target_only_when_asked(host, webrip):
    pinned, got = C.create_string_buffer(8192), C.create_string_buffer(8192)
    n = host.av1mi_host_transcode_args(b"in.mkv", b"out.mkv", 1, 0, 1080, webrip, pinned, 8192)
    assert n > 0 and host.av1mi_host_job_args(b"in.mkv", b"out.mkv", 1080, webrip, 0.0, got, 8192) == n and got.value == pinned.value
    assert host.av1mi_host_job_args(b"in.mkv", b"out.mkv", 1080, webrip, 0.12, got, 8192) == n + 2
    ref, new = pinned.value.decode().split("\n"), got.value.decode().split("\n")
    assert new == ref[:-1] + ["-av1mi_target_bpp", "0.120000", "out.mkv"]
    rc, out, err = parse(host, *new[:-1])
    assert rc == 0 and out[1] == 120000, err
