"""GPU tests of -av1mi_depth / -av1mi_dither in a transcode job (av1mi_run_transcode): the reference's argv with `chain` codes a 10-bit source as
the 8-bit stream its format=nv12 asks for — dav1d decodes 8 bits, to the frames of the session the job drives —; `source` is the job as it
always ran, byte for byte; a 12-bit 4:4:4 source with `8` is converted, then reduced."""
import ctypes as C

import numpy as np
import pytest

import depth_ref as R

pytestmark = pytest.mark.gpu

W, H, N = 136, 72, 4
G, SEGS = 2, 2


def _clip(bd, chroma444=False):
    rng = np.random.default_rng(9)
    top = (1 << bd) - 1
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = (yy, xx) if chroma444 else (yy[::2, ::2], xx[::2, ::2])
    Y = np.stack([np.clip((xx * 7 + yy * 3 + 6 * t) * (top + 1) // 1024 + rng.integers(0, 6, (H, W)), 0, top) for t in range(N)])
    U = np.stack([np.clip((380 + cx * 2 + t) * (top + 1) // 1024, 0, top) for t in range(N)])
    V = np.stack([np.clip((650 - cy * 3) * (top + 1) // 1024, 0, top) for t in range(N)])
    return [a.astype(np.uint16) for a in (Y, U, V)]


def _write(path, clip, tag):
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s\n" % (W, H, tag)).encode())
        for t in range(N):
            f.write(b"FRAME\n")
            for p in clip:
                f.write(np.ascontiguousarray(p[t]).astype("<u2").tobytes())


def _reference_argv(inp, out):
    """TranscodeArgs' argv for a 1080-line job (av1mi_host_transcode_args): the chain ends in hwdownload,format=nv12,setsar=1,format=nv12,hwupload"""
    import av1stream
    host = av1stream.lib()
    host.av1mi_host_transcode_args.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int] * 4 + [C.c_char_p, C.c_int]
    buf = C.create_string_buffer(8192)
    assert host.av1mi_host_transcode_args(str(inp).encode(), str(out).encode(), 1, 0, 1080, 0, buf, 8192) > 0
    argv = buf.value.decode().split("\n")
    assert "format=nv12" in argv[argv.index("-vf:v:0") + 1] and argv[-1] == str(out)
    return argv


def _job(argv, extra):
    import av1stream
    return av1stream.run_transcode(argv[:-1] + [str(x) for x in extra] + argv[-1:])


def _session_refs(ctx, av1mi, clip, q, **kw):
    """the references of the session the job drives, in file order: segment s holds frames s * G + t"""
    s = av1mi.GopSession(ctx, W, H, 10, q, G, SEGS, gpu_entropy=1, key_block_size=8, **kw)      # (136 is no multiple of 32: the job falls back to 8x8 key frames)
    refs = [None] * N
    try:
        for t in range(G):
            for dst, a in zip(s.input_planes(), clip):
                dst[:] = np.concatenate([a[sg * G + t] for sg in range(SEGS)])
            s.submit()
            s.collect()
            ref = s.download_reference()
            for sg in range(SEGS):
                refs[sg * G + t] = [ref[i][sg * rows:(sg + 1) * rows] for i, rows in enumerate((H, H // 2, H // 2))]
    finally:
        s.close()
    return refs


def test_the_references_argv_with_chain_codes_8_bits(ctx, av1mi, tmp_path):
    import dav1d_ref as D
    clip = _clip(10)
    _write(tmp_path / "a.y4m", clip, "420p10")
    argv = _reference_argv(tmp_path / "a.y4m", tmp_path / "a.obu")
    q = int(argv[argv.index("-global_quality:v:0") + 1])
    common = ["-g", G, "-av1mi_segments", SEGS]
    code, err = _job(argv, common + ["-av1mi_depth", "chain", "-av1mi_stats", tmp_path / "a.stats"])
    assert code == 0, err
    lines = (tmp_path / "a.stats").read_text().splitlines()
    assert " depth:10>8" in lines[0] and not any("depth:" in l for l in lines[1:])
    assert D.available(), "dav1d is what this test is about"
    got = D.decode((tmp_path / "a.obu").read_bytes())
    refs = _session_refs(ctx, av1mi, clip, q, coded_bit_depth=8, depth_dither=R.ORDERED)
    assert len(got) == N and all(p.dtype == np.uint8 for f in got for p in f), "dav1d does not report an 8-bit stream"
    assert all(np.array_equal(got[f][i], refs[f][i]) for f in range(N) for i in range(3))
    # the coded picture is the reduced source's: a sane PSNR against depth_ref's planes (the bound of tests/test_gpu_pipeline.py)
    want = R.reduce_plane(clip[0].reshape(-1, W), 0, R.ORDERED).reshape(N, H, W)
    for f in range(N):
        psnr = 10 * np.log10(255.0 ** 2 / max(np.mean((got[f][0].astype(np.float64) - want[f]) ** 2), 1e-9))
        print("frame %d: PSNR-Y %.2f dB against the reduced source" % (f, psnr))
        assert psnr > 28, (f, psnr)
    # -av1mi_dither round is another stream; Matroska says 8 bits per channel when the job describes its colour
    argv_r = argv[:-1] + [str(tmp_path / "r.obu")]
    assert _job(argv_r, common + ["-av1mi_depth", "chain", "-av1mi_dither", "round"])[0] == 0
    assert (tmp_path / "r.obu").read_bytes() != (tmp_path / "a.obu").read_bytes()
    import test_colour_signal as S
    argv_m = argv[:-1] + [str(tmp_path / "m.mkv")]
    assert _job(argv_m, common + ["-av1mi_depth", "chain", "-color_primaries", "bt709", "-color_trc", "bt709", "-colorspace", "bt709"])[0] == 0
    video = S._find((tmp_path / "m.mkv").read_bytes(), [0x18538067, 0x1654AE6B, 0xAE, 0xE0])
    col = dict(S._ebml(S._find(video, [0x55B0]), 0, len(S._find(video, [0x55B0]))))
    assert int.from_bytes(col[0x55B2], "big") == 8      # BitsPerChannel


def test_source_is_the_job_without_the_option(tmp_path):
    clip = _clip(10)
    _write(tmp_path / "a.y4m", clip, "420p10")
    common = ["-g", G, "-av1mi_segments", SEGS]
    out = {}
    for name, extra in (("none", []), ("source", ["-av1mi_depth", "source"]), ("source_dither", ["-av1mi_depth", "source", "-av1mi_dither", "ordered"])):
        argv = _reference_argv(tmp_path / "a.y4m", tmp_path / (name + ".mkv"))
        code, err = _job(argv, common + extra)
        assert code == 0, err
        out[name] = (tmp_path / (name + ".mkv")).read_bytes()
    assert out["source"] == out["none"] and out["source_dither"] == out["none"]


def test_a_12_bit_444_source_coded_at_8_bits(ctx, av1mi, tmp_path):
    import dav1d_ref as D
    clip = _clip(12, chroma444=True)
    _write(tmp_path / "b.y4m", clip, "444p12")
    argv = _reference_argv(tmp_path / "b.y4m", tmp_path / "b.obu")
    code, err = _job(argv, ["-g", G, "-av1mi_segments", SEGS, "-av1mi_depth", "8", "-av1mi_stats", tmp_path / "b.stats"])
    assert code == 0, err
    assert " depth:12>8" in (tmp_path / "b.stats").read_text().splitlines()[0]
    assert D.available()
    got = D.decode((tmp_path / "b.obu").read_bytes())
    assert len(got) == N and all(p.dtype == np.uint8 for f in got for p in f)
    assert got[0][0].shape == (H, W) and got[0][1].shape == (H // 2, W // 2)
    # luma goes 12 -> 10 (rounded, clamped: "chroma formats") -> 8 (ordered): the coded picture is that plane's
    y10 = np.minimum((clip[0].astype(np.uint32) + 2) >> 2, 1023).astype(np.uint16)
    want = R.reduce_plane(y10.reshape(-1, W), 0, R.ORDERED).reshape(N, H, W)
    for f in range(N):
        psnr = 10 * np.log10(255.0 ** 2 / max(np.mean((got[f][0].astype(np.float64) - want[f]) ** 2), 1e-9))
        assert psnr > 28, (f, psnr)
