"""GPU tests of the colour options and tone mapping of a transcode job (av1mi_run_transcode): the description and the HDR10 records reach the
stream and the Matroska file without touching a frame's bytes; -av1mi_tonemap and tonemap_vaapi code the reference's tone-mapped source and
say BT.709; a Y4M header's XCOLORRANGE reaches color_range."""
import numpy as np
import pytest

import tonemap_ref as R
import test_colour_signal as S

pytestmark = pytest.mark.gpu

W = H = 64
Q, G, SEGS, N = 128, 2, 2, 4
HDR = ["-color_primaries", "bt2020", "-color_trc", "smpte2084", "-colorspace:v:0", "bt2020nc", "-color_range", "tv",
       "-av1mi_master_display", "G(8500,39850)B(6550,2300)R(35400,14600)WP(15635,16450)L(40000000,50)", "-av1mi_max_cll", "1000,400"]


def _clip(bd=10):
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W]
    top = (1 << bd) - 1
    Y = np.stack([np.clip((xx * 14 + yy * 3 + 5 * t) * (top + 1) // 1024 + rng.integers(0, 6, (H, W)), 0, top) for t in range(N)])
    U = np.stack([np.clip((400 + xx[::2, ::2] * 3 + t) * (top + 1) // 1024, 0, top) for t in range(N)])
    V = np.stack([np.clip((620 - yy[::2, ::2] * 3) * (top + 1) // 1024, 0, top) for t in range(N)])
    return [a.astype(np.uint16 if bd == 10 else np.uint8) for a in (Y, U, V)]


def _write(path, clip, bd=10, tag=""):
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s%s\n" % (W, H, "420p10" if bd == 10 else "420jpeg", tag)).encode())
        for t in range(N):
            f.write(b"FRAME\n")
            for p in clip:
                f.write(np.ascontiguousarray(p[t]).astype("<u2" if bd == 10 else np.uint8).tobytes())


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    import av1stream
    d = tmp_path_factory.mktemp("colour")
    clip = _clip()
    _write(d / "hdr.y4m", clip)
    _write(d / "full.y4m", clip, tag=" XCOLORRANGE=FULL")
    _write(d / "sdr8.y4m", _clip(8), bd=8)
    chain = "tonemap_vaapi=format=p010:t=bt709,scale_vaapi=w=ceil(iw/2)*2:h=ceil(ih/2)*2,hwdownload,format=nv12,setsar=1,format=nv12,hwupload"
    plain_chain = chain.split(",", 1)[1]
    runs = dict(plain=("hdr.y4m", [], "obu"), hdr=("hdr.y4m", HDR + ["-av1mi_stats", d / "hdr.stats"], "obu"), plain_mkv=("hdr.y4m", [], "mkv"), hdr_mkv=("hdr.y4m", HDR, "mkv"),
                tm=("hdr.y4m", ["-av1mi_tonemap", "bt2390", "-vf:v:0", plain_chain, "-av1mi_stats", d / "tm.stats"], "obu"), tm_chain=("hdr.y4m", ["-vf:v:0", chain], "obu"),
                tm_hdr=("hdr.y4m", HDR + ["-av1mi_tonemap", "bt2390"], "obu"), tm_4000=("hdr.y4m", ["-av1mi_tonemap", "bt2390", "-av1mi_tonemap_peak", "4000"], "obu"),
                full=("full.y4m", [], "obu"), tm_full=("full.y4m", ["-av1mi_tonemap", "bt2390"], "obu"), tm_8=("sdr8.y4m", ["-av1mi_tonemap", "bt2390"], "obu"))
    out = {"dir": d, "clip": clip}
    for name, (source, extra, ext) in runs.items():
        path = d / (name + "." + ext)
        code, err = av1stream.run_transcode(["-i", d / source, "-global_quality:v:0", Q, "-g", G, "-av1mi_segments", SEGS] + extra + [path])
        out[name] = (code, err, path.read_bytes() if code == 0 else b"")
    return out


def _session_refs(ctx, av1mi, clip, **kw):
    """the references of the session the job drives, in file order: segment s holds frames s * G + t"""
    s = av1mi.GopSession(ctx, W, H, 10, Q, G, SEGS, gpu_entropy=1, key_block_size=32, **kw)
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


def test_hdr10_options_reach_the_stream_and_touch_no_frame(ctx, av1mi, jobs):
    import dav1d_ref as D
    for name in ("plain", "hdr", "plain_mkv", "hdr_mkv"):
        assert jobs[name][0] == 0, jobs[name][1]
    plain, hdr = S._obus(jobs["plain"][2]), S._obus(jobs["hdr"][2])
    assert [t for t, _ in plain] == [2, 1, 6, 2, 6] * SEGS and [t for t, _ in hdr] == [2, 1, 5, 5, 6, 2, 6] * SEGS
    assert [p for t, p in hdr if t == 6] == [p for t, p in plain if t == 6]
    assert S._color_config(plain[1][1]) == (2, 2, 2, 0)
    for i in range(0, len(hdr), 7):
        assert S._color_config(hdr[i + 1][1]) == (9, 16, 9, 0)
        cll, mdcv = hdr[i + 2][1], hdr[i + 3][1]
        assert cll[0] == 1 and S.struct.unpack(">HH", cll[1:5]) == (1000, 400)
        v = S.struct.unpack(">8HII", mdcv[1:25])
        assert mdcv[0] == 2 and v[:2] == (round(35400 * 65536 / 50000), round(14600 * 65536 / 50000)) and v[8:] == (4000 << 8, round(50 * 16384 / 10000))
    assert " colour:9/16/9/0" in (jobs["dir"] / "hdr.stats").read_text().splitlines()[0] and "colour:" not in "".join((jobs["dir"] / "hdr.stats").read_text().splitlines()[1:])
    # Matroska: the Colour element, and the same blocks
    video = S._find(jobs["hdr_mkv"][2], [0x18538067, 0x1654AE6B, 0xAE, 0xE0])
    col = dict(S._ebml(S._find(video, [0x55B0]), 0, len(S._find(video, [0x55B0]))))
    u = lambda eid: int.from_bytes(col[eid], "big")
    assert (u(0x55B1), u(0x55B2), u(0x55B9), u(0x55BA), u(0x55BB), u(0x55BC), u(0x55BD)) == (9, 10, 1, 16, 9, 1000, 400)
    mm = dict(S._ebml(col[0x55D0], 0, len(col[0x55D0])))
    assert abs(S.struct.unpack(">d", mm[0x55D9])[0] - 4000.0) < 1e-6 * 4000 and abs(S.struct.unpack(">d", mm[0x55D1])[0] - 0.708) < 1e-4
    pv = S._find(jobs["plain_mkv"][2], [0x18538067, 0x1654AE6B, 0xAE, 0xE0])
    assert 0x55B0 not in dict(S._ebml(pv, 0, len(pv)))
    if D.available():
        got, refs = D.decode(jobs["hdr"][2]), _session_refs(ctx, av1mi, jobs["clip"])
        assert len(got) == N and all((got[f][i] == refs[f][i]).all() for f in range(N) for i in range(3))


def test_tone_mapped_jobs(ctx, av1mi, jobs):
    import dav1d_ref as D
    for name in ("tm", "tm_chain", "tm_hdr", "tm_4000"):
        assert jobs[name][0] == 0, jobs[name][1]
    assert jobs["tm"][2] == jobs["tm_chain"][2] and jobs["tm"][2] != jobs["plain"][2]
    obus = S._obus(jobs["tm"][2])
    assert [t for t, _ in obus] == [2, 1, 6, 2, 6] * SEGS and all(S._color_config(p) == (1, 1, 1, 0) for t, p in obus if t == 1)
    assert " colour:1/1/1/0" in (jobs["dir"] / "tm.stats").read_text().splitlines()[0]
    # a job that describes its HDR10 source: no metadata in the output, and the mastering display's 4000 cd/m2 is the peak
    assert [t for t, _ in S._obus(jobs["tm_hdr"][2])] == [2, 1, 6, 2, 6] * SEGS
    assert jobs["tm_hdr"][2] == jobs["tm_4000"][2] and jobs["tm_hdr"][2] != jobs["tm"][2]
    if D.available():
        t = av1mi.tone_map_tables(1000)
        T = {k: np.array(getattr(t, k), np.int64) for k in ("lin", "gain", "oetf_lo", "oetf_hi")}
        mapped = R.tone_map(*[a.reshape(-1, a.shape[2]) for a in jobs["clip"]], T)
        mapped = [a.reshape(N, -1, a.shape[1]) for a in mapped]
        got = D.decode(jobs["tm"][2])
        refs = _session_refs(ctx, av1mi, jobs["clip"], tone_map=1)
        assert len(got) == N and all((got[f][i] == refs[f][i]).all() for f in range(N) for i in range(3))
        for f in range(N):      # the bound of tests/test_gpu_pipeline.py for the coded picture against its source
            mse = np.mean((got[f][0].astype(np.float64) - mapped[0][f]) ** 2)
            psnr = 10 * np.log10(1023.0 ** 2 / mse)
            print("frame %d: PSNR-Y %.2f dB against the reference's tone-mapped source" % (f, psnr))
            assert psnr > 28, (f, psnr)


def test_refusals_and_the_header_range(jobs):
    assert jobs["full"][0] == 0, jobs["full"][1]
    obus = S._obus(jobs["full"][2])
    assert all(S._color_config(p) == (2, 2, 2, 1) for t, p in obus if t == 1) and [p for t, p in obus if t == 6] == [p for t, p in S._obus(jobs["plain"][2]) if t == 6]
    assert jobs["tm_full"][0] == 1 and "XCOLORRANGE=FULL" in jobs["tm_full"][1]
    assert jobs["tm_8"][0] == 1 and "10-bit source" in jobs["tm_8"][1]
