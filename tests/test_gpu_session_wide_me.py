"""The GOP session and the product with the wide-range motion search (av1mi_gop_config.coarse_range, -av1mi_me_range): the streams are
coded the same by the GPU and the host coder and decode in dav1d to the session's references; with the option off the bytes are
the parent's; and on a fast pan the P frames cost what slow content costs.  tools/bench_wide_me.py measures the figures asserted
here (profiles/wide_me.json)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import me_ref as M

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "av1-go_amd", "host", "libav1mi_host.so")
GOP, SEGS = 4, 2          # 2 GOPs x 4 frames, coded in lockstep: segment s holds frames 4 s .. 4 s + 3 of the clip


def run_session(ctx, av1mi, clip, bd, q, coarse_range, mode=2, compare_coders=True, keep_refs=True):
    """clip: (Y, U, V) of GOP * SEGS frames.  Returns dict(streams [segment] bytes, refs [t] stacked planes, p_bytes: bytes of the P
    frames' temporal units, p_psnr_y: PSNR-Y over all P frames, fallbacks)"""
    import av1stream
    Y, U, V = clip
    h, w = Y.shape[1:]
    s = av1mi.GopSession(ctx, w, h, bd, q, GOP, SEGS, gpu_entropy=mode, quality_stats=1, coarse_range=coarse_range)
    out = dict(streams=[b""] * SEGS, refs=[], p_bytes=0)
    recs = []
    try:
        for t in range(GOP):
            for dst, a in zip(s.input_planes(), (Y, U, V)):
                dst[:] = np.concatenate([a[sg * GOP + t] for sg in range(SEGS)])
            s.submit()
            fr = s.collect()
            for sg in range(SEGS):
                tu = av1stream.session_frame_unit(w, h, bd, fr, sg)
                if mode == 2 and compare_coders:
                    assert tu == av1stream.session_frame_unit_gpu(w, h, bd, fr, sg), "frame %d segment %d: GPU tile coder and host writer disagree" % (t, sg)
                out["streams"][sg] += tu
                if t > 0:
                    out["p_bytes"] += len(tu)
            if t > 0:
                recs.append(fr["quality"][:, 0].copy())
            if keep_refs:
                out["refs"].append(s.download_reference())
        out["fallbacks"] = s.entropy_fallbacks()
    finally:
        s.close()
    out["p_psnr_y"] = av1mi.quality_psnr(np.concatenate(recs), bd)
    return out


def check_decodes(out, w, h):
    import dav1d_ref as D
    if not D.available():
        return
    for sg in range(SEGS):
        got = D.decode(out["streams"][sg])
        assert len(got) == GOP
        for t in range(GOP):
            for i, d in enumerate((1, 2, 2)):
                rows = h // d
                assert (got[t][i] == out["refs"][t][i][sg * rows:(sg + 1) * rows]).all(), "segment %d frame %d plane %d: dav1d decodes another picture" % (sg, t, i)


def sha(out):
    return hashlib.sha256(b"".join(out["streams"])).hexdigest()


CASES = {"pan8": (640, 360, 8, 110), "pan10": (1920, 1080, 10, 60)}


def clip_of(kind, w, h, bd, scale=20):
    return (M.split_clip if kind == "split" else M.pan_clip)(w, h, GOP * SEGS, bd, scale)


@pytest.mark.parametrize("kind", ["pan", "split"])
@pytest.mark.parametrize("case", ["pan8", "pan10"])
def test_wide_session_streams(ctx, av1mi, case, kind):
    """coarse_range 64, gpu_entropy 2: GPU-coded bytes == host-coded bytes, no fallback, dav1d decodes the key frame and the P frames
    to the session's references"""
    w, h, bd, q = CASES[case]
    out = run_session(ctx, av1mi, clip_of(kind, w, h, bd), bd, q, 64)
    assert out["fallbacks"] == 0
    check_decodes(out, w, h)


# SHA-256 of the two segments' streams with coarse_range 0, produced by the parent commit's library on the same clips (the fast pan)
PARENT_SHA = {
    "pan8": "54021a67c44a165ffe52f3b26449a1421a84e5b759bb02c8212e5eaa3bec33be",
    "pan10": "5054b4741bc1c1b1f4349f2cee978854ffcf42d5be835752c2a787dcaf38d1c6",
}


@pytest.mark.parametrize("case", ["pan8", "pan10"])
def test_option_off_gives_the_parents_bytes(ctx, av1mi, case):
    w, h, bd, q = CASES[case]
    out = run_session(ctx, av1mi, clip_of("pan", w, h, bd), bd, q, 0, mode=0, keep_refs=False)
    assert sha(out) == PARENT_SHA[case]


# Measured on an MI355X with tools/bench_wide_me.py (profiles/wide_me.json, "effect"), 640x360 8 bit q 110, 6 P frames:
#   fast pan (25, 15) per frame, option off: 621 189 bytes, PSNR-Y 34.717 dB
#   fast pan, coarse_range 64:               166 945 bytes, PSNR-Y 35.781 dB      -> saving 0.7312 of the bytes
#   the texture at (1.25, 0.75), option off: 103 412 bytes                            -> wide / slow = 1.6144
MEASURED_SAVING = 0.7312        # 1 - on / off
MEASURED_RATIO = 1.6144         # on / slow


def test_fast_pan_costs_what_slow_content_costs(ctx, av1mi):
    w, h, bd, q = CASES["pan8"]
    fast = clip_of("pan", w, h, bd)
    off = run_session(ctx, av1mi, fast, bd, q, 0, mode=0, keep_refs=False)
    on = run_session(ctx, av1mi, fast, bd, q, 64, mode=0, keep_refs=False)
    slow = run_session(ctx, av1mi, clip_of("pan", w, h, bd, 1), bd, q, 0, mode=0, keep_refs=False)
    print("P bytes: off %d, on %d, slow %d; PSNR-Y off %.3f on %.3f" % (off["p_bytes"], on["p_bytes"], slow["p_bytes"], off["p_psnr_y"], on["p_psnr_y"]))
    # strictly fewer bytes, by at least half of the measured saving, at equal or higher PSNR-Y
    assert on["p_bytes"] < off["p_bytes"] * (1.0 - MEASURED_SAVING / 2)
    assert on["p_psnr_y"] >= off["p_psnr_y"]
    # about what the same texture costs at a speed the +-8 search covers: within the measured ratio plus a quarter of it
    assert on["p_bytes"] <= slow["p_bytes"] * MEASURED_RATIO * 1.25


def _write_y4m(path, clip, bd):
    Y, U, V = clip
    h, w = Y.shape[1:]
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s\n" % (w, h, "420jpeg" if bd == 8 else "420p10")).encode())
        for t in range(Y.shape[0]):
            f.write(b"FRAME\n")
            for p in (Y[t], U[t], V[t]):
                f.write(np.ascontiguousarray(p).astype("<u2" if bd == 10 else np.uint8).tobytes())


def test_transcode_with_me_range(tmp_path):
    """-av1mi_me_range 64 through av1mi_run_transcode: the output decodes in dav1d, and -av1mi_stats shows the P frames' bytes drop as
    in the session"""
    import dav1d_ref as D
    host = C.CDLL(HOST)
    host.av1mi_host_run_transcode.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    w, h, bd, q = CASES["pan8"]
    _write_y4m(tmp_path / "pan.y4m", clip_of("pan", w, h, bd), bd)
    p_bytes = {}
    for name, extra in (("off", []), ("on", ["-av1mi_me_range", 64])):
        out, stats = tmp_path / (name + ".obu"), tmp_path / (name + ".stats")
        argv = ["-i", tmp_path / "pan.y4m", "-global_quality:v:0", q, "-g", GOP, "-av1mi_segments", SEGS, "-av1mi_stats", stats] + extra + [out]
        buf = C.create_string_buffer(2048)
        code = host.av1mi_host_run_transcode("\n".join(str(a) for a in argv).encode(), buf, 2048)
        assert code == 0, buf.value.decode()
        per = [dict(kv.split(":") for kv in ln.split()) for ln in stats.read_text().splitlines()[:-1]]
        assert len(per) == GOP * SEGS
        p_bytes[name] = sum(int(d["bytes"]) for d in per if d["type"] == "P")
        if D.available():
            assert len(D.decode(out.read_bytes())) == GOP * SEGS
    print("transcode P bytes: off %d, on %d" % (p_bytes["off"], p_bytes["on"]))
    assert p_bytes["on"] < p_bytes["off"] * (1.0 - MEASURED_SAVING / 2)
