"""The quality records on the GPU (include/av1mi.h "quality"; av1-go_amd/csrc/quality_kernels.hip): the kernel against the numpy
restatement (quality_ref.py), the session's records against the reference computed from the fed source and the session's own
reference frames (and dav1d's decode of the session's stream), and the product's stats file and quality gate.

Integers are compared for equality.  ssim_sum: relative 1e-12 against the correctly rounded sum (see test_quality.py: the windows'
values are the same bits, only the order of the additions differs; the kernel adds in a tree, which errs less than a running sum).
Every test runs under a time limit of its own: a GPU step that hangs ends the process instead of the tests after it running on."""
import ctypes as C
import faulthandler
import math
import os

import numpy as np
import pytest

import quality_ref as R
import scale_ref as SR
from test_quality import HOST, KINDS, RTOL, SIZES, compare, content, planes_of, reference, stack

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 240


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _r8(n):
    return (n + 7) & ~7


def device_records(ctx, bd, w, h, frames, src, dec0, dec1=None, select=None):
    bufs = [[ctx.to_device(a) for a in planes] if planes is not None else None for planes in (src, dec0, dec1)]
    d_sel = ctx.to_device(np.ascontiguousarray(select, np.uint8)) if select is not None else None
    try:
        return ctx.quality_planes(bd, w, h, frames, bufs[0], bufs[1], bufs[2], d_sel)
    finally:
        for group in bufs:
            for b in group or []:
                b.free()
        if d_sel is not None:
            d_sel.free()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h,frames", SIZES)
def test_kernel_matches_numpy(ctx, w, h, frames, bd):
    L = (1 << bd) - 1
    for kind in KINDS:
        src, dec = content(kind, bd, w, h, frames, 3)
        alt, select = None, None
        if frames > 1:
            _, alt = content("noise", bd, w, h, frames, 4)
            select = [(f + p) % 2 for f in range(frames) for p in range(3)]
        # the padding differs between the planes: it must not be counted
        args = (bd, w, h, frames, stack(src, w, h, L), stack(dec, w, h, 0), stack(alt, w, h, L) if alt else None, select)
        got = device_records(ctx, *args)
        compare(got, reference(src, dec, alt, select, bd), "%dx%d x%d, %d bit, %s" % (w, h, frames, bd, kind))
        again = device_records(ctx, *args)
        assert got.tobytes() == again.tobytes(), "two calls differ"
        first = [(f, p) for f in range(frames) for p in range(3) if select is None or select[f * 3 + p]]
        if kind == "identical":
            for f, p in first:
                assert got[f, p]["sse"] == 0 and got[f, p]["ssim_sum"] == float(got[f, p]["windows"])
        if kind == "last_column":
            for f, p in first:
                assert got[f, p]["sse"] == (L // 2 + 1) ** 2
                assert (got[f, p]["ssim_sum"] == float(got[f, p]["windows"])) == (planes_of(w, h)[p][0] % 4 != 0)


def test_kernel_full_size_batch(ctx):
    """3840 x 2160, 10 bit, 2 frames, the second candidate selected for some planes"""
    w, h, bd, frames = 3840, 2160, 10, 2
    src, dec = content("near", bd, w, h, frames, 5)
    _, alt = content("noise", bd, w, h, frames, 6)
    select = [1, 0, 1, 0, 1, 1]
    args = (bd, w, h, frames, stack(src, w, h, 0), stack(dec, w, h, 0), stack(alt, w, h, 0), select)
    got = device_records(ctx, *args)
    compare(got, reference(src, dec, alt, select, bd), "3840x2160 x2, 10 bit")
    assert got.tobytes() == device_records(ctx, *args).tobytes(), "two calls differ"


def test_kernel_refuses_bad_arguments(ctx, av1mi):
    b = ctx.alloc(1 << 16)
    try:
        for bd, w, h, frames in ((8, 15, 16, 1), (8, 16, 15, 1), (9, 64, 64, 1), (8, 64, 64, 0)):
            with pytest.raises(av1mi.Av1miError) as e:
                ctx.quality_planes(bd, w, h, frames, [b, b, b], [b, b, b])
            assert e.value.code == -1
        with pytest.raises(av1mi.Av1miError):      # a select array needs the second candidate
            ctx.quality_planes(8, 64, 64, 1, [b, b, b], [b, b, b], None, b)
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, 16, 16, 8, 100, 2, 1, visible=(12, 16), quality_stats=1)
        assert e.value.code == -1 and "16x16" in str(e.value)
    finally:
        b.free()


# ---- the session ----------------------------------------------------------------------------------------------------------

def _batches(w, h, bd, segs, n, seed):
    """n batches of `segs` frames at the true size w x h: smooth moving content"""
    import synth
    per = [synth.frames(_r8(w) + 8, _r8(h) + 8, n, bd, seed + 7 * s) for s in range(segs)]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return [[[per[s][0][t][:h, :w], per[s][1][t][:ch, :cw], per[s][2][t][:ch, :cw]] for s in range(segs)] for t in range(n)]


def _fed(batch, w, h):
    """a batch in the session's input buffers: true size rounded up to 8, the edge replicated into the padding"""
    out = []
    for i in range(3):
        pw, ph = (_r8(w), _r8(h)) if i == 0 else (_r8(w) // 2, _r8(h) // 2)
        out.append(np.concatenate([np.pad(planes[i], ((0, ph - planes[i].shape[0]), (0, pw - planes[i].shape[1])), mode="edge") for planes in batch]))
    return out


def _run(ctx, av1mi, cw, ch, bd, q, gop, segs, fed, mode, lag, quality, visible=None, source=None, via="submit"):
    import av1stream
    s = av1mi.GopSession(ctx, cw, ch, bd, q, gop, segs, gpu_entropy=mode, visible=visible, source=source, quality_stats=quality)
    outs, held, t_out = [], [], [0]

    def take():
        fr = s.collect()
        o = dict(lr_on=fr["lr_on"].copy(), quality=fr["quality"].copy() if "quality" in fr else None)
        o["units"] = [av1stream.session_temporal_unit(cw, ch, bd, fr["raw"], sg, with_sequence_header=(t_out[0] % gop == 0), visible=visible) for sg in range(segs)]
        if "tile_payload" in fr:
            o["payload"], o["tile_size"] = fr["tile_payload"].tobytes(), fr["tile_size"].copy()
        if lag == 0:
            o["ref"] = s.download_reference()
        outs.append(o)
        t_out[0] += 1
    try:
        for planes in fed:
            if via == "submit":
                for dst, a in zip(s.input_planes(), planes):
                    dst[:] = a
                s.submit()
            else:
                bufs = [ctx.to_device(a) for a in planes]
                held.append(bufs)
                s.submit_device(*bufs)
            if s.pending() > lag:
                take()
        while s.pending():
            take()
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
        for bufs in held:
            for b in bufs:
                b.free()
    return outs


def _crop(stacked, segs, tw, th):
    """stacked coded planes -> per segment (Y, U, V) at the true size"""
    out = []
    for sg in range(segs):
        planes = []
        for i, (pw, ph) in enumerate(planes_of(tw, th)):
            rows = stacked[i].shape[0] // segs
            planes.append(stacked[i][sg * rows:sg * rows + ph, :pw])
        out.append(planes)
    return out


def _check_session(ctx, av1mi, tw, th, bd, q, mode, seed, source=None, n=6, gop=3, segs=2, via="submit"):
    """tw x th: the true size of the coded frame; source: the true size of the frames fed when the session scales"""
    import dav1d_ref as D
    cw, ch = _r8(tw), _r8(th)
    visible = (tw, th) if (cw, ch) != (tw, th) else None
    if source is None:
        coded = _batches(tw, th, bd, segs, n, seed)
        fed = [_fed(b, tw, th) for b in coded]
    else:
        sw, sh = source
        frames = _batches(sw, sh, bd, segs, n, seed)
        fed = [_fed(b, sw, sh) for b in frames]
        table = {}

        def tab(a, b):
            if (a, b) not in table:
                table[(a, b)] = av1mi.scale_filter(a, b)
            return table[(a, b)]
        coded = [[list(SR.scale_frame(*planes, tw, th, bd, tab))for planes in b] for b in frames]
        coded = [[[p[:ph, :pw] for p, (pw, ph) in zip(planes, planes_of(tw, th))] for planes in b] for b in coded]
    flight = _run(ctx, av1mi, cw, ch, bd, q, gop, segs, fed, mode, 2, 1, visible, source, via)      # three batches in flight
    step = _run(ctx, av1mi, cw, ch, bd, q, gop, segs, fed, mode, 0, 1, visible, source, via)        # lock step, with the reference frames
    plain = _run(ctx, av1mi, cw, ch, bd, q, gop, segs, fed, mode, 2, 0, visible, source, via)       # the option off
    what = "%dx%d, %d bit, gpu_entropy %d" % (tw, th, bd, mode)
    for t in range(n):
        assert plain[t]["quality"] is None and flight[t]["quality"].shape == (segs, 3)
        # the option changes nothing about what is coded
        assert np.array_equal(flight[t]["lr_on"], plain[t]["lr_on"]) and flight[t]["units"] == plain[t]["units"], "%s: batch %d is coded differently" % (what, t)
        if mode == 1:
            assert flight[t]["payload"] == plain[t]["payload"] and np.array_equal(flight[t]["tile_size"], plain[t]["tile_size"])
        assert flight[t]["quality"].tobytes() == step[t]["quality"].tobytes(), "%s: batch %d, in flight and lock step differ" % (what, t)
        dec = _crop(step[t]["ref"], segs, tw, th)
        compare(flight[t]["quality"], np.array([R.frame(coded[t][sg], dec[sg], bd) for sg in range(segs)]), "%s, batch %d vs the session's reference" % (what, t))
    if D.available():
        for sg in range(segs):
            got = D.decode(b"".join(step[t]["units"][sg] for t in range(n)))
            assert len(got) == n
            for t in range(n):
                compare(flight[t]["quality"][sg:sg + 1], R.frame(coded[t][sg], got[t], bd)[None], "%s, segment %d frame %d vs dav1d" % (what, sg, t))


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("bd", [8, 10])
def test_session_records(ctx, av1mi, bd, mode):
    _check_session(ctx, av1mi, 192, 128, bd, 110, mode, 1)


@pytest.mark.parametrize("mode", [1, 0])
def test_session_records_cropped_frame(ctx, av1mi, mode):
    """visible 1366 x 768 in a coded 1368 x 768"""
    _check_session(ctx, av1mi, 1366, 768, 10, 60, mode, 2)


def test_session_records_scaled_source(ctx, av1mi):
    """source_width / source_height: the source of the records is the scaled frame"""
    _check_session(ctx, av1mi, 192, 128, 8, 110, 1, 3, source=(288, 192))


def test_session_records_device_source(ctx, av1mi):
    _check_session(ctx, av1mi, 192, 128, 10, 110, 1, 4, via="device")


def test_session_counts_the_kernel_under_its_own_key(ctx, av1mi):
    w, h, bd, gop, segs = 192, 128, 8, 3, 2
    fed = [_fed(b, w, h) for b in _batches(w, h, bd, segs, gop, 5)]
    ctx.prof_enable(1)
    try:
        for quality, want in ((0, None), (1, gop)):
            ctx.prof_reset()
            _run(ctx, av1mi, w, h, bd, 110, gop, segs, fed, 1, 2, quality)
            prof = ctx.prof_get()
            assert (prof["quality"][0] if "quality" in prof else None) == want
    finally:
        ctx.prof_enable(0)
        ctx.prof_reset()


# ---- the product ----------------------------------------------------------------------------------------------------------

def _write_y4m(path, frames, w, h, bd):
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s\n" % (w, h, "420jpeg" if bd == 8 else "420p10")).encode())
        for planes in frames:
            f.write(b"FRAME\n")
            for p in planes:
                f.write(np.ascontiguousarray(p).astype("<u2" if bd == 10 else np.uint8).tobytes())


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(HOST)
    lib.av1mi_host_run_transcode.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.av1mi_host_process_job_q.argtypes = [C.c_char_p, C.c_longlong, C.c_double, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_double]
    return lib


def _transcode(host, argv):
    buf = C.create_string_buffer(2048)
    return host.av1mi_host_run_transcode("\n".join(str(a) for a in argv).encode(), buf, 2048), buf.value.decode()


def _clip(w, h, n, bd, seed):
    return [b[0] for b in _batches(w, h, bd, 1, n, seed)]


@pytest.mark.parametrize("bd,w,h", [(8, 192, 128), (10, 202, 118)])
def test_transcode_stats_file(host, tmp_path, bd, w, h):
    import dav1d_ref as D
    n = 7
    frames = _clip(w, h, n, bd, 31)
    _write_y4m(tmp_path / "clip.y4m", frames, w, h, bd)
    out, stats = tmp_path / "clip.obu", tmp_path / "clip.stats"
    code, err = _transcode(host, ["-i", tmp_path / "clip.y4m", "-global_quality:v:0", 110, "-g", 3, "-av1mi_segments", 2, "-av1mi_stats", stats, out])
    assert code == 0, err
    lines = stats.read_text().splitlines()
    assert len(lines) == n + 1
    per = [dict(kv.split(":") for kv in ln.split()) for ln in lines[:-1]]
    assert [int(d["n"]) for d in per] == list(range(n)) and [d["type"] for d in per] == ["K" if i % 3 == 0 else "P" for i in range(n)]
    assert lines[-1].startswith("summary frames:%d bytes:%d " % (n, out.stat().st_size))
    assert sum(int(d["bytes"]) for d in per) == out.stat().st_size
    summ = dict(kv.split(":") for kv in lines[-1].split()[1:])
    keys = ["psnr_y", "psnr_u", "psnr_v", "psnr_all", "ssim_y", "ssim_u", "ssim_v", "ssim_all"]
    assert list(summ)[2:] == keys and list(per[0])[3:] == keys
    for k in keys[4:]:      # SSIM of the summary: the mean of the frame values (each printed with six decimals)
        assert float(summ[k]) == pytest.approx(np.mean([float(d[k]) for d in per]), abs=1e-6)
    if D.available():
        got = D.decode(out.read_bytes())
        assert len(got) == n
        recs = np.array([R.frame(frames[t], got[t], bd) for t in range(n)])
        want = R.summary(recs, bd)
        for k, v in zip(keys, want):
            assert float(summ[k]) == pytest.approx(v, abs=1e-5), k
        for t in range(n):
            for k, v in zip(keys, R.figures(recs[t], bd)):
                assert float(per[t][k]) == pytest.approx(v, abs=1e-5), (t, k)
    # the same bytes without the option
    out2 = tmp_path / "plain.obu"
    code, err = _transcode(host, ["-i", tmp_path / "clip.y4m", "-global_quality:v:0", 110, "-g", 3, "-av1mi_segments", 2, out2])
    assert code == 0 and out2.read_bytes() == out.read_bytes()


def test_quality_gate(host, tmp_path):
    w, h, bd, n = 192, 128, 8, 4
    _write_y4m(tmp_path / "clip.y4m", _clip(w, h, n, bd, 32), w, h, bd)
    out = tmp_path / "clip.obu"
    code, err = _transcode(host, ["-i", tmp_path / "clip.y4m", "-global_quality:v:0", 110, "-av1mi_min_psnr", 99, out])
    assert code == 3 and err.startswith("quality gate: psnr_y ") and not out.exists()
    code, err = _transcode(host, ["-i", tmp_path / "clip.y4m", "-global_quality:v:0", 110, "-av1mi_min_psnr", 1, out])
    assert code == 0 and err == "" and out.stat().st_size > 100


def test_process_job_quality_gate(host, tmp_path):
    w, h, bd, n = 192, 128, 8, 4
    src = tmp_path / "clip.y4m"
    _write_y4m(src, _clip(w, h, n, bd, 33), w, h, bd)
    before, orig = src.read_bytes(), src.stat().st_size
    status, reason = C.create_string_buffer(256), C.create_string_buffer(256)
    assert host.av1mi_host_process_job_q(str(src).encode(), orig, 5.0, str(tmp_path).encode(), 0, 0, status, reason, 256, 99.0) == 0
    assert status.value == b"skipped" and reason.value.startswith(b"quality gate: psnr_y ")
    assert (tmp_path / "clip.av1qsvd-skip").exists() and (tmp_path / "clip.av1qsvd-why.txt").read_text().startswith("quality gate: ")
    assert not (tmp_path / "clip.av1-tmp.mkv").exists() and not (tmp_path / "clip.av1mi.mkv").exists() and src.read_bytes() == before
    (tmp_path / "clip.av1qsvd-skip").unlink()
    assert host.av1mi_host_process_job_q(str(src).encode(), orig, 5.0, str(tmp_path).encode(), 0, 0, status, reason, 256, 1.0) == 0
    assert status.value == b"success" and (tmp_path / "clip.av1mi.mkv").exists() and src.read_bytes() == before
