"""The quantiser belongs to the batch (include/av1mi.h av1mi_gop_set_base_q_idx, GopSession.set_q): a session whose quantiser changes
from batch to batch codes every batch exactly as the oracle's chain does at that batch's quantiser, its device-side deblocking maps
and CDEF records follow without losing their geometry, batches in flight keep their quantiser, and a session that is only ever told
its own quantiser writes the bytes it always wrote.  The last test drives the one-pass rate controller through av1mi_run_transcode."""
import numpy as np
import pytest

import dav1d_ref as D
from test_gpu_session import _oracle_filters

pytestmark = pytest.mark.gpu

SCHEDULE = [110, 60, 200, 110]      # a change at key -> P, P -> P down, P -> P up, and a return to an earlier quantiser


def _feed(s, Y, U, V, h, segs, n, t):
    """frame t of every segment (frames of segment k: k * n + t) into the session's next input buffers"""
    planes = s.input_planes()
    for k in range(segs):
        f = k * n + t
        planes[0][k * h:(k + 1) * h] = Y[f]
        planes[1][k * h // 2:(k + 1) * h // 2] = U[f]
        planes[2][k * h // 2:(k + 1) * h // 2] = V[f]


def _fields(p):
    return [list(v) if hasattr(v, "__len__") else v for v in (getattr(p, name) for name, _ in p._fields_)]


def _decodes_to(streams, refs, h, segs, crop=None):
    for k in range(segs):
        got = D.decode(streams[k])
        assert len(got) == len(refs)
        for t in range(len(refs)):
            for i, hh in ((0, h), (1, h // 2), (2, h // 2)):
                exp = refs[t][i][k * hh:(k + 1) * hh]
                if crop:
                    ch, cw = crop[0] if i == 0 else crop[1]
                    assert got[t][i].shape == (ch, cw)
                    exp = exp[:ch, :cw]
                assert (got[t][i] == exp).all(), "segment %d frame %d plane %d: dav1d differs from the GPU" % (k, t, i)


@pytest.mark.parametrize("w,h,bd", [(192, 128, 8), (136, 72, 10)])
def test_a_changing_quantiser_matches_the_oracle_chain(ctx, av1mi, O, w, h, bd):
    gop, segs = 4, 2
    import synth
    Y, U, V = synth.frames(w, h, segs * gop, bd, 4)
    s = av1mi.GopSession(ctx, w, h, bd, SCHEDULE[0], gop, segs)
    try:
        ref = [None] * segs
        for t, q in enumerate(SCHEDULE):
            _feed(s, Y, U, V, h, segs, gop, t)
            s.set_q(q)
            s.submit()
            fr = s.collect()
            gy, gu, gv = s.download_reference()
            p = fr["params"]
            assert p.base_q_idx == q and p.frame_type == (0 if t == 0 else 1)
            pol = av1mi.policy_frame_params(q, bd, p.frame_type)
            assert _fields(pol) == _fields(p), "frame %d: the collected parameters are not the policy's at q %d" % (t, q)
            for k in range(segs):
                f = k * gop + t
                if t == 0:
                    r = O.intra_encode_frame(Y[f], U[f], V[f], bd, 8, q)
                    assert (fr["y_mode"][k] == r["modes_y"]).all() and (fr["uv_mode"][k] == r["modes_uv"]).all()
                    skip8 = np.zeros((h // 8, w // 8), np.uint8)
                else:
                    r = O.inter_encode_frame((Y[f], U[f], V[f]), ref[k], bd, q, 8)
                    assert (fr["mv"][k] == r["mvs"]).all() and (fr["skip"][k] == r["skip"]).all()
                    skip8 = r["skip"].reshape(h // 8, w // 8)
                for name in ("lev_y", "lev_u", "lev_v"):
                    assert (fr[name][k] == r[name]).all(), (t, k, name)
                ref[k], on = _oracle_filters(O, r, bd, pol, w, h, skip8, (Y[f], U[f], V[f]))
                assert fr["lr_on"][k].tolist() == on, (t, k, fr["lr_on"][k].tolist(), on)
                for got, exp, hh in ((gy, ref[k][0], h), (gu, ref[k][1], h // 2), (gv, ref[k][2], h // 2)):
                    assert (got[k * hh:(k + 1) * hh] == exp).all(), "frame %d (q %d) segment %d: reference differs from the oracle chain" % (t, q, k)
    finally:
        s.close()


@pytest.mark.skipif(not D.available(), reason="no dav1d in this image")
@pytest.mark.parametrize("w,h,bd", [(192, 128, 8), (136, 72, 10)])
def test_a_changing_quantiser_coders_and_decoder_agree(ctx, av1mi, w, h, bd):
    import av1stream
    import synth
    gop, segs = 4, 2
    Y, U, V = synth.frames(w, h, segs * gop, bd, 4)
    s = av1mi.GopSession(ctx, w, h, bd, SCHEDULE[0], gop, segs, gpu_entropy=2)
    try:
        streams, refs = [b""] * segs, []
        for t, q in enumerate(SCHEDULE):
            _feed(s, Y, U, V, h, segs, gop, t)
            s.set_q(q)
            s.submit()
            fr = s.collect()
            refs.append(s.download_reference())
            assert "tile_size" in fr and fr["params"].base_q_idx == q
            for k in range(segs):
                gpu = av1stream.session_frame_unit_gpu(w, h, bd, fr, k)
                assert gpu == av1stream.session_frame_unit(w, h, bd, fr, k, threads=4), "frame %d (q %d) segment %d: GPU coder and host writer disagree" % (t, q, k)
                streams[k] += gpu
        assert s.entropy_fallbacks() == 0
        _decodes_to(streams, refs, h, segs)
    finally:
        s.close()


@pytest.mark.skipif(not D.available(), reason="no dav1d in this image")
def test_a_changing_quantiser_with_key_frames_in_32x32_blocks(ctx, av1mi):
    """256 x 168 has a partial last superblock row: both bands of the key frame and the third map pair.  Two GOPs one after the other:
    the second key frame finds its maps at the first GOP's key quantiser, the P frames theirs at what the last P frame left"""
    import av1stream
    import synth
    w, h, bd, gop, segs = 256, 168, 10, 3, 2
    sched = [60, 60, 150, 150, 40, 40]
    Y, U, V = synth.frames(w, h, segs * len(sched), bd, 4)
    out = {}
    for mode in (1, 0):
        s = av1mi.GopSession(ctx, w, h, bd, sched[0], gop, segs, gpu_entropy=mode, key_block_size=32)
        try:
            streams, refs = [b""] * segs, []
            for t, q in enumerate(sched):
                _feed(s, Y, U, V, h, segs, len(sched), t)
                s.set_q(q)
                s.submit()
                fr = s.collect()
                assert fr["params"].base_q_idx == q and fr.get("key_block_size", 8) == (32 if t % gop == 0 else 8)
                refs.append(s.download_reference())
                for k in range(segs):
                    streams[k] += av1stream.session_temporal_unit(w, h, bd, fr["raw"], k, with_sequence_header=(t % gop == 0), threads=4)
            assert s.entropy_fallbacks() == 0
            out[mode] = (streams, refs)
        finally:
            s.close()
    assert out[1][0] == out[0][0], "GPU-coded and host-coded streams differ"
    _decodes_to(out[1][0], out[1][1], h, segs)


@pytest.mark.skipif(not D.available(), reason="no dav1d in this image")
@pytest.mark.parametrize("vw,vh,bd", [(100, 76, 8), (130, 70, 10)])
def test_a_changing_quantiser_keeps_the_off_screen_marking(ctx, av1mi, vw, vh, bd):
    """a true size that is not a multiple of 8: the maps' "off screen: never filtered" words must survive the rewrite of the levels, or
    dav1d (which filters on-screen units only) reconstructs other pictures than the session"""
    import av1stream
    import synth
    import test_av1_conformance as T
    gop, segs, sched = 3, 2, [100, 220, 30]
    w, h = (vw + 7) // 8 * 8, (vh + 7) // 8 * 8
    cvw, cvh = (vw + 1) // 2, (vh + 1) // 2
    src = [synth.frames(w + 8, h + 8, gop, bd, 3 + 5 * k) for k in range(segs)]
    s = av1mi.GopSession(ctx, w, h, bd, sched[0], gop, segs, gpu_entropy=2, visible=(vw, vh))
    try:
        streams, refs = [b""] * segs, []
        for t, q in enumerate(sched):
            planes = s.input_planes()
            for k in range(segs):
                Yc, Uc, Vc = src[k]
                planes[0][k * h:(k + 1) * h] = T._pad(Yc[t][:vh, :vw], h, w)
                planes[1][k * h // 2:(k + 1) * h // 2] = T._pad(Uc[t][:cvh, :cvw], h // 2, w // 2)
                planes[2][k * h // 2:(k + 1) * h // 2] = T._pad(Vc[t][:cvh, :cvw], h // 2, w // 2)
            s.set_q(q)
            s.submit()
            fr = s.collect()
            refs.append(s.download_reference())
            for k in range(segs):
                gpu = av1stream.session_frame_unit_gpu(w, h, bd, fr, k, visible=(vw, vh))
                assert gpu == av1stream.session_frame_unit(w, h, bd, fr, k, threads=4, visible=(vw, vh))
                streams[k] += gpu
        _decodes_to(streams, refs, h, segs, crop=((vh, vw), (cvh, cvw)))
    finally:
        s.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_a_batch_in_flight_keeps_its_quantiser(ctx, av1mi, mode):
    """set_q + submit run ahead of collect by the maximum: the payload bytes are those of the same schedule in lockstep"""
    import av1stream
    import synth
    w, h, bd, gop, segs = 192, 128, 8, 6, 2
    sched = SCHEDULE + [110, 30]
    Y, U, V = synth.frames(w, h, segs * gop, bd, 4)

    def run(lag):
        s = av1mi.GopSession(ctx, w, h, bd, sched[0], gop, segs, gpu_entropy=mode)
        units, qs = [], []

        def take():
            fr = s.collect()
            qs.append(fr["params"].base_q_idx)
            for k in range(segs):
                units.append(av1stream.session_frame_unit_gpu(w, h, bd, fr, k) if mode else av1stream.session_frame_unit(w, h, bd, fr, k, threads=4))
        try:
            for t, q in enumerate(sched):
                _feed(s, Y, U, V, h, segs, gop, t)
                s.set_q(q)
                s.submit()
                if s.pending() > lag:
                    take()
            assert s.pending() == min(lag, len(sched))
            s.set_q(255)      # told while batches are in flight: it is theirs no more
            while s.pending():
                take()
        finally:
            s.close()
        assert qs == sched
        return units

    a, b = run(0), run(av1mi.load().av1mi_gop_max_in_flight() - 1)
    assert len(a) == len(b) == len(sched) * segs
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, "frame %d segment %d: the session that ran ahead differs from lockstep (%d vs %d bytes)" % (i // segs, i % segs, len(y), len(x))
    assert len(set(len(x) for x in a)) > 2


def test_the_sessions_own_quantiser_changes_nothing_and_bad_values_are_refused(ctx, av1mi):
    import av1stream
    import synth
    w, h, bd, q, gop, segs = 192, 128, 8, 110, 3, 2
    Y, U, V = synth.frames(w, h, segs * gop, bd, 4)

    def run(tell):
        s = av1mi.GopSession(ctx, w, h, bd, q, gop, segs, gpu_entropy=2)
        units = []
        try:
            for t in range(gop):
                _feed(s, Y, U, V, h, segs, gop, t)
                if tell:
                    s.set_q(q)
                    for bad in (0, 256, -1, 1000):
                        with pytest.raises(av1mi.Av1miError) as e:
                            s.set_q(bad)
                        assert "1..255" in str(e.value)
                s.submit()
                fr = s.collect()
                assert fr["params"].base_q_idx == q
                for k in range(segs):
                    units.append(av1stream.session_frame_unit_gpu(w, h, bd, fr, k))
                    assert units[-1] == av1stream.session_frame_unit(w, h, bd, fr, k, threads=4)
            units.append(b"".join(p.tobytes() for p in s.download_reference()))
        finally:
            s.close()
        return units

    assert run(True) == run(False)


def _y4m(path, w, h, n, seed):
    import synth
    Y, U, V = synth.frames(w, h, n, 8, seed)
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg\n" % (w, h))
        for t in range(n):
            f.write(b"FRAME\n" + Y[t].tobytes() + U[t].tobytes() + V[t].tobytes())


@pytest.mark.skipif(not D.available(), reason="no dav1d in this image")
def test_a_target_bitrate_through_run_transcode(ctx, tmp_path):
    """av1mi_run_transcode with -b:v:0: the one-pass controller (host/ratecontrol.hpp) between av1mi_gop_set_base_q_idx and the
    collected bytes.  B0, the size at the fixed start quantiser, is measured; the targets are B0 / 2 and B0 / 4.  How close the
    controller comes is not asserted here (tools/bench_ratecontrol.py reports it), only that it comes closer than the fixed quantiser"""
    import ctypes as C
    import re
    import av1stream
    w, h, n, fps = 192, 128, 48, 25
    src = str(tmp_path / "in.y4m")
    _y4m(src, w, h, n, 11)

    def run(tag, *opts):
        out, stats = str(tmp_path / (tag + ".obu")), str(tmp_path / (tag + ".stats"))
        argv = ["-i", src, "-g", "8", "-av1mi_segments", "2", "-global_quality:v:0", "60", "-av1mi_stats", stats] + list(opts) + [out]
        buf = C.create_string_buffer(1024)
        code = av1stream.lib().av1mi_host_run_transcode("\n".join(argv).encode(), buf, 1024)
        assert code == 0 and buf.value == b"", buf.value
        lines = [ln for ln in open(stats).read().splitlines() if ln.startswith("n:")]
        assert len(lines) == n
        video = sum(int(re.search(r" bytes:(\d+)", ln).group(1)) for ln in lines)
        qs = [int(m.group(1)) for m in (re.search(r" q:(\d+)$", ln) for ln in lines) if m]
        return open(out, "rb").read(), video, qs

    data0, b0, qs0 = run("fixed")
    assert qs0 == [], "without a target the stats lines keep their format"
    got = {}
    for div in (2, 4):
        bps = b0 // div * 8 * fps // n                # the target in bits per second of a 25 frames/s file of n frames
        target = bps * n // (8 * fps)
        data, video, qs = run("t%d" % div, "-b:v:0", str(bps))
        again, video2, qs2 = run("t%d_again" % div, "-b:v:0", str(bps))
        assert data == again and qs == qs2, "two runs of one job differ"
        assert len(D.decode(data)) == n
        assert len(qs) == n and all(1 <= q <= 255 for q in qs) and len(set(qs)) > 1, qs
        print("target %d bytes: %d with the controller, %d at the fixed quantiser; q %s" % (target, video, b0, sorted(set(qs))))
        assert abs(video - target) < abs(b0 - target), (video, target, b0)
        got[div] = video
    assert got[4] < got[2] < b0, (got, b0)
    bps = b0 // 4 * 8 * fps // n
    data, video, qs = run("capped", "-b:v:0", str(bps), "-qmax", "70")
    assert len(qs) == n and max(qs) <= 70 and len(D.decode(data)) == n, qs
