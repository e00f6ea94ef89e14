"""GPU tests of inverse telecine inside the GOP session and the job (av1mi_gop_config.telecine, av1mi_gop_store_telecine,
av1mi_gop_submit_woven, -av1mi_ivtc).  The oracle of the session is a plain session — code that does not know the option — fed the frames
tests/telecine_ref.py weaves in numpy, which are the film frames; the oracle of the job is the plan of the whole file as one run."""
import struct

import numpy as np
import pytest

import telecine_ref as T

pytestmark = pytest.mark.gpu

GOP, SEGS, Q = 4, 2, 60
OWN = 10                     # telecined source frames: 8 film frames
V0 = 6                       # the store's position 0 (context) is video frame V0 of the endless pulldown


def _video(order, first, n, w, h, bd):
    """n video frames as buffers (true size rounded up to 8, the edge replicated): [plane][frame]"""
    fr = [T.video_frame(v, order, w, h, bd) for v in range(first, first + n)]
    return [np.stack([T.pad8(f[p], p == 0) for f in fr]) for p in range(3)]


def _outputs(s, fr):
    o = {k: fr[k].copy() for k in ("tile_size", "tile_payload", "lr_on")}
    o["frame_type"] = fr["frame_type"]
    o["ref"] = s.download_reference()
    return o


def _open(ctx, av1mi, w, h, bd, **kw):
    w8, h8 = (w + 7) & ~7, (h + 7) & ~7
    vis = dict(visible=(w, h)) if (w8, h8) != (w, h) else {}
    return av1mi.GopSession(ctx, w8, h8, bd, Q, GOP, SEGS, gpu_entropy=1, **vis, **kw), vis.get("visible")


def _collect(s, w8, h8, vis, units, t):
    import av1stream
    fr = s.collect()
    for sg in range(SEGS):
        units[sg].append(av1stream.session_temporal_unit(w8, h8, fr["raw"].bit_depth, fr["raw"], sg, with_sequence_header=(t == 0), visible=vis))
    return _outputs(s, fr)


@pytest.mark.parametrize("w, h, bd, order", [(64, 48, 8, "tff"), (64, 48, 10, "bff"), (70, 50, 8, "bff")])
def test_woven_session_equals_the_plain_session_fed_the_film(ctx, av1mi, w, h, bd, order):
    import av1stream
    import dav1d_ref as D
    w8, h8 = (w + 7) & ~7, (h + 7) & ~7
    video = _video(order, V0, OWN + 2, w, h, bd)
    want_rec = T.records(video[0], bd, w, h)
    top, bottom = T.plan(want_rec, 1, 1)
    assert len(top) == SEGS * GOP
    film0 = T.video_sources(V0 + 1, order)[1] + (T.video_sources(V0 + 1, order)[1] == T.video_sources(V0, order)[1])
    true = [(w, h), ((w + 1) // 2, (h + 1) // 2), ((w + 1) // 2, (h + 1) // 2)]
    woven = [[T.weave_plane(video[p][top[k]], video[p][bottom[k]], *true[p]) for p in range(3)] for k in range(SEGS * GOP)]
    for k in range(SEGS * GOP):      # the numpy-woven frames are the film frames
        for p, a in enumerate(T.film_frame(film0 + k, w, h, bd)):
            assert (woven[k][p] == T.pad8(a, p == 0)).all(), (k, p)
    # the plain session fed the woven frames: segment s codes outputs s GOP .. s GOP + GOP - 1
    s, vis = _open(ctx, av1mi, w, h, bd)
    base, base_units = [], [[] for _ in range(SEGS)]
    try:
        for t in range(GOP):
            for p, dst in enumerate(s.input_planes()):
                dst[:] = np.concatenate([woven[sg * GOP + t][p] for sg in range(SEGS)])
            s.submit()
            base.append(_collect(s, w8, h8, vis, base_units, t))
    finally:
        s.close()
    # the session that weaves: 12 frames into the store, two at a time; the records; the reference's plan through submit_woven
    s, vis = _open(ctx, av1mi, w, h, bd, store_frames=OWN, telecine=1)
    got, units = [], [[] for _ in range(SEGS)]
    try:
        for first in range(0, OWN + 2, SEGS):
            for p, dst in enumerate(s.input_planes()):
                dst[:] = video[p][first:first + SEGS].reshape(dst.shape)
            s.store_put(0, first, SEGS)
        rec = s.store_telecine(0, OWN + 2)
        assert rec.tobytes() == want_rec.tobytes()
        ht, hb = av1stream.plan_telecine(rec, 1, 1)
        assert ht.tolist() == top.tolist() and hb.tolist() == bottom.tolist()
        for t in range(GOP):
            s.submit_woven(0, [top[sg * GOP + t] for sg in range(SEGS)], [bottom[sg * GOP + t] for sg in range(SEGS)], 0 if t == 0 else 1)
            got.append(_collect(s, w8, h8, vis, units, t))
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    assert [o["frame_type"] for o in got] == [0, 1, 1, 1]
    for t in range(GOP):
        for k in ("tile_size", "tile_payload", "lr_on", "frame_type"):
            assert np.array_equal(base[t][k], got[t][k]), "batch %d: %s differs from the plain session fed the woven frames" % (t, k)
        for p in range(3):
            assert np.array_equal(base[t]["ref"][p], got[t]["ref"][p]), (t, p)
    assert units == base_units
    assert D.available(), "dav1d is what this part is about"
    for sg in range(SEGS):
        dec = D.decode(b"".join(units[sg]))
        assert len(dec) == GOP
        for t in range(GOP):
            for p in range(3):
                rows = got[t]["ref"][p].shape[0] // SEGS
                ref = got[t]["ref"][p][sg * rows:(sg + 1) * rows]
                assert np.array_equal(dec[t][p][:true[p][1], :true[p][0]], ref[:true[p][1], :true[p][0]]), (sg, t, p)


def test_a_flat_slot_and_the_store_positions(ctx, av1mi):
    """top -1 is a flat slot (its bottom is not read); positions run to store_frames + 1; submit_stored keeps its meaning"""
    w, h, bd = 64, 48, 8
    video = _video("tff", V0, 4, w, h, bd)
    s, _ = _open(ctx, av1mi, w, h, bd, store_frames=2, telecine=1)
    try:
        for first in (0, 2):
            for p, dst in enumerate(s.input_planes()):
                dst[:] = video[p][first:first + 2].reshape(dst.shape)
            s.store_put(0, first, 2)
        s.submit_woven(0, [3, -1], [2, 99], 0)
        s.collect()
        fed = s.download_fed()
        assert (fed[0][:h] == T.weave_plane(video[0][3], video[0][2], w, h)).all() and (fed[0][h:] == 0).all()
        s.submit_stored(0, [1, 3], 0)      # (a context position can be submitted plainly too)
        s.collect()
        assert (s.download_fed()[0] == np.concatenate([video[0][1], video[0][3]])).all()
        with pytest.raises(av1mi.Av1miError):
            s.submit_stored(0, [4, 0], 0)
        for call in (lambda: s.submit_woven(0, [4, 0], [0, 0], 0), lambda: s.submit_woven(0, [0, 0], [0, -1], 0), lambda: s.submit_woven(1, [0, 0], [0, 0], 0),
                     lambda: s.submit_woven(0, [0, 0], [0, 0], 2), lambda: s.store_telecine(0, 5), lambda: s.store_telecine(0, 0), lambda: s.store_put(0, 3, 2)):
            with pytest.raises(av1mi.Av1miError):
                call()
    finally:
        s.close()


def test_refusals_at_open_and_without_the_option(ctx, av1mi):
    def refused(why, **kw):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, 64, 48, 10, Q, GOP, SEGS, gpu_entropy=1, **kw).close()
        assert e.value.code == -1 and why in str(e.value), (why, str(e.value))
    refused("telecine 2 unknown", telecine=2, store_frames=5)
    refused("telecine 1 needs a frame store", telecine=1)
    refused("telecine 1 together with deinterlace 1", telecine=1, store_frames=5, deinterlace=1)
    refused("telecine 1 together with denoise 4", telecine=1, store_frames=5, denoise=4)
    refused("telecine 1 needs input_format 0", telecine=1, store_frames=5, input_format=av1mi.INPUT_PACKED10)
    s = av1mi.GopSession(ctx, 64, 48, 8, Q, GOP, SEGS, gpu_entropy=1, store_frames=4, telecine=0)
    try:
        for call in (lambda: s.store_telecine(0, 1), lambda: s.submit_woven(0, [0, 0], [0, 0], 0)):
            with pytest.raises(av1mi.Av1miError) as e:
                call()
            assert "telecine 0" in str(e.value)
        with pytest.raises(av1mi.Av1miError):      # the store holds store_frames frames and no more
            s.input_planes()
            s.store_put(0, 4, 1)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- the job
def _write_y4m(path, planes, w, h, bd, tag):
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30000:1001 I%s A1:1 C%s\n" % (w, h, tag, "420jpeg" if bd == 8 else "420p10")).encode())
        for t in range(planes[0].shape[0]):
            f.write(b"FRAME\n")
            for p, (pw, ph) in enumerate(((w, h), ((w + 1) // 2, (h + 1) // 2), ((w + 1) // 2, (h + 1) // 2))):
                f.write(np.ascontiguousarray(planes[p][t][:ph, :pw]).astype("<u2" if bd == 10 else np.uint8).tobytes())


def _ivf(data):
    assert data[:4] == b"DKIF"
    n, pos, out = struct.unpack_from("<I", data, 24)[0], 32, []
    while pos < len(data):
        size = struct.unpack_from("<I", data, pos)[0]
        out.append(data[pos + 12:pos + 12 + size])
        pos += 12 + size
    assert len(out) == n
    return struct.unpack_from("<II", data, 16), out


@pytest.mark.parametrize("bd, tag", [(8, "m"), (10, "t")])
def test_the_job_over_two_groups(tmp_path, bd, tag):
    """23 source frames, -g 4 x 2 segments: groups of 10 source frames (8 outputs), 10 and 3 (a tail: 3 outputs); the second and third
    group see a context frame in front, the first and second one behind"""
    import av1stream
    import dav1d_ref as D
    w, h, n = 64, 48, 23
    video = _video("bff", 3, n, w, h, bd)
    _write_y4m(tmp_path / "tc.y4m", video, w, h, bd, tag)
    code, err = av1stream.run_transcode(["-i", tmp_path / "tc.y4m", "-global_quality:v:0", Q, "-g", GOP, "-av1mi_segments", SEGS, "-av1mi_ivtc", 1,
                                         "-av1mi_stats", tmp_path / "tc.stats", tmp_path / "tc.ivf"])
    assert code == 0, err
    per, rate, frames, ratio = av1stream.job_output_ratio(["-i", "x.y4m", "-g", GOP, "-av1mi_ivtc", 1, "out.ivf"], tag, (30000, 1001), n)
    assert (rate, frames, ratio) == ((24000, 1001), 19, (4, 5))
    got_rate, units = _ivf((tmp_path / "tc.ivf").read_bytes())
    assert got_rate == rate and len(units) == frames
    top, bottom = T.plan(T.records(video[0], bd, w, h))
    lines = [ln for ln in (tmp_path / "tc.stats").read_text().splitlines() if ln.startswith("n:")]
    pairs = [tuple(int(v) for v in [tok for tok in ln.split() if tok.startswith("ivtc:")][0][5:].split("/")) for ln in lines]
    assert pairs == list(zip(top.tolist(), bottom.tolist()))
    assert D.available(), "dav1d is what this part is about"
    assert len(D.decode(b"".join(units))) == frames
    # a stream gives the file's bytes: every source frame is read once and in order, so a FIFO feeds the job like a file
    import os
    import threading
    fifo = tmp_path / "tc.fifo"
    os.mkfifo(fifo)
    writer = threading.Thread(target=lambda: open(fifo, "wb").write((tmp_path / "tc.y4m").read_bytes()))
    writer.start()
    code, err = av1stream.run_transcode(["-i", fifo, "-global_quality:v:0", Q, "-g", GOP, "-av1mi_segments", SEGS, "-av1mi_ivtc", 1,
                                         "-av1mi_stats", tmp_path / "fifo.stats", tmp_path / "fifo.ivf"])
    writer.join()
    assert code == 0, err
    assert (tmp_path / "fifo.ivf").read_bytes() == (tmp_path / "tc.ivf").read_bytes() and (tmp_path / "fifo.stats").read_text() == (tmp_path / "tc.stats").read_text()
    # a container that carries timecodes takes the same rate
    code, err = av1stream.run_transcode(["-i", tmp_path / "tc.y4m", "-global_quality:v:0", Q, "-g", GOP, "-av1mi_segments", SEGS, "-av1mi_ivtc", 1, tmp_path / "tc.mkv"])
    assert code == 0, err
    mkv = (tmp_path / "tc.mkv").read_bytes()
    at = mkv.index(b"\x23\xE3\x83")
    assert abs(int.from_bytes(mkv[at + 4:at + 4 + (mkv[at + 3] & 0x7F)], "big") - 1e9 * 1001 / 24000) < 1      # DefaultDuration in ns: 1001 / 24000 s, rounded either way
