"""GPU tests of field-rate deinterlacing (av1mi_deinterlace_gather_fields, av1mi_gop_config.deinterlace_fields,
-av1mi_deinterlace_rate field): the field-rate instantiation of k_deint_gather against tests/deinterlace_fields_ref.py bit for bit, a
session whose stored batches take output positions, and the product on interlaced and progressive sources."""
import struct

import numpy as np
import pytest

import deint_clips as K
import deinterlace_fields_ref as F

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- kernel
def _tables(ctx, planes, index, bd):
    """the store's run on the device, and the table / phase arrays of a launch whose segment s shows OUTPUT position index[s] (-1 = a
    flat slot): P, C, N follow the source frame index[s] >> 1, clamped at the run's ends"""
    n = planes[0].shape[0]
    dt = np.uint8 if bd == 8 else np.uint16
    planes = [np.ascontiguousarray(a, dt) for a in planes]
    nbytes = [a[0].nbytes for a in planes]
    d_store = [ctx.to_device(a) for a in planes]
    pos = lambda o: (max((o >> 1) - 1, 0), o >> 1, min((o >> 1) + 1, n - 1))
    table = np.array([[[d_store[p].ptr + q * nbytes[p] if o >= 0 else 0 for q in pos(o)] for p in range(len(planes))] for o in index], np.uint64)
    phase = np.array([o & 1 if o >= 0 else 0 for o in index], np.uint8)
    return planes, nbytes, d_store, table, phase


def _fields_against_reference(ctx, planes, sizes, true_sizes, bd, k, index, junk_phase_bits=False):
    """checks every destination plane against the reference's 2 n outputs, and that nothing beyond it is written"""
    S = len(index)
    planes, nbytes, d_store, table, phase = _tables(ctx, planes, index, bd)
    if junk_phase_bits:
        phase = phase | np.uint8(0xA4)      # only the low bit is read
    dt = planes[0].dtype
    d_table, d_phase = ctx.to_device(table), ctx.to_device(phase)
    guard = 64
    d_dst = [ctx.to_device(np.full(S * b + guard, 0xA5, np.uint8)) for b in nbytes]
    try:
        ctx.deinterlace_gather_fields(bd, sizes, true_sizes, k, S, d_table, d_phase, d_dst)
        for p in range(3):
            want = F.fields(planes[p], true_sizes[p][0], true_sizes[p][1], k)
            raw = d_dst[p].download((S * nbytes[p] + guard,), np.uint8)
            assert (raw[S * nbytes[p]:] == 0xA5).all(), "plane %d: written beyond its end" % p
            got = raw[:S * nbytes[p]].view(dt).reshape((S,) + planes[p].shape[1:])
            for s, o in enumerate(index):
                w = want[o] if o >= 0 else np.zeros_like(want[0])
                bad = np.argwhere(got[s] != w)
                assert bad.size == 0, "plane %d segment %d (output %d): %d samples differ, the first at (y, x) = %s" % (p, s, o, len(bad), bad[0])
    finally:
        for b in d_store + d_dst + [d_table, d_phase]:
            b.free()


def _sizes(name):
    c = K.CASES[name]
    (w, h), (sx, sy) = c["size"], c["chroma"]
    return [(w, h), (w >> sx, h >> sy), (w >> sx, h >> sy)]


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("name", list(K.CASES))
def test_field_rate_gather_is_the_reference(ctx, name, bd, k):
    """launches that mix phases (0, 1, 1 and more), one of them with a flat slot; together they show every output of the run of 3"""
    planes = K.case_clip(name, bd, k)
    _fields_against_reference(ctx, planes, _sizes(name), K.case_true_sizes(name), bd, k, [0, 3, 5])            # phases 0, 1, 1
    _fields_against_reference(ctx, planes, _sizes(name), K.case_true_sizes(name), bd, k, [4, -1, 1, 2], junk_phase_bits=True)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("bd", [8, 10])
def test_field_rate_gather_short_runs(ctx, n, bd):
    """runs of one and two frames of the smallest plane: a frame is its own neighbour at the ends of a run, in both phases"""
    for k in (0, 1):
        planes = K.case_clip("8x8", bd, k, n=n)
        _fields_against_reference(ctx, planes, _sizes("8x8"), K.case_true_sizes("8x8"), bd, k, list(range(2 * n - 1, -1, -1)) + [1])


def test_field_rate_gather_twelve_bits_a_grey_source_and_one_line(ctx):
    """uint16 samples up to 4095; a layout without chroma planes; a plane of true height 1 is copied in both phases"""
    Y = (K.pan_plane(40, 24, 3, 10, 0, 9).astype(np.uint16) << 2) | 3
    index = [3, 4, 5]
    _, nb, d_store, table, phase = _tables(ctx, [Y], index, 12)
    full = np.zeros((3, 3, 3), np.uint64)
    full[:, 0] = table[:, 0]
    d_table, d_phase, d_dst = ctx.to_device(full), ctx.to_device(phase), ctx.to_device(np.zeros(3 * nb[0], np.uint8))
    ctx.deinterlace_gather_fields(12, [(40, 24), (0, 0), (0, 0)], [(40, 24), (1, 1), (1, 1)], 1, 3, d_table, d_phase, [d_dst, None, None])
    got = d_dst.download((3, 24, 40), np.uint16)
    assert (got == F.fields(Y, 40, 24, 1)[3:6]).all()
    for b in d_store + [d_table, d_phase, d_dst]:
        b.free()
    line = K.pan_plane(40, 8, 2, 8, 0, 2)
    want = np.repeat(np.repeat(line[:, :1, :], 8, axis=1), 2, axis=0)
    assert (F.fields(line, 40, 1, 0) == want).all()
    _fields_against_reference(ctx, [line, line[:, :4, :20].copy(), line[:, :4, :20].copy()], [(40, 8), (20, 4), (20, 4)], [(40, 1), (20, 1), (20, 1)], 8, 0, [3, 0, 2])


@pytest.mark.parametrize("bd", [8, 10])
def test_all_phases_zero_write_what_the_same_rate_gather_writes(ctx, bd):
    for name in ("38x22", "1040x8"):
        index = [4, -1, 0, 2]
        planes, nbytes, d_store, table, phase = _tables(ctx, K.case_clip(name, bd, 1), index, bd)
        assert not phase.any()
        d_table, d_phase = ctx.to_device(table), ctx.to_device(phase)
        S = len(index)
        d_a = [ctx.to_device(np.full(S * b, 0x11, np.uint8)) for b in nbytes]
        d_b = [ctx.to_device(np.full(S * b, 0x22, np.uint8)) for b in nbytes]
        ctx.deinterlace_gather(bd, _sizes(name), K.case_true_sizes(name), 1, S, d_table, d_a)
        ctx.deinterlace_gather_fields(bd, _sizes(name), K.case_true_sizes(name), 1, S, d_table, d_phase, d_b)
        for a, b, nb in zip(d_a, d_b, nbytes):
            assert (a.download((S * nb,), np.uint8) == b.download((S * nb,), np.uint8)).all(), name
        for b in d_store + d_a + d_b + [d_table, d_phase]:
            b.free()


def test_field_rate_gather_refuses_bad_arguments(ctx, av1mi):
    d = ctx.to_device(np.zeros(4096, np.uint8))
    ok = dict(bit_depth=8, plane_sizes=[(8, 8), (4, 4), (4, 4)], true_sizes=[(8, 8), (4, 4), (4, 4)], parity=0, segments=1, d_table=d, d_phase=d, d_dst=[d, d, d])
    ctx.deinterlace_gather_fields(**ok)      # (a table of zeros: flat slots)
    for bad in (dict(bit_depth=9), dict(parity=2), dict(segments=0), dict(d_phase=None), dict(true_sizes=[(9, 8), (4, 4), (4, 4)]), dict(true_sizes=[(8, 0), (4, 4), (4, 4)]),
                dict(plane_sizes=[(16, 8), (4, 4), (4, 4)]), dict(plane_sizes=[(8, 8), (6, 4), (4, 4)], true_sizes=[(8, 8), (6, 4), (4, 4)])):
        with pytest.raises(av1mi.Av1miError) as e:
            ctx.deinterlace_gather_fields(**dict(ok, **bad))
        assert "av1mi_deinterlace_gather_fields" in str(e.value)
    ctx.sync()
    d.free()


# ---------------------------------------------------------------------------------------------- session
W, H, BD, Q, S, G = 192, 128, 8, 110, 3, 4      # tests/test_gpu_deinterlace.py's


def test_session_takes_output_positions(ctx, av1mi):
    clip = K.pan_clip(W, H, 3, BD, 0)
    want = [F.fields(a, a.shape[2], a.shape[1], 0) for a in clip]
    s = av1mi.GopSession(ctx, W, H, BD, Q, G, S, gpu_entropy=1, store_frames=3, deinterlace=1, deinterlace_fields=1)
    try:
        for dst, a in zip(s.input_planes(), clip):
            dst[:] = a.reshape(dst.shape)
        s.store_put(0, 0, 3)
        for index in ([0, 3, 5], [1, -1, 4]):
            s.submit_stored(0, index, 0)
            for p, got in enumerate(s.download_fed()):
                w = np.concatenate([want[p][o] if o >= 0 else np.zeros_like(want[p][0]) for o in index])
                assert (got == w).all(), "index %s plane %d: the fed buffer is not the reference's output" % (index, p)
            s.collect()
        for index in ([0, 6, 1], [0, 1, -2]):
            with pytest.raises(av1mi.Av1miError):
                s.submit_stored(0, index, 0)      # beyond the 6 output positions of 3 stored frames
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    s = av1mi.GopSession(ctx, W, H, BD, Q, G, S, store_frames=6, deinterlace=2, deinterlace_fields=1)
    try:
        s.input_planes()
        s.store_put(0, 0, 2)
        s.submit_stored(0, [3, 0, -1], 0)
        s.collect()
        with pytest.raises(av1mi.Av1miError):
            s.submit_stored(0, [0, 1, 4], 0)      # inside the store's 12 positions, beyond the run of 2 frames
    finally:
        s.close()


def test_session_argument_rules(ctx, av1mi):
    for kw in (dict(deinterlace_fields=1), dict(deinterlace_fields=1, store_frames=4), dict(deinterlace_fields=2, store_frames=4, deinterlace=1),
               dict(deinterlace_fields=-1, store_frames=4, deinterlace=1)):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, W, H, BD, Q, G, S, **kw)
        assert "deinterlace_fields" in str(e.value)


def test_a_session_with_the_field_zero_is_the_session_without_it(ctx, av1mi):
    clip = K.pan_clip(W, H, S, BD, 0)
    got = []
    for kw in (dict(), dict(deinterlace_fields=0)):
        s = av1mi.GopSession(ctx, W, H, BD, Q, G, S, gpu_entropy=1, store_frames=S, deinterlace=1, **kw)
        try:
            for dst, a in zip(s.input_planes(), clip):
                dst[:] = a.reshape(dst.shape)
            s.store_put(0, 0, S)
            frames = []
            for t, index in enumerate(([0, 1, 2], [2, -1, 1])):
                s.submit_stored(0, index, t)
                fr = s.collect()
                frames.append({k: v.copy() for k, v in fr.items() if isinstance(v, np.ndarray)})
            with pytest.raises(av1mi.Av1miError):
                s.submit_stored(0, [0, 1, 3], 0)      # a store position, not an output position
            got.append(frames)
        finally:
            s.close()
    for a, b in zip(*got):
        assert a.keys() == b.keys() and len(a) > 0
        for key in a:
            assert a[key].shape == b[key].shape and (a[key] == b[key]).all(), key


# ---------------------------------------------------------------------------------------------- product
N = 16      # source frames: groups of 6, 6 and 4 (12, 12 and 8 output frames): both stores, three runs


def _ivf_units(data):
    assert data[:4] == b"DKIF"
    n, pos, out = struct.unpack_from("<I", data, 24)[0], 32, []
    while pos < len(data):
        size = struct.unpack_from("<I", data, pos)[0]
        out.append(data[pos + 12:pos + 12 + size])
        pos += 12 + size
    assert len(out) == n
    return out


def _default_duration(mkv):
    """the video track's DefaultDuration (element 0x23E383) in ns"""
    at = mkv.index(b"\x23\xE3\x83")
    size = mkv[at + 3] & 0x7F
    return int.from_bytes(mkv[at + 4:at + 4 + size], "big")


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """every transcode of the product tests, run once: name -> (exit code, error text, output bytes)"""
    import av1stream
    d = tmp_path_factory.mktemp("deint_fields")
    src = K.pan_clip(W, H, N, BD, 0)
    K.write_y4m(d / "it.y4m", src, BD, interlace="t")
    run = S * G // 2      # the job's groups: S G output frames = S G / 2 source frames
    ref = [np.concatenate([F.fields(a[g0:g0 + run], a.shape[2], a.shape[1], 0) for g0 in range(0, N, run)]) for a in src]
    assert ref[0].shape[0] == 2 * N
    K.write_y4m(d / "ref_fp.y4m", ref, BD, interlace="p", fps=60)      # the reference's 2 N frames, progressive, at twice the rate
    auto, field = ["-av1mi_deinterlace", "auto"], ["-av1mi_deinterlace_rate", "field"]
    runs = dict(A=("it.y4m", auto + field, "ivf"), B=("ref_fp.y4m", [], "ivf"),
                mkv_field=("it.y4m", auto + field, "mkv"), mkv_frame=("it.y4m", auto, "mkv"),
                frame=("it.y4m", auto + ["-av1mi_deinterlace_rate", "frame"], "ivf"), frame_absent=("it.y4m", auto, "ivf"),
                off=("it.y4m", ["-av1mi_deinterlace", "off"] + field, "ivf"), absent=("it.y4m", [], "ivf"),
                ip_auto_field=("ref_fp.y4m", auto + field, "ivf"), ip_auto=("ref_fp.y4m", auto, "ivf"),
                cuts=("it.y4m", auto + field + ["-av1mi_scenecut", 15, "-av1mi_stats", d / "cuts.stats"], "ivf"),
                rate=("it.y4m", auto + field + ["-b:v:0", "400k"], "ivf"),
                odd=("it.y4m", auto + field + ["-g", 5], "ivf"))
    out = {}
    for name, (source, extra, ext) in runs.items():
        path = d / (name + "." + ext)
        code, err = av1stream.run_transcode(["-i", d / source, "-global_quality:v:0", Q, "-g", G, "-av1mi_segments", S] + extra + [path])
        out[name] = (code, err, path.read_bytes() if code == 0 else b"")
    out["cuts.stats"] = (d / "cuts.stats").read_text() if out["cuts"][0] == 0 else ""
    return out


def test_field_rate_transcode_equals_the_reference_fields_coded_at_twice_the_rate(outputs):
    import dav1d_ref as D
    for name in ("A", "B"):
        assert outputs[name][0] == 0, outputs[name][1]
    assert outputs["A"][2] == outputs["B"][2]
    units = _ivf_units(outputs["A"][2])
    assert len(units) == 2 * N
    assert struct.unpack_from("<II", outputs["A"][2], 16) == (60, 1)
    if D.available():
        assert len(D.decode(b"".join(units))) == 2 * N


def test_matroska_frames_last_half_as_long(outputs):
    for name in ("mkv_field", "mkv_frame"):
        assert outputs[name][0] == 0, outputs[name][1]
    frame, field = _default_duration(outputs["mkv_frame"][2]), _default_duration(outputs["mkv_field"][2])
    assert frame == 33333333 and abs(2 * field - frame) <= 1, (frame, field)


def test_frame_rate_off_and_progressive_sources_take_todays_path(outputs):
    for name in ("frame", "frame_absent", "off", "absent", "ip_auto_field", "ip_auto"):
        assert outputs[name][0] == 0, outputs[name][1]
    assert outputs["frame"][2] == outputs["frame_absent"][2] and len(_ivf_units(outputs["frame"][2])) == N
    assert outputs["off"][2] == outputs["absent"][2]
    assert outputs["ip_auto_field"][2] == outputs["ip_auto"][2] == outputs["B"][2]
    assert outputs["frame"][2] != outputs["absent"][2]


def test_scene_cuts_a_target_and_an_odd_gop(outputs):
    assert outputs["cuts"][0] == 0, outputs["cuts"][1]
    assert len(_ivf_units(outputs["cuts"][2])) == 2 * N
    lines = outputs["cuts.stats"].splitlines()
    assert len(lines) == 2 * N + 1 and lines[-1].startswith("summary frames:%d " % (2 * N))
    per = [dict(kv.split(":") for kv in ln.split()) for ln in lines[:-1]]
    assert [int(p["n"]) for p in per] == list(range(2 * N))
    assert outputs["rate"][0] == 0, outputs["rate"][1]
    assert len(_ivf_units(outputs["rate"][2])) == 2 * N
    code, err, _ = outputs["odd"]
    assert code == 1 and "-g" in err and "even" in err
