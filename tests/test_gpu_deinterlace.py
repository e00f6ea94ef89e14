"""GPU tests of the deinterlacing option (av1mi_gop_config.deinterlace, -av1mi_deinterlace): k_deint_gather against
tests/deinterlace_ref.py bit for bit, a session that gathers through it, and the product on interlaced and progressive sources."""
import numpy as np
import pytest

import deint_clips as K
import deinterlace_ref as R

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- kernel
def _gather_against_reference(ctx, planes, sizes, true_sizes, bd, k, index):
    """planes: [n, H, W] per plane, the store's run; index: the store position per segment (-1 = a flat slot).  Checks every
    destination plane against the reference run, and that nothing beyond it is written."""
    n, S = planes[0].shape[0], len(index)
    dt = np.uint8 if bd == 8 else np.uint16
    planes = [np.ascontiguousarray(a, dt) for a in planes]
    nbytes = [a[0].nbytes for a in planes]
    d_store = [ctx.to_device(a) for a in planes]
    pos = lambda f: (max(f - 1, 0), f, min(f + 1, n - 1))
    table = np.array([[[d_store[p].ptr + q * nbytes[p] if index[s] >= 0 else 0 for q in pos(index[s])] for p in range(3)] for s in range(S)], np.uint64)
    d_table = ctx.to_device(table)
    guard = 64
    d_dst = [ctx.to_device(np.full(S * b + guard, 0xA5, np.uint8)) for b in nbytes]
    try:
        ctx.deinterlace_gather(bd, sizes, true_sizes, k, S, d_table, d_dst)
        for p in range(3):
            want = R.run(planes[p], true_sizes[p][0], true_sizes[p][1], k)
            raw = d_dst[p].download((S * nbytes[p] + guard,), np.uint8)
            assert (raw[S * nbytes[p]:] == 0xA5).all(), "plane %d: written beyond its end" % p
            got = raw[:S * nbytes[p]].view(dt).reshape((S,) + planes[p].shape[1:])
            for s in range(S):
                w = want[index[s]] if index[s] >= 0 else np.zeros_like(want[0])
                bad = np.argwhere(got[s] != w)
                assert bad.size == 0, "plane %d segment %d (position %d): %d samples differ, the first at (y, x) = %s" % (p, s, index[s], len(bad), bad[0])
    finally:
        for b in d_store + d_dst + [d_table]:
            b.free()


def _sizes(name):
    c = K.CASES[name]
    (w, h), (sx, sy) = c["size"], c["chroma"]
    return [(w, h), (w >> sx, h >> sy), (w >> sx, h >> sy)]


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("name", list(K.CASES))
def test_deinterlace_gather_is_the_reference(ctx, name, bd, k):
    """three segments that pick the run's positions out of order, one of them a flat slot: P and N follow the position"""
    planes = K.case_clip(name, bd, k)
    n = planes[0].shape[0]
    _gather_against_reference(ctx, planes, _sizes(name), K.case_true_sizes(name), bd, k, [n - 1, -1, 0])
    _gather_against_reference(ctx, planes, _sizes(name), K.case_true_sizes(name), bd, k, [1, 2, 1, 0])


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("bd", [8, 10])
def test_deinterlace_gather_short_runs(ctx, n, bd):
    """runs of one and two frames of the smallest plane: a frame is its own neighbour at the ends of a run"""
    for k in (0, 1):
        planes = K.case_clip("8x8", bd, k, n=n)
        _gather_against_reference(ctx, planes, _sizes("8x8"), K.case_true_sizes("8x8"), bd, k, [n - 1, 0])
        if n == 1:
            assert all((R.run(a, 8 >> (p > 0), 8 >> (p > 0), k) == a).all() for p, a in enumerate(planes))


def test_deinterlace_gather_twelve_bits_a_grey_source_and_one_line(ctx):
    """uint16 samples up to 4095; a layout without chroma planes; a plane of true height 1 is copied"""
    Y = (K.pan_plane(40, 24, 3, 10, 0, 9).astype(np.uint16) << 2) | 3
    dt_sizes = [(40, 24), (0, 0), (0, 0)]
    n, nb = 3, Y[0].nbytes
    d_y = ctx.to_device(Y)
    table = np.zeros((2, 3, 3), np.uint64)
    for s, f in enumerate((1, 2)):
        table[s, 0] = [d_y.ptr + q * nb for q in (f - 1, f, min(f + 1, n - 1))]
    d_table, d_dst = ctx.to_device(table), ctx.to_device(np.zeros(2 * nb, np.uint8))
    ctx.deinterlace_gather(12, dt_sizes, [(40, 24), (1, 1), (1, 1)], 1, 2, d_table, [d_dst, None, None])
    got = d_dst.download((2, 24, 40), np.uint16)
    assert (got == R.run(Y, 40, 24, 1)[1:3]).all()
    for b in (d_y, d_table, d_dst):
        b.free()
    line = K.pan_plane(40, 8, 2, 8, 0, 2)
    want = np.repeat(line[:, :1, :], 8, axis=1)
    assert (R.run(line, 40, 1, 0) == want).all()
    _gather_against_reference(ctx, [line, line[:, :4, :20].copy(), line[:, :4, :20].copy()], [(40, 8), (20, 4), (20, 4)], [(40, 1), (20, 1), (20, 1)], 8, 0, [1, 0])


def test_deinterlace_gather_refuses_bad_arguments(ctx, av1mi):
    d = ctx.to_device(np.zeros(4096, np.uint8))
    ok = dict(bit_depth=8, plane_sizes=[(8, 8), (4, 4), (4, 4)], true_sizes=[(8, 8), (4, 4), (4, 4)], parity=0, segments=1, d_table=d, d_dst=[d, d, d])
    ctx.deinterlace_gather(**ok)      # (a table of zeros: flat slots)
    for bad in (dict(bit_depth=9), dict(parity=2), dict(segments=0), dict(true_sizes=[(9, 8), (4, 4), (4, 4)]), dict(true_sizes=[(8, 0), (4, 4), (4, 4)]),
                dict(plane_sizes=[(16, 8), (4, 4), (4, 4)]), dict(plane_sizes=[(8, 8), (6, 4), (4, 4)], true_sizes=[(8, 8), (6, 4), (4, 4)])):
        with pytest.raises(av1mi.Av1miError):
            ctx.deinterlace_gather(**dict(ok, **bad))
    ctx.sync()
    d.free()


# ---------------------------------------------------------------------------------------------- session
W, H, BD, Q, S, G = 192, 128, 8, 110, 3, 4


@pytest.fixture(scope="module")
def clip():
    return K.pan_clip(W, H, S * G, BD, 0)


@pytest.fixture(scope="module")
def woven(clip):
    """the reference run over the 12 frames, per plane"""
    return [R.run(a, a.shape[2], a.shape[1], 0) for a in clip]


def test_session_gathers_through_the_deinterlacer(ctx, av1mi, clip, woven):
    import av1stream
    import dav1d_ref as D
    s = av1mi.GopSession(ctx, W, H, BD, Q, G, S, gpu_entropy=1, store_frames=S * G, deinterlace=1)
    streams, refs = [b""] * S, []
    try:
        for f0 in range(0, S * G, S):
            for dst, a in zip(s.input_planes(), clip):
                dst[:] = a[f0:f0 + S].reshape(dst.shape)
            s.store_put(0, f0, S)
        with pytest.raises(av1mi.Av1miError):
            s.submit_stored(1, [0] * S, 0)          # the other store holds nothing
        for t in range(G):
            index = [sg * G + t for sg in range(S)]
            s.submit_stored(0, index, 0 if t == 0 else 1)
            for p, got in enumerate(s.download_fed()):
                want = np.concatenate([woven[p][f] for f in index])
                assert (got == want).all(), "batch %d plane %d: the fed buffer is not the reference's frame" % (t, p)
            fr = s.collect()
            for sg in range(S):
                streams[sg] += av1stream.session_frame_unit_gpu(W, H, BD, fr, sg)
            refs.append(s.download_reference())
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    if D.available():
        for sg in range(S):
            got = D.decode(streams[sg])
            assert len(got) == G
            for t in range(G):
                for i, d in enumerate((1, 2, 2)):
                    rows = H // d
                    assert (got[t][i] == refs[t][i][sg * rows:(sg + 1) * rows]).all(), "segment %d frame %d plane %d: dav1d decodes another picture" % (sg, t, i)


def test_stored_422_session_deinterlaces_converts_and_scales(ctx, av1mi):
    """every source stage behind one store: a 4:2:2 8-bit source of true size 70 x 38 (buffers 72 x 40, the texture goes on into the
    padding) is deinterlaced, converted (its luma plane passes through) and scaled to 48 x 24; 2 segments, 3 batches, all in flight.
    The fed buffers are the reference's frames, and the bytes those of a plain 4:2:0 session at 48 x 24 fed what the numpy
    references make of them"""
    import chroma_formats_ref as CR
    import test_gpu_chroma_formats as TC
    import test_gpu_scale as TS
    tw, th, w, h, segs, gop, q = 70, 38, 48, 24, 2, 3, 110
    clip = K.pan_clip(72, 40, segs * gop, 8, 0, seed=11, chroma=(1, 0))
    true = [(tw, th)] + [CR.true_chroma_size(CR.C422, tw, th)] * 2
    run = [R.run(a, tw_p, th_p, 0) for a, (tw_p, th_p) in zip(clip, true)]
    index = [[sg * gop + t for sg in range(segs)] for t in range(gop)]
    fed = [[np.concatenate([run[p][f] for f in idx]) for p in range(3)] for idx in index]
    table = TS._lib_table(av1mi)
    scaled = []
    for planes in fed:
        y, u, v = CR.convert_stack(CR.C422, 8, 8, tw, th, segs, planes)
        frames = [[y[sg * 40:sg * 40 + th, :tw], u[sg * 20:sg * 20 + 19, :35], v[sg * 20:sg * 20 + 19, :35]] for sg in range(segs)]
        scaled.append(TS._expected(frames, w, h, 8, table))
    base = [{k: v for k, v in o.items() if not k.startswith("ref_")} for o in TC._run(ctx, av1mi, w, h, 8, q, gop, segs, scaled)]
    s = av1mi.GopSession(ctx, w, h, 8, q, gop, segs, gpu_entropy=1, source=(tw, th), source_chroma=CR.C422, store_frames=segs * gop, deinterlace=1)
    got = []
    try:
        for f0 in range(0, segs * gop, segs):
            for dst, a in zip(s.input_planes(), clip):
                dst[:] = a[f0:f0 + segs].reshape(dst.shape)
            s.store_put(0, f0, segs)
        for t in range(gop):
            s.submit_stored(0, index[t], 0 if t == 0 else 1)
            for p, a in enumerate(s.download_fed()):
                assert a.shape == fed[t][p].shape and (a == fed[t][p]).all(), "batch %d plane %d: the fed buffer is not the reference's frame" % (t, p)
        assert s.pending() == gop
        for t in range(gop):
            fr = s.collect()
            got.append({k: v.copy() for k, v in fr.items() if isinstance(v, np.ndarray)})
            got[-1]["frame_type"] = fr["frame_type"]
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    TC._same(base, got, "stored 4:2:2, deinterlaced and scaled")


def test_session_argument_rules(ctx, av1mi):
    for kw in (dict(deinterlace=1), dict(deinterlace=3, store_frames=4), dict(deinterlace=-1, store_frames=4)):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, W, H, BD, Q, G, S, **kw)
        assert "deinterlace" in str(e.value)
    with pytest.raises(av1mi.Av1miError):
        av1mi.GopSession(ctx, W, H, 10, Q, G, S, input_format=av1mi.INPUT_PACKED10, store_frames=4, deinterlace=1)
    s = av1mi.GopSession(ctx, W, H, BD, Q, G, S, store_frames=6, deinterlace=2)
    try:
        s.input_planes()
        s.store_put(0, 0, 3)
        with pytest.raises(av1mi.Av1miError):
            s.submit_stored(0, [0, 1, 3], 0)      # beyond the run of 3 frames
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- product
N = 16      # a group of 12 frames and one of 4: both stores, two runs


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """every transcode of the product tests, run once: name -> (exit code, error text, output bytes)"""
    import av1stream
    d = tmp_path_factory.mktemp("deint")
    src = K.pan_clip(W, H, N, BD, 0)
    K.write_y4m(d / "it.y4m", src, BD, interlace="t")
    K.write_y4m(d / "lies.y4m", src, BD, interlace="p")          # the same interlaced frames under a header that says progressive
    ref = [np.concatenate([R.run(a[g0:g0 + S * G], a.shape[2], a.shape[1], 0) for g0 in range(0, N, S * G)]) for a in src]
    K.write_y4m(d / "ref_ip.y4m", ref, BD, interlace="p")        # deinterlaced by the reference, run = group
    runs = dict(A=("it.y4m", ["-av1mi_deinterlace", "auto"]), B=("ref_ip.y4m", []), off=("it.y4m", ["-av1mi_deinterlace", "off"]), absent=("it.y4m", []),
                ip_auto=("ref_ip.y4m", ["-av1mi_deinterlace", "auto"]), chain=("it.y4m", ["-vf:v:0", "yadif,format=nv12"]),
                chain_field=("it.y4m", ["-vf:v:0", "yadif=mode=1"]), forced=("lies.y4m", ["-av1mi_deinterlace", "tff"]),
                cuts=("it.y4m", ["-av1mi_deinterlace", "auto", "-av1mi_scenecut", 15]))
    out = {}
    for name, (source, extra) in runs.items():
        path = d / (name + ".ivf")
        code, err = av1stream.run_transcode(["-i", d / source, "-global_quality:v:0", Q, "-g", G, "-av1mi_segments", S] + extra + [path])
        out[name] = (code, err, path.read_bytes() if code == 0 else b"")
    return out


def test_transcode_of_an_interlaced_source_equals_the_reference_deinterlaced_one(outputs):
    for name in ("A", "B"):
        assert outputs[name][0] == 0, outputs[name][1]
    assert outputs["A"][2] == outputs["B"][2]
    assert outputs["A"][2] != outputs["absent"][2]


def test_option_off_and_a_progressive_source_under_auto_take_todays_path(outputs):
    for name in ("off", "absent", "ip_auto"):
        assert outputs[name][0] == 0, outputs[name][1]
    assert outputs["off"][2] == outputs["absent"][2]
    assert outputs["ip_auto"][2] == outputs["B"][2]


def test_a_chain_with_yadif_deinterlaces_and_a_field_rate_mode_is_refused(outputs):
    assert outputs["chain"][0] == 0, outputs["chain"][1]
    assert outputs["chain"][2] == outputs["A"][2]
    code, err, _ = outputs["chain_field"]
    assert code == 1 and "yadif=mode=1" in err


def test_a_forced_parity_and_the_scene_analysis_beside_it(outputs):
    assert outputs["forced"][0] == 0, outputs["forced"][1]
    assert outputs["forced"][2] == outputs["A"][2]
    assert outputs["cuts"][0] == 0 and outputs["cuts"][2][:4] == b"DKIF", outputs["cuts"][1]      # the analysis runs on the frames as fed


def test_a_mixed_source_is_refused_under_auto(tmp_path):
    import av1stream
    K.write_y4m(tmp_path / "im.y4m", K.pan_clip(64, 64, 2, 8, 0), 8, interlace="m")
    code, err = av1stream.run_transcode(["-i", tmp_path / "im.y4m", "-av1mi_deinterlace", "auto", tmp_path / "o.ivf"])
    assert code == 1 and "Im" in err
