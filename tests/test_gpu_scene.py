"""GPU tests of the scene-cut option (av1mi_gop_config.store_frames, -av1mi_scenecut): the analysis kernels against tests/scene_ref.py bit
for bit, the gather, a session fed from its frame store against an ordinary one, and the product putting its key frames on the cuts."""
import struct

import numpy as np
import pytest

import scene_clips as K
import scene_ref as R

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- analysis
def _run(kind, w, h, n, bd, seed):
    rng = np.random.default_rng(seed)
    hi = 1 << bd
    if kind == "random":           # independent noise: flat quarter planes, so the minimum SAD is often reached by several displacements
        return rng.integers(0, hi, (n, h, w)).astype(np.uint16)
    if kind == "identical":        # inter must come out 0
        return np.repeat(rng.integers(0, hi, (1, h, w)), n, axis=0).astype(np.uint16)
    if kind == "coarse":           # 32x32 patches of few levels: ties between displacements inside a patch, large SADs at its edges
        a = rng.integers(0, 4, (n, (h + 31) // 32, (w + 31) // 32)) * (hi // 4)
        return np.repeat(np.repeat(a, 32, axis=1), 32, axis=2)[:, :h, :w].astype(np.uint16)
    Y = K.cut_clip(w, h, n, bd, (n // 2,))[0]      # moving texture with a cut in the middle
    return Y.astype(np.uint16)


@pytest.mark.parametrize("size", [(64, 64), (72, 40), (136, 72)])
@pytest.mark.parametrize("bd", [8, 10])
def test_scene_analyse_is_the_reference(ctx, av1mi, size, bd):
    w, h = size
    for i, (kind, n) in enumerate((("random", 3), ("identical", 3), ("coarse", 4), ("clip", 5))):
        Y = _run(kind, w, h, n, bd, 100 * bd + i)
        want = R.records(Y, bd)
        got = ctx.scene_analyse(Y, bd)
        assert got.tobytes() == want.astype(av1mi.SCENE_DTYPE).tobytes(), "%s %dx%d %d bit: got %s, want %s" % (kind, w, h, bd, got, want)
        assert got["inter_sad"][0] == 0 and (got["blocks"] == ((w + 31) // 32) * ((h + 31) // 32)).all()
        if kind == "identical":
            assert (got["inter_sad"] == 0).all() and (got["intra_sad"] > 0).all()
    assert ctx.scene_analyse(Y, bd).tobytes() == got.tobytes()      # the same bytes every time


def test_scene_analyse_covers_a_row_of_several_runs_and_twelve_bits(ctx, av1mi):
    """a plane wider than one workgroup's run of blocks (48 blocks = 1536 luma samples), and the 12-bit view"""
    rng = np.random.default_rng(5)
    Y = rng.integers(0, 256, (2, 40, 1640)).astype(np.uint16)
    assert ctx.scene_analyse(Y, 8).tobytes() == R.records(Y, 8).astype(av1mi.SCENE_DTYPE).tobytes()
    Y = rng.integers(0, 4096, (3, 40, 72)).astype(np.uint16)
    assert ctx.scene_analyse(Y, 12).tobytes() == R.records(Y, 12).astype(av1mi.SCENE_DTYPE).tobytes()


def test_scene_analyse_refuses_bad_arguments(ctx, av1mi):
    for shape, bd in (((2, 36, 64), 8), ((2, 64, 60), 8), ((2, 64, 64), 9)):
        with pytest.raises(av1mi.Av1miError):
            ctx.scene_analyse(np.zeros(shape, np.uint16), bd)


# ---------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("case", [(8, 8, 8), (72, 40, 8), (72, 40, 10), (8, 8, 10)])
def test_frames_gather(ctx, av1mi, case):
    w, h, bd = case
    bps, S, N = (1 if bd == 8 else 2), 3, 5
    rng = np.random.default_rng(w + bd)
    nbytes = [w * h * bps, w * h * bps // 4, w * h * bps // 4]
    store = [rng.integers(0, 256, (N, b), dtype=np.uint8) for b in nbytes]
    d_store = [ctx.to_device(a) for a in store]
    index = [4, -1, 1]
    table = np.array([[d_store[p].ptr + index[s] * nbytes[p] if index[s] >= 0 else 0 for p in range(3)] for s in range(S)], np.uint64)
    d_table = ctx.to_device(table)
    guard = 64       # bytes behind every destination that must stay untouched
    d_dst = [ctx.to_device(np.full(S * b + guard, 0xA5, np.uint8)) for b in nbytes]
    ctx.frames_gather(nbytes, S, d_table, d_dst)
    for p in range(3):
        got = d_dst[p].download((S * nbytes[p] + guard,), np.uint8)
        for s in range(S):
            want = store[p][index[s]] if index[s] >= 0 else np.zeros(nbytes[p], np.uint8)
            assert (got[s * nbytes[p]:(s + 1) * nbytes[p]] == want).all(), "plane %d segment %d" % (p, s)
        assert (got[S * nbytes[p]:] == 0xA5).all(), "plane %d: written beyond its end" % p
    for b in d_store + d_dst + [d_table]:
        b.free()


def test_frames_gather_planes_that_are_not_whole_units_and_absent_planes(ctx, av1mi):
    """a plane of 40 bytes moves in single dwords; a plane of 0 bytes (a grey source's chroma) is not touched"""
    rng = np.random.default_rng(9)
    S, nbytes = 3, [40, 0, 8200]
    store = [rng.integers(0, 256, (2, max(b, 1)), dtype=np.uint8) for b in nbytes]
    d_store = [ctx.to_device(np.ascontiguousarray(a[:, :b]) if b else a) for a, b in zip(store, nbytes)]
    index = [1, 0, -1]
    # (sources of a plane that is not whole units are 4-byte aligned only: frame 1 of the 40-byte plane starts at byte 40)
    table = np.array([[d_store[p].ptr + index[s] * nbytes[p] if index[s] >= 0 and nbytes[p] else 0 for p in range(3)] for s in range(S)], np.uint64)
    d_table = ctx.to_device(table)
    d_dst = [ctx.to_device(np.full(S * b + 64, 0x5A, np.uint8)) for b in nbytes]
    ctx.frames_gather(nbytes, S, d_table, d_dst)
    for p in (0, 2):
        got = d_dst[p].download((S * nbytes[p] + 64,), np.uint8)
        for s in range(S):
            want = store[p][index[s], :nbytes[p]] if index[s] >= 0 else np.zeros(nbytes[p], np.uint8)
            assert (got[s * nbytes[p]:(s + 1) * nbytes[p]] == want).all()
        assert (got[S * nbytes[p]:] == 0x5A).all()
    assert (d_dst[1].download((64,), np.uint8) == 0x5A).all()
    for b in d_store + d_dst + [d_table]:
        b.free()


# ---------------------------------------------------------------------------------------------- session
W, H, BD, Q, S, G = 192, 128, 8, 110, 3, 4


@pytest.fixture(scope="module")
def clip():
    import synth
    return synth.frames(W, H, S * G, BD, 3)


def _stacked(clip, frames):
    """the planes of a batch: `frames` (a clip position per segment, None = zeros) stacked"""
    return [np.concatenate([a[f] if f is not None else np.zeros_like(a[0]) for f in frames]) for a in clip]


def _collect(av1stream, s, fr, exists, streams):
    for sg in range(S):
        if exists[sg]:
            streams[sg] += av1stream.session_frame_unit_gpu(W, H, BD, fr, sg)


def _fill_store(s, clip, store):
    for f0 in range(0, S * G, S):
        for dst, a in zip(s.input_planes(), _stacked(clip, range(f0, f0 + S))):
            dst[:] = a
        s.store_put(store, f0, S)


def test_stored_session_identity_layout_gives_the_ordinary_sessions_bytes(ctx, av1mi, clip):
    import av1stream
    out = {}
    for stored in (False, True):
        s = av1mi.GopSession(ctx, W, H, BD, Q, G, S, gpu_entropy=1, store_frames=S * G if stored else 0)
        got = []
        try:
            if stored:
                _fill_store(s, clip, 1)
                recs = s.store_analyse(1, S * G)
                assert recs.tobytes() == R.records(clip[0], BD).astype(av1mi.SCENE_DTYPE).tobytes()
                with pytest.raises(av1mi.Av1miError):
                    s.submit()
            for t in range(G):
                if stored:
                    s.submit_stored(1, [sg * G + t for sg in range(S)], 0 if t == 0 else 1)
                else:
                    for dst, a in zip(s.input_planes(), _stacked(clip, [sg * G + t for sg in range(S)])):
                        dst[:] = a
                    s.submit()
                fr = s.collect()
                got.append((fr["tile_size"].copy(), fr["tile_payload"].copy(), fr["lr_on"].copy(), fr["frame_type"]))
            assert s.entropy_fallbacks() == 0
        finally:
            s.close()
        out[stored] = got
    for t in range(G):
        for a, b in zip(out[False][t][:3], out[True][t][:3]):
            assert a.tobytes() == b.tobytes(), "batch %d: the stored session codes other bytes" % t
        assert out[False][t][3] == out[True][t][3]


def test_stored_session_with_a_shifted_boundary_decodes_to_its_references(ctx, av1mi, clip):
    """GOPs of 3, 5 and 4 frames (a GOP longer than gop_length), flat slots where a GOP has ended; the second group reuses store 0 while
    nothing waits on the host"""
    import av1stream
    import dav1d_ref as D
    start, ln = [0, 3, 8], [3, 5, 4]
    s = av1mi.GopSession(ctx, W, H, BD, Q, G, S, gpu_entropy=1, store_frames=S * G)
    streams, refs = [b""] * S, []
    try:
        _fill_store(s, clip, 0)
        for t in range(max(ln)):
            exists = [t < ln[sg] for sg in range(S)]
            s.submit_stored(0, [start[sg] + t if exists[sg] else -1 for sg in range(S)], 0 if t == 0 else 1)
            if t == 1:
                _fill_store(s, clip, 1)          # the other store is filled while batches of this one are in flight
            if t == 2:
                _fill_store(s, clip, 0)          # the same frames again into the store in use: ordered behind its readers by events
            fr = s.collect()
            _collect(av1stream, s, fr, exists, streams)
            refs.append(s.download_reference())
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    if D.available():
        for sg in range(S):
            got = D.decode(streams[sg])
            assert len(got) == ln[sg]
            for t in range(ln[sg]):
                for i, d in enumerate((1, 2, 2)):
                    rows = H // d
                    assert (got[t][i] == refs[t][i][sg * rows:(sg + 1) * rows]).all(), "segment %d frame %d plane %d: dav1d decodes another picture" % (sg, t, i)


def test_store_argument_rules(ctx, av1mi):
    with pytest.raises(av1mi.Av1miError):
        av1mi.GopSession(ctx, W, H, 10, Q, G, S, input_format=av1mi.INPUT_PACKED10, store_frames=4)
    s = av1mi.GopSession(ctx, W, H, BD, Q, G, S)
    try:
        for call in (lambda: s.store_put(0, 0, 1), lambda: s.store_analyse(0, 1), lambda: s.submit_stored(0, [0] * S, 0)):
            with pytest.raises(av1mi.Av1miError):
                call()
    finally:
        s.close()
    s = av1mi.GopSession(ctx, W, H, BD, Q, G, S, store_frames=6)
    try:
        s.input_planes()
        for call in (lambda: s.store_put(2, 0, 1), lambda: s.store_put(0, 4, 3), lambda: s.store_put(0, 0, S + 1), lambda: s.submit_stored(0, [0] * S, 0),
                     lambda: s.store_analyse(0, 7)):
            with pytest.raises(av1mi.Av1miError):
                call()
        s.store_put(0, 0, 3)
        for call in (lambda: s.submit_stored(0, [0, 6, 1], 0), lambda: s.submit_stored(0, [0, 1, 2], -1), lambda: s.submit_stored(1, [0, 1, 2], 0)):
            with pytest.raises(av1mi.Av1miError):
                call()
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- product
def _ivf_units(data):
    assert data[:4] == b"DKIF"
    n, pos, out = struct.unpack_from("<I", data, 24)[0], 32, []
    while pos < len(data):
        size = struct.unpack_from("<I", data, pos)[0]
        out.append(data[pos + 12:pos + 12 + size])
        pos += 12 + size
    assert len(out) == n
    return out


def test_transcode_puts_the_key_frames_on_the_cuts(tmp_path):
    import av1stream
    import dav1d_ref as D
    c = K.DEFAULT_CLIPS
    n, cuts = c["cut"]["n"], list(c["cut"]["cuts"])
    K.write_y4m(tmp_path / "cuts.y4m", K.cut_clip(c["w"], c["h"], n, 8, cuts), 8)
    size, keys, flagged = {}, {}, {}
    for name, extra in (("absent", []), ("zero", ["-av1mi_scenecut", 0]), ("on", ["-av1mi_scenecut", av1stream.SCENECUT_DEFAULT])):
        out, stats = tmp_path / (name + ".ivf"), tmp_path / (name + ".stats")
        code, err = av1stream.run_transcode(["-i", tmp_path / "cuts.y4m", "-global_quality:v:0", 110, "-g", 8, "-av1mi_segments", 3, "-av1mi_stats", stats] + extra + [out])
        assert code == 0, err
        per = [dict(kv.split(":") for kv in ln.split()) for ln in stats.read_text().splitlines()[:-1]]
        assert [int(d["n"]) for d in per] == list(range(n))
        keys[name] = [int(d["n"]) for d in per if d["type"] == "K"]
        flagged[name] = [int(d["n"]) for d in per if d.get("cut") == "1"]
        size[name] = out.stat().st_size
        if D.available():
            assert len(D.decode(b"".join(_ivf_units(out.read_bytes())))) == n
    print("bytes: option absent %d, at 0 %d, at the default %d" % (size["absent"], size["zero"], size["on"]))
    assert (tmp_path / "absent.ivf").read_bytes() == (tmp_path / "zero.ivf").read_bytes()
    assert keys["absent"] == keys["zero"] == [0, 8, 16] and flagged["absent"] == flagged["zero"] == []
    assert keys["on"] == [0] + cuts and flagged["on"] == cuts
    assert size["on"] < size["absent"]
