"""GPU tests of motion-compensated denoising (av1mi_gop_config.denoise_range): k_denoise_search + k_denoise_mc_gather + k_grain_sum against
tests/denoise_mc_ref.py bit for bit, in planes, records and vectors; a session that gathers through them; the transcode job."""
import functools

import numpy as np
import pytest

import denoise_mc_clips as K
import denoise_mc_ref as M
import denoise_ref as R

pytestmark = pytest.mark.gpu

FRAMES = 4


def _layout(w, h, chroma):
    cw, ch = {"420": (w // 2, h // 2), "422": (w // 2, h), "444": (w, h)}[chroma]
    return [(w, h), (cw, ch), (cw, ch)]


# (buffer size, true size, bit depth, chroma layout): one block with every window clamped and chroma rows of 8 bytes in dword form; partial
# blocks right and bottom, the true edge inside the buffer, 16-bit samples; 66 blocks across (more than one workgroup), a half-height block
# row and a partial last cell; chroma blocks without subsampling and with horizontal subsampling only
SHAPES = {"16x16": ((16, 16), (16, 16), 8, "420"), "72x40": ((72, 40), (70, 38), 10, "420"), "1048x24": ((1048, 24), (1048, 24), 8, "420"),
          "48x32-444": ((48, 32), (48, 32), 8, "444"), "48x32-422": ((48, 32), (48, 32), 8, "422")}


@functools.lru_cache(maxsize=None)
def _case(name):
    (W, H), true, bd, chroma = SHAPES[name]
    sizes = _layout(W, H, chroma)
    return sizes, K.true_sizes(sizes, true), bd, K.translating(sizes, FRAMES, bd, 3, 2, true=true)


@functools.lru_cache(maxsize=None)
def _reference(name, strength, rng):
    sizes, true, bd, planes = _case(name)
    return M.run(planes, true, bd, strength, rng)


def _gather_against_reference(ctx, av1mi, planes, sizes, true_sizes, bd, strength, rng, index, want=None, twice=False):
    """planes: [n, H, W] per plane, the store's run; index: the store position per segment (-1 = a flat slot).  Checks every destination
    plane, every record and every vector against the reference run, and that nothing beyond the outputs is written."""
    n, S = planes[0].shape[0], len(index)
    dt = np.uint8 if bd == 8 else np.uint16
    planes = [np.ascontiguousarray(a, dt) for a in planes]
    want_planes, want_recs, want_vec = want if want is not None else M.run(planes, true_sizes, bd, strength, rng)
    nbytes = [a[0].nbytes for a in planes]
    nblk = want_vec.shape[1]
    d_store = [ctx.to_device(a) for a in planes]
    pos = lambda f: (max(f - 1, 0), f, min(f + 1, n - 1))
    table = np.array([[[d_store[p].ptr + q * nbytes[p] if index[s] >= 0 else 0 for q in pos(index[s])] for p in range(3)] for s in range(S)], np.uint64)
    d_table = ctx.to_device(table)
    guard = 64
    d_dst = [ctx.to_device(np.full(S * b + guard, 0xA5, np.uint8)) for b in nbytes]
    rec_bytes = S * 3 * av1mi.GRAIN_BINS * av1mi.GRAIN_DTYPE.itemsize
    d_rec = ctx.to_device(np.full(rec_bytes + guard, 0xA5, np.uint8))
    vec_bytes = S * nblk * av1mi.DENOISE_VEC_DTYPE.itemsize
    d_vec = ctx.to_device(np.full(vec_bytes + guard, 0xA5, np.uint8))
    try:
        ctx.denoise_mc_gather(bd, sizes, true_sizes, strength, rng, S, d_table, d_dst, d_rec, d_vec)
        got_rec = d_rec.download((S, 3, av1mi.GRAIN_BINS), av1mi.GRAIN_DTYPE)
        assert (d_rec.download((rec_bytes + guard,), np.uint8)[rec_bytes:] == 0xA5).all(), "records: written beyond their end"
        raw = d_vec.download((vec_bytes + guard,), np.uint8)
        assert (raw[vec_bytes:] == 0xA5).all(), "vectors: written beyond their end"
        got_vec = raw[:vec_bytes].view(av1mi.DENOISE_VEC_DTYPE).reshape(S, nblk)
        for s in range(S):      # the vectors first: a search failure, not a filter failure
            wv = want_vec[index[s]] if index[s] >= 0 else np.zeros(nblk, M.VEC_DTYPE)
            bad = np.flatnonzero(got_vec[s].view(np.uint32) != wv.view(np.uint32))
            assert bad.size == 0, "segment %d (position %d): %d vectors differ, the first at block %d: %s, not %s" % (s, index[s], len(bad), bad[0], got_vec[s][bad[0]], wv[bad[0]])
        for p in range(3):
            raw = d_dst[p].download((S * nbytes[p] + guard,), np.uint8)
            assert (raw[S * nbytes[p]:] == 0xA5).all(), "plane %d: written beyond its end" % p
            got = raw[:S * nbytes[p]].view(dt).reshape((S,) + planes[p].shape[1:])
            for s in range(S):
                w = want_planes[p][index[s]] if index[s] >= 0 else np.zeros_like(want_planes[p][0])
                bad = np.argwhere(got[s] != w)
                assert bad.size == 0, "plane %d segment %d (position %d): %d samples differ, the first at (y, x) = %s" % (p, s, index[s], len(bad), bad[0])
                wr = want_recs[p][index[s]] if index[s] >= 0 else R.empty_record()
                for k in ("sum_sq", "count", "reserved"):
                    assert (got_rec[s, p][k] == wr[k]).all(), "plane %d segment %d (position %d): record field %s differs: %s, not %s" % (p, s, index[s], k, got_rec[s, p][k], wr[k])
        if twice:      # the same bytes run to run; the same planes without records and with the vectors in the context
            first = [b.download((S * nb,), np.uint8) for b, nb in zip(d_dst, nbytes)]
            ctx.denoise_mc_gather(bd, sizes, true_sizes, strength, rng, S, d_table, d_dst, d_rec, d_vec)
            assert d_rec.download((S, 3, av1mi.GRAIN_BINS), av1mi.GRAIN_DTYPE).tobytes() == got_rec.tobytes()
            assert d_vec.download((vec_bytes,), np.uint8).tobytes() == got_vec.tobytes()
            assert all((b.download((S * nb,), np.uint8) == a).all() for b, nb, a in zip(d_dst, nbytes, first))
            for rec, vec in ((None, d_vec), (d_rec, None)):
                for b in d_dst:
                    ctx.memset(b, 0x5A, b.nbytes - guard)
                ctx.denoise_mc_gather(bd, sizes, true_sizes, strength, rng, S, d_table, d_dst, rec, vec)
                assert all((b.download((S * nb,), np.uint8) == a).all() for b, nb, a in zip(d_dst, nbytes, first))
            assert d_rec.download((S, 3, av1mi.GRAIN_BINS), av1mi.GRAIN_DTYPE).tobytes() == got_rec.tobytes()
        return got_rec, got_vec
    finally:
        for b in d_store + d_dst + [d_table, d_rec, d_vec]:
            b.free()


@pytest.mark.parametrize("rng", [4, 8])
@pytest.mark.parametrize("strength", [4, 16])
@pytest.mark.parametrize("name", list(SHAPES))
def test_mc_gather_is_the_reference(ctx, av1mi, name, strength, rng):
    sizes, true, bd, planes = _case(name)
    want = _reference(name, strength, rng)
    rec, vec = _gather_against_reference(ctx, av1mi, planes, sizes, true, bd, strength, rng, [1, 2], want, twice=(strength, rng) == (4, 8))
    v = vec.view(np.int8)
    assert (v > 0).any() and (v < 0).any()      # the clip moves: vectors of both signs
    _gather_against_reference(ctx, av1mi, planes, sizes, true, bd, strength, rng, [2, -1, 0, 3, 1], want)      # a flat slot and both ends of the run


@pytest.mark.parametrize("bd", [8, 10])
def test_mc_gather_extreme_content(ctx, av1mi, bd):
    """all 0, all max, 0 / max alternating in space and time, and C = 0 under F = max everywhere: the search's accumulator holds 256 x max
    plus the bias, the filter's packed sums 9 x max; range 8"""
    top = (1 << bd) - 1
    sizes = _layout(72, 40, "420")
    dt = np.uint8 if bd == 8 else np.uint16
    y, x = np.mgrid[0:40, 0:72]
    board = (((x + y) & 1) * top).astype(dt)
    for frames in ([np.zeros_like(board)] * 3, [np.full_like(board, top)] * 3, [board, top - board, board], [board, board, board],
                   [np.full_like(board, top), np.zeros_like(board), np.full_like(board, top)]):
        Y = np.stack(frames)
        planes = [Y, Y[:, :20, :36].copy(), Y[:, 20:, 36:].copy()]
        for strength in (1, 16):
            _gather_against_reference(ctx, av1mi, planes, sizes, sizes, bd, strength, 8, [1, 1])


def test_mc_gather_owns_its_vector_scratch(ctx, av1mi):
    """the context's vectors (d_vectors NULL) survive a plain av1mi_denoise_gather that grows the context's partials in between"""
    sizes, true, bd, planes = _case("16x16")
    want = _reference("16x16", 4, 8)
    _gather_against_reference(ctx, av1mi, planes, sizes, true, bd, 4, 8, [1, 2], want, twice=True)
    big, S = [(2096, 48), (1048, 24), (1048, 24)], 4      # flat slots of a larger geometry than any test before it: the partials grow
    d_table = ctx.to_device(np.zeros(S * 9, np.uint64))
    d_dst = [ctx.alloc(S * w * h) for w, h in big]
    d_rec = ctx.alloc(S * 3 * av1mi.GRAIN_BINS * av1mi.GRAIN_DTYPE.itemsize)
    try:
        ctx.denoise_gather(8, big, big, 4, S, d_table, d_dst, d_rec)
        assert not d_rec.download((S, 3, av1mi.GRAIN_BINS), av1mi.GRAIN_DTYPE)["count"].any()
    finally:
        for b in d_dst + [d_table, d_rec]:
            b.free()
    _gather_against_reference(ctx, av1mi, planes, sizes, true, bd, 4, 8, [1, 2], want, twice=True)


def test_mc_gather_refuses_bad_arguments(ctx, av1mi):
    d = ctx.to_device(np.zeros(8192, np.uint8))
    ok = dict(bit_depth=8, plane_sizes=[(16, 16), (8, 8), (8, 8)], true_sizes=[(16, 16), (8, 8), (8, 8)], strength=4, rng=8, segments=1, d_table=d, d_dst=[d, d, d])
    ctx.denoise_mc_gather(**ok)      # (a table of zeros: flat slots)
    for bad in (dict(bit_depth=12), dict(strength=0), dict(strength=17), dict(segments=0), dict(rng=0), dict(rng=3), dict(rng=16),
                dict(true_sizes=[(17, 16), (8, 8), (8, 8)]), dict(true_sizes=[(16, 16), (7, 8), (8, 8)]),
                dict(plane_sizes=[(0, 0), (8, 8), (8, 8)], true_sizes=[(0, 0), (8, 8), (8, 8)])):
        with pytest.raises(av1mi.Av1miError):
            ctx.denoise_mc_gather(**dict(ok, **bad))
    ctx.sync()
    d.free()


# ---------------------------------------------------------------------------------------------- session
W, H, Q, S, G = 192, 128, 110, 2, 3


def _run_session(ctx, av1mi, bd, clip, **kw):
    """the clip through a stored session, segment sg coding frames sg * G ..: per batch the fed planes, the grain records and the units"""
    import av1stream
    s = av1mi.GopSession(ctx, W, H, bd, Q, G, S, gpu_entropy=1, store_frames=S * G, **kw)
    out = []
    try:
        for f0 in range(0, S * G, S):
            for dst, a in zip(s.input_planes(), clip):
                dst[:] = a[f0:f0 + S].reshape(dst.shape)
            s.store_put(0, f0, S)
        for t in range(G):
            s.submit_stored(0, [sg * G + t for sg in range(S)], 0 if t == 0 else 1)
            fed = s.download_fed()
            fr = s.collect()
            out.append(dict(fed=fed, grain=fr["grain"].copy() if "grain" in fr else None, units=[av1stream.session_frame_unit_gpu(W, H, bd, fr, sg) for sg in range(S)]))
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    return out


@pytest.fixture(scope="module")
def session_clip():
    return K.translating(_layout(W, H, "420"), S * G, 8, 21, 2)


def test_session_gathers_through_the_search(ctx, av1mi, session_clip):
    sizes = _layout(W, H, "420")
    want_planes, want_recs, _ = M.run(session_clip, sizes, 8, 8, 8)
    got = _run_session(ctx, av1mi, 8, session_clip, denoise=8, denoise_range=8)
    for t, b in enumerate(got):
        index = [sg * G + t for sg in range(S)]
        for p in range(3):
            assert (b["fed"][p] == np.concatenate([want_planes[p][f] for f in index])).all(), "batch %d plane %d: the fed buffer is not the reference's frame" % (t, p)
            for sg, f in enumerate(index):
                for k in ("sum_sq", "count"):
                    assert (b["grain"][sg, p][k] == want_recs[p][f][k]).all(), "batch %d segment %d plane %d: the %s of the records differ" % (t, sg, p, k)
    assert sum(int(b["grain"]["count"].sum()) for b in got) > 0


def test_session_with_range_0_is_the_session_as_it_was(ctx, av1mi, session_clip):
    unset, zero, on = (_run_session(ctx, av1mi, 8, session_clip, denoise=8, **kw) for kw in ({}, dict(denoise_range=0), dict(denoise_range=8)))
    for a, b in zip(unset, zero):
        assert a["units"] == b["units"] and a["grain"].tobytes() == b["grain"].tobytes()
        assert all((x == y).all() for x, y in zip(a["fed"], b["fed"]))
    assert any(a["units"] != b["units"] for a, b in zip(unset, on))


def test_session_argument_rules(ctx, av1mi):
    for kw in (dict(denoise_range=8, store_frames=4), dict(denoise_range=8, denoise=0, store_frames=4), dict(denoise_range=3, denoise=4, store_frames=4),
               dict(denoise_range=16, denoise=4, store_frames=4), dict(denoise_range=-4, denoise=4, store_frames=4)):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, W, H, 8, Q, G, S, **kw)
        assert "denoise_range" in str(e.value)
    with pytest.raises(av1mi.Av1miError) as e:      # what denoise refuses stays refused
        av1mi.GopSession(ctx, W, H, 8, Q, G, S, denoise=4, denoise_range=8)
    assert "store" in str(e.value)


# ---------------------------------------------------------------------------------------------- product
def test_transcode_with_range_codes_less(tmp_path):
    """a translating grainy Y4M, 8 bits, 2 GOPs of 5 frames, sigma 2 under strength 4: with -av1mi_denoise_range 8 the stream decodes in
    dav1d to 10 frames of the source's size, middle frames carry film grain parameters, and it is smaller than at range 0"""
    import av1stream
    import dav1d_ref as D
    import deint_clips as C
    n = 10
    clip = K.translating(_layout(W, H, "420"), n, 8, 31, 2)
    C.write_y4m(tmp_path / "pan.y4m", clip, 8, interlace="p")
    size, grain = {}, {}
    for rng in (0, 8):
        path = tmp_path / ("r%d.obu" % rng)
        code, err = av1stream.run_transcode(["-i", tmp_path / "pan.y4m", "-global_quality:v:0", Q, "-g", 5, "-av1mi_segments", 2, "-av1mi_denoise", 4, "-av1mi_denoise_range", rng,
                                             "-av1mi_stats", tmp_path / ("r%d.txt" % rng), path])
        assert code == 0, err
        data = path.read_bytes()
        size[rng] = len(data)
        lines = [l for l in (tmp_path / ("r%d.txt" % rng)).read_text().splitlines() if l.startswith("n:")]
        assert len(lines) == n
        grain[rng] = [int(l.split(" grain:")[1].split()[0]) for l in lines]
        if rng:
            assert D.available(), "dav1d is needed to check the stream"
            frames = D.decode(data)
            assert len(frames) == n and all(f[0].shape == (H, W) and f[1].shape == (H // 2, W // 2) for f in frames)
    print("coded bytes: %d at range 0, %d at range 8; grain values %s / %s" % (size[0], size[8], grain[0], grain[8]))
    assert grain[8][0] == 0 and grain[8][-1] == 0 and max(grain[8][1:-1]) > 0      # the ends of the run pass through; middle frames carry parameters
    assert size[8] < size[0]
