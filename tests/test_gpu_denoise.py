"""GPU tests of the denoising option (av1mi_gop_config.denoise): k_denoise_gather + k_grain_sum against tests/denoise_ref.py bit for bit,
in output and in records, and a session that gathers through them."""
import types

import numpy as np
import pytest

import denoise_ref as R

pytestmark = pytest.mark.gpu


def _clip(sizes, n, bd, seed, sigma=3):
    """per plane [n, H, W]: a ramp under a square that moves 5 samples per frame, plus noise: every weight from 0 to 16 occurs"""
    rng = np.random.default_rng(seed)
    out = []
    for (w, h) in sizes:
        y, x = np.mgrid[0:h, 0:w]
        fr = []
        for f in range(n):
            a = (60 + (x * 3 + y * 2) % 120).astype(np.int64)
            a[h // 4:h // 4 + max(h // 3, 1), (2 + 5 * f) % w:(2 + 5 * f) % w + max(w // 6, 1)] = 230
            a = (a << (bd - 8)) + np.rint(rng.normal(0, sigma * (1 << (bd - 8)), a.shape)).astype(np.int64)
            fr.append(np.clip(a, 0, (1 << bd) - 1))
        out.append(np.stack(fr).astype(np.uint8 if bd == 8 else np.uint16))
    return out


def _records(ctx, av1mi, d, S):
    return d.download((S, 3, av1mi.GRAIN_BINS), av1mi.GRAIN_DTYPE)


def _gather_against_reference(ctx, av1mi, planes, sizes, true_sizes, bd, strength, index, twice=False):
    """planes: [n, H, W] per plane, the store's run; index: the store position per segment (-1 = a flat slot).  Checks every destination
    plane and every record against the reference run, and that nothing beyond the planes is written."""
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
    rec_bytes = S * 3 * av1mi.GRAIN_BINS * av1mi.GRAIN_DTYPE.itemsize
    d_rec = ctx.to_device(np.full(rec_bytes + guard, 0xA5, np.uint8))
    try:
        ctx.denoise_gather(bd, sizes, true_sizes, strength, S, d_table, d_dst, d_rec)
        got_rec = _records(ctx, av1mi, d_rec, S)
        assert (d_rec.download((rec_bytes + guard,), np.uint8)[rec_bytes:] == 0xA5).all(), "records: written beyond their end"
        for p in range(3):
            want, want_rec = R.run(planes[p], true_sizes[p][0], true_sizes[p][1], bd, strength)
            raw = d_dst[p].download((S * nbytes[p] + guard,), np.uint8)
            assert (raw[S * nbytes[p]:] == 0xA5).all(), "plane %d: written beyond its end" % p
            got = raw[:S * nbytes[p]].view(dt).reshape((S,) + planes[p].shape[1:])
            for s in range(S):
                w = want[index[s]] if index[s] >= 0 else np.zeros_like(want[0])
                bad = np.argwhere(got[s] != w)
                assert bad.size == 0, "plane %d segment %d (position %d): %d samples differ, the first at (y, x) = %s" % (p, s, index[s], len(bad), bad[0])
                wr = want_rec[index[s]] if index[s] >= 0 else R.empty_record()
                for k in ("sum_sq", "count", "reserved"):
                    assert (got_rec[s, p][k] == wr[k]).all(), "plane %d segment %d (position %d): record field %s differs: %s, not %s" % (p, s, index[s], k, got_rec[s, p][k], wr[k])
        if twice:      # the same bytes run to run, and the same planes without records
            ctx.denoise_gather(bd, sizes, true_sizes, strength, S, d_table, d_dst, d_rec)
            assert _records(ctx, av1mi, d_rec, S).tobytes() == got_rec.tobytes()
            first = [b.download((S * nb,), np.uint8) for b, nb in zip(d_dst, nbytes)]
            ctx.denoise_gather(bd, sizes, true_sizes, strength, S, d_table, d_dst, None)
            assert all((b.download((S * nb,), np.uint8) == a).all() for b, nb, a in zip(d_dst, nbytes, first))
        return got_rec
    finally:
        for b in d_store + d_dst + [d_table, d_rec]:
            b.free()


def _sizes(w, h):
    return [(w, h), (w // 2, h // 2), (w // 2, h // 2)]


# (buffer size, true size, bit depth): chroma rows of 4 bytes take the dword form; two waves across and a partial last cell; a band
# boundary, the true edge inside the buffer and 16-bit samples
SHAPES = {"8x8": ((8, 8), (8, 8), 8), "1048x24": ((1048, 24), (1048, 24), 8), "72x40": ((72, 40), (70, 38), 10)}


@pytest.mark.parametrize("strength", [1, 4, 16])
@pytest.mark.parametrize("name", list(SHAPES))
def test_denoise_gather_is_the_reference(ctx, av1mi, name, strength):
    (W, H), (w, h), bd = SHAPES[name]
    true = [(w, h), ((w + 1) // 2, (h + 1) // 2), ((w + 1) // 2, (h + 1) // 2)]
    planes = _clip(_sizes(W, H), 4, bd, 3, sigma=max(strength / 3, 0.5))
    for a, (tw, th) in zip(planes, true):      # the input's padding must not matter
        a[:, th:, :] = (1 << bd) - 1
        a[:, :, tw:] = 0
    rec = _gather_against_reference(ctx, av1mi, planes, _sizes(W, H), true, bd, strength, [1, 2], twice=strength == 4)
    assert rec["count"].sum() > 0
    _gather_against_reference(ctx, av1mi, planes, _sizes(W, H), true, bd, strength, [2, -1, 0, 3, 1])      # a flat slot and the ends of the run


@pytest.mark.parametrize("bd", [8, 10])
def test_denoise_gather_a_flat_slot_and_short_runs(ctx, av1mi, bd):
    sizes = _sizes(72, 40)
    planes = _clip(sizes, 3, bd, 5)
    _gather_against_reference(ctx, av1mi, planes, sizes, sizes, bd, 6, [-1, 1])
    for n in (1, 2):      # a run of one frame, and of two: ends only
        rec = _gather_against_reference(ctx, av1mi, [a[:n] for a in planes], sizes, sizes, bd, 6, [n - 1, 0])
        assert rec["count"].sum() == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_denoise_gather_extreme_content(ctx, av1mi, bd):
    """all 0, all max, and 0 / max alternating in space and time: the packed sums reach 9 x max and must not wrap"""
    top = (1 << bd) - 1
    sizes = _sizes(72, 40)
    dt = np.uint8 if bd == 8 else np.uint16
    y, x = np.mgrid[0:40, 0:72]
    board = (((x + y) & 1) * top).astype(dt)
    for frames in ([np.zeros_like(board)] * 3, [np.full_like(board, top)] * 3, [board, top - board, board], [board, board, board],
                   [np.zeros_like(board), np.full_like(board, top), np.zeros_like(board)]):
        Y = np.stack(frames)
        planes = [Y, Y[:, :20, :36].copy(), Y[:, 20:, 36:].copy()]
        for strength in (1, 16):
            _gather_against_reference(ctx, av1mi, planes, sizes, sizes, bd, strength, [1, 1])


def test_denoise_gather_refuses_bad_arguments(ctx, av1mi):
    d = ctx.to_device(np.zeros(8192, np.uint8))
    ok = dict(bit_depth=8, plane_sizes=[(8, 8), (4, 4), (4, 4)], true_sizes=[(8, 8), (4, 4), (4, 4)], strength=4, segments=1, d_table=d, d_dst=[d, d, d])
    ctx.denoise_gather(**ok)      # (a table of zeros: flat slots)
    for bad in (dict(bit_depth=12), dict(strength=0), dict(strength=17), dict(segments=0), dict(true_sizes=[(9, 8), (4, 4), (4, 4)]),
                dict(plane_sizes=[(20, 8), (4, 4), (4, 4)], true_sizes=[(13, 8), (4, 4), (4, 4)])):
        with pytest.raises(av1mi.Av1miError):
            ctx.denoise_gather(**dict(ok, **bad))
    ctx.sync()
    d.free()


def test_the_three_gathers_refuse_their_planes_in_the_same_words(ctx, av1mi):
    """a true size above the buffer's, and a destination that is not 16-byte aligned: one sentence, under the called function's name"""
    d = ctx.to_device(np.zeros(8192, np.uint8))
    odd = types.SimpleNamespace(ptr=d.ptr + 4)      # the same memory, 4 bytes in
    ok = dict(bit_depth=8, plane_sizes=[(8, 8), (4, 4), (4, 4)], true_sizes=[(8, 8), (4, 4), (4, 4)], segments=1, d_table=d, d_dst=[d, d, d])
    calls = {"av1mi_deinterlace_gather": lambda **kw: ctx.deinterlace_gather(parity=0, **kw),
             "av1mi_denoise_gather": lambda **kw: ctx.denoise_gather(strength=4, **kw),
             "av1mi_denoise_mc_gather": lambda **kw: ctx.denoise_mc_gather(strength=4, rng=4, **kw)}
    for bad in (dict(true_sizes=[(9, 8), (4, 4), (4, 4)]), dict(d_dst=[d, odd, d])):
        said = {}
        for name, call in calls.items():
            with pytest.raises(av1mi.Av1miError) as e:
                call(**dict(ok, **bad))
            code = "av1mi error %d: " % e.value.code      # (Av1miError puts the return code in front of the library's text)
            assert str(e.value).startswith(code + name + ": "), str(e.value)
            said[name] = str(e.value)[len(code + name):]
        assert len(set(said.values())) == 1, said
    ctx.sync()
    d.free()


# ---------------------------------------------------------------------------------------------- session
W, H, Q, S, G = 192, 128, 110, 2, 3


def _session_clip(bd):
    return _clip(_sizes(W, H), S * G, bd, 21, sigma=2)


def _run_session(ctx, av1mi, bd, clip, **kw):
    """the clip through a stored session, segment sg coding frames sg * G ..: per batch the fed planes, the collected frame and the
    reference frames; the stream per segment"""
    import av1stream
    s = av1mi.GopSession(ctx, W, H, bd, Q, G, S, gpu_entropy=2, store_frames=S * G, **kw)
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
            units = [av1stream.session_frame_unit_gpu(W, H, bd, fr, sg) for sg in range(S)]
            assert units == [av1stream.session_frame_unit(W, H, bd, fr, sg) for sg in range(S)], "batch %d: GPU tile coder and host writer disagree" % t
            g = av1stream.FilmGrain()      # any legal parameters: white luma grain, a constant scaling function
            g.apply_grain, g.grain_seed, g.num_y_points, g.grain_scaling_minus_8, g.overlap_flag = 1, 100 + t, 2, 3, 1
            g.point_y_value[1], g.point_y_scaling[0], g.point_y_scaling[1] = 255, 48, 48
            grainy = [av1stream.session_frame_unit_gpu(W, H, bd, fr, sg, film_grain=g, film_grain_present=1) for sg in range(S)]
            # the session's own writer (av1mi_session_temporal_unit_grain), the one the product uses
            assert grainy == [av1stream.session_temporal_unit(W, H, bd, fr["raw"], sg, with_sequence_header=t == 0, film_grain=g, film_grain_present=1) for sg in range(S)]
            assert units == [av1stream.session_temporal_unit(W, H, bd, fr["raw"], sg, with_sequence_header=t == 0) for sg in range(S)]
            assert grainy == [av1stream.session_frame_unit(W, H, bd, fr, sg, film_grain=g, film_grain_present=1) for sg in range(S)]
            out.append(dict(grainy=grainy, fed=fed, grain=fr["grain"].copy() if "grain" in fr else None, raw_grain=fr["raw"].grain, units=units, refs=s.download_reference()))
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    return out


@pytest.mark.parametrize("bd", [8, 10])
def test_session_gathers_through_the_denoiser(ctx, av1mi, bd):
    import dav1d_ref as D
    clip = _session_clip(bd)
    want = [R.run(a, a.shape[2], a.shape[1], bd, 4) for a in clip]
    got = _run_session(ctx, av1mi, bd, clip, denoise=4)
    for t, b in enumerate(got):
        index = [sg * G + t for sg in range(S)]
        for p in range(3):
            assert (b["fed"][p] == np.concatenate([want[p][0][f] for f in index])).all(), "batch %d plane %d: the fed buffer is not the reference's frame" % (t, p)
            for sg, f in enumerate(index):
                for k in ("sum_sq", "count"):
                    assert (b["grain"][sg, p][k] == want[p][1][f][k]).all(), "batch %d segment %d plane %d: the %s of the records differ" % (t, sg, p, k)
    assert sum(int(b["grain"]["count"].sum()) for b in got) > 0
    assert D.available(), "dav1d is needed to check the session's streams"
    if True:
        import dav1d_grain as DG
        for sg in range(S):
            frames = D.decode(b"".join(b["units"][sg] for b in got))
            assert len(frames) == G
            with_grain = b"".join(b["grainy"][sg] for b in got)      # the same frames under film grain parameters: grain off, the same pictures
            assert all((x == y).all() for fa, fb in zip(DG.decode(with_grain, False), frames) for x, y in zip(fa, fb))
            assert any((x != y).any() for fa, fb in zip(DG.decode(with_grain, True), frames) for x, y in zip(fa, fb))
            for t in range(G):
                for i, d in enumerate((1, 2, 2)):
                    rows = H // d
                    assert (frames[t][i] == got[t]["refs"][i][sg * rows:(sg + 1) * rows]).all(), "segment %d frame %d plane %d: dav1d decodes another picture" % (sg, t, i)


def test_session_without_denoise_is_the_session_as_it_was(ctx, av1mi):
    clip = _session_clip(8)
    unset, zero, on = (_run_session(ctx, av1mi, 8, clip, **kw) for kw in ({}, dict(denoise=0), dict(denoise=4)))
    for a, b in zip(unset, zero):
        assert a["raw_grain"] is None and b["raw_grain"] is None and a["units"] == b["units"]
        assert all((x == y).all() for x, y in zip(a["fed"], b["fed"]))
    assert any(a["units"] != b["units"] for a, b in zip(unset, on))


def test_session_argument_rules(ctx, av1mi):
    for kw in (dict(denoise=4), dict(denoise=17, store_frames=4), dict(denoise=-1, store_frames=4), dict(denoise=4, store_frames=4, deinterlace=1),
               dict(denoise=4, store_frames=4, source_bit_depth=12)):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, W, H, 10 if "source_bit_depth" in kw else 8, Q, G, S, **kw)
        assert "denoise" in str(e.value)
    s = av1mi.GopSession(ctx, W, H, 8, Q, G, S, store_frames=6, denoise=2)
    try:
        s.input_planes()
        s.store_put(0, 0, 2)
        with pytest.raises(av1mi.Av1miError):
            s.submit_stored(0, [0, 2], 0)      # beyond the run of 2 frames
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- product
def _obus(data):
    """(type, payload) of the OBUs of a Section-5 stream (every OBU here has a size field)"""
    i = 0
    while i < len(data):
        hdr = data[i]
        i += 1 + ((hdr >> 2) & 1)
        size, shift = 0, 0
        while True:
            b = data[i]; i += 1
            size |= (b & 0x7f) << shift; shift += 7
            if not b & 0x80:
                break
        yield (hdr >> 3) & 15, data[i:i + size]
        i += size


def test_transcode_with_denoise_signals_film_grain(tmp_path):
    """a 10-frame noisy Y4M through av1mi_run_transcode -av1mi_denoise 4 -av1mi_stats: the sequence header of the Matroska file's stream
    has film_grain_params_present set (its last bit before the trailing one), the stats lines carry grain:, middle frames a value > 0"""
    import av1stream
    import deint_clips as K
    import dav1d_grain as DG
    n = 10
    clip = _clip(_sizes(W, H), 1, 8, 31, sigma=0)
    rng = np.random.default_rng(32)
    noisy = [np.clip(np.repeat(a, n, axis=0) + np.rint(rng.normal(0, 2, (n,) + a.shape[1:])), 0, 255).astype(np.uint8) for a in clip]
    K.write_y4m(tmp_path / "noisy.y4m", noisy, 8, interlace="p")
    outs = {}
    for name, extra in (("on", ["-av1mi_denoise", 4]), ("nofg", ["-av1mi_denoise", 4, "-av1mi_film_grain", 0]), ("off", [])):
        code, err = av1stream.run_transcode(["-i", tmp_path / "noisy.y4m", "-global_quality:v:0", Q, "-g", 5, "-av1mi_segments", 2, "-av1mi_stats", tmp_path / (name + ".txt")] + extra +
                                            [tmp_path / (name + ".mkv")])
        assert code == 0, err
        outs[name] = ((tmp_path / (name + ".mkv")).read_bytes(), (tmp_path / (name + ".txt")).read_text().splitlines())
    def present(mkv):      # the sequence header OBU sits in the codec private data (av1C), 4 bytes in
        i = mkv.index(bytes([0x81, 0x1F])) + 4
        kind, payload = next(_obus(mkv[i:]))
        assert kind == 1
        bits = "".join("{:08b}".format(b) for b in payload).rstrip("0")[:-1]      # without trailing_bits
        return bits[-1] == "1"
    assert present(outs["on"][0]) and not present(outs["nofg"][0]) and not present(outs["off"][0])
    frames = [l for l in outs["on"][1] if l.startswith("n:")]
    assert len(frames) == n and all(" grain:" in l for l in frames)
    values = [int(l.split(" grain:")[1].split()[0]) for l in frames]
    assert values[0] == 0 and values[-1] == 0 and max(values) > 0      # the ends of the run pass through: no grain to put back
    assert all(" grain:" in l for l in outs["nofg"][1] if l.startswith("n:")) and not any(" grain:" in l for l in outs["off"][1])
    assert len(outs["on"][0]) < len(outs["off"][0])                    # the noise is not coded
