"""GPU: av1mi_lr_search (k_lr_search + k_lr_pick) against its restatement (lr_search_ref.py: the oracle's restoration of the whole plane
per candidate, summed per unit) — the cost table and the chosen indices bit for bit — and the restoration with the chosen units."""
import numpy as np
import pytest

import dav1d_ref as D
import lr_search_ref as R
from lf_util import test_image as make_image
from oracle import oracle as ORACLE

pytestmark = pytest.mark.gpu


def _dims(h, w):
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


def _search(ctx, av1mi, cdef, dbl, src, bd, q):
    """cdef / dbl / src: per plane [frame, row, column].  Returns (table [frame, unit, candidate], choice [frame, unit], the three
    planes' unit records [frame, rows, cols, 8]) and leaves nothing on the device"""
    nf, h, w = cdef[0].shape
    n = av1mi.lr_search_units(w, h)
    d = [ctx.to_device(a) for a in cdef + dbl + src]
    nbytes = av1mi.lr_search_scratch_bytes(w, h, nf)
    assert nbytes >= nf * n * 72 and nbytes % 16 == 0
    scr = ctx.to_device(np.full(nbytes, 0xA5, np.uint8))                     # the call zeroes it itself
    counts = [_units(hh, ww) for hh, ww in _dims(h, w)]
    assert sum(counts) == n
    d_units = [ctx.to_device(np.full(nf * k * 8, 0x55, np.uint8)) for k in counts]
    d_choice = ctx.to_device(np.full(nf * n + 4, 0xEE, np.uint8))
    ctx.lr_search(av1mi.LrSearchJob(w, h, bd, nf, 64, q, w, w // 2, *[b.ptr for b in d], scr.ptr, *[b.ptr for b in d_units], d_choice.ptr))
    table = scr.download((nbytes // 8,), np.uint64)[:nf * n * 9].reshape(nf, n, 9).astype(np.int64)
    choice = d_choice.download((nf * n + 4,), np.uint8)
    assert (choice[-4:] == 0xEE).all()
    units = [b.download((nf, ORACLE.lr_units(64, hh), ORACLE.lr_units(64, ww), 8), np.int8) for b, (hh, ww) in zip(d_units, _dims(h, w))]
    for b in d + [scr, d_choice] + d_units:
        b.free()
    return table, choice[:-4].reshape(nf, n), units


def _units(h, w):
    """units of a plane of h x w samples: the oracle's count"""
    return ORACLE.lr_units(64, h) * ORACLE.lr_units(64, w)


def _check(O, av1mi, cdef, dbl, src, bd, q, table, choice, units):
    """the table, the indices and the records against the restatement; the property of the pick.  Returns the expected indices"""
    nf, h, w = cdef[0].shape
    lmb = R.lam(O, q, bd)
    counts = [_units(hh, ww) for hh, ww in _dims(h, w)]
    first = np.concatenate([[0], np.cumsum(counts)])
    exp_all = []
    for f in range(nf):
        exp = R.frame_tables(O, [a[f] for a in cdef], [a[f] for a in dbl], [a[f] for a in src], bd)
        assert (table[f] == exp).all(), ("cost table", f, np.argwhere(table[f] != exp)[:4], table[f][table[f] != exp][:4], exp[table[f] != exp][:4])
        for p in range(3):
            sl = slice(first[p], first[p + 1])
            idx, j = R.pick(exp[sl], int(p > 0), lmb)
            assert choice[f, sl].tolist() == idx.tolist(), ("choice", f, p)
            got_j = table[f, sl] + lmb * np.array([av1mi.lr_search_bits(int(p > 0), c) for c in range(9)], np.int64)
            chosen = got_j[np.arange(counts[p]), choice[f, sl]]
            assert (chosen <= got_j[:, R.POLICY]).all() and (chosen <= got_j[:, 0]).all()
            assert units[p][f].reshape(-1, 8).tolist() == [R.record(int(p > 0), c) for c in idx]
            exp_all.append(idx)
    return exp_all


def _frames(rng, h, w, bd, nf, noise):
    """sources of different content per frame; the CDEF planes lie around them (left half: +- noise, right half: closer), the
    deblocked planes are unrelated pictures — only the rows beside the stripes are read from them"""
    mx = (1 << bd) - 1
    src = [np.stack([make_image(rng, hh, ww, bd) for _ in range(nf)]) for hh, ww in _dims(h, w)]
    cdef = []
    for s in src:
        n = rng.integers(-noise, noise + 1, s.shape)
        n[:, :, s.shape[2] // 2:] //= 4
        cdef.append(np.clip(s.astype(int) + n, 0, mx).astype(s.dtype))
    dbl = [np.stack([make_image(rng, hh, ww, bd) for _ in range(nf)]) for hh, ww in _dims(h, w)]
    return cdef, dbl, src


# luma sizes: 136 x 200 the stripe split and edge units; 144 x 200 a 72 x 100 chroma plane; 40 x 24 one unit per plane; 96 x 102 the
# scalar route in every plane (102 and 51 columns); 300 x 260 edge units of 1.5 units
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("h,w,q", [(136, 200, 23), (144, 200, 160), (40, 24, 128), (96, 102, 60), (300, 260, 200)])
def test_search_equals_the_restatement(ctx, av1mi, O, h, w, q, bd):
    rng = np.random.default_rng(h * 3 + w + bd)
    cdef, dbl, src = _frames(rng, h, w, bd, 2, 3 << (bd - 8))
    table, choice, units = _search(ctx, av1mi, cdef, dbl, src, bd, q)
    _check(O, av1mi, cdef, dbl, src, bd, q, table, choice, units)


@pytest.mark.parametrize("bd", [8, 10])
def test_search_on_a_full_swing_checkerboard(ctx, av1mi, O, bd):
    """CDEF planes that alternate between 0 and the largest sample against the inverse pattern as source: the sharpening filter drives
    the intermediate into its clamp, every sample of "none" errs by the full range, and the per-lane and per-wave sums are as large as
    they get.  The second frame has the pattern in pairs of columns"""
    h, w, mx = 136, 200, (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    def board(hh, ww, step):
        y, x = np.mgrid[0:hh, 0:ww]
        return ((((x // step) + y) & 1) * mx).astype(dt)
    cdef = [np.stack([board(hh, ww, 1), board(hh, ww, 2)]) for hh, ww in _dims(h, w)]
    src = [(mx - c).astype(dt) for c in cdef]
    dbl = [s.copy() for s in src]
    table, choice, units = _search(ctx, av1mi, cdef, dbl, src, bd, 23)
    assert table[0, :, 0].max() >= 64 * 56 * mx * mx
    _check(O, av1mi, cdef, dbl, src, bd, 23, table, choice, units)


@pytest.mark.parametrize("bd", [8, 10])
def test_restoration_with_the_chosen_units(ctx, av1mi, O, bd):
    """av1mi_lr_yuv_decide fed the search's three unit arrays (d_units_v: V's own records): where a plane's restoration stays ON the
    restored plane is the oracle's with the chosen units, the choices are not all the policy's, and U and V chose differently"""
    rng = np.random.default_rng(400 + bd)
    h, w, nf, q = 136, 200, 2, 60
    cdef, dbl, src = _frames(rng, h, w, bd, nf, 4 << (bd - 8))
    for p, (hh, ww) in enumerate(_dims(h, w)):                  # smooth sources under the same noise: a low-pass gains there
        y, x = np.mgrid[0:hh, 0:ww]
        for f in range(nf):
            s = ((40 + 3 * f + 0.5 * x + 0.3 * y + 20 * np.sin(x / (9.0 + p) + y / 13.0)) * (1 << (bd - 8))).astype(int)
            cdef[p][f] = np.clip(cdef[p][f].astype(int) - src[p][f].astype(int) + s, 0, (1 << bd) - 1)
            src[p][f] = s
    src[2][:, :, w // 8:] = cdef[2][:, :, w // 8:]              # V is already exact right of its first quarter: "none" there, unlike U
    table, choice, units = _search(ctx, av1mi, cdef, dbl, src, bd, q)
    _check(O, av1mi, cdef, dbl, src, bd, q, table, choice, units)
    assert (choice != R.POLICY).any() and (choice != 0).any() and (units[1] != units[2]).any()
    d = [ctx.to_device(a) for a in cdef + dbl]
    out = [ctx.alloc(a.nbytes) for a in cdef]
    d_src = [ctx.to_device(a) for a in src]
    d_units = [ctx.to_device(u) for u in units]
    per = [u.shape[1] * u.shape[2] for u in units]
    scr, on = ctx.alloc(ctx.lr_yuv_decide_scratch_bytes(h, nf)), ctx.to_device(np.full(3 * nf, 9, np.uint8))
    ctx.lr_yuv_decide(av1mi.LrDecideJob(w, h, bd, nf, 64, w, w // 2, *[b.ptr for b in d + out + d_src], d_units[0].ptr, d_units[1].ptr, per[0], per[1],
                                        scr.ptr, on.ptr, 1, d_units[2].ptr, per[2]))
    flags = on.download((nf, 3), np.uint8)
    got = [o.download(a.shape, a.dtype) for o, a in zip(out, cdef)]
    for b in d + out + d_src + d_units + [scr, on]:
        b.free()
    assert flags[:, 2].any(), "V's restoration is off in every frame: its own units were not exercised"
    for f in range(nf):
        for p in range(3):
            exp = O.lr_plane(cdef[p][f], dbl[p][f], bd, int(p > 0), 64, units[p][f])
            assert flags[f, p] == O.lr_select((src[p][f],), (cdef[p][f],), (exp,), bd, int(p > 0))[1][0]
            if flags[f, p]:
                assert (got[p][f] == exp).all(), (f, p)


def test_search_refuses_what_it_does_not_support(ctx, av1mi):
    z = ctx.alloc(4096)
    ok = [64, 64, 8, 1, 64, 100, 64, 32] + [z.ptr] * 14
    for field, value in ((4, 128), (2, 12), (0, 63), (5, 256), (6, 32), (8, 0), (21, 0)):
        a = list(ok)
        a[field] = value
        with pytest.raises(av1mi.Av1miError):
            ctx.lr_search(av1mi.LrSearchJob(*a))
    z.free()


def _session_run(ctx, av1mi, w, h, bd, q, planes, gpu_entropy, lr_search, nt=3, S=2, fallback=False):
    """S segments x nt frames through a GOP session; returns per segment the stream, per frame the references [plane][segment rows],
    the collected choices, and the profile's restoration launches.  fallback: the GPU coder must hand at least one batch back"""
    import av1stream
    sess = av1mi.GopSession(ctx, w, h, bd, q, nt, S, gpu_entropy=gpu_entropy, lr_search=lr_search)
    streams, refs, choices = [b""] * S, [], []
    ctx.prof_reset()
    ctx.prof_enable(1)
    for t in range(nt):
        for dst, a in zip(sess.input_planes(), planes):
            dst[:] = np.concatenate([a[(t + s) % len(a)] for s in range(S)])
        sess.submit()
        fr = sess.collect()
        for s in range(S):
            streams[s] += av1stream.session_temporal_unit(w, h, bd, fr["raw"], s, with_sequence_header=(t == 0))
        refs.append(sess.download_reference())
        choices.append(fr["lr_choice"].copy() if "lr_choice" in fr else None)
    launches = ctx.prof_get().get("loop_restoration", (0, 0.0))[0]
    ctx.prof_enable(0)
    fallbacks = sess.entropy_fallbacks()
    sess.close()
    assert fallbacks >= 1 if fallback else fallbacks == 0
    return streams, refs, choices, launches


SESSIONS = [(192, 128, 8, 23), (200, 136, 10, 160), (192, 128, 10, 160), (200, 136, 8, 23)]


def _half_flat(w, h, bd):
    """four frames whose left half is flat and whose right half is textured: the search cannot choose alike everywhere"""
    import synth
    planes = [np.array(a) for a in synth.frames(w, h, 4, bd, 11)]
    for a in planes:
        a[:, :, :a.shape[2] // 2] = a[:, :, :a.shape[2] // 2].mean().astype(a.dtype)
    return planes


def _decodes_to(streams, refs, h, nt):
    for s, stream in enumerate(streams):
        got = D.decode(stream)
        assert len(got) == nt
        for t in range(nt):
            for p in range(3):
                hp = h >> (p > 0)
                assert (np.asarray(got[t][p]) == refs[t][p][s * hp:(s + 1) * hp]).all(), (s, t, p)


@pytest.mark.parametrize("w,h,bd,q", SESSIONS)
def test_session_with_the_search(ctx, av1mi, w, h, bd, q):
    """lr_search 1: the tiles coded on the GPU with the chosen units are the host writer's bytes from the downloaded symbols and
    records (gpu_entropy 0: the same references and choices), and not every unit takes the policy's record.  lr_search 0 launches what
    it always did: the two restoration passes per batch, against five with the search (zeroing, search, pick, two passes)"""
    planes = _half_flat(w, h, bd)
    nt = 3
    gpu, refs, choices, n_on = _session_run(ctx, av1mi, w, h, bd, q, planes, 1, 1)
    host, refs0, choices0, _ = _session_run(ctx, av1mi, w, h, bd, q, planes, 0, 1)
    assert gpu == host, "GPU-coded tiles and the host writer disagree"
    assert all((a == b).all() for x, y in zip(refs, refs0) for a, b in zip(x, y)) and all((a == b).all() for a, b in zip(choices, choices0))
    assert any((c != R.POLICY).any() for c in choices)
    _, _, off_choices, n_off = _session_run(ctx, av1mi, w, h, bd, q, planes, 1, 0)
    assert off_choices == [None] * nt and n_off == 2 * nt and n_on == 5 * nt


@pytest.mark.skipif(not D.available(), reason="no dav1d in this image")
@pytest.mark.parametrize("w,h,bd,q", SESSIONS)
def test_dav1d_decodes_the_sessions_streams_to_its_references(ctx, av1mi, w, h, bd, q):
    gpu, refs, choices, _ = _session_run(ctx, av1mi, w, h, bd, q, _half_flat(w, h, bd), 1, 1)
    assert any((c != R.POLICY).any() for c in choices)
    _decodes_to(gpu, refs, h, 3)


@pytest.mark.skipif(not D.available(), reason="no dav1d in this image")
@pytest.mark.parametrize("bd", [8, 10])
def test_a_batch_the_gpu_coder_hands_back_is_coded_with_its_units(ctx, av1mi, bd):
    """white noise in the right half at base_q_idx 2: a tile needs more list words than the GPU coder holds, the session hands the
    symbols out with the records the coder had been started with, and the host writer codes every unit's own record from
    av1mi_gop_frame.lr_units: dav1d decodes the stream to the session's references, and some unit differs from the policy's record"""
    w, h, q, nt = 128, 128, 2, 2
    rng = np.random.default_rng(bd)
    planes = [rng.integers(0, 1 << bd, (nt, hh, ww)).astype(np.uint8 if bd == 8 else np.uint16) for hh, ww in _dims(h, w)]
    for a in planes:
        a[:, :, :a.shape[2] // 2] = 1 << (bd - 1)
    streams, refs, choices, _ = _session_run(ctx, av1mi, w, h, bd, q, planes, 1, 1, nt=nt, S=1, fallback=True)
    assert any((c != R.POLICY).any() for c in choices)
    _decodes_to(streams, refs, h, nt)


def test_transcode_job_with_the_search_writes_the_lr_field(ctx, av1mi, tmp_path):
    """-av1mi_lr_search 1 -av1mi_stats through av1mi_run_transcode: every frame line carries lr:<units filtered>/<units> — the units of
    the three planes (192 x 136: 6 + 2 + 2) and, of them, those with a Wiener record in a plane whose restoration stayed ON, equal to
    what a session with the job's configuration reports for the same frames; without the option no line has the field"""
    import av1stream
    import deint_clips as K
    w, h, n, q, G, S = 192, 136, 6, 60, 3, 2
    clip = [np.concatenate([a, a[:2]]) for a in _half_flat(w, h, 8)]      # four frames, then two of them again
    K.write_y4m(tmp_path / "clip.y4m", clip, 8, interlace="p")
    lines = {}
    for name, extra in (("on", ["-av1mi_lr_search", 1]), ("off", [])):
        code, err = av1stream.run_transcode(["-i", tmp_path / "clip.y4m", "-global_quality:v:0", q, "-g", G, "-av1mi_segments", S, "-av1mi_stats", tmp_path / (name + ".txt")] + extra +
                                            [tmp_path / (name + ".mkv")])
        assert code == 0, err
        lines[name] = [l for l in (tmp_path / (name + ".txt")).read_text().splitlines() if l.startswith("n:")]
    assert len(lines["on"]) == n and not any(" lr:" in l for l in lines["off"])
    got = {int(l.split()[0][2:]): l.split(" lr:")[1].split()[0] for l in lines["on"]}
    # the same frames through a session opened as the job opens it: segment s codes frames s G .. s G + G - 1
    sess = av1mi.GopSession(ctx, w, h, 8, q, G, S, gpu_entropy=1, key_block_size=32, quality_stats=1, lr_search=1)
    counts = [_units(hh, ww) for hh, ww in _dims(h, w)]
    first = np.concatenate([[0], np.cumsum(counts)])
    want = {}
    for t in range(G):
        for dst, a in zip(sess.input_planes(), clip):
            dst[:] = np.concatenate([a[s * G + t] for s in range(S)])
        sess.submit()
        fr = sess.collect()
        for s in range(S):
            filtered = sum(int((fr["lr_choice"][s, first[p]:first[p + 1]] != 0).sum()) for p in range(3) if fr["lr_on"][s, p])
            want[s * G + t] = "%d/%d" % (filtered, sum(counts))
    sess.close()
    assert got == want and sum(counts) == 10
