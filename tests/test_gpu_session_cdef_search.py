"""GPU: GOP sessions with cdef_search (av1mi_gop_config.cdef_search): the GPU-coded stream decodes in dav1d to the session's references,
the host writer given the collected symbols and cdef_idx produces the same bytes, a session with cdef_search = 0 produces the bytes
of a session opened without the field, and a transcode job with -av1mi_cdef_search writes the cdef: field.  (The binding cannot fetch a
session's deblocked planes, so the indices are checked for range and for leaving set 0; the stage entry is pinned bit for bit in
test_gpu_cdef_search.py.)"""
import numpy as np
import pytest

import dav1d_ref as D

pytestmark = pytest.mark.gpu


def _planes(w, h, bd):
    """four frames: synthetic motion, the left third flat, so that the superblocks cannot all choose alike"""
    import synth
    planes = [np.array(a) for a in synth.frames(w, h, 4, bd, 11)]
    for a in planes:
        a[:, :, :a.shape[2] // 3] = a[:, :, :a.shape[2] // 3].mean().astype(a.dtype)
    return planes


def _run(ctx, av1mi, w, h, bd, q, planes, gpu_entropy, cdef_search, key_block_size, nt=3, S=2, visible=None):
    """S segments x nt frames; returns per segment the stream, per frame the references, per frame the collected indices"""
    import av1stream
    kw = {} if cdef_search is None else dict(cdef_search=cdef_search)
    sess = av1mi.GopSession(ctx, w, h, bd, q, nt, S, gpu_entropy=gpu_entropy, key_block_size=key_block_size, visible=visible, **kw)
    streams, refs, idx = [b""] * S, [], []
    for t in range(nt):
        for dst, a in zip(sess.input_planes(), planes):
            dst[:] = np.concatenate([a[(t + s) % len(a)] for s in range(S)])
        sess.submit()
        fr = sess.collect()
        for s in range(S):
            streams[s] += av1stream.session_temporal_unit(w, h, bd, fr["raw"], s, with_sequence_header=(t == 0), visible=visible)
        refs.append(sess.download_reference())
        if cdef_search:
            assert fr["cdef_bits"] == cdef_search
            p = fr["params"]
            assert (fr["cdef_y"], fr["cdef_uv"]) == av1mi.cdef_search_sets(p, cdef_search) and fr["cdef_y"][0] == p.cdef_y
            idx.append(fr["cdef_idx"].copy())
        else:
            assert "cdef_idx" not in fr
    assert sess.entropy_fallbacks() == 0
    sess.close()
    return streams, refs, idx


def _decodes_to(streams, refs, h, nt, vh=None, vw=None):
    for s, stream in enumerate(streams):
        got = D.decode(stream)
        assert len(got) == nt
        for t in range(nt):
            for p in range(3):
                hp = h >> (p > 0)
                ref = refs[t][p][s * hp:(s + 1) * hp]
                if vh is not None:
                    ref = ref[:(vh + (p > 0)) >> (p > 0), :(vw + (p > 0)) >> (p > 0)]
                assert (np.asarray(got[t][p]) == ref).all(), (s, t, p)


@pytest.mark.parametrize("bd,kbs", [(8, 8), (10, 32)])
@pytest.mark.parametrize("q,bits", [(128, 3), (40, 2)])
def test_session_with_the_search(ctx, av1mi, bd, kbs, q, bits):
    w, h, nt = 192, 128, 3
    planes = _planes(w, h, bd)
    gpu, refs, idx = _run(ctx, av1mi, w, h, bd, q, planes, 1, bits, kbs)
    host, refs0, idx0 = _run(ctx, av1mi, w, h, bd, q, planes, 0, bits, kbs)
    assert gpu == host, "GPU-coded tiles and the host writer disagree"
    assert all((a == b).all() for x, y in zip(refs, refs0) for a, b in zip(x, y)) and all((a == b).all() for a, b in zip(idx, idx0))
    assert all(i.shape == (2, 6) and i.max() < (1 << bits) for i in idx) and any(i.any() for i in idx)
    if D.available():
        _decodes_to(gpu, refs, h, nt)


def test_session_on_the_padded_path(ctx, av1mi):
    """true size 200 x 132 coded as 200 x 136: partial superblocks at both edges, the sums stop at the true size"""
    w, h, bd, q, nt = 200, 136, 8, 128, 3
    planes = _planes(w, h, bd)
    gpu, refs, idx = _run(ctx, av1mi, w, h, bd, q, planes, 1, 3, 8, visible=(200, 132))
    host, _, idx0 = _run(ctx, av1mi, w, h, bd, q, planes, 0, 3, 8, visible=(200, 132))
    assert gpu == host and all((a == b).all() for a, b in zip(idx, idx0))
    assert all(i.shape == (2, 12) and i.max() < 8 for i in idx) and any(i.any() for i in idx)
    if D.available():
        _decodes_to(gpu, refs, h, nt, 132, 200)


def test_search_off_is_the_session_without_the_field(ctx, av1mi):
    w, h, bd, q = 192, 128, 8, 128
    planes = _planes(w, h, bd)
    off, refs_off, _ = _run(ctx, av1mi, w, h, bd, q, planes, 1, 0, 32)
    plain, refs_plain, _ = _run(ctx, av1mi, w, h, bd, q, planes, 1, None, 32)
    assert off == plain and all((a == b).all() for x, y in zip(refs_off, refs_plain) for a, b in zip(x, y))
    on, _, _ = _run(ctx, av1mi, w, h, bd, q, planes, 1, 3, 32)
    assert on != plain


def test_config_outside_0_to_3_is_refused(ctx, av1mi):
    for bad in (4, -1):
        with pytest.raises(av1mi.Av1miError):
            av1mi.GopSession(ctx, 192, 128, 8, 100, 3, 1, cdef_search=bad)


def test_transcode_job_with_the_search_writes_the_cdef_field(ctx, av1mi, tmp_path):
    import av1stream
    import deint_clips as K
    w, h, n, q, G, S = 192, 136, 6, 128, 3, 2
    clip = [np.concatenate([a, a[:2]]) for a in _planes(w, h, 8)]
    K.write_y4m(tmp_path / "clip.y4m", clip, 8, interlace="p")
    lines = {}
    for name, extra in (("on", ["-av1mi_cdef_search", 3]), ("off", [])):
        code, err = av1stream.run_transcode(["-i", tmp_path / "clip.y4m", "-global_quality:v:0", q, "-g", G, "-av1mi_segments", S, "-av1mi_stats", tmp_path / (name + ".txt")] + extra +
                                            [tmp_path / (name + ".mkv")])
        assert code == 0, err
        lines[name] = [l for l in (tmp_path / (name + ".txt")).read_text().splitlines() if l.startswith("n:")]
    assert len(lines["on"]) == n and not any(" cdef:" in l for l in lines["off"])
    moved = 0
    for l in lines["on"]:
        a, b = l.split(" cdef:")[1].split()[0].split("/")
        assert int(b) == 9 and 0 <= int(a) <= 9
        moved += int(a)
    assert moved > 0
    assert (tmp_path / "on.mkv").stat().st_size > 0
    if D.available():      # the track's blocks behind the sequence header of its codec private data (av1C: 4 bytes, then the OBUs)
        from test_mux import read_mkv
        _, tracks, blocks = read_mkv(tmp_path / "on.mkv")
        video = [b for b in blocks if b["track"] == 1]
        assert len(video) == n and len(D.decode(tracks[1][0x63A2][4:] + b"".join(b["data"] for b in video))) == n
