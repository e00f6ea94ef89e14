"""GPU: GOP sessions with lf_search (av1mi_gop_config.lf_search): every segment's stream, built by av1mi_session_temporal_unit from the
collected batch (whose frame header then carries the segment's own levels), decodes in dav1d to the session's references — on the
fused path, the padded path, with the two other searches and with a quantiser that changes between batches; a session with lf_search = 0
produces the bytes of a session opened without the field; a transcode job with -av1mi_lf_search 1 writes the lf: field.  (The binding
cannot fetch a session's reconstruction, so the levels are checked for membership in the candidates and for differing between the
segments; the stage entry is pinned bit for bit in test_gpu_lf_search.py.)"""
import numpy as np
import pytest

import dav1d_ref as D
import lf_search_ref as R

pytestmark = pytest.mark.gpu


def _planes(w, h, bd, n=4):
    """per segment a list of n frames (Y, U, V): segment 0 synthetic motion; segment 1 flat blocks with small steps, drifting"""
    import synth
    a = [np.array(p) for p in synth.frames(w, h, n, bd, 11)]
    seg0 = [[p[t] for p in a] for t in range(n)]
    rng = np.random.default_rng(bd)
    base = R.content(1, rng, w + 16, h + 16, bd)[0]
    seg1 = [[np.ascontiguousarray(p[t >> (i > 0):(t >> (i > 0)) + (h >> (i > 0)), :w >> (i > 0)]) for i, p in enumerate(base)] for t in range(n)]
    return [seg0, seg1]


def _run(ctx, av1mi, w, h, bd, q, segs, lf_search, key_block_size, nt=3, visible=None, qs=None, **kw):
    """2 segments x nt frames with the GPU coder; returns per segment the stream, per frame the references, per frame (levels, choice)"""
    import av1stream
    S = len(segs)
    if lf_search is not None:
        kw["lf_search"] = lf_search
    sess = av1mi.GopSession(ctx, w, h, bd, q, nt, S, gpu_entropy=1, key_block_size=key_block_size, visible=visible, **kw)
    streams, refs, picks = [b""] * S, [], []
    for t in range(nt):
        if qs:
            sess.set_q(qs[t])
        for i, dst in enumerate(sess.input_planes()):
            dst[:] = np.concatenate([segs[s][t][i] for s in range(S)])
        sess.submit()
        fr = sess.collect()
        for s in range(S):
            streams[s] += av1stream.session_temporal_unit(w, h, bd, fr["raw"], s, with_sequence_header=(t == 0), visible=visible)
        refs.append(sess.download_reference())
        if lf_search:
            p = fr["params"]
            assert fr["lf_levels"].shape == (S, 4) and fr["lf_choice"].shape == (S, 2) and fr["lf_choice"].max() < 8
            for s in range(S):      # the levels are the chosen candidates' of the batch's policy levels (its frame type and quantiser)
                cy, cc = (int(x) for x in fr["lf_choice"][s])
                assert fr["lf_levels"][s].tolist() == av1mi.lf_search_levels(p, cy)[:2] + av1mi.lf_search_levels(p, cc)[2:], (t, s)
            picks.append((fr["lf_levels"].copy(), fr["lf_choice"].copy()))
        else:
            assert "lf_levels" not in fr and "lf_choice" not in fr
    assert sess.entropy_fallbacks() == 0
    sess.close()
    return streams, refs, picks


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


def _segments_differ(picks):
    return any((lv[0] != lv[1]).any() for lv, _ in picks)


@pytest.mark.parametrize("bd,kbs", [(8, 8), (10, 32)])
@pytest.mark.parametrize("q", [128, 40])
def test_session_with_the_search(ctx, av1mi, bd, kbs, q):
    w, h, nt = 192, 128, 3
    streams, refs, picks = _run(ctx, av1mi, w, h, bd, q, _planes(w, h, bd), 1, kbs)
    assert _segments_differ(picks), [lv.tolist() for lv, _ in picks]
    assert D.available(), "dav1d is what this test checks the streams with"
    _decodes_to(streams, refs, h, nt)


def test_session_on_the_padded_path(ctx, av1mi):
    """true size 130 x 70 coded as 136 x 72: the unfused deblocking launches take the per-frame maps, the sums stop at the true size"""
    w, h, bd, q, nt = 136, 72, 8, 128, 3
    streams, refs, picks = _run(ctx, av1mi, w, h, bd, q, _planes(w, h, bd), 1, 8, visible=(130, 70))
    assert D.available(), "dav1d is what this test checks the streams with"
    _decodes_to(streams, refs, h, nt, 70, 130)


def test_session_with_the_two_other_searches(ctx, av1mi):
    w, h, bd, q, nt = 192, 128, 8, 128, 3
    streams, refs, picks = _run(ctx, av1mi, w, h, bd, q, _planes(w, h, bd), 1, 32, cdef_search=2, lr_search=1)
    assert D.available(), "dav1d is what this test checks the streams with"
    _decodes_to(streams, refs, h, nt)


def test_session_whose_quantiser_changes_between_batches(ctx, av1mi):
    w, h, bd, nt = 192, 128, 10, 3
    streams, refs, picks = _run(ctx, av1mi, w, h, bd, 128, _planes(w, h, bd), 1, 32, qs=[60, 150, 100])
    assert D.available(), "dav1d is what this test checks the streams with"
    _decodes_to(streams, refs, h, nt)


def test_search_off_is_the_session_without_the_field(ctx, av1mi):
    w, h, bd, q = 192, 128, 8, 128
    segs = _planes(w, h, bd)
    off, refs_off, _ = _run(ctx, av1mi, w, h, bd, q, segs, 0, 32)
    plain, refs_plain, _ = _run(ctx, av1mi, w, h, bd, q, segs, None, 32)
    assert off == plain and all((a == b).all() for x, y in zip(refs_off, refs_plain) for a, b in zip(x, y))
    on, _, picks = _run(ctx, av1mi, w, h, bd, q, segs, 1, 32)
    assert on != plain and any(ch.any() for _, ch in picks)


def test_config_outside_0_and_1_is_refused(ctx, av1mi):
    for bad in (2, -1):
        with pytest.raises(av1mi.Av1miError):
            av1mi.GopSession(ctx, 192, 128, 8, 100, 3, 1, lf_search=bad)


def test_transcode_job_with_the_search_writes_the_lf_field(ctx, av1mi, tmp_path):
    import av1stream
    import deint_clips as K
    w, h, n, q, G, S = 192, 136, 6, 128, 3, 2
    seg0 = _planes(w, h, 8, 6)[0]
    clip = [np.stack([fr[i] for fr in seg0]) for i in range(3)]
    K.write_y4m(tmp_path / "clip.y4m", clip, 8, interlace="p")
    lines = {}
    for name, extra in (("on", ["-av1mi_lf_search", 1]), ("off", [])):
        code, err = av1stream.run_transcode(["-i", tmp_path / "clip.y4m", "-global_quality:v:0", q, "-g", G, "-av1mi_segments", S, "-av1mi_stats", tmp_path / (name + ".txt")] + extra +
                                            [tmp_path / (name + ".mkv")])
        assert code == 0, err
        lines[name] = [l for l in (tmp_path / (name + ".txt")).read_text().splitlines() if l.startswith("n:")]
    assert len(lines["on"]) == n and not any(" lf:" in l for l in lines["off"])
    for l in lines["on"]:
        a, b = l.split(" lf:")[1].split()[0].split("/")
        assert 0 <= int(a) <= 63 and 0 <= int(b) <= 63
    assert (tmp_path / "on.mkv").stat().st_size > 0
    assert D.available(), "dav1d is what this test checks the stream with"
    from test_mux import read_mkv      # the track's blocks behind the sequence header of its codec private data (av1C: 4 bytes, then the OBUs)
    _, tracks, blocks = read_mkv(tmp_path / "on.mkv")
    video = [b for b in blocks if b["track"] == 1]
    assert len(video) == n and len(D.decode(tracks[1][0x63A2][4:] + b"".join(b["data"] for b in video))) == n
