"""GPU: GOP sessions with the three filter searches together (lf_search, cdef_search, lr_search), on the two paths no other test takes
them down: the padded path at 10 bit (the unfused deblocking and CDEF launches with the per-frame maps, every sum stopping at the true
size), and more batches in flight than the session has slots, where every batch's results travel through its slot's mirrors."""
import numpy as np
import pytest

import dav1d_ref as D
from test_gpu_session_lf_search import _decodes_to, _planes

pytestmark = pytest.mark.gpu

SEARCHES = dict(lf_search=1, cdef_search=2, lr_search=1)
ARRAYS = ("lr_units0", "lr_units1", "lr_units2", "lr_choice", "cdef_idx", "lf_levels", "lf_choice")


def _results(fr):
    """a collected batch's search arrays (and the coder's tile sizes and payloads), copied out: the views are the slot's pinned memory"""
    out = {"lr_units%d" % p: fr["lr_units"][p].copy() for p in range(3)}
    out.update({k: fr[k].copy() for k in ("lr_choice", "cdef_idx", "lf_levels", "lf_choice", "tile_size", "tile_payload")})
    return out


def test_three_searches_on_the_padded_path(ctx, av1mi):
    """true size 130 x 70 coded as 136 x 72 at 10 bit, the quantiser changing per batch: every segment's stream decodes in dav1d to the
    session's references over the true size, and every batch carries all the searches' arrays in the shapes the binding documents"""
    import av1stream
    w, h, vw, vh, bd, nt, S = 136, 72, 130, 70, 10, 3, 2
    segs = _planes(w, h, bd)
    sess = av1mi.GopSession(ctx, w, h, bd, 128, nt, S, gpu_entropy=1, key_block_size=8, visible=(vw, vh), **SEARCHES)
    streams, refs = [b""] * S, []
    for t, q in enumerate((60, 150, 100)):
        sess.set_q(q)
        for i, dst in enumerate(sess.input_planes()):
            dst[:] = np.concatenate([segs[s][t][i] for s in range(S)])
        sess.submit()
        fr = sess.collect()
        units = [2, 1, 1]      # 64 x 64 restoration units of 136 x 72 luma, 68 x 36 chroma
        assert [a.shape for a in fr["lr_units"]] == [(S, n, 8) for n in units] and fr["lr_choice"].shape == (S, sum(units))
        assert fr["cdef_bits"] == 2 and fr["cdef_idx"].shape == (S, 3 * 2) and fr["cdef_idx"].max() < 4
        assert fr["lf_levels"].shape == (S, 4) and fr["lf_choice"].shape == (S, 2) and fr["lf_choice"].max() < 8
        for s in range(S):
            streams[s] += av1stream.session_temporal_unit(w, h, bd, fr["raw"], s, with_sequence_header=(t == 0), visible=(vw, vh))
        refs.append(sess.download_reference())
    assert sess.entropy_fallbacks() == 0
    sess.close()
    assert D.available(), "dav1d is what this test checks the streams with"
    _decodes_to(streams, refs, h, nt, vh, vw)


def _batches(ctx, av1mi, segs, qs, in_flight):
    """len(qs) batches with at most in_flight of them submitted and not yet collected; every batch's results in submission order"""
    w, h, bd, S = 192, 128, 8, 2
    sess = av1mi.GopSession(ctx, w, h, bd, 128, len(qs), S, gpu_entropy=1, key_block_size=8, **SEARCHES)
    assert in_flight < sess.max_in_flight() < len(qs)
    got, pending = [], 0
    for t, q in enumerate(qs):
        if pending == in_flight:
            got.append(_results(sess.collect()))
            pending -= 1
        sess.set_q(q)
        for i, dst in enumerate(sess.input_planes()):
            dst[:] = np.concatenate([segs[s][t][i] for s in range(S)])
        sess.submit()
        pending += 1
    while pending:
        got.append(_results(sess.collect()))
        pending -= 1
    assert sess.entropy_fallbacks() == 0
    sess.close()
    return got


def test_slot_mirrors_under_pipelining(ctx, av1mi):
    """5 batches through 3 slots, in lockstep and with two batches in flight: every batch collects the same arrays either way.  Batches
    that share a slot (t and t - 3) differ in their search arrays in the lockstep run itself, so a mirror that kept an earlier batch's
    bytes would show"""
    qs = (60, 150, 100, 128, 40)
    segs = _planes(192, 128, 8, len(qs))
    lock, piped = _batches(ctx, av1mi, segs, qs, 1), _batches(ctx, av1mi, segs, qs, 2)
    for t in (3, 4):
        assert (lock[t]["lf_levels"] != lock[t - 3]["lf_levels"]).any(), t
        assert any((lock[t][k] != lock[t - 3][k]).any() for k in ARRAYS if k != "lf_levels"), t
    for t in range(len(qs)):
        for k in lock[t]:
            assert lock[t][k].shape == piped[t][k].shape and (lock[t][k] == piped[t][k]).all(), (t, k)
