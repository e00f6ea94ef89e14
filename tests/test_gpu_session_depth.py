"""GPU tests of the depth reduction inside the GOP session (av1mi_gop_config.coded_bit_depth / depth_dither).  The oracle is a plain 8-bit
session — code that does not know the option — fed the planes tests/depth_ref.py makes of the 10-bit source: the session with the option must
hand out its payloads and reference frames byte for byte.  No tolerance anywhere."""
import numpy as np
import pytest

import depth_ref as R

pytestmark = pytest.mark.gpu

W, H, GOP, SEGS = 72, 40, 3, 2


def _frames(w, h, seed, lo=0, hi=1023):
    """GOP batches of SEGS stacked 10-bit frames: a moving ramp with noise, codes over the whole range"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(GOP):
        yy, xx = np.mgrid[0:SEGS * h, 0:w]
        Y = np.clip(lo + ((xx + 2 * t) * (hi - lo)) // w + (yy % h) * 3 + rng.integers(0, 12, (SEGS * h, w)), 0, 1023).astype(np.uint16)
        U = np.clip(300 + (xx[::2, ::2] * 400) // w + t + rng.integers(0, 6, (SEGS * h // 2, w // 2)), 0, 1023).astype(np.uint16)
        V = np.clip(720 - (yy[::2, ::2] % h) * 5 + rng.integers(0, 6, (SEGS * h // 2, w // 2)), 0, 1023).astype(np.uint16)
        out.append((Y, U, V))
    return out


def _outputs(s, fr):
    o = {k: fr[k].copy() for k in ("tile_size", "tile_payload", "lr_on")}
    o["frame_type"], o["bit_depth"] = fr["frame_type"], fr["raw"].bit_depth
    p = fr["params"]
    o["header"] = (p.base_q_idx, list(p.lf_level), p.cdef_y, p.cdef_uv, p.cdef_damping)
    o["quality"] = fr["quality"].copy() if "quality" in fr else None
    o["ref_y"], o["ref_u"], o["ref_v"] = s.download_reference()
    return o


def _session(ctx, av1mi, bd, fed, q=60, w=W, h=H, device=False, units=None, qs=None, **kw):
    """the batches of `fed` through a session; device: through av1mi_gop_submit_device; units: a list that receives the temporal units of
    segment 0; qs: a quantiser per batch (av1mi_gop_set_base_q_idx)"""
    import av1stream
    s = av1mi.GopSession(ctx, w, h, bd, q, GOP, SEGS, gpu_entropy=1, **kw)
    outs, bufs = [], []
    try:
        for t, planes in enumerate(fed):
            if qs:
                s.set_q(qs[t])
            if device:
                bufs = [ctx.to_device(np.ascontiguousarray(a)) for a in planes]
                s.submit_device(*bufs)
            else:
                for dst, a in zip(s.input_planes(), planes):
                    dst[:] = np.asarray(a).reshape(dst.shape)
                s.submit()
            fr = s.collect()
            outs.append(_outputs(s, fr))
            if units is not None:
                units.append(av1stream.session_temporal_unit(w, h, fr["raw"].bit_depth, fr["raw"], 0, with_sequence_header=(t == 0), visible=kw.get("visible")))
            if device:
                for b, a in zip(bufs, planes):
                    assert np.array_equal(b.download(a.shape, a.dtype), a), "the session wrote the caller's planes"
                    b.free()
                bufs = []
        assert s.entropy_fallbacks() == 0
    finally:
        for b in bufs:
            b.free()
        s.close()
    return outs


def _same(base, got, what):
    assert len(base) == len(got) == GOP and [o["frame_type"] for o in base] == [0, 1, 1]
    for t, (a, b) in enumerate(zip(base, got)):
        assert b["bit_depth"] == 8 and b["ref_y"].dtype == np.uint8
        for k in a:
            if a[k] is not None and k != "quality":
                assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], "%s: batch %d, %s differs from the plain 8-bit session fed the reference's output" % (what, t, k)


@pytest.fixture(scope="module")
def source():
    return _frames(W, H, 5)


@pytest.mark.parametrize("q", [60, 24])
@pytest.mark.parametrize("mode", [R.ROUND, R.ORDERED])
def test_session_equals_the_plain_8_bit_session(ctx, av1mi, source, mode, q):
    reduced = [R.reduce(*f, mode) for f in source]
    assert all(a.dtype == np.uint8 for f in reduced for a in f)
    base = _session(ctx, av1mi, 8, reduced, q)
    assert all(o["bit_depth"] == 8 for o in base)
    _same(base, _session(ctx, av1mi, 10, source, q, coded_bit_depth=8, depth_dither=mode), "submit, mode %d, q %d" % (mode, q))
    _same(base, _session(ctx, av1mi, 10, source, q, device=True, coded_bit_depth=8, depth_dither=mode), "submit_device, mode %d, q %d" % (mode, q))
    if mode == R.ORDERED and q == 60:      # the two modes are two streams
        other = _session(ctx, av1mi, 10, source, q, coded_bit_depth=8, depth_dither=R.ROUND)
        assert not np.array_equal(other[0]["ref_y"], base[0]["ref_y"])


def test_behind_a_crop_window(ctx, av1mi):
    """fed whole 96x56 frames, the window 72x40+8+6 of them is what is reduced and coded"""
    big = _frames(96, 56, 6)
    x, y = 8, 6
    window = []
    for Y, U, V in big:
        cut = lambda a, rows, r0, c0, h, w: np.concatenate([a[sg * rows + r0:sg * rows + r0 + h, c0:c0 + w] for sg in range(SEGS)])
        window.append((cut(Y, 56, y, x, H, W), cut(U, 28, y // 2, x // 2, H // 2, W // 2), cut(V, 28, y // 2, x // 2, H // 2, W // 2)))
    base = _session(ctx, av1mi, 8, [R.reduce(*f, R.ORDERED) for f in window])
    _same(base, _session(ctx, av1mi, 10, big, source=(96, 56), crop=(x, y, W, H), coded_bit_depth=8, depth_dither=R.ORDERED), "behind a crop window")


def test_behind_the_tone_map(ctx, av1mi, source):
    import tonemap_ref as TM
    t = av1mi.tone_map_tables(1000)
    T = {k: np.array(getattr(t, k), np.int64) for k in ("lin", "gain", "oetf_lo", "oetf_hi")}
    K = {"to_rgb": list(t.to_rgb), "gamut": [list(r) for r in t.gamut], "to_yuv": [list(r) for r in t.to_yuv]}
    mapped = [tuple(np.asarray(a).astype(np.uint16) for a in TM.tone_map(*f, T, K)) for f in source]
    base = _session(ctx, av1mi, 8, [R.reduce(*f, R.ORDERED) for f in mapped])
    _same(base, _session(ctx, av1mi, 10, source, tone_map=1, coded_bit_depth=8, depth_dither=R.ORDERED), "behind the tone map")


@pytest.mark.parametrize("visible", [None, (70, 38)])
def test_dav1d_decodes_an_8_bit_stream_to_the_references(ctx, av1mi, source, visible):
    """... also at a true size that is not a multiple of 8 (70x38 in 72x40: the caller replicates the edge into the padding, at 10 bits)"""
    import dav1d_ref as D
    fed = source
    if visible:
        vw, vh = visible
        fed = []
        for Y, U, V in source:
            Y, U, V = Y.copy(), U.copy(), V.copy()
            for a, w, h, rows in ((Y, vw, vh, H), (U, vw // 2, vh // 2, H // 2), (V, vw // 2, vh // 2, H // 2)):
                a[:, w:] = a[:, w - 1:w]
                for sg in range(SEGS):
                    a[sg * rows + h:(sg + 1) * rows] = a[sg * rows + h - 1]
            fed.append((Y, U, V))
    kw = dict(visible=visible) if visible else {}
    base = _session(ctx, av1mi, 8, [R.reduce(*f, R.ORDERED) for f in fed], **kw)
    units = []
    got = _session(ctx, av1mi, 10, fed, units=units, coded_bit_depth=8, depth_dither=R.ORDERED, **kw)
    _same(base, got, "true size %s" % (visible,))
    assert D.available(), "dav1d is what this test is about"
    dec = D.decode(b"".join(units))
    assert len(dec) == GOP
    vw, vh = visible or (W, H)
    for t in range(GOP):
        for p, k in enumerate(("ref_y", "ref_u", "ref_v")):
            h, w = (vh, vw) if p == 0 else ((vh + 1) // 2, (vw + 1) // 2)
            assert dec[t][p].dtype == np.uint8, "dav1d does not see an 8-bit stream"
            assert np.array_equal(dec[t][p][:h, :w], got[t][k][:h, :w]), "frame %d plane %d: dav1d decodes something else" % (t, p)


def test_quality_records_measure_against_the_8_bit_planes(ctx, av1mi, source):
    import quality_ref as QR
    reduced = [R.reduce(*f, R.ORDERED) for f in source]
    got = _session(ctx, av1mi, 10, source, quality_stats=1, coded_bit_depth=8, depth_dither=R.ORDERED)
    for t in range(GOP):
        for sg in range(SEGS):
            src = [a[sg * r:(sg + 1) * r] for a, r in zip(reduced[t], (H, H // 2, H // 2))]
            dec = [got[t][k][sg * r:(sg + 1) * r] for k, r in zip(("ref_y", "ref_u", "ref_v"), (H, H // 2, H // 2))]
            want = QR.frame(src, dec, 8)
            rec = got[t]["quality"][sg]
            assert rec["sse"].tolist() == want["sse"].tolist() and rec["samples"].tolist() == want["samples"].tolist(), (t, sg)
            assert av1mi.quality_psnr(rec, 8) == pytest.approx(QR.psnr(want, 8), rel=1e-12)
            for p in range(3):
                assert av1mi.quality_ssim(rec[p]) == pytest.approx(QR.ssim(want[p]), abs=1e-9)


def test_rate_controlled_session(ctx, av1mi, source):
    """a quantiser per batch: the policy and the quantiser tables follow it at the CODED depth"""
    qs = [60, 90, 40]
    reduced = [R.reduce(*f, R.ORDERED) for f in source]
    base = _session(ctx, av1mi, 8, reduced, qs=qs)
    got = _session(ctx, av1mi, 10, source, qs=qs, coded_bit_depth=8, depth_dither=R.ORDERED)
    _same(base, got, "a quantiser per batch")
    for t, q in enumerate(qs):      # what the frame header carries is the 8-bit policy's
        p8 = av1mi.policy_frame_params(q, 8, 0 if t == 0 else 1)
        assert got[t]["header"] == (q, list(p8.lf_level), p8.cdef_y, p8.cdef_uv, p8.cdef_damping)


def test_without_the_option_nothing_changes(ctx, av1mi, source):
    """coded_bit_depth 0 (and bit_depth itself) = a config that never heard of the fields"""
    base = _session(ctx, av1mi, 10, source)
    assert all(o["bit_depth"] == 10 and o["ref_y"].dtype == np.uint16 for o in base)
    for kw in (dict(coded_bit_depth=0, depth_dither=0), dict(coded_bit_depth=10)):
        got = _session(ctx, av1mi, 10, source, **kw)
        for t in range(GOP):
            for k in base[t]:
                if base[t][k] is not None:
                    assert np.array_equal(base[t][k], got[t][k]) if isinstance(base[t][k], np.ndarray) else base[t][k] == got[t][k], (kw, t, k)


def test_refusals_at_open(ctx, av1mi):
    def refused(why, bd=10, **kw):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, W, H, bd, 60, GOP, SEGS, gpu_entropy=1, **kw).close()
        assert e.value.code == -1 and why in str(e.value), (why, str(e.value))
    refused("coded_bit_depth 9 not supported", coded_bit_depth=9)
    refused("nothing to reduce", bd=8, coded_bit_depth=8)
    refused("depth_dither 1 needs coded_bit_depth 8", depth_dither=1)
    refused("depth_dither 2 unknown", coded_bit_depth=8, depth_dither=2)
    refused("together with denoise", coded_bit_depth=8, denoise=4, store_frames=4)
