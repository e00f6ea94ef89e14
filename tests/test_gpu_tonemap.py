"""GPU tests of tone mapping (include/av1mi.h "tone mapping", av1mi_gop_config.tone_map; av1-go_amd/csrc/tonemap_kernels.hip): av1mi_tone_map
against tests/tonemap_ref.py, and the session's defining property — a tone_map session yields the bytes of a plain session fed the reference's
output of the same padded planes.  No tolerance anywhere: every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import tonemap_ref as R

pytestmark = pytest.mark.gpu

Q, GOP, SEGS = 128, 2, 2


def _tables(av1mi, peak):
    """the library's tables: as the structure the kernel reads, and as the reference's dictionary"""
    t = av1mi.tone_map_tables(peak)
    T = {k: np.array(getattr(t, k), np.int64) for k in ("lin", "gain", "oetf_lo", "oetf_hi")}
    K = {"to_rgb": list(t.to_rgb), "gamut": [list(r) for r in t.gamut], "to_yuv": [list(r) for r in t.to_yuv]}
    return t, T, K


def _contents(w, h, frames):
    rng = np.random.default_rng(w * 7 + h + frames)
    rows = h * frames
    rnd = lambda hh, ww: rng.integers(0, 1024, (hh, ww)).astype(np.uint16)
    yield "random", (rnd(rows, w), rnd(rows // 2, w // 2), rnd(rows // 2, w // 2))
    for v in (0, 1023):
        yield "all %d" % v, tuple(np.full(s, v, np.uint16) for s in ((rows, w), (rows // 2, w // 2), (rows // 2, w // 2)))
    sweep = ((np.arange(rows * w) * 1024) // (rows * w)).reshape(rows, w).astype(np.uint16)
    yield "neutral sweep", (sweep, np.full((rows // 2, w // 2), 512, np.uint16), np.full((rows // 2, w // 2), 512, np.uint16))


def _run(ctx, av1mi, w, h, frames, planes, d_tab):
    bufs = [ctx.to_device(p) for p in planes]
    try:
        ctx.tone_map(w, h, frames, bufs[0], bufs[1], bufs[2], d_tab)
        return [b.download(p.shape, np.uint16) for b, p in zip(bufs, planes)]
    finally:
        for b in bufs:
            b.free()


@pytest.fixture(scope="module")
def tab1000(ctx, av1mi):
    t, T, K = _tables(av1mi, 1000)
    d = ctx.to_device(np.frombuffer(bytes(t), np.uint8))
    yield d, T, K
    d.free()


@pytest.mark.parametrize("w,h,frames", [(16, 8, 1), (24, 16, 3), (20, 6, 3), (12, 4, 1), (136, 72, 1), (136, 72, 3)])
def test_tone_map_is_the_reference(ctx, av1mi, tab1000, w, h, frames):
    """16x8: two whole cells a row; 24x16: three; 20 and 12 wide: rows of 40 and 24 bytes end in half a cell; 136x72: more than one workgroup"""
    d_tab, T, K = tab1000
    for name, planes in _contents(w, h, frames):
        want = R.tone_map(*planes, T, K)
        got = _run(ctx, av1mi, w, h, frames, planes, d_tab)
        for p in range(3):
            assert np.array_equal(got[p], want[p]), "%dx%d x %d, %s: plane %d differs from the reference" % (w, h, frames, name, p)
        if name == "neutral sweep":
            assert (got[1] == 512).all() and (got[2] == 512).all()


@pytest.mark.parametrize("peak", [400, 10000])
def test_every_luma_code_against_swept_chroma(ctx, av1mi, peak):
    """2048x8: all 1024 Y codes twice in every row, U sweeping along the rows and V down them"""
    t, T, K = _tables(av1mi, peak)
    w, h = 2048, 8
    Y = np.tile(np.arange(w) % 1024, (h, 1)).astype(np.uint16)
    U = np.tile((np.arange(w // 2) * 1023) // (w // 2 - 1), (h // 2, 1)).astype(np.uint16)
    V = np.tile(((np.arange(h // 2) * 1023) // (h // 2 - 1))[:, None], (1, w // 2)).astype(np.uint16)
    d_tab = ctx.to_device(np.frombuffer(bytes(t), np.uint8))
    try:
        got = _run(ctx, av1mi, w, h, 1, (Y, U, V), d_tab)
    finally:
        d_tab.free()
    want = R.tone_map(Y, U, V, T, K)
    for p in range(3):
        assert np.array_equal(got[p], want[p]), "peak %d: plane %d differs from the reference" % (peak, p)


def test_tone_map_refuses_bad_arguments(ctx, av1mi, tab1000):
    d_tab = tab1000[0]
    b = ctx.alloc(4096)
    try:
        for w, h, frames in ((18, 8, 1), (16, 7, 1), (0, 8, 1), (16, 8, 0)):
            with pytest.raises(av1mi.Av1miError):
                ctx.tone_map(w, h, frames, b, b, b, d_tab)
    finally:
        b.free()


# ---------------------------------------------------------------------------------------------- the session
def _frames(w, h, seed):
    """GOP batches of SEGS stacked HDR-looking frames: smooth ramps with noise, codes over the whole range"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(GOP):
        yy, xx = np.mgrid[0:SEGS * h, 0:w]
        Y = np.clip((xx * 900) // w + (yy % h) * 2 + 3 * t + rng.integers(0, 24, (SEGS * h, w)), 0, 1023).astype(np.uint16)
        U = np.clip(300 + (xx[::2, ::2] * 400) // w + rng.integers(0, 8, (SEGS * h // 2, w // 2)), 0, 1023).astype(np.uint16)
        V = np.clip(700 - (yy[::2, ::2] % h) * 3 + rng.integers(0, 8, (SEGS * h // 2, w // 2)), 0, 1023).astype(np.uint16)
        out.append((Y, U, V))
    return out


def _outputs(s, fr):
    o = {k: fr[k].copy() for k in ("tile_size", "tile_payload", "lr_on")}
    o["frame_type"] = fr["frame_type"]
    o["ref_y"], o["ref_u"], o["ref_v"] = s.download_reference()
    return o


def _session(ctx, av1mi, w, h, fed, **kw):
    s = av1mi.GopSession(ctx, w, h, 10, Q, GOP, SEGS, gpu_entropy=1, **kw)
    outs = []
    try:
        for planes in fed:
            for dst, a in zip(s.input_planes(), planes):
                dst[:] = np.asarray(a).reshape(dst.shape)
            s.submit()
            outs.append(_outputs(s, s.collect()))
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    return outs


def _same(base, got, what):
    assert len(base) == len(got) == GOP and [o["frame_type"] for o in base] == [0, 1]
    for t, (a, b) in enumerate(zip(base, got)):
        for k in a:
            assert np.array_equal(a[k], b[k]), "%s: batch %d, %s differs from the plain session fed the reference's output" % (what, t, k)


@pytest.fixture(scope="module")
def plain(ctx, av1mi):
    """64x64 frames, their tone-mapped twins (peak 1000: the default) and the plain session's output for those"""
    _, T, K = _tables(av1mi, 1000)
    frames = _frames(64, 64, 11)
    mapped = [R.tone_map(*f, T, K) for f in frames]
    return frames, mapped, _session(ctx, av1mi, 64, 64, mapped)


def test_session_fed_planar(ctx, av1mi, plain):
    frames, mapped, base = plain
    assert not all(np.array_equal(a, b) for f, m in zip(frames, mapped) for a, b in zip(f, m))
    _same(base, _session(ctx, av1mi, 64, 64, frames, tone_map=1), "planar")
    _same(base, _session(ctx, av1mi, 64, 64, frames, tone_map=1, tone_map_peak=1000), "planar, peak given")


def test_session_fed_packed10(ctx, av1mi, plain):
    frames, mapped, base = plain
    import input_formats_ref as F
    fed = [av1mi.input_pack(F.PACKED10, 10, *f) for f in frames]
    _same(base, _session(ctx, av1mi, 64, 64, fed, tone_map=1, input_format=F.PACKED10), "PACKED10")


def test_session_behind_a_scale(ctx, av1mi):
    """128x128 -> 64x64: the plain session is fed the reference's output of the planes the scaler makes (av1mi_scale_planes: the same kernel)"""
    _, T, K = _tables(av1mi, 1000)
    big = _frames(128, 128, 12)
    small = []
    for f in big:
        src = [ctx.to_device(a) for a in f]
        dst = [ctx.alloc(n) for n in (SEGS * 64 * 64 * 2, SEGS * 32 * 32 * 2, SEGS * 32 * 32 * 2)]
        try:
            ctx.scale_planes(10, 128, 128, 64, 64, SEGS, src, dst)
            small.append([d.download(s, np.uint16) for d, s in zip(dst, ((SEGS * 64, 64), (SEGS * 32, 32), (SEGS * 32, 32)))])
        finally:
            for b in src + dst:
                b.free()
    base = _session(ctx, av1mi, 64, 64, [R.tone_map(*f, T, K) for f in small])
    _same(base, _session(ctx, av1mi, 64, 64, big, tone_map=1, source=(128, 128)), "behind a 2:1 scale")


def test_session_from_the_frame_store(ctx, av1mi, plain):
    frames, mapped, base = plain
    s = av1mi.GopSession(ctx, 64, 64, 10, Q, GOP, SEGS, gpu_entropy=1, tone_map=1, store_frames=SEGS * GOP)
    got = []
    try:
        # the store's run in file order: segment sg holds frames sg * GOP + t
        for sg in range(SEGS):
            for t in range(GOP):
                for dst, a, rows in zip(s.input_planes(), frames[t], (64, 32, 32)):
                    dst[:rows] = a[sg * rows:(sg + 1) * rows]
                s.store_put(0, sg * GOP + t, 1)
        for t in range(GOP):
            s.submit_stored(0, [sg * GOP + t for sg in range(SEGS)], 0 if t == 0 else 1)
            got.append(_outputs(s, s.collect()))
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    _same(base, got, "from the frame store")


def test_session_refusals(ctx, av1mi):
    def refused(why, **kw):
        bd = kw.pop("bd", 10)
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, 64, 64, bd, Q, GOP, SEGS, gpu_entropy=1, **kw).close()
        assert e.value.code == -1 and why in str(e.value), (why, str(e.value))      # AV1MI_E_INVAL
    refused("tone_map needs bit_depth 10", bd=8, tone_map=1)
    refused("together with denoise", tone_map=1, denoise=4, store_frames=4)
    refused("tone_map_peak 50 out of range", tone_map=1, tone_map_peak=50)
    refused("tone_map_peak 1000 needs tone_map", tone_map_peak=1000)
    refused("tone_map 2 unknown", tone_map=2)
    s = av1mi.GopSession(ctx, 64, 64, 10, Q, GOP, SEGS, gpu_entropy=1, tone_map=1)
    try:
        b = ctx.alloc(SEGS * 64 * 64 * 2)
        try:
            with pytest.raises(av1mi.Av1miError) as e:
                s.submit_device(b, b, b, 0)
            assert e.value.code == -1 and "overwrite the caller's planes" in str(e.value)
        finally:
            b.free()
    finally:
        s.close()
