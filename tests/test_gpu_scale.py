"""Scaling on the GPU (include/av1mi.h "scaling"; av1-go_amd/csrc/scale_kernels.hip): the kernel against the numpy restatement of the
definition (scale_ref.py) evaluated with the LIBRARY's coefficient table, the session fed source frames against a plain session fed
the frames numpy scaled, and the product.  No tolerance anywhere: every comparison is equality."""
import ctypes as C
import os

import numpy as np
import pytest

import input_formats_ref as F
import scale_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64      # bytes behind every output plane that the kernel must leave alone
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "av1-go_amd", "host", "libav1mi_host.so")


def _r8(n):
    return (n + 7) & ~7


def _content(kind, bd, sw, sh, frames, seed):
    """frames x (Y, U, V) at the true sizes; every frame differs (a row of the next frame leaking into a frame's last rows shows)"""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(frames):
        planes = []
        for w, h in ((sw, sh), ((sw + 1) // 2, (sh + 1) // 2), ((sw + 1) // 2, (sh + 1) // 2)):
            if kind == "random":
                a = rng.integers(0, 1 << bd, (h, w))
            elif kind == "zeros":
                a = np.zeros((h, w), np.int64)
            elif kind == "max":
                a = np.full((h, w), (1 << bd) - 1)
            else:
                a = (np.arange(h * w).reshape(h, w) * 3 + 37 * f) % (1 << bd)
            planes.append(a.astype(np.uint8 if bd == 8 else np.uint16))
        out.append(planes)
    return out


def _stack_source(frames, sw, sh, bd, fill):
    """the frames in buffers of the source size rounded up to 8, stacked; the padding holds `fill` (the kernel must not read it)"""
    dt = frames[0][0].dtype
    out = []
    for i in range(3):
        pw, ph = (_r8(sw), _r8(sh)) if i == 0 else (_r8(sw) // 2, _r8(sh) // 2)
        buf = np.full((len(frames), ph, pw), fill, dt)
        for f, planes in enumerate(frames):
            h, w = planes[i].shape
            buf[f, :h, :w] = planes[i]
        out.append(buf.reshape(len(frames) * ph, pw))
    return out


def _lib_table(av1mi):
    cache = {}

    def table(n, m):
        if (n, m) not in cache:
            cache[(n, m)] = av1mi.scale_filter(n, m)
        return cache[(n, m)]
    return table


def _expected(frames, dw, dh, bd, table):
    per = [R.scale_frame(*planes, dw, dh, bd, table) for planes in frames]
    return [np.concatenate([fr[i] for fr in per]) for i in range(3)]


def _scale(ctx, bd, sw, sh, dw, dh, src):
    """stacked source planes -> stacked coded planes through av1mi_scale_planes; checks the guard bytes behind each output"""
    dt = np.uint8 if bd == 8 else np.uint16
    frames = src[0].shape[0] // _r8(sh)
    shapes = [(frames * _r8(dh), _r8(dw))] + [(frames * _r8(dh) // 2, _r8(dw) // 2)] * 2
    d_in = [ctx.to_device(p) for p in src]
    d_out = []
    for shp in shapes:
        n = shp[0] * shp[1] * np.dtype(dt).itemsize
        b = ctx.alloc(n + GUARD)
        ctx.memset(b, 0xA5, n + GUARD)
        d_out.append(b)
    ctx.scale_planes(bd, sw, sh, dw, dh, frames, d_in, d_out)
    ctx.sync()
    out = []
    for b, shp in zip(d_out, shapes):
        n = shp[0] * shp[1] * np.dtype(dt).itemsize
        raw = b.download((n + GUARD,), np.uint8)
        assert (raw[n:] == 0xA5).all(), "the kernel wrote behind a plane"
        out.append(raw[:n].view(dt).reshape(shp))
    for b in d_in + d_out:
        b.free()
    return out


# (source, target, frames): T = 6 both ways; 6 / 8 mixed enlarging + reducing with a target that is not a multiple of 8; T = 6 with an
# odd source; the identity; T = 12; T = 10; the ratio limits 4:1 (T = 24) and 1:4; a target with padding in both directions
CASES = [((1440, 1080), (1920, 1080), 1), ((96, 80), (136, 72), 3), ((853, 480), (854, 480), 2), ((136, 72), (136, 72), 2),
         ((384, 216), (192, 108), 3), ((320, 180), (200, 110), 2), ((1024, 16), (256, 64), 2), ((135, 71), (136, 72), 2), ((200, 120), (130, 70), 3)]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("src,dst,frames", CASES)
def test_scale_planes_matches_numpy(ctx, av1mi, src, dst, frames, bd):
    (sw, sh), (dw, dh) = src, dst
    table = _lib_table(av1mi)
    for kind in ("random", "ramp", "max", "zeros"):
        fr = _content(kind, bd, sw, sh, frames, 11)
        got = _scale(ctx, bd, sw, sh, dw, dh, _stack_source(fr, sw, sh, bd, 0 if kind == "max" else (1 << bd) - 1))
        want = _expected(fr, dw, dh, bd, table)
        for p in range(3):
            assert np.array_equal(got[p], want[p]), "%s content: plane %d differs" % (kind, p)
    # the padding of the target is the replicated edge (also part of the comparison above)
    if dw & 7:
        assert (got[0][:, dw:] == got[0][:, dw - 1:dw]).all()


def test_scale_planes_tap_counts_are_covered(av1mi):
    seen = set()
    for (sw, sh), (dw, dh), _ in CASES:
        seen.add(av1mi.scale_filter(sw, dw)[0])
        seen.add(av1mi.scale_filter(max(sh, 8), max(dh, 8))[0])
    assert {6, 10, 12, 24} <= seen


def test_scale_planes_full_size_batch(ctx, av1mi):
    """3840 x 2160 -> 1920 x 1080, 12 frames, 10 bit: the batch the product scales (T = 12, the specialised kernel)"""
    sw, sh, dw, dh, frames, bd = 3840, 2160, 1920, 1080, 12, 10
    fr = _content("random", bd, sw, sh, frames, 5)
    got = _scale(ctx, bd, sw, sh, dw, dh, _stack_source(fr, sw, sh, bd, 0))
    want = _expected(fr, dw, dh, bd, _lib_table(av1mi))
    for p in range(3):
        assert np.array_equal(got[p], want[p]), "plane %d differs" % p


def test_scale_planes_refuses_bad_arguments(ctx, av1mi):
    b = ctx.alloc(1 << 20)
    try:
        for args in ((9, 64, 64, 64, 64, 1), (8, 64, 64, 300, 64, 1), (8, 300, 64, 64, 64, 1), (8, 8, 64, 16, 64, 1), (8, 4104, 64, 2048, 64, 1), (8, 64, 64, 64, 64, 0)):
            with pytest.raises(av1mi.Av1miError):
                ctx.scale_planes(*args, [b, b, b], [b, b, b])
    finally:
        b.free()


# ---- session equivalence -------------------------------------------------------------------------------------------------

def _source_batches(sw, sh, bd, segs, n, seed):
    """n batches of `segs` source frames at their true sizes; smooth moving content (synth) cropped to the true size"""
    import synth
    per = [synth.frames(_r8(sw) + 8, _r8(sh) + 8, n, bd, seed + 7 * s) for s in range(segs)]
    cw, ch = (sw + 1) // 2, (sh + 1) // 2
    return [[[per[s][0][t][:sh, :sw], per[s][1][t][:ch, :cw], per[s][2][t][:ch, :cw]] for s in range(segs)] for t in range(n)]


def _run(ctx, av1mi, w, h, bd, q, gop, segs, batches, fmt, via, mode, source=None, lag=0, visible=None, key_block_size=0, refs=True):
    """every array a session hands out per batch and, in lockstep, its reference planes; batches: per batch the stacked planes in the
    geometry the session is fed (the coded size, or the source size rounded up to 8)"""
    s = av1mi.GopSession(ctx, w, h, bd, q, gop, segs, gpu_entropy=mode, visible=visible, key_block_size=key_block_size, input_format=fmt, source=source)
    outs, held = [], []

    def take():
        fr = s.collect()
        o = {k: v.copy() for k, v in fr.items() if isinstance(v, np.ndarray)}
        o["frame_type"] = fr["frame_type"]
        if refs and lag == 0:
            o["ref_y"], o["ref_u"], o["ref_v"] = s.download_reference()
        outs.append(o)
    try:
        for planes in batches:
            wire = planes if fmt == F.PLANAR else F.pack(fmt, bd, *planes)
            if via == "submit":
                for dst, a in zip(s.input_planes(), wire):
                    dst[:] = a if fmt == F.PLANAR else a.view(np.uint8).ravel()
                s.submit()
            else:
                bufs = [ctx.to_device(a) for a in wire]
                held.append(bufs)
                s.submit_device(bufs[0], bufs[1], bufs[2] if len(bufs) > 2 else None)
            if s.pending() > lag:
                take()
        while s.pending():
            take()
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
        for bufs in held:
            for b in bufs:
                b.free()
    return outs


def _same(a, b, what):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        assert sorted(x) == sorted(y), "%s batch %d: %s vs %s" % (what, t, sorted(x), sorted(y))
        for k in x:
            assert np.array_equal(x[k], y[k]), "%s: batch %d, %s differs from the plain session fed the numpy-scaled frames" % (what, t, k)


def _check(ctx, av1mi, src, w, h, bd, q, gop, segs, n, fmts, seed, vias=("submit", "device"), modes=(1, 0), **kw):
    sw, sh = src
    vw, vh = kw.get("visible") or (w, h)
    table = _lib_table(av1mi)
    frames = _source_batches(sw, sh, bd, segs, n, seed)
    fed = [_stack_source(b, sw, sh, bd, (1 << bd) - 1) for b in frames]
    scaled = [_expected(b, vw, vh, bd, table) for b in frames]
    for mode in modes:
        base = _run(ctx, av1mi, w, h, bd, q, gop, segs, scaled, F.PLANAR, "submit", mode, **kw)
        assert ("tile_size" in base[0]) == (mode == 1) and ("ref_y" in base[0] or kw.get("lag") or not kw.get("refs", True))
        for fmt in fmts:
            for via in vias:
                got = _run(ctx, av1mi, w, h, bd, q, gop, segs, fed, fmt, via, mode, source=src, **kw)
                _same(base, got, "source %dx%d, format %d via %s, gpu_entropy %d" % (sw, sh, fmt, via, mode))


def test_scaling_session_8bit_planar_and_nv12(ctx, av1mi):
    _check(ctx, av1mi, (144, 96), 192, 128, 8, 110, 3, 2, 3, [F.PLANAR, F.NV12], 1)


def test_scaling_session_10bit_formats(ctx, av1mi):
    _check(ctx, av1mi, (270, 142), 136, 72, 10, 60, 3, 3, 3, [F.PLANAR, F.PACKED10, F.P010], 2)


def test_scaling_session_cropped_target(ctx, av1mi):
    _check(ctx, av1mi, (171, 99), 136, 72, 10, 60, 3, 2, 3, [F.PLANAR, F.PACKED10], 3, visible=(130, 70))


def test_scaling_session_key_block_size_32(ctx, av1mi):
    _check(ctx, av1mi, (360, 240), 256, 168, 10, 60, 3, 2, 3, [F.PLANAR, F.P010], 4, key_block_size=32)


@pytest.mark.parametrize("fmt,bd", [(F.PLANAR, 8), (F.PACKED10, 10), (F.NV12, 8)])
def test_scaling_three_batches_in_flight(ctx, av1mi, fmt, bd):
    """8 batches, two GOPs, submit t + 2 before collect t: the slots' source buffers, intermediate planes and scaled planes are reused
    while their previous readers may still run (the events between upload, conversion, scaling and the block pipeline)"""
    w, h, q, gop, segs, n = 328, 184, 100, 4, 3, 8
    _check(ctx, av1mi, (480, 270), w, h, bd, q, gop, segs, n, [fmt], 6, modes=(1,), lag=2, refs=False)
    _check(ctx, av1mi, (480, 270), w, h, bd, q, gop, segs, n, [fmt], 6, modes=(0,), vias=("submit",), lag=2, refs=False)


def test_identity_source_and_launch_counts(ctx, av1mi):
    """source == target scales with the unit impulse: the plain session's bytes.  A plain session launches nothing of the input kind,
    a scaling planar session one launch per batch, a scaling packed session two (conversion + scaling)"""
    w, h, bd, gop, segs = 136, 72, 10, 3, 2
    frames = _source_batches(w, h, bd, segs, gop, 7)
    fed = [_stack_source(b, w, h, bd, 0) for b in frames]
    ctx.prof_enable(1)
    try:
        outs = {}
        for name, fmt, source, launches in (("plain", F.PLANAR, None, None), ("identity", F.PLANAR, (w, h), gop), ("packed", F.PACKED10, (w, h), 2 * gop)):
            ctx.prof_reset()
            outs[name] = _run(ctx, av1mi, w, h, bd, 100, gop, segs, fed, fmt, "submit", 1, source=source)
            prof = ctx.prof_get()
            assert "intra_pipeline" in prof and "inter_pipeline" in prof
            assert (prof["input_convert"][0] if "input_convert" in prof else None) == launches, name
        _same(outs["plain"], outs["identity"], "identity")
        _same(outs["plain"], outs["packed"], "identity, packed")
    finally:
        ctx.prof_enable(0)
        ctx.prof_reset()


def test_open_refuses_bad_source_sizes(ctx, av1mi):
    for source in ((64, 0), (0, 64), (600, 64), (64, 600), (8, 64), (4104, 2048)):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, 128, 128, 8, 100, 2, 1, source=source)
        assert e.value.code == -1 and "source" in str(e.value)


# ---- the product ----------------------------------------------------------------------------------------------------------

def _write_y4m(path, planes_per_frame, w, h, bd, sar):
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30:1 Ip A%s C%s\n" % (w, h, sar, "420jpeg" if bd == 8 else "420p10")).encode())
        for planes in planes_per_frame:
            f.write(b"FRAME\n")
            for p in planes:
                f.write(np.ascontiguousarray(p).astype("<u2" if bd == 10 else np.uint8).tobytes())


def _host():
    host = C.CDLL(HOST)
    host.av1mi_run_transcode.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t]
    host.av1mi_host_transcode_args.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int] * 4 + [C.c_char_p, C.c_int]
    return host


def _reference_argv(host, src, out, webrip):
    buf = C.create_string_buffer(8192)
    n = host.av1mi_host_transcode_args(str(src).encode(), str(out).encode(), 1, 0, 288, int(webrip), buf, 8192)
    assert n > 0
    return buf.value.decode().split("\n")


def _transcode(host, argv):
    err = C.create_string_buffer(1024)
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    assert host.av1mi_run_transcode(len(argv), arr, err, 1024) == 0, err.value


def _clip(sw, sh, n, bd, seed):
    import synth
    Y, U, V = synth.frames(_r8(sw) + 8, _r8(sh) + 8, n, bd, seed)
    cw, ch = (sw + 1) // 2, (sh + 1) // 2
    return [[Y[t][:sh, :sw], U[t][:ch, :cw], V[t][:ch, :cw]] for t in range(n)]


def _mkv_has(data, ident):
    """in the headers of a Matroska file (everything before the first cluster: the payloads may hold any bytes)"""
    return bytes(ident) in data[:data.index(bytes([0x1F, 0x43, 0xB6, 0x75]))]


@pytest.mark.parametrize("bd", [8, 10])
def test_transcode_scales_an_anamorphic_source(tmp_path, av1mi, bd):
    """360 x 288 at A16:15 through the argv the reference builds for a web-rip job == the numpy-prescaled 384 x 288 A1:1 clip through
    the same argv (whose chain then evaluates to the source size: today's path)"""
    host = _host()
    sw, sh, dw, dh, n = 360, 288, 384, 288, 5
    frames = _clip(sw, sh, n, bd, 21)
    table = _lib_table(av1mi)
    scaled = [R.scale_frame(*f, dw, dh, bd, table) for f in frames]
    _write_y4m(tmp_path / "ana.y4m", frames, sw, sh, bd, "16:15")
    _write_y4m(tmp_path / "square.y4m", scaled, dw, dh, bd, "1:1")
    outs = {}
    for name in ("ana", "square"):
        for ext in ("obu", "mkv"):
            out = tmp_path / ("%s.%s" % (name, ext))
            _transcode(host, _reference_argv(host, tmp_path / (name + ".y4m"), out, True))
            outs[name, ext] = out.read_bytes()
    assert len(outs["ana", "obu"]) > 100
    assert outs["ana", "obu"] == outs["square", "obu"] and outs["ana", "mkv"] == outs["square", "mkv"]
    assert not _mkv_has(outs["ana", "mkv"], [0x54, 0xB0])      # square pixels after scaling: no DisplayWidth
    import dav1d_ref as D
    if D.available():
        got = D.decode(outs["ana", "obu"])
        assert len(got) == n and all(g[0].shape == (dh, dw) for g in got)
    # the non-web-rip chain on the same source: the pixels are not resampled, the track carries the display size
    out = tmp_path / "plain.mkv"
    _transcode(host, _reference_argv(host, tmp_path / "ana.y4m", out, False))
    _write_y4m(tmp_path / "same.y4m", frames, sw, sh, bd, "1:1")
    out2 = tmp_path / "same.obu"
    _transcode(host, _reference_argv(host, tmp_path / "same.y4m", out2, False))
    out3 = tmp_path / "plain.obu"
    _transcode(host, _reference_argv(host, tmp_path / "ana.y4m", out3, False))
    assert out3.read_bytes() == out2.read_bytes()
    data = out.read_bytes()
    assert _mkv_has(data, [0x54, 0xB0, 0x82, 0x01, 0x80]) and _mkv_has(data, [0x54, 0xBA, 0x82, 0x01, 0x20])      # DisplayWidth 384, DisplayHeight 288


def test_transcode_codes_an_odd_source_at_the_even_size(tmp_path, av1mi):
    """135 x 71 with the plain chain: ceil(iw / 2) * 2 = 136 x 72, scaled (T = 6), not cropped"""
    host = _host()
    sw, sh, n, bd = 135, 71, 4, 8
    frames = _clip(sw, sh, n, bd, 22)
    table = _lib_table(av1mi)
    scaled = [R.scale_frame(*f, 136, 72, bd, table) for f in frames]
    _write_y4m(tmp_path / "odd.y4m", frames, sw, sh, bd, "1:1")
    _write_y4m(tmp_path / "even.y4m", scaled, 136, 72, bd, "1:1")
    outs = []
    for name in ("odd", "even"):
        out = tmp_path / (name + ".obu")
        _transcode(host, _reference_argv(host, tmp_path / (name + ".y4m"), out, False))
        outs.append(out.read_bytes())
    assert len(outs[0]) > 100 and outs[0] == outs[1]
    # an explicit target wins over the chain
    out = tmp_path / "explicit.obu"
    argv = _reference_argv(host, tmp_path / "even.y4m", out, True)
    _transcode(host, argv[:-1] + ["-av1mi_scale", "96x48", argv[-1]])
    import dav1d_ref as D
    if D.available():
        got = D.decode(out.read_bytes())
        assert len(got) == n and got[0][0].shape == (48, 96)
