"""The session's input formats on the GPU (include/av1mi.h enum av1mi_input_format; av1-go_amd/csrc/input_kernels.hip): the
conversion kernel against the numpy restatement of the formats (input_formats_ref.py), and the core claim — a session fed the
packed / semi-planar form of a source produces byte for byte what the planar session produces (which the rest of the suite pins
to the oracle and dav1d).  No tolerance anywhere: every comparison is equality."""
import ctypes as C
import os

import numpy as np
import pytest

import input_formats_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64      # bytes behind every output plane that the kernel must leave alone


def _bd(fmt):
    return 8 if fmt == R.NV12 else 10


def _convert(ctx, fmt, bd, width, rows, wire):
    """wire planes (flat uint8) -> planar planes through av1mi_input_convert; checks the guard bytes behind each output"""
    dt = np.uint8 if bd == 8 else np.uint16
    shapes = ((rows, width), (rows // 2, width // 2), (rows // 2, width // 2))
    d_in = [ctx.to_device(p) for p in wire]
    d_out = []
    for sh in shapes:
        n = sh[0] * sh[1] * np.dtype(dt).itemsize
        b = ctx.alloc(n + GUARD)
        ctx.memset(b, 0xA5, n + GUARD)
        d_out.append(b)
    ctx.input_convert(fmt, bd, width, rows, d_in, d_out)
    ctx.sync()
    out = []
    for b, sh in zip(d_out, shapes):
        n = sh[0] * sh[1] * np.dtype(dt).itemsize
        raw = b.download((n + GUARD,), np.uint8)
        assert (raw[n:] == 0xA5).all(), "the kernel wrote behind a plane"
        out.append(raw[:n].view(dt).reshape(sh))
    for b in d_in + d_out:
        b.free()
    return out


@pytest.mark.parametrize("width,rows", [(8, 8), (136, 72 * 3), (1920, 1080 * 2)])
@pytest.mark.parametrize("fmt", [R.PACKED10, R.P010, R.NV12])
def test_convert_matches_numpy(ctx, fmt, width, rows):
    bd = _bd(fmt)
    for kind in ("random", "ramp", "max", "zeros"):
        planes = R.content(kind, bd, width, rows, 7)
        got = _convert(ctx, fmt, bd, width, rows, R.pack(fmt, bd, *planes))
        for p in range(3):
            assert (got[p] == planes[p]).all(), "format %d, %s content: plane %d differs" % (fmt, kind, p)
    if fmt == R.P010:      # the six low bits of a P010 sample are ignored
        planes = R.content("random", bd, width, rows, 8)
        got = _convert(ctx, fmt, bd, width, rows, R.pack(fmt, bd, *planes, low_bits=np.random.default_rng(9)))
        for p in range(3):
            assert (got[p] == planes[p]).all(), "P010 with garbage in the low bits: plane %d differs" % p


@pytest.mark.parametrize("fmt", [R.PACKED10, R.P010])
def test_convert_matches_numpy_on_a_full_4k_batch(ctx, fmt):
    """3840 x 2160 x 12 segments: the batch the product uploads; unit indices beyond 2^24, every workgroup strides several times"""
    width, rows = 3840, 2160 * 12
    planes = R.content("random", 10, width, rows, 3)
    got = _convert(ctx, fmt, 10, width, rows, R.pack(fmt, 10, *planes, low_bits=np.random.default_rng(4)))
    for p in range(3):
        assert np.array_equal(got[p], planes[p]), "plane %d differs" % p


def test_convert_refuses_bad_arguments(ctx, av1mi):
    b = ctx.alloc(4096)
    try:
        for fmt, bd in ((R.PLANAR, 10), (R.PACKED10, 8), (R.P010, 8), (R.NV12, 10), (9, 10)):
            with pytest.raises(av1mi.Av1miError):
                ctx.input_convert(fmt, bd, 8, 8, [b, b, b], [b, b, b])
        with pytest.raises(av1mi.Av1miError):
            ctx.input_convert(R.PACKED10, 10, 12, 8, [b, b, b], [b, b, b])      # width not a multiple of 8
    finally:
        b.free()


# ---- session equivalence -------------------------------------------------------------------------------------------------

def _frames(w, h, bd, segs, n, seed, visible=None):
    """n batches of stacked planar planes [segs * h, w] (+ chroma), different content in every batch and segment"""
    import synth
    per = [synth.frames(w, h, n, bd, seed + 7 * s) for s in range(segs)]
    out = []
    for t in range(n):
        planes = [np.concatenate([per[s][i][t] for s in range(segs)]) for i in range(3)]
        if visible:      # the caller replicates the true last column / row into the padding
            vw, vh = visible
            for i in range(3):
                pw, ph, pvw, pvh = (w, h, vw, vh) if i == 0 else (w // 2, h // 2, (vw + 1) // 2, (vh + 1) // 2)
                a = planes[i].reshape(segs, ph, pw)
                a[:, :, pvw:] = a[:, :, pvw - 1:pvw]
                a[:, pvh:, :] = a[:, pvh - 1:pvh, :]
        out.append(planes)
    return out


def _run(ctx, av1mi, w, h, bd, q, gop, segs, batches, fmt, via, mode, lag=0, visible=None, key_block_size=0, refs=True):
    """every array a session hands out per batch (tile sizes + payloads, or the symbols) and, in lockstep, its reference planes"""
    s = av1mi.GopSession(ctx, w, h, bd, q, gop, segs, gpu_entropy=mode, visible=visible, key_block_size=key_block_size, input_format=fmt)
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
            wire = planes if fmt == R.PLANAR else R.pack(fmt, bd, *planes)
            if via == "submit":
                for dst, a in zip(s.input_planes(), wire):
                    dst[:] = a if fmt == R.PLANAR else a.view(np.uint8).ravel()
                s.submit()
            else:
                bufs = [ctx.to_device(a) for a in wire]
                held.append(bufs)      # the caller's buffers stay valid until the batch has been collected
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
            assert np.array_equal(x[k], y[k]), "%s: batch %d, %s differs from the planar session" % (what, t, k)


def _check(ctx, av1mi, w, h, bd, q, gop, segs, n, fmts, seed, vias=("submit", "device"), modes=(1, 0), **kw):
    batches = _frames(w, h, bd, segs, n, seed, kw.get("visible"))
    for mode in modes:
        base = _run(ctx, av1mi, w, h, bd, q, gop, segs, batches, R.PLANAR, "submit", mode, **kw)
        assert ("tile_size" in base[0]) == (mode == 1) and "ref_y" in base[0]
        for fmt in fmts:
            for via in vias:
                got = _run(ctx, av1mi, w, h, bd, q, gop, segs, batches, fmt, via, mode, **kw)
                _same(base, got, "format %d via %s, gpu_entropy %d" % (fmt, via, mode))


def test_nv12_session_equals_planar(ctx, av1mi):
    _check(ctx, av1mi, 192, 128, 8, 110, 3, 2, 3, [R.NV12], 1)


def test_10bit_sessions_equal_planar(ctx, av1mi):
    _check(ctx, av1mi, 136, 72, 10, 60, 3, 3, 3, [R.PACKED10, R.P010], 2)


def test_cropped_size_sessions_equal_planar(ctx, av1mi):
    _check(ctx, av1mi, 136, 72, 10, 60, 3, 2, 3, [R.PACKED10, R.P010], 3, visible=(130, 70))


def test_key_block_size_32_sessions_equal_planar(ctx, av1mi):
    _check(ctx, av1mi, 256, 168, 10, 60, 3, 2, 3, [R.PACKED10, R.P010], 4, key_block_size=32)


def test_full_size_packed_session_equals_planar(ctx, av1mi):
    _check(ctx, av1mi, 3840, 2160, 10, 128, 3, 2, 3, [R.PACKED10], 5)


@pytest.mark.parametrize("fmt,bd", [(R.PACKED10, 10), (R.P010, 10), (R.NV12, 8)])
@pytest.mark.parametrize("mode", [1, 0])
def test_three_batches_in_flight_and_buffer_reuse(ctx, av1mi, fmt, bd, mode):
    """8 batches of different content, two GOPs, submit t + 2 before collect t: every slot's wire buffers and planar planes are
    reused more than twice while their previous readers may still run — the bytes must be those of the planar session in lockstep
    (a missing event between the upload, the conversion and the kernels shows up here)"""
    w, h, q, gop, segs, n = 328, 184, 100, 4, 3, 8
    batches = _frames(w, h, bd, segs, n, 6)
    base = _run(ctx, av1mi, w, h, bd, q, gop, segs, batches, R.PLANAR, "submit", mode, lag=0, refs=False)
    for via in ("submit", "device"):
        for lag in (2, 0):
            got = _run(ctx, av1mi, w, h, bd, q, gop, segs, batches, fmt, via, mode, lag=lag, refs=False)
            _same(base, got, "format %d via %s lag %d, gpu_entropy %d" % (fmt, via, lag, mode))


def test_open_refuses_bad_formats_and_the_planar_path_gains_no_launch(ctx, av1mi):
    for fmt, bd in ((4, 10), (-1, 8), (R.PACKED10, 8), (R.P010, 8), (R.NV12, 10)):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, 64, 64, bd, 100, 2, 1, input_format=fmt)
        assert e.value.code == -1 and "input_format" in str(e.value)
    w, h, bd, gop, segs = 136, 72, 10, 3, 2
    batches = _frames(w, h, bd, segs, gop, 7)
    ctx.prof_enable(1)
    try:
        for fmt, launches in ((R.PLANAR, None), (R.PACKED10, gop)):
            ctx.prof_reset()
            _run(ctx, av1mi, w, h, bd, 100, gop, segs, batches, fmt, "submit", 1, refs=False)
            prof = ctx.prof_get()
            assert "intra_pipeline" in prof and "inter_pipeline" in prof
            assert (prof["input_convert"][0] if "input_convert" in prof else None) == launches
        n, ms = C.c_int(), C.c_double()
        ctx.prof_reset()
        _run(ctx, av1mi, w, h, bd, 100, gop, segs, batches, R.PLANAR, "device", 1, refs=False)
        kinds = [ctx.lib.av1mi_kernel_kind_name(k) for k in range(av1mi.N_KERNEL_KINDS)]
        k_input = kinds.index(b"input_convert")
        assert k_input == av1mi.N_KERNEL_KINDS - 1
        ctx._chk(ctx.lib.av1mi_prof_get(ctx.h, k_input, C.byref(n), C.byref(ms)))
        assert n.value == 0
    finally:
        ctx.prof_enable(0)
        ctx.prof_reset()


# ---- the product ----------------------------------------------------------------------------------------------------------

def _write_y4m(path, w, h, n, bd):
    import synth
    Y, U, V = synth.frames((w + 1) // 2 * 2, (h + 1) // 2 * 2, n, bd, 12)
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s\n" % (w, h, "420jpeg" if bd == 8 else "420p10")).encode())
        for i in range(n):
            f.write(b"FRAME\n")
            for p, (pw, ph) in zip((Y[i], U[i], V[i]), ((w, h), ((w + 1) // 2, (h + 1) // 2), ((w + 1) // 2, (h + 1) // 2))):
                f.write(np.ascontiguousarray(p[:ph, :pw]).astype("<u2" if bd == 10 else np.uint8).tobytes())


@pytest.mark.parametrize("w,h,bd", [(136, 72, 10), (854, 480, 10), (136, 72, 8)])
def test_transcode_with_pack10_writes_the_same_file(tmp_path, w, h, bd):
    """-av1mi_pack10 1: the reader threads pack each (edge-padded) frame into the session's pinned buffers; same bytes out.  With an
    8-bit source the option is accepted and changes nothing.  11 frames, GOP 4, 2 segments: a short last GOP and an absent segment"""
    host = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "av1-go_amd", "host", "libav1mi_host.so"))
    host.av1mi_run_transcode.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t]
    src = tmp_path / "clip.y4m"
    _write_y4m(src, w, h, 11, bd)
    err = C.create_string_buffer(1024)
    outs = []
    for extra, name in (([], "plain.obu"), (["-av1mi_pack10", "1"], "packed.obu"), (["-av1mi_pack10", "0"], "zero.obu")):
        argv = ["-i", str(src), "-global_quality:v:0", "110", "-g", "4", "-av1mi_segments", "2"] + extra + [str(tmp_path / name)]
        arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
        assert host.av1mi_run_transcode(len(argv), arr, err, 1024) == 0, err.value
        outs.append((tmp_path / name).read_bytes())
    assert len(outs[0]) > 100 and outs[1] == outs[0] and outs[2] == outs[0]
