"""Chroma formats on the GPU (include/av1mi.h "chroma formats"; k_chroma_convert in av1-go_amd/csrc/input_kernels.hip): the kernel
against the numpy reference written from the header (chroma_formats_ref.py), a session fed a 4:2:2 / 4:4:4 / grey / 12-bit source
against a planar 4:2:0 session fed the numpy-converted frames, and the product.  No tolerance anywhere: every comparison is equality."""
import ctypes as C
import os

import numpy as np
import pytest

import chroma_formats_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64      # bytes behind every output plane that the kernel must leave alone
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "av1-go_amd", "host", "libav1mi_host.so")


# ---- the kernel -----------------------------------------------------------------------------------------------------------------

def _convert(ctx, chroma, src_bd, bd, w, h, frames, planes):
    """the stacked source buffers -> the stacked 4:2:0 planes through av1mi_chroma_convert; checks the guard bytes behind each output.
    Where the depths are equal the luma plane is not part of the call (None comes back for it)"""
    W8, H8, dt = R.up8(w), R.up8(h), R.dtype(bd)
    shapes = [(frames * H8, W8), (frames * H8 // 2, W8 // 2), (frames * H8 // 2, W8 // 2)]
    luma = src_bd != bd
    d_in = [ctx.to_device(p) if p is not None and (i or luma) else None for i, p in enumerate(planes)]
    d_out = []
    for i, sh in enumerate(shapes):
        if i == 0 and not luma:
            d_out.append(None)
            continue
        n = sh[0] * sh[1] * np.dtype(dt).itemsize
        b = ctx.alloc(n + GUARD)
        ctx.memset(b, 0xA5, n + GUARD)
        d_out.append(b)
    ctx.chroma_convert(chroma, src_bd, bd, w, h, frames, d_in, d_out)
    ctx.sync()
    out = []
    for b, sh in zip(d_out, shapes):
        if b is None:
            out.append(None)
            continue
        n = sh[0] * sh[1] * np.dtype(dt).itemsize
        raw = b.download((n + GUARD,), np.uint8)
        assert (raw[n:] == 0xA5).all(), "the kernel wrote behind a plane"
        out.append(raw[:n].view(dt).reshape(sh))
    for b in d_in + d_out:
        if b is not None:
            b.free()
    return out


# true size and frames: the smallest (every lane an edge lane) | several cells, frames must not mix at the vertical clamp | a true size
# inside its buffers (a single padding byte read shows up) | odd ceil(w / 2), rows that are no multiple of 16 bytes | a full frame
SHAPES = [(8, 8, 1), (72, 40, 3), (70, 38, 3), (1366, 768, 2), (1920, 1080, 1)]


@pytest.mark.parametrize("w,h,frames", SHAPES)
@pytest.mark.parametrize("src_bd,bd", R.DEPTHS)
@pytest.mark.parametrize("chroma", R.LAYOUTS)
def test_chroma_convert_matches_numpy(ctx, chroma, src_bd, bd, w, h, frames):
    ones = (1 << (8 if src_bd == 8 else 16)) - 1      # 0xFF.. in everything beyond the true size of every source plane
    for k, kind in enumerate(R.KINDS):
        planes = R.content(kind, chroma, src_bd, w, h, frames, seed=11 + k, padding=ones if (w & 7 or h & 7) else None)
        want = R.convert_stack(chroma, src_bd, bd, w, h, frames, planes)
        got = _convert(ctx, chroma, src_bd, bd, w, h, frames, planes)
        assert (got[0] is None) == (src_bd == bd)
        for p in range(3):
            if got[p] is not None:
                assert got[p].shape == want[p].shape and np.array_equal(got[p], want[p]), \
                    "layout %d, %d -> %d bits, %dx%d x %d, %s content: plane %d differs" % (chroma, src_bd, bd, w, h, frames, kind, p)


def test_chroma_convert_refuses_bad_arguments(ctx, av1mi):
    b = ctx.alloc(1 << 16)
    try:
        for args in ((4, 8, 8, 64, 64, 1), (-1, 8, 8, 64, 64, 1), (R.C444, 12, 8, 64, 64, 1), (R.C444, 10, 8, 64, 64, 1), (R.C444, 8, 10, 64, 64, 1),
                     (R.C444, 12, 12, 64, 64, 1), (R.C422, 9, 9, 64, 64, 1), (R.C422, 8, 8, 4, 64, 1), (R.C422, 8, 8, 64, 0, 1), (R.C422, 8, 8, 64, 64, 0)):
            with pytest.raises(av1mi.Av1miError) as e:
                ctx.chroma_convert(*args, [b, b, b], [b, b, b])
            assert e.value.code == -1
        with pytest.raises(av1mi.Av1miError):
            ctx.chroma_convert(R.C444, 8, 8, 64, 64, 1, [b, None, b], [b, b, b])      # a missing chroma plane
        with pytest.raises(av1mi.Av1miError):
            ctx.chroma_convert(R.C400, 12, 10, 64, 64, 1, [None, None, None], [b, b, b])      # 12 bits: the luma plane is converted
    finally:
        b.free()


# ---- session equivalence ----------------------------------------------------------------------------------------------------------

def _source_batches(chroma, src_bd, w, h, segs, n, first, luma_edge=False):
    """n batches of `segs` stacked source frames of true size w x h in the layout's buffers; smooth moving content (synth); everything
    beyond the true size holds 0xFF.. — except, with luma_edge, the luma padding, which replicates the edge (the caller's duty where
    the luma plane passes through and the session does not scale)"""
    import synth
    gen = 8 if src_bd == 8 else 10
    W8, H8 = R.up8(w), R.up8(h)
    rng = np.random.default_rng(first)
    shapes = R.buffer_shapes(chroma, w, h)
    per = [synth.frames(2 * W8, 2 * H8, n, gen, first + 9 * s) for s in range(segs)]      # chroma of a frame twice the size = full-size chroma
    ones = (1 << (8 if src_bd == 8 else 16)) - 1
    out = []
    for t in range(n):
        planes = []
        for p in range(3):
            if shapes[p] is None:
                planes.append(None)
                continue
            tw, th = (w, h) if p == 0 else R.true_chroma_size(chroma, w, h)
            buf = np.full((segs,) + shapes[p], ones, R.dtype(src_bd))
            for s in range(segs):
                a = per[s][0][t][:H8, :W8] if p == 0 else per[s][p][t][::H8 // shapes[p][0], ::W8 // shapes[p][1]]
                a = a.astype(np.int64)
                if src_bd == 12:
                    a = (a << 2) | rng.integers(0, 4, a.shape)
                buf[s, :th, :tw] = a[:th, :tw]
            if p == 0 and luma_edge:
                buf[:, :, tw:] = buf[:, :, tw - 1:tw]
                buf[:, th:, :] = buf[:, th - 1:th, :]
            planes.append(buf.reshape(segs * shapes[p][0], shapes[p][1]))
        out.append(planes)
    return out


def _run(ctx, av1mi, w, h, bd, q, gop, segs, batches, via="submit", mode=1, **kw):
    """every array a session hands out per batch (tile sizes + payloads or symbols, quality records) and its reference planes"""
    s = av1mi.GopSession(ctx, w, h, bd, q, gop, segs, gpu_entropy=mode, **kw)
    outs, held = [], []
    try:
        for planes in batches:
            if via == "submit":
                fed = s.input_planes()
                assert len(fed) == sum(p is not None for p in planes)
                for dst, a in zip(fed, [p for p in planes if p is not None]):
                    assert dst.shape == a.shape and dst.dtype == a.dtype
                    dst[:] = a
                s.submit()
            else:
                bufs = [ctx.to_device(a) if a is not None else None for a in planes]
                held.append(bufs)
                s.submit_device(*bufs)
            fr = s.collect()
            o = {k: v.copy() for k, v in fr.items() if isinstance(v, np.ndarray)}
            o["frame_type"] = fr["frame_type"]
            o["ref_y"], o["ref_u"], o["ref_v"] = s.download_reference()
            outs.append(o)
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
        for bufs in held:
            for b in bufs:
                if b is not None:
                    b.free()
    return outs


def _same(a, b, what):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        assert sorted(x) == sorted(y), "%s batch %d: %s vs %s" % (what, t, sorted(x), sorted(y))
        for k in x:
            assert np.array_equal(x[k], y[k]), "%s: batch %d, %s differs from the 4:2:0 session fed the numpy-converted frames" % (what, t, k)


def _check(ctx, av1mi, chroma, src_bd, w, h, q, seed, true=None, vias=("submit", "device"), modes=(1,), segs=2, gop=3, **kw):
    """a session fed the source in its layout == a planar 4:2:0 session fed convert(...) of the same source; true: the true size of
    the fed frames when it is not the coded size w x h (a cropped size, or a scaling session's source)"""
    bd = 10 if src_bd == 12 else src_bd
    tw, th = true or (w, h)
    through = src_bd == bd and "source" not in kw
    batches = _source_batches(chroma, src_bd, tw, th, segs, gop, seed, luma_edge=through)
    converted = [R.convert_stack(chroma, src_bd, bd, tw, th, segs, b) for b in batches]
    for mode in modes:
        base = _run(ctx, av1mi, w, h, bd, q, gop, segs, converted, "submit", mode, **kw)
        assert ("tile_size" in base[0]) == (mode == 1) and [o["frame_type"] for o in base] == [0, 1, 1]
        for via in vias:
            got = _run(ctx, av1mi, w, h, bd, q, gop, segs, batches, via, mode, source_chroma=chroma, source_bit_depth=src_bd, **kw)
            _same(base, got, "layout %d at %d bits via %s, gpu_entropy %d" % (chroma, src_bd, via, mode))
    return base


def test_444_10bit_session_equals_420(ctx, av1mi):
    _check(ctx, av1mi, R.C444, 10, 136, 72, 60, 1, modes=(1, 0))


def test_422_8bit_session_equals_420(ctx, av1mi):
    _check(ctx, av1mi, R.C422, 8, 136, 72, 110, 2)


def test_12bit_420_and_grey_8bit_sessions_equal_420(ctx, av1mi):
    _check(ctx, av1mi, R.C420, 12, 136, 72, 60, 3)
    base = _check(ctx, av1mi, R.C400, 8, 136, 72, 110, 4)
    assert all((o["ref_u"] == 128).all() and (o["ref_v"] == 128).all() for o in base)      # flat chroma codes to flat chroma


def test_444_session_with_scaling(ctx, av1mi):
    """a 1440 x 1080-shaped 4:4:4 source at 144 x 108, shown at 4:3 -> 192 x 108 (coded 192 x 112): chroma, then scale"""
    _check(ctx, av1mi, R.C444, 8, 192, 112, 110, 5, true=(144, 108), source=(144, 108), visible=(192, 108))
    _check(ctx, av1mi, R.C444, 12, 192, 112, 60, 6, true=(144, 108), source=(144, 108), visible=(192, 108), vias=("submit",))


def test_device_batches_with_a_luma_plane_that_passes_through_to_the_scaler(ctx, av1mi):
    """a 4:4:4 8-bit source of 40 x 24 in device memory, scaled to 24 x 16, one segment, a key and an inter batch: the scaler reads the
    CALLER's luma plane (chroma, then scale; no plane of the session's lies between).  The bytes of the same session fed through
    input_planes(), and the caller's luma buffers come back unchanged"""
    w, h, q, gop = 24, 16, 110, 2
    batches = _source_batches(R.C444, 8, 40, 24, 1, gop, 14)
    kw = dict(source=(40, 24), source_chroma=R.C444, source_bit_depth=8)
    base = _run(ctx, av1mi, w, h, 8, q, gop, 1, batches, "submit", **kw)
    assert [o["frame_type"] for o in base] == [0, 1]
    s = av1mi.GopSession(ctx, w, h, 8, q, gop, 1, gpu_entropy=1, **kw)
    held = [[ctx.to_device(a) for a in planes] for planes in batches]
    got = []
    try:
        for bufs in held:
            s.submit_device(*bufs)
            fr = s.collect()
            got.append({k: v.copy() for k, v in fr.items() if isinstance(v, np.ndarray)})
            got[-1]["frame_type"] = fr["frame_type"]
            got[-1]["ref_y"], got[-1]["ref_u"], got[-1]["ref_v"] = s.download_reference()
        assert s.entropy_fallbacks() == 0
        for bufs, planes in zip(held, batches):
            assert (bufs[0].download(planes[0].shape, planes[0].dtype) == planes[0]).all(), "the session wrote the caller's luma plane"
    finally:
        s.close()
        for bufs in held:
            for b in bufs:
                b.free()
    _same(base, got, "4:4:4 from device memory, scaled")


def test_cropped_size_sessions(ctx, av1mi):
    """70 x 38 coded at 72 x 40: a luma plane that passes through (4:2:2 10-bit; the caller replicates its edge) and one that is
    converted (4:4:4 12-bit; its padding undefined as well)"""
    _check(ctx, av1mi, R.C422, 10, 72, 40, 60, 7, true=(70, 38), visible=(70, 38))
    _check(ctx, av1mi, R.C444, 12, 72, 40, 60, 8, true=(70, 38), visible=(70, 38))


def test_quality_records_are_measured_against_the_converted_frame(ctx, av1mi):
    base = _check(ctx, av1mi, R.C444, 10, 136, 72, 60, 9, vias=("submit",), quality_stats=1)
    assert all("quality" in o and o["quality"].shape == (2, 3) and (o["quality"]["samples"] > 0).all() for o in base)


def test_open_refusals_and_a_plain_session_gains_no_launch(ctx, av1mi):
    for kw in (dict(source_chroma=4), dict(source_chroma=-1), dict(source_bit_depth=9), dict(source_bit_depth=16),
               dict(bd=8, source_bit_depth=12), dict(bd=8, source_bit_depth=10), dict(bd=10, source_bit_depth=8),
               dict(bd=10, source_chroma=R.C444, input_format=av1mi.INPUT_P010), dict(bd=8, source_chroma=R.C422, input_format=av1mi.INPUT_NV12),
               dict(bd=10, source_bit_depth=12, input_format=av1mi.INPUT_PACKED10)):
        bd = kw.pop("bd", 10)
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, 64, 64, bd, 100, 2, 1, **kw)
        assert e.value.code == -1 and "source_" in str(e.value), kw
    w, h, bd, gop, segs = 136, 72, 10, 3, 2
    src = _source_batches(R.C444, 10, w, h, segs, gop, 10, luma_edge=True)
    plain = [R.convert_stack(R.C444, 10, 10, w, h, segs, b) for b in src]
    ctx.prof_enable(1)
    try:
        outs = {}
        for name, batches, kw, launches in (("plain", plain, {}, None), ("explicit 4:2:0", plain, dict(source_chroma=R.C420, source_bit_depth=10), None),
                                            ("4:4:4", src, dict(source_chroma=R.C444), gop), ("4:4:4 scaled", src, dict(source_chroma=R.C444, source=(w, h)), 2 * gop)):
            ctx.prof_reset()
            outs[name] = _run(ctx, av1mi, w, h, bd, 100, gop, segs, batches, **kw)
            prof = ctx.prof_get()
            assert "intra_pipeline" in prof and "inter_pipeline" in prof
            assert (prof["input_convert"][0] if "input_convert" in prof else None) == launches, name
        for name in ("explicit 4:2:0", "4:4:4", "4:4:4 scaled"):      # (scaled to its own size: the identity)
            _same(outs["plain"], outs[name], name)
    finally:
        ctx.prof_enable(0)
        ctx.prof_reset()


# ---- the product ------------------------------------------------------------------------------------------------------------------

def _host():
    host = C.CDLL(HOST)
    host.av1mi_run_transcode.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t]
    host.av1mi_host_transcode_args.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int] * 4 + [C.c_char_p, C.c_int]
    return host


def _transcode(host, argv):
    err = C.create_string_buffer(1024)
    arr = (C.c_char_p * len(argv))(*[str(a).encode() for a in argv])
    return host.av1mi_run_transcode(len(argv), arr, err, 1024), err.value.decode()


def _oracle_gop(O, frames, bd, q):
    """the oracle's closed-GOP chain (key + P frames, the library's filter policy) on 4:2:0 frames: what a decoder must output"""
    import pipeline as P
    import test_av1_conformance as CF
    refs, ref = [], None
    for t, (Y, U, V) in enumerate(frames):
        h, w = Y.shape
        if t == 0:
            ref = CF._chain(O, P, Y, U, V, bd, q)[2][3]
        else:
            r = O.inter_encode_frame((Y, U, V), ref, bd, q, 8)
            ref = CF._filters(O, P, r, bd, q, 1, w, h, r["skip"].reshape(h // 8, w // 8), (Y, U, V))[1][2]
        refs.append(ref)
    return refs


@pytest.mark.parametrize("tag,chroma,src_bd", [("444p10", R.C444, 10), ("422", R.C422, 8)])
def test_transcode_of_a_444_and_a_422_file(tmp_path, O, tag, chroma, src_bd):
    """136 x 72 x 4 frames through the argv the reference builds (its chain ends in format=nv12): exit 0, and dav1d decodes the output
    to the oracle chain run on convert(...) of the source.  The same file without a format= filter and without -av1mi_format is
    refused with the colourspace text"""
    import dav1d_ref as D
    host = _host()
    w, h, n = 136, 72, 4
    batches = _source_batches(chroma, src_bd, w, h, 1, n, 13)
    src = tmp_path / "src.y4m"
    with open(src, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s\n" % (w, h, tag)).encode())
        for planes in batches:
            f.write(b"FRAME\n")
            for p in planes:
                f.write(np.ascontiguousarray(p).astype(np.uint8 if src_bd == 8 else "<u2").tobytes())
    out = tmp_path / "out.obu"
    buf = C.create_string_buffer(8192)
    assert host.av1mi_host_transcode_args(str(src).encode(), str(out).encode(), 1, 0, 288, 0, buf, 8192) > 0
    argv = buf.value.decode().split("\n")
    assert "format=nv12" in argv[argv.index("-vf:v:0") + 1]
    assert _transcode(host, argv) == (0, "")
    q = int(argv[argv.index("-global_quality:v:0") + 1])
    if D.available():
        want = _oracle_gop(O, [R.convert(chroma, src_bd, src_bd, w, h, planes) for planes in batches], src_bd, q)
        got = D.decode(out.read_bytes())
        assert len(got) == n
        for t in range(n):
            for i in range(3):
                assert got[t][i].shape == want[t][i].shape and (got[t][i] == want[t][i]).all(), "frame %d plane %d differs from the oracle chain" % (t, i)
    # -av1mi_format 420 instead of a chain: the same bytes
    out2 = tmp_path / "out2.obu"
    assert _transcode(host, ["-i", src, "-global_quality:v:0", q, "-av1mi_format", "420", out2]) == (0, "")
    assert out2.read_bytes() == out.read_bytes()
    # neither: refused as before
    out3 = tmp_path / "out3.obu"
    code, err = _transcode(host, ["-i", src, "-global_quality:v:0", q, out3])
    assert code == 1 and "unsupported Y4M colourspace " + tag in err and not out3.exists()
