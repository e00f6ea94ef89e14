"""GPU tests of cropping (include/av1mi.h "bar detection", av1mi_gop_config.crop_*; av1-go_amd/csrc/crop_kernels.hip): av1mi_crop_analyse
against tests/crop_ref.py, the session's defining property — a session with a window fed whole frames yields the bytes of a session
without one fed the pre-cropped frames — and the product.  No tolerance anywhere: every comparison is equality."""
import numpy as np
import pytest

import crop_ref as R

pytestmark = pytest.mark.gpu

LIMIT = 24


def _r8(n):
    return (n + 7) & ~7


# ---------------------------------------------------------------------------------------------- kernel
def _frames(bd, w, h):
    """five frames of true size w x h: the threshold, a picture touching the top edge, all dark, no bars, noise around the limit"""
    rng = np.random.default_rng(5 + bd)
    f = np.zeros((5, h, w), np.int64)
    f[0] = LIMIT                      # every row sums to exactly LIMIT * w, every column to LIMIT * h: dark ...
    f[0, 9, 40 % w] = LIMIT + 1       # ... and one more in row 9 / that column: not dark
    f[1, :h - 20] = 200
    f[3] = rng.integers(60, 256, (h, w))
    f[4] = rng.integers(LIMIT - 6, LIMIT + 7, (h, w))
    if bd > 8:                        # m8 drops the low bits, whatever they hold
        f = (f << (bd - 8)) | rng.integers(0, 1 << (bd - 8), f.shape)
    return f


def _buffers(frames, bd):
    n, h, w = frames.shape
    Y = np.full((n, _r8(h), _r8(w)), (1 << bd) - 1, np.uint8 if bd == 8 else np.uint16)      # the padding: never to be read
    Y[:, :h, :w] = frames
    return Y


@pytest.mark.parametrize("bd", [8, 10])
def test_crop_analyse_is_the_reference(ctx, bd):
    w, h = 90, 70
    Y = _buffers(_frames(bd, w, h), bd)
    want = R.records(Y, bd, w, h, LIMIT)
    assert tuple(want[0]) == (9, h - 1 - 9, 40, w - 1 - 40) and tuple(want[1]) == (0, 20, 0, 0) and tuple(want[2]) == (h, h, w, w) and tuple(want[3]) == (0, 0, 0, 0)
    got = ctx.crop_analyse(Y, bd, (w, h), LIMIT)
    assert got.tolist() == want.tolist()
    for limit in (0, 23, 25, 255):
        assert ctx.crop_analyse(Y, bd, (w, h), limit).tolist() == R.records(Y, bd, w, h, limit).tolist(), limit


@pytest.mark.parametrize("bd,w,h", [(8, 16, 16), (10, 8, 8), (8, 10, 9), (10, 13, 11), (8, 1100, 70), (10, 530, 131), (12, 40, 24)])
def test_crop_analyse_sizes(ctx, bd, w, h):
    """a width of one 16-byte unit; a width below one; more than one tile across (1024 / 512 samples) and down (64 rows); 12 bits"""
    rng = np.random.default_rng(w * 131 + h)
    f = rng.integers(LIMIT - 8, LIMIT + 9, (3, h, w)).astype(np.int64)
    f[1, :, : w // 3] = 0
    f[1, h - h // 4:] = 1
    f[2] = 0
    Y = _buffers(f << (bd - 8), bd)
    assert ctx.crop_analyse(Y, bd, (w, h), LIMIT).tolist() == R.records(Y, bd, w, h, LIMIT).tolist()


def test_crop_analyse_refuses_bad_arguments(ctx, av1mi):
    Y = np.zeros((1, 72, 96), np.uint8)
    for bd, true, limit in ((9, (90, 70), 24), (8, (97, 70), 24), (8, (90, 73), 24), (8, (88, 70), 24), (8, (90, 64), 24), (8, (0, 70), 24), (8, (90, 70), 256), (8, (90, 70), -1)):
        with pytest.raises(av1mi.Av1miError):
            ctx.crop_analyse(Y, bd, true, limit)
    with pytest.raises(av1mi.Av1miError):
        ctx.crop_analyse(np.zeros((1, 72, 90), np.uint8), 8, (90, 70), 24)      # the buffer's width is not a multiple of 8


# ---------------------------------------------------------------------------------------------- session
Q, GOP, SEGS = 110, 3, 2


def _source(sw, sh, bd, win, seed, chroma444=False):
    """GOP batches of SEGS whole frames [Y, U, V] at their true sizes: random NOISE everywhere, a smooth moving picture inside the window"""
    import synth
    x, y, cw, ch = win
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bd == 8 else np.uint16
    per = [synth.frames(_r8(cw) + 8, _r8(ch) + 8, GOP, bd, seed + 7 * s) for s in range(SEGS)]
    out = []
    for t in range(GOP):
        batch = []
        for s in range(SEGS):
            Y = rng.integers(0, 1 << bd, (sh, sw)).astype(dt)
            Y[y:y + ch, x:x + cw] = per[s][0][t][:ch, :cw]
            if chroma444:      # full-size chroma planes: the picture's chroma enlarged, noise around it
                U, V = (rng.integers(0, 1 << bd, (sh, sw)).astype(dt) for _ in range(2))
                for P, k in ((U, 1), (V, 2)):
                    P[y:y + ch, x:x + cw] = np.repeat(np.repeat(per[s][k][t][:ch // 2, :cw // 2], 2, axis=0), 2, axis=1)
            else:
                hw, hh = (sw + 1) // 2, (sh + 1) // 2
                U, V = (rng.integers(0, 1 << bd, (hh, hw)).astype(dt) for _ in range(2))
                U[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2] = per[s][1][t][:ch // 2, :cw // 2]
                V[y // 2:(y + ch) // 2, x // 2:(x + cw) // 2] = per[s][2][t][:ch // 2, :cw // 2]
            batch.append([Y, U, V])
        out.append(batch)
    return out


def _stack(batch, shapes, fill):
    """SEGS frames (three planes each, at their true sizes) -> stacked buffers of shapes[p] = (rows, width) per frame; the padding holds
    `fill`, or with fill None the frame's own last column / row (what a session without scaling expects)"""
    out = []
    for p, (ph, pw) in enumerate(shapes):
        buf = np.full((len(batch), ph, pw), fill or 0, batch[0][p].dtype)
        for s, planes in enumerate(batch):
            h, w = planes[p].shape
            if fill is None:
                buf[s] = np.pad(planes[p], ((0, ph - h), (0, pw - w)), mode="edge")
            else:
                buf[s, :h, :w] = planes[p]
        out.append(buf.reshape(len(batch) * ph, pw))
    return out


def _420(w8, h8):
    return [(h8, w8), (h8 // 2, w8 // 2), (h8 // 2, w8 // 2)]


def _session(ctx, av1mi, w, h, bd, fed, **kw):
    s = av1mi.GopSession(ctx, w, h, bd, Q, GOP, SEGS, gpu_entropy=1, **kw)
    outs = []
    try:
        for planes in fed:
            for dst, a in zip(s.input_planes(), planes):
                assert dst.shape == a.shape, (dst.shape, a.shape)
                dst[:] = a
            s.submit()
            fr = s.collect()
            o = {k: fr[k].copy() for k in ("tile_size", "tile_payload", "lr_on")}
            o["frame_type"] = fr["frame_type"]
            o["ref_y"], o["ref_u"], o["ref_v"] = s.download_reference()
            outs.append(o)
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    return outs


def _same(base, got, what):
    assert len(base) == len(got) == GOP and [o["frame_type"] for o in base] == [0, 1, 1]
    for t, (a, b) in enumerate(zip(base, got)):
        for k in a:
            assert np.array_equal(a[k], b[k]), "%s: batch %d, %s differs from the session without a window fed the pre-cropped frames" % (what, t, k)


def _window_property(ctx, av1mi, src, win, bd, seed, target=None, **kw):
    """the defining property for one geometry.  target: the coded true size where the window is scaled to it"""
    sw, sh = src
    x, y, cw, ch = win
    tw, th = target or (cw, ch)
    w, h = _r8(tw), _r8(th)
    visible = (tw, th) if (w, h) != (tw, th) else None
    frames = _source(sw, sh, bd, win, seed)
    cut = [[R.window(f, x, y, cw, ch) for f in batch] for batch in frames]
    fill = (1 << bd) - 1
    fed = [_stack(batch, _420(_r8(sw), _r8(sh)), fill) for batch in frames]
    if target:      # against the scaling session fed the pre-cropped frames
        base = _session(ctx, av1mi, w, h, bd, [_stack(batch, _420(_r8(cw), _r8(ch)), fill) for batch in cut], source=(cw, ch), visible=visible, **kw)
    else:
        base = _session(ctx, av1mi, w, h, bd, [_stack(batch, _420(w, h), None) for batch in cut], visible=visible, **kw)
    got = _session(ctx, av1mi, w, h, bd, fed, source=src, crop=win, visible=visible, **kw)
    _same(base, got, "source %dx%d window %dx%d+%d+%d %d-bit" % (sw, sh, cw, ch, x, y, bd))
    return base


def test_window_rows_start_off_a_16_byte_boundary_8bit(ctx, av1mi):
    """luma rows of the window start 2 bytes past a 16-byte boundary, chroma rows at an odd byte (x / 2 = 9)"""
    _window_property(ctx, av1mi, (96, 80), (18, 22, 64, 48), 8, 1)


def test_window_rows_start_off_a_16_byte_boundary_10bit(ctx, av1mi):
    """x = 14: luma rows start 28 bytes in (12 past a boundary), chroma rows 14 bytes in"""
    _window_property(ctx, av1mi, (96, 80), (14, 22, 64, 48), 10, 2)


@pytest.mark.parametrize("bd", [8, 10])
def test_window_that_is_no_multiple_of_8(ctx, av1mi, bd):
    """52 x 38: coded 56 x 40, visible 52 x 38; the padding replicates the WINDOW's last column / row, not the frame's noise behind it"""
    _window_property(ctx, av1mi, (96, 80), (18, 22, 52, 38), bd, 3)


@pytest.mark.parametrize("bd", [8, 10])
def test_window_ends_at_the_last_true_column_and_row(ctx, av1mi, bd):
    """a 90 x 70 source in 96 x 72 buffers whose padding holds the maximum: the window's last column is the source's column 89"""
    _window_property(ctx, av1mi, (90, 70), (26, 22, 64, 48), bd, 4)


def test_window_with_key_frames_in_32x32_blocks(ctx, av1mi):
    _window_property(ctx, av1mi, (96, 80), (18, 14, 64, 64), 8, 5, key_block_size=32)


@pytest.mark.parametrize("bd", [8, 10])
def test_window_scaled_clamps_at_the_window_edge(ctx, av1mi, bd):
    """64 x 48 of a 160 x 120 source scaled to 32 x 24 (12 taps): the taps that reach beyond the window read its edge, not the noise"""
    _window_property(ctx, av1mi, (160, 120), (42, 30, 64, 48), bd, 6, target=(32, 24))


def test_window_scaled_to_a_size_that_is_no_multiple_of_8(ctx, av1mi):
    _window_property(ctx, av1mi, (160, 120), (42, 30, 64, 48), 8, 7, target=(44, 30))


def test_window_behind_the_frame_store_and_the_deinterlacer(ctx, av1mi):
    """deinterlace 1 runs in the gather on the WHOLE fed frame, the window follows: the reference session is fed deinterlace_ref's
    frames, sliced"""
    import deinterlace_ref as DR
    src, win, bd = (96, 80), (18, 22, 64, 48), 8
    x, y, cw, ch = win
    frames = _source(96, 80, bd, win, 8)
    # the store's run in file order: segment s holds frames s * GOP + t
    run = [np.stack([frames[t][s][p] for s in range(SEGS) for t in range(GOP)]) for p in range(3)]
    woven = [DR.run(a, a.shape[2], a.shape[1], 0) for a in run]
    cut = [[R.window([woven[p][s * GOP + t] for p in range(3)], x, y, cw, ch) for s in range(SEGS)] for t in range(GOP)]
    base = _session(ctx, av1mi, cw, ch, bd, [_stack(batch, _420(cw, ch), None) for batch in cut])
    s = av1mi.GopSession(ctx, cw, ch, bd, Q, GOP, SEGS, gpu_entropy=1, source=src, crop=win, store_frames=SEGS * GOP, deinterlace=1)
    got = []
    try:
        for f0 in range(0, SEGS * GOP, SEGS):
            for dst, a in zip(s.input_planes(), run):
                dst[:] = a[f0:f0 + SEGS].reshape(dst.shape)
            s.store_put(0, f0, SEGS)
        for t in range(GOP):
            s.submit_stored(0, [sg * GOP + t for sg in range(SEGS)], 0 if t == 0 else 1)
            fr = s.collect()
            o = {k: fr[k].copy() for k in ("tile_size", "tile_payload", "lr_on")}
            o["frame_type"] = fr["frame_type"]
            o["ref_y"], o["ref_u"], o["ref_v"] = s.download_reference()
            got.append(o)
        assert s.entropy_fallbacks() == 0
    finally:
        s.close()
    _same(base, got, "stored, deinterlaced, window")


def test_window_of_a_444_10bit_source(ctx, av1mi):
    """the chroma stage converts the whole 4:4:4 frame, the window is cut from its 4:2:0 output (chroma, then crop: two stages)"""
    import chroma_formats_ref as CR
    src, win, bd = (96, 80), (18, 22, 64, 48), 10
    x, y, cw, ch = win
    frames = _source(96, 80, bd, win, 9, chroma444=True)
    fed = [_stack(batch, [(80, 96)] * 3, 1023) for batch in frames]
    cut = []
    for planes in fed:
        cy, cu, cv = CR.convert_stack(CR.C444, 10, 10, 96, 80, SEGS, planes)
        cut.append([R.window([cy[s * 80:(s + 1) * 80], cu[s * 40:(s + 1) * 40], cv[s * 40:(s + 1) * 40]], x, y, cw, ch) for s in range(SEGS)])
    base = _session(ctx, av1mi, cw, ch, bd, [_stack(batch, _420(cw, ch), None) for batch in cut])
    got = _session(ctx, av1mi, cw, ch, bd, fed, source=src, crop=win, source_chroma=av1mi.CHROMA_444, source_bit_depth=10)
    _same(base, got, "4:4:4 10-bit, window")


def test_window_composes_with_nv12_quality_and_coarse_range(ctx, av1mi):
    """a wire format in front (convert, then crop), the quality records measured against the cropped frame, the coarse search"""
    import input_formats_ref as F
    src, win, bd = (96, 80), (18, 22, 64, 48), 8
    x, y, cw, ch = win
    frames = _source(96, 80, bd, win, 10)
    cut = [[R.window(f, x, y, cw, ch) for f in batch] for batch in frames]
    kw = dict(quality_stats=1, coarse_range=16)

    def run(w, h, fed, fmt, **more):
        s = av1mi.GopSession(ctx, w, h, bd, Q, GOP, SEGS, gpu_entropy=1, input_format=fmt, **kw, **more)
        outs = []
        try:
            for planes in fed:
                wire = planes if fmt == F.PLANAR else F.pack(fmt, bd, *planes)
                for dst, a in zip(s.input_planes(), wire):
                    dst[:] = a if fmt == F.PLANAR else a.view(np.uint8).ravel()
                s.submit()
                fr = s.collect()
                o = {k: fr[k].copy() for k in ("tile_size", "tile_payload", "lr_on", "quality")}
                o["ref_y"], o["ref_u"], o["ref_v"] = s.download_reference()
                outs.append(o)
        finally:
            s.close()
        return outs
    base = run(cw, ch, [_stack(batch, _420(cw, ch), None) for batch in cut], F.PLANAR)
    got = run(cw, ch, [_stack(batch, _420(96, 80), 255) for batch in frames], F.NV12, source=src, crop=win)
    for t, (a, b) in enumerate(zip(base, got)):
        for k in a:
            assert np.array_equal(a[k], b[k]), "NV12 + window: batch %d, %s differs" % (t, k)


def test_session_refuses_bad_windows(ctx, av1mi):
    for kw in (dict(crop=(18, 22, 64, 48)), dict(source=(96, 80), crop=(17, 22, 64, 48)), dict(source=(96, 80), crop=(34, 22, 64, 48)),
               dict(source=(90, 70), crop=(28, 22, 64, 48))):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, 64, 48, 8, Q, GOP, SEGS, **kw)
        assert "crop window" in str(e.value)


def test_session_without_a_window_launches_what_it_did(ctx, av1mi):
    """a plain session launches nothing of the input kind; a window of the target's size costs one launch per batch (k_crop_copy), a
    scaled window one (k_scale)"""
    frames = _source(96, 80, 8, (18, 22, 64, 48), 11)
    cut = [[R.window(f, 18, 22, 64, 48) for f in batch] for batch in frames]
    ctx.prof_enable(1)
    try:
        for fed, kw, launches in (([_stack(b, _420(64, 48), None) for b in cut], {}, None),
                                  ([_stack(b, _420(96, 80), 255) for b in frames], dict(source=(96, 80), crop=(18, 22, 64, 48)), GOP)):
            ctx.prof_reset()
            _session(ctx, av1mi, 64, 48, 8, fed, **kw)
            prof = ctx.prof_get()
            assert (prof["input_convert"][0] if "input_convert" in prof else None) == launches
    finally:
        ctx.prof_enable(0)


# ---------------------------------------------------------------------------------------------- product
N, TG, TS = 8, 4, 2
PLAIN_CHAIN = "scale_vaapi=w=ceil(iw/2)*2:h=ceil(ih/2)*2,hwdownload,format=nv12,setsar=1,format=nv12,hwupload"


def _letterboxed(bd):
    """(barred, picture): a 128 x 64 picture at y = 16 of a 128 x 96 frame between bars of 16 (8-bit) / 64 (10-bit), chroma bars at mid grey"""
    import synth
    Y, U, V = synth.frames(128, 64, N, bd, 21)
    pic = [np.stack(Y), np.stack(U), np.stack(V)]
    dt = pic[0].dtype
    bar = [np.full((N, 96, 128), 16 << (bd - 8), dt), np.full((N, 48, 64), 1 << (bd - 1), dt), np.full((N, 48, 64), 1 << (bd - 1), dt)]
    bar[0][:, 16:80] = pic[0]
    bar[1][:, 8:40] = pic[1]
    bar[2][:, 8:40] = pic[2]
    return bar, pic


@pytest.fixture(scope="module", params=[8, 10])
def outputs(request, tmp_path_factory):
    import av1stream
    import deint_clips as K
    bd = request.param
    d = tmp_path_factory.mktemp("crop%d" % bd)
    bar, pic = _letterboxed(bd)
    K.write_y4m(d / "bars.y4m", bar, bd, interlace="p")
    K.write_y4m(d / "pic.y4m", pic, bd, interlace="p")
    runs = dict(auto=("bars.y4m", ["-av1mi_crop", "auto", "-av1mi_stats", d / "auto.stats"]), pre=("pic.y4m", ["-av1mi_stats", d / "pre.stats"]),
                chain=("bars.y4m", ["-vf:v:0", "crop=128:64:0:16," + PLAIN_CHAIN]), pre_chain=("pic.y4m", ["-vf:v:0", PLAIN_CHAIN]),
                explicit=("bars.y4m", ["-av1mi_crop", "128:64:0:16"]), nobars=("pic.y4m", ["-av1mi_crop", "auto"]),
                off=("bars.y4m", ["-av1mi_crop", "off"]), absent=("bars.y4m", []), outside=("bars.y4m", ["-av1mi_crop", "128:64:0:48"]))
    out = {"bd": bd, "dir": d}
    for name, (source, extra) in runs.items():
        path = d / (name + ".obu")
        code, err = av1stream.run_transcode(["-i", d / source, "-global_quality:v:0", Q, "-g", TG, "-av1mi_segments", TS] + extra + [path])
        out[name] = (code, err, path.read_bytes() if code == 0 else b"")
    return out


def test_auto_crop_equals_the_pre_cropped_source(ctx, av1mi, outputs):
    import dav1d_ref as D
    for name in ("auto", "pre"):
        assert outputs[name][0] == 0, outputs[name][1]
    assert outputs["auto"][2] == outputs["pre"][2] and outputs["auto"][2] != outputs["absent"][2]
    first = (outputs["dir"] / "auto.stats").read_text().splitlines()[0]
    assert " crop:128x64+0+16" in first and "crop:" not in (outputs["dir"] / "pre.stats").read_text()
    assert "crop:" not in "".join((outputs["dir"] / "auto.stats").read_text().splitlines()[1:])
    if not D.available():
        return
    # dav1d decodes 128 x 64 frames: the references of a session with the window fed the whole frames, as the product drives it
    bd = outputs["bd"]
    bar, _ = _letterboxed(bd)
    got = D.decode(outputs["auto"][2])
    assert len(got) == N and all(f[0].shape == (64, 128) and f[1].shape == (32, 64) for f in got)
    s = av1mi.GopSession(ctx, 128, 64, bd, Q, TG, TS, gpu_entropy=1, key_block_size=32, source=(128, 96), crop=(0, 16, 128, 64))
    try:
        for t in range(TG):
            for dst, a in zip(s.input_planes(), bar):
                dst[:] = np.concatenate([a[sg * TG + t] for sg in range(TS)])
            s.submit()
            s.collect()
            ref = s.download_reference()
            for sg in range(TS):
                for i, rows in enumerate((64, 32, 32)):
                    assert (got[sg * TG + t][i] == ref[i][sg * rows:(sg + 1) * rows]).all(), "frame %d plane %d: dav1d decodes another picture than the session's reference" % (sg * TG + t, i)
    finally:
        s.close()


def test_explicit_crop_in_the_chain_and_as_an_option(outputs):
    for name in ("chain", "pre_chain", "explicit"):
        assert outputs[name][0] == 0, outputs[name][1]
    assert outputs["chain"][2] == outputs["pre_chain"][2] == outputs["pre"][2]
    assert outputs["explicit"][2] == outputs["pre"][2]
    code, err, _ = outputs["outside"]
    assert code == 1 and "lies outside the 128x96 picture" in err


def test_nothing_to_crop_takes_todays_path(outputs):
    for name in ("nobars", "off", "absent"):
        assert outputs[name][0] == 0, outputs[name][1]
    assert outputs["nobars"][2] == outputs["pre"][2]
    assert outputs["off"][2] == outputs["absent"][2]
