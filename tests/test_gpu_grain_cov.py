"""GPU tests of the grain covariance (include/av1mi.h "grain covariance", av1mi_gop_config.grain_cov, -av1mi_grain_lag): k_grain_cov +
k_grain_cov_sum against tests/grain_cov_ref.py bit for bit, fed directly, behind both denoising gathers, in a session and in a job."""
import numpy as np
import pytest

import denoise_ref as R
import grain_cov_ref as GC

pytestmark = pytest.mark.gpu


def _sizes(w, h):
    return [(w, h), (w // 2, h // 2), (w // 2, h // 2)]


def _true(w, h):
    return [(w, h), ((w + 1) // 2, (h + 1) // 2), ((w + 1) // 2, (h + 1) // 2)]


def _cov(ctx, av1mi, fed, out, sizes, true, bd, twice=False):
    """fed[p], out[p]: [S, H, W] per plane (fed[p][s] may be None: a flat slot's null C) -> the records [S, 3] of av1mi_grain_cov, checked for
    writes beyond their end; out is what a gather would have written"""
    S = len(out[0])
    dt = np.uint8 if bd == 8 else np.uint16
    bufs, rows = [], []
    for s in range(S):
        for p in range(3):
            c = None if fed[p][s] is None else ctx.to_device(np.ascontiguousarray(fed[p][s], dt))
            bufs.append(c)
            rows.append([0, c.ptr if c is not None else 0, 0])
    d_table = ctx.to_device(np.array(rows, np.uint64))
    d_out = [ctx.to_device(np.ascontiguousarray(np.stack(out[p]), dt)) for p in range(3)]
    nbytes = S * 3 * av1mi.GRAIN_COV_DTYPE.itemsize
    guard = 64
    d_cov = ctx.to_device(np.full(nbytes + guard, 0xA5, np.uint8))
    try:
        ctx.grain_cov(bd, sizes, true, S, d_table, d_out, d_cov)
        raw = d_cov.download((nbytes + guard,), np.uint8)
        assert (raw[nbytes:] == 0xA5).all(), "records: written beyond their end"
        if twice:
            ctx.grain_cov(bd, sizes, true, S, d_table, d_out, d_cov)
            assert d_cov.download((nbytes + guard,), np.uint8).tobytes() == raw.tobytes(), "two calls, other bytes"
        return raw[:nbytes].view(np.int64).reshape(S, 3, GC.DY, GC.DX)
    finally:
        for b in bufs + d_out + [d_table, d_cov]:
            if b is not None:
                b.free()


def _check(got, fed, out, true):
    for s in range(got.shape[0]):
        for p in range(3):
            want = GC.plane(fed[p][s], out[p][s], true[p][0], true[p][1])
            bad = np.argwhere(got[s, p] != want)
            assert bad.size == 0, "segment %d plane %d: %d sums differ, the first at (dy, dx + 6) = %s: %d, not %d" % (
                s, p, len(bad), bad[0], got[s, p][tuple(bad[0])], want[tuple(bad[0])])


# (buffer size, true size, bit depth): 4x4 chroma planes, whose offsets beyond the plane come out 0, in the dword form; several workgroups
# across a row and a partial last cell; a band boundary, the true edge inside the buffer and 16-bit samples
SHAPES = {"8x8": ((8, 8), (8, 8), 8), "1048x24": ((1048, 24), (1048, 24), 8), "72x40": ((72, 40), (70, 38), 10)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_grain_cov_is_the_reference(ctx, av1mi, name):
    (W, H), (w, h), bd = SHAPES[name]
    sizes, true = _sizes(W, H), _true(w, h)
    rng = np.random.default_rng(7)
    top = (1 << bd) - 1
    fed, out = [], []
    for (pw, ph), (tw, th) in zip(sizes, true):
        c = rng.integers(0, top + 1, (ph, pw))
        o = np.clip(c + np.rint(rng.normal(0, 6 << (bd - 8), c.shape)).astype(np.int64), 0, top)
        for a, fill in ((c, top), (o, 0)):      # garbage beyond the true size, different in the two: it must not enter
            a[th:, :] = fill
            a[:, tw:] = top - fill
        fed.append([c, None])                   # the second segment is a flat slot: no C, zeros written
        out.append([o, np.zeros_like(o)])
    got = _cov(ctx, av1mi, fed, out, sizes, true, bd, twice=True)
    _check(got, fed, out, true)
    assert got[0, 0, 0, 6] > 0 and not got[1].any()
    if name == "8x8":      # a 4x4 plane has no pair at |dx| >= 4
        assert not got[0, 1][:, :3].any() and not got[0, 1][:, 10:].any() and got[0, 1][3, 6] != 0


def test_grain_cov_extreme_content(ctx, av1mi):
    """r alternates +1023 / -1023 over 1048x24 at 10 bits: sum[0][6] = 1048 x 24 x 1023^2 > 2^32, and a lane's share of a band reaches
    the stated 256 products of 1023^2"""
    bd, (W, H) = 10, (1048, 24)
    sizes = _sizes(W, H)
    fed, out = [], []
    for pw, ph in sizes:
        y, x = np.mgrid[0:ph, 0:pw]
        c = ((x + y) & 1) * 1023
        fed.append([c, 1023 - c])
        out.append([1023 - c, c])
    got = _cov(ctx, av1mi, fed, out, sizes, sizes, bd)
    _check(got, fed, out, sizes)
    assert got[0, 0, 0, 6] == W * H * 1023 ** 2 and got[0, 0, 0, 6] > 1 << 32 and got[0, 0, 0, 7] < -(1 << 32)


@pytest.mark.parametrize("rng", [0, 4])
def test_grain_cov_behind_both_gathers(ctx, av1mi, rng):
    """a clip with a moving block through av1mi_denoise_gather (rng 0) / av1mi_denoise_mc_gather, av1mi_grain_cov on what they wrote"""
    import test_gpu_denoise as TD
    bd, (W, H), strength, n = 8, (72, 40), 4, 4
    sizes = _sizes(W, H)
    planes = TD._clip(sizes, n, bd, 3, sigma=2)
    index = list(range(n))
    nbytes = [a[0].nbytes for a in planes]
    d_store = [ctx.to_device(a) for a in planes]
    pos = lambda f: (max(f - 1, 0), f, min(f + 1, n - 1))
    d_table = ctx.to_device(np.array([[[d_store[p].ptr + q * nbytes[p] for q in pos(f)] for p in range(3)] for f in index], np.uint64))
    d_dst = [ctx.alloc(n * b) for b in nbytes]
    d_cov = ctx.alloc(n * 3 * av1mi.GRAIN_COV_DTYPE.itemsize)
    try:
        if rng:
            ctx.denoise_mc_gather(bd, sizes, sizes, strength, rng, n, d_table, d_dst)
        else:
            ctx.denoise_gather(bd, sizes, sizes, strength, n, d_table, d_dst)
        ctx.grain_cov(bd, sizes, sizes, n, d_table, d_dst, d_cov)
        got = d_cov.download((n, 3, GC.DY, GC.DX), np.int64)
        wrote = [d_dst[p].download(planes[p].shape, planes[p].dtype) for p in range(3)]
    finally:
        for b in d_store + d_dst + [d_table, d_cov]:
            b.free()
    if not rng:      # the plain gather's output is the reference's (tests/test_gpu_denoise.py): the covariance is the reference's too
        for p in range(3):
            assert (wrote[p] == R.run(planes[p], sizes[p][0], sizes[p][1], bd, strength)[0]).all()
    _check(got, [list(a) for a in planes], [list(a) for a in wrote], sizes)
    assert not got[0].any() and not got[n - 1].any(), "the ends of the run pass through: zero records"
    assert all(got[f, p, 0, 6] > 0 for f in (1, 2) for p in range(3))


# ---------------------------------------------------------------------------------------------- session
W, H, Q, S, G = 192, 128, 110, 2, 3


def _run_session(ctx, av1mi, clip, **kw):
    import av1stream
    s = av1mi.GopSession(ctx, W, H, 8, Q, G, S, gpu_entropy=2, store_frames=S * G, **kw)
    out = []
    try:
        for f0 in range(0, S * G, S):
            for dst, a in zip(s.input_planes(), clip):
                dst[:] = a[f0:f0 + S].reshape(dst.shape)
            s.store_put(0, f0, S)
        for t in range(G):
            s.submit_stored(0, [sg * G + t for sg in range(S)], 0 if t == 0 else 1)
            fr = s.collect()
            out.append(dict(units=[av1stream.session_temporal_unit(W, H, 8, fr["raw"], sg, with_sequence_header=t == 0) for sg in range(S)],
                            cov=fr["grain_cov"]["sum"].copy() if "grain_cov" in fr else None, raw_cov=fr["raw"].grain_cov))
    finally:
        s.close()
    return out


@pytest.mark.parametrize("rng", [0, 8])
def test_session_delivers_the_covariance_and_codes_the_same_bytes(ctx, av1mi, rng):
    import test_gpu_denoise as TD
    clip = TD._clip(_sizes(W, H), S * G, 8, 21, sigma=2)
    kw = dict(denoise=4, denoise_range=rng) if rng else dict(denoise=4)
    plain, unset, on = (_run_session(ctx, av1mi, clip, **dict(kw, **more)) for more in ({}, dict(grain_cov=0), dict(grain_cov=1)))
    for a, b, c in zip(plain, unset, on):
        assert a["raw_cov"] is None and b["raw_cov"] is None and a["units"] == b["units"] == c["units"]
    if not rng:
        want = [R.run(a, a.shape[2], a.shape[1], 8, 4)[0] for a in clip]
        for t, b in enumerate(on):
            for sg in range(S):
                f = sg * G + t
                for p in range(3):
                    ref = GC.plane(clip[p][f], want[p][f], clip[p].shape[2], clip[p].shape[1])
                    assert (b["cov"][sg, p] == ref).all(), "batch %d segment %d plane %d: not the reference's covariance" % (t, sg, p)
    # the run is the store's S * G frames: its first frame is batch 0's segment 0, its last one the last batch's last segment
    assert not on[0]["cov"][0].any() and not on[G - 1]["cov"][S - 1].any() and all(on[1]["cov"][sg, p, 0, 6] > 0 for sg in range(S) for p in range(3))


def test_session_refuses_grain_cov_without_denoise(ctx, av1mi):
    for kw in (dict(grain_cov=1, store_frames=4), dict(grain_cov=2, denoise=4, store_frames=4), dict(grain_cov=-1, denoise=4, store_frames=4)):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, W, H, 8, Q, G, S, **kw)
        assert "grain_cov" in str(e.value)


def test_grain_cov_refuses_bad_arguments(ctx, av1mi):
    d = ctx.to_device(np.zeros(8192, np.uint8))
    ok = dict(bit_depth=8, plane_sizes=[(8, 8), (4, 4), (4, 4)], true_sizes=[(8, 8), (4, 4), (4, 4)], segments=1, d_table=d, d_out=[d, d, d], d_cov=d)
    ctx.grain_cov(**ok)
    for bad in (dict(bit_depth=12), dict(segments=0), dict(true_sizes=[(9, 8), (4, 4), (4, 4)]), dict(d_cov=None),
                dict(plane_sizes=[(20, 8), (4, 4), (4, 4)], true_sizes=[(13, 8), (4, 4), (4, 4)])):
        with pytest.raises(av1mi.Av1miError):
            ctx.grain_cov(**dict(ok, **bad))
    ctx.sync()
    d.free()


# ---------------------------------------------------------------------------------------------- product
def test_transcode_with_grain_lag_codes_coloured_grain(tmp_path):
    """a still ramp under grain smoothed by [1 2 1] x [1 2 1], 10 frames: -av1mi_denoise 8 -av1mi_grain_lag 2 gives frame headers with
    ar_coeff_lag 2 (the stats lines' ar: field says what was coded; the grain dav1d synthesises from the stream is correlated with its
    right-hand neighbour, which white grain is not), and -av1mi_grain_lag 0 is the job without the option, byte for byte"""
    import av1stream
    import dav1d_grain as DG
    import deint_clips as K
    import grain_ar_loop as L
    assert DG.available(), "dav1d is needed to check the stream"
    n = 10
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:H, 0:W]
    clean = [np.full((H, W), 120.0) + 40 * (x >= W // 2), np.full((H // 2, W // 2), 128.0), np.full((H // 2, W // 2), 128.0)]
    clip = [np.clip(np.rint(a[None] + np.stack([L.coloured(rng, a.shape, 4.0) for _ in range(n)])), 0, 255).astype(np.uint8) for a in clean]
    K.write_y4m(tmp_path / "grainy.y4m", clip, 8, interlace="p")
    data, lines = {}, {}
    for name, extra in (("lag2", ["-av1mi_grain_lag", 2]), ("lag0", ["-av1mi_grain_lag", 0]), ("none", [])):
        path = tmp_path / (name + ".obu")
        code, err = av1stream.run_transcode(["-i", tmp_path / "grainy.y4m", "-global_quality:v:0", Q, "-g", 5, "-av1mi_segments", 2, "-av1mi_denoise", 8,
                                             "-av1mi_stats", tmp_path / (name + ".txt")] + extra + [path])
        assert code == 0, err
        data[name] = path.read_bytes()
        lines[name] = [l for l in (tmp_path / (name + ".txt")).read_text().splitlines() if l.startswith("n:")]
    assert data["lag0"] == data["none"] and lines["lag0"] == lines["none"] and not any(" ar:" in l for l in lines["none"])
    ar = [int(l.split(" ar:")[1].split()[0]) for l in lines["lag2"]]
    assert len(ar) == n and ar[0] == ar[-1] == 0 and all(v == 2 for v in ar[1:-1]), ar      # the ends of the run pass through: no grain at all
    on, off = DG.decode(data["lag2"], True), DG.decode(data["lag2"], False)
    assert len(on) == n
    white_on, white_off = DG.decode(data["none"], True), DG.decode(data["none"], False)
    rho = L.rho_of(on[2][0].astype(np.float64) - off[2][0])[(1, 0)]
    rho_white = L.rho_of(white_on[2][0].astype(np.float64) - white_off[2][0])[(1, 0)]
    print("rho(1, 0) of the synthesised grain: %.3f with -av1mi_grain_lag 2, %.3f without" % (rho, rho_white))
    # the injected rho(1, 0) is 2/3 (L.INJECTED): more than half of it must come back; white grain over 192 x 128 samples stays within
    # 3 / sqrt(N) = 0.02 of 0, taken five times over for the overlap of the decoder's blocks
    assert rho > 1 / 3 and abs(rho_white) < 0.1
