"""GPU tests of the peak records (include/av1mi.h "peak records"; av1-go_amd/csrc/peak_kernels.hip): av1mi_peak_analyse against
tests/peak_ref.py, record for record.  No tolerance anywhere: every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import peak_ref as R

pytestmark = pytest.mark.gpu

# (buffer, true size): one workgroup; an odd true width, whose last pixel shares a chroma sample with the padding's neighbour; a true size
# that is no multiple of 8; chroma rows that are no whole 16-byte units; several workgroups down (16 rows each)
SIZES = [((8, 8), (8, 8)), ((16, 8), (9, 8)), ((96, 72), (90, 70)), ((264, 136), (263, 135)), ((528, 264), (523, 259))]


def _content(buf, true, frames, seed):
    """planes Y [frames, H8, W8], U / V [frames, H8 / 2, W8 / 2]: a PQ ramp over the whole code range (it shifts from frame to frame), patches
    of saturated chroma that make each of R', G', B' the maximum and that clamp at 0 and at 1023, in-picture samples above 1023, noise, and
    0xFFFF in everything at or beyond the true size"""
    (W8, H8), (w, h) = buf, true
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H8, 0:W8]
    Y = np.stack([(xx * 1100 // max(W8 - 1, 1) + yy * 37 + 131 * f) % 1100 for f in range(frames)])      # 0 .. 1099: the ramp runs past 1023
    Y += rng.integers(0, 3, Y.shape)
    U = np.full((frames, H8 // 2, W8 // 2), 512, np.int64) + rng.integers(-6, 7, (frames, H8 // 2, W8 // 2))
    V = np.full((frames, H8 // 2, W8 // 2), 512, np.int64) + rng.integers(-6, 7, (frames, H8 // 2, W8 // 2))
    ch, cw = H8 // 2, W8 // 2
    q = lambda a, i, j: a[:, i * ch // 4:(i + 1) * ch // 4 + 1, j * cw // 4:(j + 1) * cw // 4 + 1]      # chroma patch (i, j) of a 4 x 4 grid
    q(V, 0, 1)[:] = 960; q(U, 0, 1)[:] = 400      # R' the maximum, clamped at 1023 where the ramp is bright; B' and G' at 0 where it is dark
    q(U, 1, 2)[:] = 960; q(V, 1, 2)[:] = 450      # B' the maximum
    q(U, 2, 0)[:] = 64; q(V, 2, 0)[:] = 64        # G' the maximum; R' and B' clamped at 0
    q(U, 3, 3)[:] = 1023; q(V, 3, 3)[:] = 0       # out of the nominal range
    q(U, 2, 2)[:] = 3000; q(V, 2, 2)[:] = 1024    # above 1023: counts as 1023
    Y[:, :: 5, :: 7] += 40000                     # in-picture luma above 1023
    Y, U, V = (np.clip(a, 0, 0xFFFE).astype(np.uint16) for a in (Y, U, V))
    Y[:, h:, :] = 0xFFFF; Y[:, :, w:] = 0xFFFF
    for c in (U, V):
        c[:, (h + 1) // 2:, :] = 0xFFFF; c[:, :, (w + 1) // 2:] = 0xFFFF
    return Y, U, V


@pytest.fixture(scope="module")
def cases():
    """content and reference per (size, frames), computed once and left unchanged"""
    out = {}
    for buf, true in SIZES:
        for frames in (1, 5):
            planes = _content(buf, true, frames, 7 * buf[0] + frames)
            out[buf, true, frames] = planes, R.records(*planes, *true)
    return out


def test_the_content_has_what_it_should(cases):
    (Y, U, V), want = cases[(528, 264), (523, 259), 5]
    w, h = 523, 259
    M = R.max_rgb(Y[:, :h, :w], U[:, :130, :262], V[:, :130, :262])
    K = R.T.constants()["to_rgb"]
    y = K[0] * (np.minimum(Y[:, :h, :w].astype(np.int64), 1023) - 64) + 8192
    up = lambda c: np.repeat(np.repeat(np.minimum(c.astype(np.int64), 1023), 2, 1), 2, 2)[:, :h, :w] - 512
    r, g, b = (y + K[1] * up(V)) >> 14, (y - K[2] * up(V) - K[3] * up(U)) >> 14, (y + K[4] * up(U)) >> 14
    for first, others in ((r, (g, b)), (g, (r, b)), (b, (r, g))):
        assert ((first > others[0]) & (first > others[1])).any()      # each of the three is the maximum somewhere
        assert (first < 0).any() and (first > 1023).any()             # and clamps at both ends
    assert (want["hist"] > 0).sum(axis=1).min() > 900 and (Y[:, :h, :w] > 1023).any() and (U[:, :130, :262] > 1023).any()
    assert (Y[:, h:] == 0xFFFF).all() and (Y[:, :, w:] == 0xFFFF).all() and (U[:, 130:] == 0xFFFF).all() and (V[:, :, 262:] == 0xFFFF).all()
    assert (M == 1023).any() and (M == 0).any() and len({r.tobytes() for r in want}) == 5      # the frames differ


@pytest.mark.parametrize("frames", [1, 5])
@pytest.mark.parametrize("buf,true", SIZES)
def test_peak_analyse_is_the_reference(ctx, cases, buf, true, frames):
    planes, want = cases[buf, true, frames]
    assert want["pixels"].tolist() == [true[0] * true[1]] * frames and want["hist"].sum(axis=1).tolist() == [true[0] * true[1]] * frames
    got = ctx.peak_analyse(*planes, true)
    assert got.dtype == R.PEAK_DTYPE and got.tobytes() == want.tobytes(), (buf, true, frames)


def test_padding_is_not_read(ctx, cases):
    """the padding columns and rows of all three planes filled with other garbage: the same bytes"""
    for buf, true in (((96, 72), (90, 70)), ((16, 8), (9, 8)), ((264, 136), (263, 135))):
        (Y, U, V), want = cases[buf, true, 5]
        (w, h), Z = true, [a.copy() for a in (Y, U, V)]
        Z[0][:, h:, :] = 0; Z[0][:, :, w:] = 940
        Z[1][:, (h + 1) // 2:, :] = 1; Z[1][:, :, (w + 1) // 2:] = 1023
        Z[2][:, (h + 1) // 2:, :] = 1023; Z[2][:, :, (w + 1) // 2:] = 2
        assert ctx.peak_analyse(*Z, true).tobytes() == ctx.peak_analyse(Y, U, V, true).tobytes() == want.tobytes()


def _raw(ctx, shape, true, frames, d_y, d_u, d_v, d_out):
    ctx.lib.av1mi_peak_analyse.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4
    return ctx.lib.av1mi_peak_analyse(ctx.h, shape[0], shape[1], true[0], true[1], frames, d_y, d_u, d_v, d_out)


def test_guard_bytes_stay_intact(ctx, cases):
    """the records are written between guard bytes, and the planes end where the allocation's guard begins"""
    buf, true, frames, G = (96, 72), (90, 70), 5, 64
    planes, want = cases[buf, true, frames]
    size = frames * R.PEAK_DTYPE.itemsize
    guard = np.full(G // 2, 0xA5A5, np.uint16)
    d = [ctx.to_device(np.concatenate([a.reshape(-1), guard])) for a in planes]
    d_out = ctx.to_device(np.full(size + 2 * G, 0xA5, np.uint8))
    try:
        ctx._chk(_raw(ctx, buf, true, frames, d[0].ptr, d[1].ptr, d[2].ptr, d_out.ptr + G))
        raw = d_out.download((size + 2 * G,), np.uint8)
        assert (raw[:G] == 0xA5).all() and (raw[G + size:] == 0xA5).all()
        assert raw[G:G + size].tobytes() == want.tobytes()
        for b, a in zip(d, planes):
            back = b.download((a.size + G // 2,), np.uint16)
            assert (back[a.size:] == 0xA5A5).all() and (back[:a.size] == a.reshape(-1)).all()
    finally:
        for b in d + [d_out]:
            b.free()


def test_every_pixel_in_one_bin(ctx):
    """a flat 256 x 256 frame: all 65536 pixels in one bin, every atomic on one counter"""
    for y, u, v in ((300, 512, 700), (940, 512, 512), (64, 512, 512)):
        Y, U, V = np.full((1, 256, 256), y, np.uint16), np.full((1, 128, 128), u, np.uint16), np.full((1, 128, 128), v, np.uint16)
        M = int(R.max_rgb(Y[:, :1, :1], U[:, :1, :1], V[:, :1, :1])[0, 0, 0])
        r = ctx.peak_analyse(Y, U, V, (256, 256))[0]
        assert int(r["hist"][M]) == 65536 and int(r["hist"].sum()) == 65536 and int(r["pixels"]) == 65536, (y, u, v)
    assert M == 0


def test_two_runs_give_equal_bytes(ctx, cases):
    planes, want = cases[(528, 264), (523, 259), 5]
    first = ctx.peak_analyse(*planes, (523, 259))
    small, small_want = cases[(96, 72), (90, 70), 1]      # (the scratch, grown for the first, is reused)
    assert ctx.peak_analyse(*small, (90, 70)).tobytes() == small_want.tobytes()
    assert ctx.peak_analyse(*planes, (523, 259)).tobytes() == first.tobytes() == want.tobytes()


def test_the_plan_of_measured_records(ctx, cases):
    """kernel -> host plan == numpy reference -> numpy plan"""
    import av1stream
    for key in (((528, 264), (523, 259), 5), ((96, 72), (90, 70), 1)):
        planes, want = cases[key]
        peak, codes = av1stream.plan_peak(ctx.peak_analyse(*planes, key[1]))
        assert (peak, codes.tolist()) == R.plan(want)
    Y, U, V = np.full((2, 64, 64), 64, np.uint16), np.full((2, 32, 32), 512, np.uint16), np.full((2, 32, 32), 512, np.uint16)
    Y[1, 8:24, 8:24] = 700      # a patch of code 743, 792 cd/m2, in an otherwise black clip
    peak, codes = av1stream.plan_peak(ctx.peak_analyse(Y, U, V, (64, 64)))
    assert (peak, codes.tolist()) == R.plan(R.records(Y, U, V, 64, 64)) and codes.tolist() == [0, (19133 * 636 + 8192) >> 14] and peak == 792


def test_peak_analyse_refuses_bad_arguments(ctx, av1mi):
    buf, true = (96, 72), (90, 70)
    Y, U, V = np.zeros((1, 72, 96), np.uint16), np.zeros((1, 36, 48), np.uint16), np.zeros((1, 36, 48), np.uint16)
    for bad in ((97, 70), (90, 73), (88, 70), (90, 64), (0, 70), (90, 0)):      # a true size out of range
        with pytest.raises(av1mi.Av1miError):
            ctx.peak_analyse(Y, U, V, bad)
    d = [ctx.to_device(np.zeros(a.size + 16, np.uint16)) for a in (Y, U, V)]
    d_out = ctx.alloc(R.PEAK_DTYPE.itemsize + 16)
    p = [b.ptr for b in d]
    try:
        for offs, out_off, frames in (((8, 0, 0), 0, 1), ((0, 8, 0), 0, 1), ((0, 0, 4), 0, 1), ((0, 0, 0), 2, 1), ((0, 0, 0), 0, 0), ((0, 0, 0), 0, 65536), ((0, 0, 0), 0, -1)):
            assert _raw(ctx, buf, true, frames, p[0] + offs[0], p[1] + offs[1], p[2] + offs[2], d_out.ptr + out_off) != 0, (offs, out_off, frames)
        for shape in ((90, 72), (96, 70), (0, 72), (96, 16392)):      # a buffer that is no multiple of 8, or out of range
            assert _raw(ctx, shape, true, 1, p[0], p[1], p[2], d_out.ptr) != 0, shape
        for k in range(4):
            args = p + [d_out.ptr]
            args[k] = None
            assert _raw(ctx, buf, true, 1, *args) != 0
        ctx._chk(_raw(ctx, buf, true, 1, p[0], p[1], p[2], d_out.ptr))      # and the call they all differ from by one argument is taken
        ctx.sync()
    finally:
        for b in d + [d_out]:
            b.free()
