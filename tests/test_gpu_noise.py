"""GPU tests of the noise records (include/av1mi.h "noise records"; av1-go_amd/csrc/noise_kernels.hip): av1mi_noise_analyse against
tests/noise_ref.py, record for record.  No tolerance anywhere: every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import noise_ref as R

pytestmark = pytest.mark.gpu

# (buffer, true size): one block, one workgroup; one block beside a partial column of blocks; a true size that is no multiple of 8; rows
# that are not whole 16-byte units at 8 bits; more than one workgroup down (32 rows each), a unit whose second block is cut
SIZES = [((8, 8), (8, 8)), ((16, 8), (9, 8)), ((96, 72), (90, 70)), ((264, 136), (264, 136)), ((528, 264), (523, 259))]


def _content(bd, buf, true, pairs, seed):
    """2 * pairs planes [2 pairs, H8, W8]: noisy texture (sigma differs from pair to pair), blocks below and above the nominal range, a
    region that moves (bin 255), and 0xFF garbage in everything at or beyond the true size; deep samples carry low bits"""
    (W8, H8), (w, h) = buf, true
    rng = np.random.default_rng(seed)
    Y = np.concatenate([R.clip(W8, H8, 2, 0.5 + 2.5 * i, seed + i) for i in range(pairs)]).astype(np.int64)
    for i in range(pairs):
        Y[2 * i:2 * i + 2, : H8 // 3, : W8 // 4] = 3 + i            # below the range
        Y[2 * i:2 * i + 2, H8 - H8 // 4:, W8 - W8 // 4:] = 252      # above it
        Y[2 * i + 1, H8 // 3: H8 // 2, W8 // 2:] = rng.integers(16, 236, (H8 // 2 - H8 // 3, W8 - W8 // 2))      # moved
    if bd > 8:
        Y = (Y << (bd - 8)) | rng.integers(0, 1 << (bd - 8), Y.shape)
    Y = Y.astype(np.uint8 if bd == 8 else np.uint16)
    Y[:, h:, :] = 0xFF if bd == 8 else 0xFFFF
    Y[:, :, w:] = 0xFF if bd == 8 else 0xFFFF
    return Y


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("buf,true", SIZES)
def test_noise_analyse_is_the_reference(ctx, bd, buf, true):
    for pairs in (1, 5):
        Y = _content(bd, buf, true, pairs, 11 * bd + buf[0])
        want = R.records(Y, bd, *true)
        assert want["blocks"].tolist() == [(true[0] // 8) * (true[1] // 8)] * pairs
        got = ctx.noise_analyse(Y, bd, true)
        assert got.dtype == R.NOISE_DTYPE and got.tobytes() == want.tobytes(), (bd, buf, true, pairs)
        if pairs == 5 and buf[0] >= 96:
            assert len({r.tobytes() for r in want}) == 5 and all(int(r["eligible"]) > 0 for r in want)      # the pairs differ


@pytest.mark.parametrize("bd", [8, 10])
def test_padding_is_not_read(ctx, bd):
    """the padding columns and rows, and the partial blocks, filled with other garbage: the same records"""
    buf, true = (96, 72), (90, 70)
    Y = _content(bd, buf, true, 2, 5)
    Z = Y.copy()
    Z[:, 70:, :] = 0
    Z[:, :, 90:] = 1
    Z[:, 64:70, :] = 77 << (bd - 8)      # the partial row of blocks
    Z[:, :, 88:90] = 78 << (bd - 8)      # the partial column
    assert ctx.noise_analyse(Z, bd, true).tobytes() == ctx.noise_analyse(Y, bd, true).tobytes() == R.records(Y, bd, *true).tobytes()


def _raw(ctx, bd, Y, true, pairs, d_y=None, d_out=None):
    ctx.lib.av1mi_noise_analyse.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    return ctx.lib.av1mi_noise_analyse(ctx.h, bd, Y.shape[2], Y.shape[1], true[0], true[1], pairs, d_y, d_out)


def test_guard_bytes_stay_intact(ctx):
    """the records are written between guard bytes, and the planes end where the allocation's guard begins"""
    bd, buf, true, pairs, G = 8, (96, 72), (90, 70), 3, 64
    Y = _content(bd, buf, true, pairs, 9)
    size = pairs * R.NOISE_DTYPE.itemsize
    d_y = ctx.to_device(np.concatenate([Y.reshape(-1), np.full(G, 0xA5, np.uint8)]))
    d_out = ctx.to_device(np.full(size + 2 * G, 0xA5, np.uint8))
    try:
        ctx._chk(_raw(ctx, bd, Y, true, pairs, d_y.ptr, d_out.ptr + G))
        raw = d_out.download((size + 2 * G,), np.uint8)
        assert (raw[:G] == 0xA5).all() and (raw[G + size:] == 0xA5).all()
        assert raw[G:G + size].tobytes() == R.records(Y, bd, *true).tobytes()
        assert (d_y.download((Y.size + G,), np.uint8)[Y.size:] == 0xA5).all()
    finally:
        d_y.free()
        d_out.free()


def test_every_block_in_one_bin(ctx):
    """two flat 256 x 256 planes at level 128: all 1024 blocks in bin 0, every atomic on one counter; at level 8 nothing is eligible"""
    Y = np.full((2, 256, 256), 128, np.uint8)
    r = ctx.noise_analyse(Y, 8, (256, 256))[0]
    assert int(r["hist"][0]) == 1024 and int(r["hist"].sum()) == 1024 and (int(r["eligible"]), int(r["blocks"])) == (1024, 1024)
    r = ctx.noise_analyse(np.full((2, 256, 256), 8, np.uint8), 8, (256, 256))[0]
    assert int(r["hist"].sum()) == 0 and (int(r["eligible"]), int(r["blocks"])) == (0, 1024)
    Z = np.full((2, 256, 256), 128 << 2, np.uint16)
    Z[1] += 64      # 16 codes of difference everywhere: bin 255
    r = ctx.noise_analyse(Z, 10, (256, 256))[0]
    assert int(r["hist"][255]) == 1024 and int(r["eligible"]) == 1024


def test_two_runs_give_equal_bytes(ctx):
    Y = _content(10, (528, 264), (523, 259), 5, 21)
    first = ctx.noise_analyse(Y, 10, (523, 259))
    small = ctx.noise_analyse(_content(8, (96, 72), (90, 70), 1, 22), 8, (90, 70))      # (the scratch, grown for the first, is reused)
    assert small.tobytes() == R.records(_content(8, (96, 72), (90, 70), 1, 22), 8, 90, 70).tobytes()
    assert ctx.noise_analyse(Y, 10, (523, 259)).tobytes() == first.tobytes()


def test_the_plan_of_measured_records(ctx):
    """kernel -> host plan == numpy reference -> numpy plan, on a noisy still clip and on one that pans as a whole"""
    import av1stream
    for sigma, pan, want in ((4.0, (0, 0), 6), (4.0, (5, 3), 0), (0, (0, 0), 0)):
        Y = R.sample(R.clip(192, 128, 8, sigma, 7, pan))
        k, q, s16 = av1stream.plan_denoise(ctx.noise_analyse(Y, 8, (192, 128)))
        assert (k, q.tolist(), s16) == R.plan(R.records(Y, 8, 192, 128)) and k == want, (sigma, pan, k)


def test_noise_analyse_refuses_bad_arguments(ctx, av1mi):
    Y = np.zeros((2, 72, 96), np.uint8)
    for bd, true in ((9, (90, 70)), (8, (97, 70)), (8, (90, 73)), (8, (88, 70)), (8, (90, 64)), (8, (0, 70))):
        with pytest.raises(av1mi.Av1miError):
            ctx.noise_analyse(Y, bd, true)
    with pytest.raises(av1mi.Av1miError):
        ctx.noise_analyse(np.zeros((2, 72, 90), np.uint8), 8, (90, 70))      # the buffer's width is not a multiple of 8
    with pytest.raises(av1mi.Av1miError):
        ctx.noise_analyse(np.zeros((0, 72, 96), np.uint8), 8, (90, 70))      # pairs 0
    d_y, d_out = ctx.to_device(np.zeros(2 * 72 * 96 + 16, np.uint8)), ctx.alloc(R.NOISE_DTYPE.itemsize + 16)
    try:
        for y_off, out_off, pairs in ((8, 0, 1), (0, 2, 1), (0, 0, 0), (0, 0, 32768), (0, 0, -1)):
            assert _raw(ctx, 8, Y, (90, 70), pairs, d_y.ptr + y_off, d_out.ptr + out_off) != 0, (y_off, out_off, pairs)
        assert _raw(ctx, 8, Y, (90, 70), 1, None, d_out.ptr) != 0 and _raw(ctx, 8, Y, (90, 70), 1, d_y.ptr, None) != 0
        ctx._chk(_raw(ctx, 8, Y, (90, 70), 1, d_y.ptr, d_out.ptr))      # and the call they all differ from by one argument is taken
        ctx.sync()
    finally:
        d_y.free()
        d_out.free()
