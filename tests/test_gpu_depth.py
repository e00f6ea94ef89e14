"""GPU tests of av1mi_depth_reduce (k_depth_reduce, depth_kernels.hip) against tests/depth_ref.py: bit exact in both modes, at the sizes where
the kernel's cells change shape — a row shorter than a cell, a whole and a short cell, frames back to back — on ramps, constants and noise;
nothing outside the output planes is written, the inputs are not written at all, and the argument rules hold."""
import ctypes as C

import numpy as np
import pytest

import depth_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = [(8, 8, 1), (24, 16, 1), (136, 72, 3)]      # width, height, frames


def _contents(w, h, frames):
    """name -> (Y, U, V) of a batch, uint16"""
    shapes = [(frames * h, w), (frames * h // 2, w // 2), (frames * h // 2, w // 2)]
    rng = np.random.default_rng(w * 1000 + h)
    ramp = []
    for k, (r, c) in enumerate(shapes):      # all 1024 codes, in an order that puts every code at both parities of x and y
        i = np.arange(r * c, dtype=np.int64).reshape(r, c)
        ramp.append(((i * 7 + (i // c) * 3 + k * 341) % 1024).astype(np.uint16))
    out = {"ramp": ramp, "zero": [np.zeros(s, np.uint16) for s in shapes], "max": [np.full(s, 1023, np.uint16) for s in shapes],
           "noise": [rng.integers(0, 1024, s, dtype=np.uint16) for s in shapes]}
    if w >= 136:
        assert all(len(np.unique(p)) == 1024 for p in ramp)
    return out


@pytest.mark.parametrize("w,h,frames", SIZES)
@pytest.mark.parametrize("mode", [R.ROUND, R.ORDERED])
def test_bit_exact_and_contained(ctx, w, h, frames, mode):
    for name, planes in _contents(w, h, frames).items():
        d_in = [ctx.to_device(a) for a in planes]
        d_out = [ctx.to_device(np.full(a.size + GUARD, 0xA5, np.uint8)) for a in planes]
        try:
            ctx.depth_reduce(mode, w, h, frames, d_in, d_out)
            ctx.sync()
            for p, a in enumerate(planes):
                got = d_out[p].download((a.size + GUARD,), np.uint8)
                assert np.array_equal(got[:a.size].reshape(a.shape), R.reduce_plane(a, p, mode)), "%s, plane %d" % (name, p)
                assert (got[a.size:] == 0xA5).all(), "%s, plane %d: the bytes behind the plane were written" % (name, p)
                assert np.array_equal(d_in[p].download(a.shape, np.uint16), a), "%s, plane %d: the input was written" % (name, p)
        finally:
            for b in d_in + d_out:
                b.free()


def test_the_parity_does_not_shift_between_frames(ctx):
    """three equal frames back to back reduce to three equal frames, each the single frame's reduction"""
    w, h = 136, 72
    one = _contents(w, h, 1)["noise"]
    planes = [np.concatenate([a] * 3) for a in one]
    d_in = [ctx.to_device(a) for a in planes]
    d_out = [ctx.alloc(a.size) for a in planes]
    try:
        ctx.depth_reduce(R.ORDERED, w, h, 3, d_in, d_out)
        ctx.sync()
        for p, a in enumerate(one):
            got = d_out[p].download(planes[p].shape, np.uint8)
            want = R.reduce_plane(a, p, R.ORDERED)
            for f in range(3):
                assert np.array_equal(got[f * a.shape[0]:(f + 1) * a.shape[0]], want), (p, f)
    finally:
        for b in d_in + d_out:
            b.free()


def test_arguments(ctx, av1mi):
    b = ctx.alloc(3 * 72 * 136 * 2 + 16)
    lib = ctx.lib
    lib.av1mi_depth_reduce.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2
    good = (C.c_void_p * 3)(b.ptr, b.ptr, b.ptr)

    def rc(mode=1, w=136, h=72, frames=3, src=good, dst=good):
        return lib.av1mi_depth_reduce(ctx.h, mode, w, h, frames, src, dst)
    try:
        for kw in (dict(mode=2), dict(mode=-1), dict(w=132), dict(h=68), dict(w=0), dict(h=4), dict(w=16392), dict(h=16392), dict(frames=0), dict(frames=-1),
                   dict(src=(C.c_void_p * 3)(b.ptr, None, b.ptr)), dict(dst=(C.c_void_p * 3)(b.ptr, b.ptr, None)), dict(src=None), dict(dst=None)):
            assert rc(**kw) == -1, kw      # AV1MI_E_INVAL
            assert lib.av1mi_last_error(ctx.h).startswith(b"av1mi_depth_reduce"), kw
    finally:
        ctx.sync()
        b.free()
