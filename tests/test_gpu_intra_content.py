"""GPU parity of the fused intra pipeline (k_intra_pipe<8|16|32>, k_intra_modes, intra_fast.hpp) on the hard content of
tests/intra_clips.py: all eight outputs of Context.intra_encode_arrays — modes, levels and reconstruction of the three planes — equal
the oracle's key-frame loop (oracle/av1o_pipeline.c av1o_intra_encode_frame) bit for bit, frame by frame.  What
tests/test_gpu_intra_pipe.py's blurred, limited-range clip never does happens here in many blocks: exact ties among the 13 candidates
with and without DC among them (the first minimum must win, over the U + V pair in chroma), upsampled edge values that the clip at 0
and at the top value changes, neighbours that chose a smooth mode (edge filter type 1), samples 0 and top at both depths, rows
further apart than the plane is wide, jobs that are a band of taller frames, tile counts that leave a partial workgroup.
tests/test_intra_clips.py shows (CPU, oracle alone) that the clips do these things and that the oracle's decisions are the ones a
second, independent restatement makes."""
import numpy as np
import pytest

import intra_clips as IC
import intra_ref

pytestmark = pytest.mark.gpu
KEYS = ("modes_y", "modes_uv", "lev_y", "lev_u", "lev_v", "rec_y", "rec_u", "rec_v")
Q = 60
DEPTHS = (8, 10)

_clips, _expected = {}, {}


def clip(name, w, h, bd):
    key = (name, w, h, bd)
    if key not in _clips:
        _clips[key] = IC.flat(w, h, bd, 128 << (bd - 8)) if name == "flat_mid" else IC.clip(name, w, h, bd)
    return _clips[key]


def expected(O, name, w, h, bd, bs, q, open_loop):
    """the oracle's result for one clip, computed once and shared by the tests that run the clip with the same settings; never changed"""
    key = (name, w, h, bd, bs, q, open_loop)
    if key not in _expected:
        Y, U, V = clip(name, w, h, bd)
        _expected[key] = O.intra_encode_frame(Y, U, V, bd, bs, q, open_loop=open_loop)
    return _expected[key]


def run_and_compare(ctx, O, names, w, h, bd, bs, q, open_loop=False, **geometry):
    Y, U, V = IC.stack([clip(n, w, h, bd) for n in names])
    got = ctx.intra_encode_arrays(Y, U, V, bd, bs, q, open_loop=open_loop, **geometry)
    for f, name in enumerate(names):
        exp = expected(O, name, w, h, bd, bs, q, open_loop)
        for k in KEYS:
            g, e = got[k][f], exp[k]
            assert g.shape == e.shape and (g == e).all(), (
                "clip %s, %dx%d, %d bit, block size %d, q %d, %s loop, %s: %s of frame %d (of %d) differs from the oracle at %s: got %s, expected %s"
                % (name, w, h, bd, bs, q, "open" if open_loop else "closed", geometry or "compact", k, f, len(names),
                   np.argwhere(g != e)[:4].tolist(), g[g != e][:4].tolist(), e[g != e][:4].tolist()))
    return got


@pytest.mark.parametrize("bs", [8, 16, 32])
@pytest.mark.parametrize("bd", DEPTHS)
def test_stacked_clips(ctx, O, bd, bs):
    """14 frames at 8 bits, 15 at 10, of the smallest size whose tiles are partial both ways: 84 / 90 tiles, a partial last workgroup"""
    w, h = IC.SIZES[bs]
    run_and_compare(ctx, O, IC.stacked_names(bd), w, h, bd, bs, Q)


@pytest.mark.parametrize("q", [255, 1])
@pytest.mark.parametrize("bs", [8, 32])
@pytest.mark.parametrize("bd", DEPTHS)
def test_checker_noise_and_binary_at_the_quantiser_ends(ctx, O, bd, bs, q):
    """q 255: the reconstruction is little more than the prediction, errors of one block's edges run through the whole tile;
    q 1: the levels are as large as they get"""
    w, h = IC.SIZES[bs]
    run_and_compare(ctx, O, ["checker2", "checker1", "noise", "binary"], w, h, bd, bs, q)


@pytest.mark.parametrize("bs", [8, 16])
@pytest.mark.parametrize("bd", DEPTHS)
def test_open_loop(ctx, O, bd, bs):
    """k_intra_modes decides on the source's own neighbours (global loads, guarded at the frame's first row and column), then
    k_intra_pipe<.., true> codes one prediction per block: the stack, one block per plane, and at 8x8 less than a tile down"""
    w, h = IC.SIZES[bs]
    try:
        run_and_compare(ctx, O, IC.stacked_names(bd), w, h, bd, bs, Q, open_loop=True)
        run_and_compare(ctx, O, ["noise", "binary", "checker1", "flat0", "flat_top"], bs, bs, bd, bs, Q, open_loop=True)
        if bs == 8:
            run_and_compare(ctx, O, ["noise", "binary", "checker2", "diag"], 72, 40, bd, bs, Q, open_loop=True)
    finally:
        O.set_intra_open_loop(False)


@pytest.mark.parametrize("bs", [8, 16, 32])
@pytest.mark.parametrize("bd", DEPTHS)
def test_one_block_per_plane(ctx, O, bd, bs):
    """nothing is available: DC predicts mid-grey, V, D45 and D67 one below it, H and D203 one above, the others something in
    between.  On mid-grey DC ties with PAETH at a SAD of 0 and must win; on black V wins its tie with D45 and D67, on white H
    wins its tie with D203 (the restatement of tests/intra_ref.py says so, and so does the oracle's loop)."""
    names = ["flat_mid", "flat0", "flat_top", "noise", "binary", "checker1", "diag"]
    got = run_and_compare(ctx, O, names, bs, bs, bd, bs, Q)
    for f, (name, mode) in enumerate((("flat_mid", 0), ("flat0", 1), ("flat_top", 2))):
        src = clip(name, bs, bs, bd)
        d = intra_ref.frame_decisions(O, src, src, bd, bs)      # (no neighbour is read: any plane does for the reconstruction)
        for kind, key in (("y", "modes_y"), ("uv", "modes_uv")):
            assert d[kind]["mode"].tolist() == [mode] and d[kind]["tied"].all(), (name, kind, d[kind])
            assert got[key][f].tolist() == [mode], "clip %s, %d bit, block size %d: %s = %s, the first minimum is %d" % (name, bd, bs, key, got[key][f].tolist(), mode)


@pytest.mark.parametrize("bd", DEPTHS)
def test_72x40(ctx, O, bd):
    """less than a tile down, chroma 36 wide: rows of 4x4 chroma blocks that end 4 samples into a 64-byte line"""
    run_and_compare(ctx, O, IC.stacked_names(bd), 72, 40, bd, 8, Q)


@pytest.mark.parametrize("bs", [8, 32])
@pytest.mark.parametrize("bd", DEPTHS)
def test_padded_rows_bands_and_mode_gaps(ctx, O, bd, bs):
    """stride_y = w + 24, stride_uv = w / 2 + 4, frame_rows = h + 64 (the job is the top band of taller frames, as the GOP session's
    32x32 band of a key frame is), modes_frame_stride = blocks + 5: the results equal the oracle's on the compact arrays, and every
    byte of row padding, of the rows and levels between the bands and of the gaps between the frames' modes still holds its sentinel"""
    w, h = IC.SIZES[bs]
    names = ["noise", "binary", "checker2"]
    nb = (w // bs) * (h // bs)
    got = run_and_compare(ctx, O, names, w, h, bd, bs, Q, stride_y=w + 24, stride_uv=w // 2 + 4, frame_rows=h + 64, modes_frame_stride=nb + 5)
    sample = 0xA5 if bd == 8 else 0xA5A5
    shapes = {}
    for p, rows, width, pad in (("y", h, w, 24), ("u", h // 2, w // 2, 4), ("v", h // 2, w // 2, 4)):
        shapes["rec_pad_" + p] = ((len(names), rows, pad), sample)
        shapes["rec_gap_" + p] = ((len(names), 64 if p == "y" else 32, width + pad), sample)
        shapes["lev_gap_" + p] = ((len(names), (64 if p == "y" else 32) * width), np.int16(0xA5A5 - 0x10000))
    shapes["modes_gap_y"] = shapes["modes_gap_uv"] = ((len(names), 5), 0xA5)
    for k, (shape, sentinel) in shapes.items():
        assert got[k].shape == shape, (k, got[k].shape, shape)
        assert (got[k] == sentinel).all(), ("%d bit, block size %d: the kernel wrote into %s at %s: %s"
                                            % (bd, bs, k, np.argwhere(got[k] != sentinel)[:4].tolist(), got[k][got[k] != sentinel][:4].tolist()))


def test_bad_geometry_is_refused(ctx, av1mi):
    w, h = 16, 16
    Y, U, V = IC.stack([clip("noise", w, h, 8)])
    nb = 4
    for geometry in (dict(stride_y=w - 4), dict(stride_uv=w // 2 - 4), dict(stride_y=w + 2), dict(stride_uv=w // 2 + 2), dict(stride_uv=0),
                     dict(frame_rows=h - 8), dict(frame_rows=h + 4), dict(modes_frame_stride=nb - 1)):
        with pytest.raises(av1mi.Av1miError):
            ctx.intra_encode_arrays(Y, U, V, 8, 8, Q, **geometry)
    got = ctx.intra_encode_arrays(Y, U, V, 8, 8, Q, stride_y=w + 4, stride_uv=w // 2 + 4, frame_rows=h + 8, modes_frame_stride=nb + 1)
    assert got["rec_y"].shape == (1, h, w) and got["modes_gap_uv"].shape == (1, 1)      # ... and a possible one is not
