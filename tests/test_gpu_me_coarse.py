"""The coarse motion search on the GPU (include/av1mi.h "motion search"; av1-go_amd/csrc/me_coarse_kernels.hip and k_me_int's centres):
quarter planes, centres and integer vectors equal the numpy reference tests/me_ref.py bit for bit; with coarse_range 0 the inter
pipeline is the one the oracle has always checked; and a wide-range P frame's residual tail is the oracle's arithmetic on the vector
the search chose."""
import ctypes as C

import numpy as np
import pytest

import me_ref as M
import synth

pytestmark = pytest.mark.gpu


def _check(ctx, src, ref, bd, rng_, cr, ref_alt=None, sel=None, what=""):
    got = ctx.me_search(src, ref, bd, rng_, cr, ref_alt, sel)
    for f in range(src.shape[0]):
        r = ref[f] if sel is None or sel[f][0] else ref_alt[f]
        exp = M.search(src[f], r, bd, rng_, cr)
        for k in ("q_src", "q_ref", "centres", "mvs"):
            if exp[k] is None:
                assert got[k] is None
                continue
            assert got[k][f].shape == exp[k].shape, (what, k, f)
            assert (got[k][f] == exp[k]).all(), (what, k, f, np.argwhere(got[k][f] != exp[k])[:4])
    return got


def _directions(Y):
    """frame pairs of a panning clip in four directions: forwards, backwards, and both with the picture upside down; [4, h, w] each"""
    a, b = Y[0], Y[1]
    return np.stack([b, a, b[::-1], a[::-1]]), np.stack([a, b, a[::-1], b[::-1]])


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("rc", [1, 8, 16])
def test_search_matches_reference_towards_every_edge(ctx, bd, rc):
    """200x136 (partial tiles both ways), four stacked frames panning towards each corner, at a speed inside the range (20 = (25, 15)
    per frame) and one far past it and past the picture's edges (scale 60 = (75, 45): the windows of the edge tiles lie mostly
    outside the plane)"""
    for scale in (20, 60):
        Y, _, _ = M.pan_clip(200, 136, 2, bd, scale)
        src, ref = _directions(Y)
        got = _check(ctx, src, ref, bd, 8, 4 * rc, what="scale %d" % scale)
        if scale == 20 and rc == 16:      # the tile in the middle follows each direction
            mid = got["centres"][:, 1 * 4 + 1]
            assert [tuple(np.sign(c)) for c in mid] == [(1, 1), (-1, -1), (1, -1), (-1, 1)], mid


@pytest.mark.parametrize("rng_", [0, 3, 15])
def test_search_ranges_other_than_8(ctx, rng_):
    Y, _, _ = M.pan_clip(136, 72, 2, 8, 12)
    src, ref = _directions(Y)
    _check(ctx, src, ref, 8, rng_, 32)


def test_search_1080_rows_10_bit(ctx):
    """1920x1080, 10 bit: 1080 = 16 tile rows + 56 rows; two stacked frames"""
    Y, _, _ = M.pan_clip(1920, 1080, 3, 10, 20)
    _check(ctx, Y[1:], Y[:2], 10, 8, 64)


def test_static_frame_centres_are_zero(ctx):
    """source == reference, with a flat area where every displacement ties: rank 0 wins"""
    Y, _, _ = M.pan_clip(200, 136, 2, 8, 3)
    Y = Y.copy()
    Y[:, 40:, :96] = 77
    got = _check(ctx, Y, Y, 8, 8, 64)
    assert (got["centres"] == 0).all() and (got["mvs"] == 0).all()


def test_reference_selected_per_frame(ctx):
    """d_ref_sel mixes restored and CDEF planes across stacked frames: each frame's quarter plane and window come from its own plane"""
    for bd in (8, 10):
        Y, _, _ = M.pan_clip(200, 136, 6, bd, 16)
        src, ref, alt = Y[1:6], Y[0:5], Y[0:5][:, ::-1].copy()
        sel = np.array([[1, 1, 1], [0, 1, 1], [1, 0, 0], [0, 0, 0], [0, 1, 0]], np.uint8)
        _check(ctx, src, ref, bd, 8, 32, alt, sel)


def test_without_coarse_range_the_pipeline_is_the_oracles(ctx, O):
    """coarse_range 0: the search returns zero centres and the vectors of the reference with them, and av1mi_inter_encode equals the
    oracle's inter encoder loop in every output, as it always has"""
    for bd, (w, h, q) in ((8, (200, 104, 60)), (10, (136, 72, 128))):
        Y, U, V = synth.frames(w, h, 3, bd, first=2)
        got = _check(ctx, Y[1:], Y[:2], bd, 8, 0)
        assert (got["centres"] == 0).all()
        enc = ctx.inter_encode_arrays((Y[1:], U[1:], V[1:]), (Y[:2], U[:2], V[:2]), bd, q, 8, coarse_range=0)
        for f in range(2):
            exp = O.inter_encode_frame((Y[1 + f], U[1 + f], V[1 + f]), (Y[f], U[f], V[f]), bd, q, 8)
            for k in ("mvs", "skip", "lev_y", "lev_u", "lev_v", "rec_y", "rec_u", "rec_v"):
                assert (enc[k][f] == exp[k]).all(), (k, bd, f)


def _quantize_inter(O, coef, dcq, acq):
    """the oracle's quantiser with the inter frames' AC rounding (av1o_pipeline.c AV1O_AC_ROUND_INTER = 51; oracle.txq_plane rounds as
    key frames do, so the tail is put together from the same parts it is made of)"""
    coef = np.ascontiguousarray(coef, np.int32)
    lev = np.zeros(coef.shape, np.int16)
    O.lib().av1o_quantize_r(coef.ctypes.data_as(C.c_void_p), coef.size, dcq, acq, 0, 51, lev.ctypes.data_as(C.c_void_p), None)
    return lev


@pytest.mark.parametrize("bd", [8, 10])
def test_wide_range_frame_tail_is_the_oracles_arithmetic(ctx, O, bd):
    """a P frame panning by (25, 15), coarse_range 64: the final vectors reach the pan; and for every fourth block the prediction is
    oracle.mc_block at the final vector, levels and reconstruction the oracle's transform, quantiser and inverse on that residual"""
    w, h, q = 200, 136, 100
    Y, U, V = M.pan_clip(w, h, 2, bd, 20)
    enc = ctx.inter_encode_arrays((Y[1:], U[1:], V[1:]), (Y[:1], U[:1], V[:1]), bd, q, 8, coarse_range=64)
    mv = enc["mvs"][0].reshape(h // 8, w // 8, 2)
    inner = mv[:14, :16]                   # the pan comes from the bottom right: blocks whose match lies inside the picture, in whole tiles
    assert (np.abs(inner[..., 0] - 200) <= 8).mean() > 0.9 and (np.abs(inner[..., 1] - 120) <= 8).mean() > 0.9
    # the integer stage under it is the reference's
    srch = ctx.me_search(Y[1:], Y[:1], bd, 8, 64)
    assert (np.abs(enc["mvs"][0].astype(int) - srch["mvs"][0]) <= 6).all()
    dcq, acq = O.dc_q(q, bd), O.ac_q(q, bd)
    planes = ((Y, 8, 1, "y"), (U, 4, 0, "u"))
    for blk in range(0, (h // 8) * (w // 8), 4):
        by, bx = divmod(blk, w // 8)
        mvx, mvy = (int(v) for v in enc["mvs"][0][blk])
        for P, bs, tx, name in planes:
            x, y = bx * bs, by * bs
            pred = O.mc_block(P[0], bd, x, y, bs, bs, mvx * 2 if bs == 8 else mvx, mvy * 2 if bs == 8 else mvy)
            resid = P[1][y:y + bs, x:x + bs].astype(np.int32) - pred.astype(np.int32)
            lev = _quantize_inter(O, O.fwd_txfm2d(resid.astype(np.int16), tx, 0, bd), dcq, acq)
            assert (enc["lev_" + name][0][blk] == lev).all(), (name, blk)
            rec = O.inv_txfm2d_add(O.dequantize(lev, dcq, acq, 0, bd), pred, tx, 0, bd)
            assert (enc["rec_" + name][0][y:y + bs, x:x + bs] == rec).all(), (name, blk)


def test_bad_coarse_range_is_refused(ctx, av1mi):
    Y, _, _ = M.pan_clip(64, 64, 2, 8, 1)
    for bad in (6, 68, -4):
        with pytest.raises(av1mi.Av1miError) as e:
            ctx.me_search(Y[1:], Y[:1], 8, 8, bad)
        assert "coarse_range" in str(e.value)
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.GopSession(ctx, 64, 64, 8, 100, 2, 1, coarse_range=bad)
        assert "coarse_range" in str(e.value)
