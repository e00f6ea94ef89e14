"""The forward-transform, quantiser and dequantiser kernels against tests/txq_model.py (a model that shares nothing with oracle/ or
csrc/) at worst-case input: residuals that maximise a coefficient, the quantiser's zero-bin and clamp edges, all 65536 levels through
the dequantiser — through the stand-alone kernels (grid and list form) and through the fused inter and intra pipelines."""
import numpy as np
import pytest

import txq_model as M

pytestmark = pytest.mark.gpu
SIZE_IDS = [M.size_name(ts) for ts in range(M.N_SIZES)]


# ---- forward transform, grid form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", range(M.N_SIZES), ids=SIZE_IDS)
def test_fwd_grid_worst_case_inputs(ctx, O, ts):
    """one launch per amplitude: every valid type's worst-case inputs as the blocks of a grid, 5 blocks per row, an odd number of blocks
    (never a multiple of the 4 .. 64 blocks of a workgroup), the types per block: bit for bit the oracle's, and within the model's
    budget"""
    h, w = M.TX_H[ts], M.TX_W[ts]
    ch, cw = M.coef_shape(ts)
    for amp in (255, 1023):
        blocks = [(tt, x) for tt in range(M.N_TYPES) if M.valid(ts, tt) for _, x in M.worst_case_inputs(ts, tt, amp)]
        blocks += [(0, x) for _, x in M.random_inputs(ts, 0, amp, 1 + len(blocks) % 2)]
        nb, nbx = len(blocks), 5
        assert nb % 2 == 1
        res = np.zeros(((nb + nbx - 1) // nbx * h, nbx * w), np.int16)
        for b, (_, x) in enumerate(blocks):
            by, bx = divmod(b, nbx)
            res[by * h:by * h + h, bx * w:bx * w + w] = x
        tts = np.array([tt for tt, _ in blocks], np.uint8)
        d_res, d_types, d_coef = ctx.to_device(res), ctx.to_device(tts), ctx.alloc(nb * ch * cw * 4)
        ctx.fwd_txfm_grid(ts, d_res, res.shape[1], d_coef, nbx, nb, d_types)
        got = d_coef.download((nb, ch, cw), np.int32)
        for d in (d_res, d_types, d_coef):
            d.free()
        for b, (tt, x) in enumerate(blocks):
            assert (got[b] == O.fwd_txfm2d(x, ts, tt)).all(), (M.size_name(ts), O.TX_TYPE_NAMES[tt], amp, b)
            err = np.abs(got[b] - M.fwd2d(x, ts, tt)).max()
            assert err <= M.budget(ts, tt, amp), (M.size_name(ts), O.TX_TYPE_NAMES[tt], amp, b, err)


# ---- forward transform, list form -----------------------------------------------------------------------------------------------
SENTINEL = 0x5A5A5A5A


@pytest.mark.parametrize("ts,types", [(1, (0, 3, 9, 5, 12)), (8, (1, 6, 10, 15, 8))], ids=["8x8", "16x8"])
def test_fwd_list_scattered_blocks(ctx, O, av1mi, ts, types):
    """av1mi_fwd_txfm_list: blocks at scattered places of a 96 x 64 residual plane, coefficient slots reversed with a gap, the types from
    the list; the slots the list does not name keep their sentinel; zero blocks is a no-op"""
    rng = np.random.default_rng(21 + ts)
    h, w = M.TX_H[ts], M.TX_W[ts]
    n = h * w
    H, W = 64, 96
    res = rng.integers(-1023, 1024, (H, W)).astype(np.int16)
    pos = [(8, 0), (40, 8), (80, 56), (0, 56), (16, 24)]
    slots = len(pos) + 2
    lst = np.zeros(len(pos), av1mi.TXB_DTYPE)
    exp = np.full((slots, h, w), SENTINEL, np.int32)
    for i, ((x, y), tt) in enumerate(zip(pos, types)):
        assert M.valid(ts, tt) and x + w <= W and y + h <= H
        res[y:y + h, x:x + w] = M.worst_case_inputs(ts, tt, 1023)[13 + i][1]       # the maximisers
        slot = len(pos) + 1 - i   # reversed, with a gap: slots 0 and 1 belong to nobody
        lst[i] = (slot * n, x, y, tt, 0)
        exp[slot] = O.fwd_txfm2d(res[y:y + h, x:x + w], ts, tt)
        assert np.abs(exp[slot] - M.fwd2d(res[y:y + h, x:x + w], ts, tt)).max() <= M.budget(ts, tt, 1023)
    d_res, d_list = ctx.to_device(res), ctx.to_device(lst)
    d_coef = ctx.to_device(np.full((slots, h, w), SENTINEL, np.int32))
    ctx.fwd_txfm_list(ts, d_res, W, d_coef, d_list, 0)
    assert (d_coef.download(exp.shape, np.int32) == SENTINEL).all()
    ctx.fwd_txfm_list(ts, d_res, W, d_coef, d_list, len(pos))
    got = d_coef.download(exp.shape, np.int32)
    assert (got[:2] == SENTINEL).all() and (got == exp).all()
    assert (d_res.download(res.shape, np.int16) == res).all()
    for d in (d_res, d_list, d_coef):
        d.free()


def test_fwd_list_refuses_what_the_host_can_see(ctx, av1mi):
    """a stride that is no multiple of 4, a size that does not exist, a missing list; and a (size, type) pair that does not exist where
    the type is an argument (the uniform type of the grid form: the types of a list live in device memory, which the launcher does
    not read back)"""
    d = ctx.alloc(4096)
    for bad in (lambda: ctx.fwd_txfm_list(1, d, 6, d, d, 1), lambda: ctx.fwd_txfm_list(19, d, 8, d, d, 1),
                lambda: ctx.fwd_txfm_list(1, d, 0, d, d, 1), lambda: ctx.fwd_txfm_list(1, d, 8, d, d, -1),
                lambda: ctx.fwd_txfm_grid(4, d, 64, d, 1, 1, None, 1), lambda: ctx.fwd_txfm_grid(3, d, 32, d, 1, 1, None, 3),
                lambda: ctx.fwd_txfm_grid(1, d, 6, d, 1, 1)):
        with pytest.raises(av1mi.Av1miError):
            bad()
    d.free()


# ---- quantiser ------------------------------------------------------------------------------------------------------------------
def quant_block_run(dcq, acq, ls, per, n=1024):
    """n coefficients in blocks of `per`: the edge coefficients of the AC step in turn, and at the head of every block those of the DC
    step in turn"""
    ac, dc = M.quant_edge_coefs(acq, ls, 64, seed=2), M.quant_edge_coefs(dcq, ls, 64, seed=1)
    run = np.resize(ac, n)
    run[::per] = np.resize(dc, n // per)
    return run.astype(np.int32)


def run_quantize(ctx, coef, per, dcq, acq, ls):
    d_coef, d_lv, d_dq = ctx.to_device(coef), ctx.alloc(coef.size * 2), ctx.alloc(coef.size * 4)
    ctx.quantize(d_coef, d_lv, d_dq, coef.size, per, dcq, acq, ls)
    out = d_lv.download(coef.shape, np.int16), d_dq.download(coef.shape, np.int32)
    for d in (d_coef, d_lv, d_dq):
        d.free()
    return out


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ls", [0, 1, 2])
def test_quantize_edges_equal_the_integer_model(ctx, O, bd, ls):
    """k_quantize on 1024 coefficients (one workgroup) per step of a spread and per block length 16 (every fourth lane starts a block)
    and 1024: levels and dequantised values are the integer model's"""
    for qi in (0, 1, 60, 128, 200, 255):
        dcq, acq = O.dc_q(qi, bd), O.ac_q(qi, bd)
        for per in (16, 1024):
            coef = quant_block_run(dcq, acq, ls, per)
            lv, dq = run_quantize(ctx, coef, per, dcq, acq, ls)
            elv, edq = M.quantize(coef, dcq, acq, ls, 64, per)
            assert (lv == elv).all() and (dq == edq).all(), (bd, ls, qi, per)


@pytest.mark.parametrize("per", [16, 1024])
def test_quantize_grid_stride_loop_turns(ctx, O, per):
    """the launcher caps the grid at 2048 workgroups of 256 lanes of 4 coefficients: the smallest run above that (one more block of
    1024) makes the first lanes go round again"""
    dcq, acq, ls = O.dc_q(128, 10), O.ac_q(128, 10), 1
    base = quant_block_run(dcq, acq, ls, per)
    reps = 2048 * 256 * 4 // 1024 + 1
    lv, dq = run_quantize(ctx, np.tile(base, reps), per, dcq, acq, ls)
    elv, edq = M.quantize(base, dcq, acq, ls, 64, per)
    assert (lv.reshape(reps, -1) == elv).all() and (dq.reshape(reps, -1) == edq).all()


# ---- dequantiser ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_dequantize_all_levels_equal_spec_7_12_3(ctx, O, bd):
    """all 65536 int16 levels in one launch per (step, log scale): through the 24-bit wrap (step 513 and above), the bd + 8 bit clamp
    and level -32768"""
    d_lv, d_dq = ctx.to_device(M.ALL_LEVELS), ctx.alloc(65536 * 4)
    for q in M.dequant_steps(O, bd):
        for ls in (0, 1, 2):
            ctx.dequantize(d_lv, d_dq, 65536, 1024, q, q, ls, bd)
            assert (d_dq.download((65536,), np.int32) == M.dequantize_all_levels(q, ls, bd)).all(), (bd, q, ls)
    ctx.dequantize(d_lv, d_dq, 64, 16, 9, 700, 0, bd)                       # the head of every block takes dc_q
    assert (d_dq.download((64,), np.int32) == M.dequantize(M.ALL_LEVELS[:64], 9, 700, 0, bd, 16)).all()
    d_lv.free()
    d_dq.free()


# ---- the same arithmetic inside the fused kernels -------------------------------------------------------------------------------
QINDEX = 40


def expected_block(O, src, pred, ts, dcq, acq, ac_round, bd):
    """levels = the model's quantiser on the oracle's forward transform of (source - prediction), which must itself lie inside the
    range the model's bound covers (|c| + rnd <= 32767); reconstruction = the dav1d-pinned inverse of the model's dequantised levels"""
    coef = O.fwd_txfm2d((src.astype(np.int32) - pred.astype(np.int32)).astype(np.int16), ts, 0, bd)
    assert np.abs(coef).max() + max(M.quant_round(dcq, 0, 64), M.quant_round(acq, 0, ac_round)) <= 32767
    lev, _ = M.quantize(coef, dcq, acq, 0, ac_round)
    rec = O.inv_txfm2d_add(M.dequantize(lev, dcq, acq, 0, bd).astype(np.int32), pred, ts, 0, bd)
    return lev, rec


@pytest.mark.parametrize("bd,amp_y", [(8, 127), (10, 500)])
def test_inter_pipe_tail_on_worst_case_residuals(ctx, O, bd, amp_y):
    """a 72 x 40 P frame, search range 0, on a constant reference: whichever vector wins, the prediction is the constant, so the residuals
    are the generator's 8 x 8 (luma) and 4 x 4 (chroma) worst cases, tiled.  Levels and reconstruction of the fused kernel are the
    model's quantiser (AC rounding 51) and the pinned inverse.  amp_y: the largest the constant leaves room for with 64 * amp + rnd
    inside the int16 clamp (expected_block asserts it)"""
    w, h, base = 72, 40, 1 << (bd - 1)
    dt = np.uint8 if bd == 8 else np.uint16
    dcq, acq = O.dc_q(QINDEX, bd), O.ac_q(QINDEX, bd)
    pats = {"y": [x for _, x in M.worst_case_inputs(1, 0, amp_y)], "u": [x for _, x in M.worst_case_inputs(0, 0, base - 1)]}
    pats["v"] = [-x for x in pats["u"][::-1]]
    src, ref = {}, {}
    for p, bs in (("y", 8), ("u", 4), ("v", 4)):
        pw, ph = (w, h) if p == "y" else (w // 2, h // 2)
        ref[p] = np.full((1, ph, pw), base, dt)
        s = np.zeros((ph, pw), np.int32)
        for b in range((ph // bs) * (pw // bs)):
            by, bx = divmod(b, pw // bs)
            s[by * bs:by * bs + bs, bx * bs:bx * bs + bs] = base + pats[p][b % len(pats[p])]
        assert s.min() >= 0 and s.max() < 1 << bd
        src[p] = s.astype(dt)[None]
    got = ctx.inter_encode_arrays((src["y"], src["u"], src["v"]), (ref["y"], ref["u"], ref["v"]), bd, QINDEX, search_range=0)
    for p, bs, ts in (("y", 8, 1), ("u", 4, 0), ("v", 4, 0)):
        pw = w if p == "y" else w // 2
        for b in range(got["lev_" + p].shape[1]):
            by, bx = divmod(b, pw // bs)
            sl = (slice(by * bs, by * bs + bs), slice(bx * bs, bx * bs + bs))
            lev, rec = expected_block(O, src[p][0][sl], ref[p][0][sl], ts, dcq, acq, 51, bd)
            assert (got["lev_" + p][0][b] == lev).all(), (p, bd, b)
            assert (got["rec_" + p][0][sl] == rec).all(), (p, bd, b)
    assert np.count_nonzero(got["lev_y"]) > 500


@pytest.mark.parametrize("bd,amp_y,amp_c", [(8, 127, 127), (10, 250, 500)])
def test_intra_pipe_tail_on_worst_case_residuals(ctx, O, bd, amp_y, amp_c):
    """k_intra_pipe on frames of one 16 x 16 block (8 x 8 chroma), one frame per worst-case pattern around the base value 2^(bd-1).
    With nothing to predict from, the prediction is known: the base value for DC, base - 1 for V, base + 1 for H (spec 7.11.2); for
    the other modes the kernel may choose it is the dav1d-pinned predictor's.  Chroma carries a pattern in U and its negative in V,
    which ties every mode's cost with DC's, so DC (first) wins and the transform stays DCT_DCT.  Levels: the model's quantiser (AC
    rounding 64) on the forward transform of source - prediction; reconstruction: the pinned inverse"""
    base = 1 << (bd - 1)
    dt = np.uint8 if bd == 8 else np.uint16
    dcq, acq = O.dc_q(QINDEX, bd), O.ac_q(QINDEX, bd)
    py = [x for _, x in M.worst_case_inputs(2, 0, amp_y)]
    pc = [x for _, x in M.worst_case_inputs(1, 0, amp_c)]
    Y = np.stack([base + x for x in py]).astype(dt)
    U = np.stack([base + x for x in pc]).astype(dt)
    V = np.stack([base - x for x in pc]).astype(dt)
    got = ctx.intra_encode_arrays(Y, U, V, bd, 16, QINDEX)
    assert (got["modes_uv"] == 0).all()
    known = {0: base, 1: base - 1, 2: base + 1}
    for f in range(len(py)):
        mode = int(got["modes_y"][f, 0])
        pred = O.intra_predict(np.zeros((16, 16), dt), 0, 0, 16, 16, mode, 0, bd, 0, 0, 0, 0).astype(dt)
        if mode in known:
            assert (pred == known[mode]).all()
        lev, rec = expected_block(O, Y[f], pred, 2, dcq, acq, 64, bd)
        assert (got["lev_y"][f, 0] == lev).all() and (got["rec_y"][f] == rec).all(), ("y", bd, f, mode)
        for name, P in (("u", U), ("v", V)):
            lev, rec = expected_block(O, P[f], np.full((8, 8), base, dt), 1, dcq, acq, 64, bd)
            assert (got["lev_" + name][f, 0] == lev).all() and (got["rec_" + name][f] == rec).all(), (name, bd, f)
    assert 0 in got["modes_y"] and np.count_nonzero(got["lev_y"]) > 100
