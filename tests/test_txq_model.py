"""The CPU oracle's forward transform, quantiser and dequantiser against tests/txq_model.py — a model that shares nothing with oracle/
or csrc/ — at the inputs where fixed-point arithmetic goes wrong: residuals that maximise a coefficient, the edges of the quantiser's
zero bin and of its int16 clamp, and every int16 level through the dequantiser's 24-bit wrap.  tests/test_gpu_txq_model.py holds the
kernels to the same model."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import txq_model as M

GOLD = os.path.join(os.path.dirname(__file__), "golden", "txq_model_observed.json")
SIZE_IDS = [M.size_name(ts) for ts in range(M.N_SIZES)]


# ---- the model itself -----------------------------------------------------------------------------------------------------------
def test_model_names_the_oracles_sizes_and_types(O):
    assert list(M.TX_W) == O.TX_W and list(M.TX_H) == O.TX_H
    assert [M.valid(ts, tt) for ts in range(19) for tt in range(16)] == [O.txfm_valid(ts, tt) for ts in range(19) for tt in range(16)]
    for tt, name in enumerate(O.TX_TYPE_NAMES):             # a name reads vertical_horizontal
        kinds = {"DCT": M.DCT, "ADST": M.ADST, "FLIPADST": M.FLIPADST, "IDTX": M.IDTX}
        if name == "IDTX":
            want = (M.IDTX, M.IDTX)
        elif name[:2] in ("V_", "H_"):
            want = (kinds[name[2:]], M.IDTX) if name[0] == "V" else (M.IDTX, kinds[name[2:]])
        else:
            want = tuple(kinds[p] for p in name.split("_"))
        assert M.TYPE_KINDS[tt] == want, name


def test_bases_are_scaled_orthonormal():
    for n in (4, 8, 16, 32, 64):
        for kind in (M.DCT, M.ADST, M.FLIPADST, M.IDTX):
            if (kind in (M.ADST, M.FLIPADST) and n > 16) or (kind == M.IDTX and n > 32):
                continue
            b = M.basis(kind, n)
            assert np.abs(b.T @ b - n / 2 * np.eye(n)).max() < 1e-9, (kind, n)
    assert (M.basis(M.FLIPADST, 8) == M.basis(M.ADST, 8)[::-1]).all()


def test_gain_table_is_the_derivation():
    for ts in range(M.N_SIZES):
        assert abs(M.GAIN[ts] - M.derived_gain(ts)) < 1e-12 * M.GAIN[ts], M.size_name(ts)
        s0, s1, s2 = M.design(ts)[0]     # the budget's design must describe a transform of that gain, or the budget is of another design
        assert abs(2.0 ** (s0 + s1 + s2) * (M.SQRT2 if M.is_rect2(ts) else 1) - M.GAIN[ts]) < 1e-12


@pytest.mark.parametrize("ts", range(M.N_SIZES), ids=SIZE_IDS)
def test_gain_table_against_the_normative_inverse(O, ts):
    """round(model(x)) through the oracle's inverse (spec 7.13.3, pinned to dav1d) on a flat 512 prediction at 10 bit gives x back
    within +-1, for band-limited x: every x where no side is 64, and where one is, x made of the 8 x 8 lowest frequencies (rounded to
    whole samples, which is all that leaves the band).  The gain belongs to the size, not to the type: every valid type is fed where no
    side is 64; where one is, the types with the identity across it are left out, because the identity hands the 64-point pass's own
    rounding on unaveraged (64x32 H_DCT: real-valued error of the inverse 1.21, so 2 in whole samples; the same gain passes with
    DCT_DCT)"""
    rng = np.random.default_rng(300 + ts)
    h, w = M.TX_H[ts], M.TX_W[ts]
    for tt in range(M.N_TYPES):
        if not M.valid(ts, tt) or (max(h, w) == 64 and M.IDTX in M.TYPE_KINDS[tt]):
            continue
        for rep in range(3):
            if max(h, w) == 64:
                low = np.zeros(M.coef_shape(ts))
                low[:8, :8] = rng.uniform(-1, 1, (8, 8))
                x = M.inv2d(low, ts, tt)
                x = np.rint(x * (200 / np.abs(x).max()))      # whole samples: band-limited up to their rounding
            else:
                x = rng.integers(-255, 256, (h, w)).astype(np.float64)
            coef = np.rint(M.fwd2d(x, ts, tt)).astype(np.int32)
            rec = O.inv_txfm2d_add(coef, np.full((h, w), 512, np.uint16), ts, tt, 10).astype(np.float64) - 512
            assert np.abs(rec - x).max() <= 1.0, (M.size_name(ts), O.TX_TYPE_NAMES[tt], rep)


def test_maximisers_maximise():
    """the generator's claim: no residual bounded by A gives |coef[u, v]| more than A * sum |Bc[:, u] (x) Br[:, v]| * gain, and the
    maximiser reaches it"""
    for ts, tt in ((1, 0), (8, 7), (4, 0), (13, 2)):
        inputs = dict(M.worst_case_inputs(ts, tt, 1023))
        bc, br = M.bases(ts, tt)
        for u, v in M.maximiser_positions(ts, tt):
            top = 1023 * M.GAIN[ts] * np.abs(np.outer(bc[:, u], br[:, v])).sum()
            assert abs(abs(M.fwd2d(inputs["max@%d,%d" % (u, v)], ts, tt)[u, v]) - top) < 1e-6 * top
            for x in inputs.values():
                assert abs(M.fwd2d(x, ts, tt)[u, v]) <= top * (1 + 1e-12)


# ---- forward transform ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(GOLD) as f:
        return {d["size"]: d for d in json.load(f)}


@pytest.mark.parametrize("ts", range(M.N_SIZES), ids=SIZE_IDS)
def test_oracle_forward_within_the_models_budget(O, golden, ts):
    """|oracle - model| <= budget(size, type, A) on the worst-case and random inputs of every valid type, A = 255 and 1023; the golden
    file's record of the largest error is what is measured now and lies under its budget"""
    for amp in (255, 1023):
        for tt in range(M.N_TYPES):
            if not M.valid(ts, tt):
                continue
            bud = M.budget(ts, tt, amp)
            for name, x in M.worst_case_inputs(ts, tt, amp) + M.random_inputs(ts, tt, amp):
                err = np.abs(O.fwd_txfm2d(x, ts, tt) - M.fwd2d(x, ts, tt)).max()
                assert err <= bud, (M.size_name(ts), O.TX_TYPE_NAMES[tt], amp, name, err, bud)
    rec = golden[M.size_name(ts)]
    assert rec == json.loads(json.dumps(M.observe_size(O.fwd_txfm2d, ts))), "tests/golden/txq_model_observed.json is stale: tools/gen_txq_observed.py"
    for amp in ("255", "1023"):
        assert rec["forward_error"][amp]["observed"] <= rec["forward_error"][amp]["budget"]


@pytest.mark.parametrize("ts", range(M.N_SIZES), ids=SIZE_IDS)
def test_coefficient_ranges_at_10_bit_worst_case(O, golden, ts):
    """the value ranges the kernels' comments claim (txq_model docstring, RANGE CLAIMS), measured on the inputs that maximise a
    coefficient at A = 1023; the oracle's own largest coefficient obeys the output claim as well"""
    for tt in range(M.N_TYPES):
        if not M.valid(ts, tt):
            continue
        for name, x in M.worst_case_inputs(ts, tt, 1023):
            for claim, v in M.range_claims(x, ts, tt).items():
                assert v < M.RANGE_LIMITS[claim], (M.size_name(ts), O.TX_TYPE_NAMES[tt], name, claim, v)
            assert np.abs(O.fwd_txfm2d(x, ts, tt)).max() < 1 << 18
    rec = golden[M.size_name(ts)]
    assert rec["coef_max_10bit"] < 1 << 18
    for claim, d in rec["claims"].items():
        assert d["limit"] == M.RANGE_LIMITS[claim] and d["measured"] < d["limit"], claim
    assert 3 * (1 << 17) < M.RANGE_LIMITS["sine4"]            # the inverse 4-point sine transform: operands clamped to bd + 8 = 18 bits


# ---- quantiser ------------------------------------------------------------------------------------------------------------------
def oracle_quantize_r(O, coef, dcq, acq, ls, ac_round):
    coef = np.ascontiguousarray(coef, np.int32)
    lev, dq = np.zeros(coef.shape, np.int16), np.zeros(coef.shape, np.int32)
    nz = O.lib().av1o_quantize_r(coef.ctypes.data_as(C.c_void_p), coef.size, dcq, acq, ls, ac_round, lev.ctypes.data_as(C.c_void_p),
                                 dq.ctypes.data_as(C.c_void_p))
    return lev, dq, nz


def quantiser_run(dcq, acq, ls, r, k):
    """the edge coefficients of step acq with rounding r, led by the k-th edge coefficient of the DC step"""
    dc_edges = M.quant_edge_coefs(dcq, ls, 64, seed=1)
    return np.concatenate([dc_edges[k % len(dc_edges):][:1], M.quant_edge_coefs(acq, ls, r, seed=2)])


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("ls", [0, 1, 2])
def test_oracle_quantiser_is_the_integer_model(O, bd, ls):
    """every q index: the oracle's levels and dequantised values equal the model's exactly, for AC rounding 64 (O.quantize), 58 and 51
    (av1o_quantize_r); and the levels obey the bound against the ideal quantiser"""
    for qi in range(256):
        dcq, acq = O.dc_q(qi, bd), O.ac_q(qi, bd)
        for r in (64, 58, 51):
            coef = quantiser_run(dcq, acq, ls, r, qi)
            lev, dq, nz = O.quantize(coef, dcq, acq, ls) if r == 64 else oracle_quantize_r(O, coef, dcq, acq, ls, r)
            elev, edq = M.quantize(coef, dcq, acq, ls, r)
            assert (lev == elev).all() and (dq == edq).all() and nz == np.count_nonzero(elev), (bd, ls, qi, r)
            if r == 64:
                assert all((a == b).all() for a, b in zip(oracle_quantize_r(O, coef, dcq, acq, ls, 64)[:2], (lev, dq)))
            if qi % 8 == 0 or qi == 255:
                M.check_quantiser_against_ideal(coef, lev, dcq, acq, ls, r)


# ---- dequantiser ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_oracle_dequantiser_is_spec_7_12_3_over_all_levels(O, bd):
    assert 32767 * 512 < 1 << 24 <= 32767 * 513
    for q in M.dequant_steps(O, bd):
        for ls in (0, 1, 2):
            want = M.dequantize_all_levels(q, ls, bd)
            assert (O.dequantize(M.ALL_LEVELS, q, q, ls, bd) == want).all(), (bd, q, ls)
    # the wrap and the clamp are inside what was compared
    assert M.dequantize_one(32767, 513, 0, bd) == min(32767 * 513 - (1 << 24), (1 << (7 + bd)) - 1) and M.dequantize_one(-32768, 512, 0, bd) == 0
    assert M.dequantize_one(-32767, 512, 0, bd) == -(1 << (7 + bd)) and M.dequantize_one(32767, 100, 1, bd) == (1 << (7 + bd)) - 1
    assert (O.dequantize(np.array([-3, 5, -32768], np.int16), 9, 700, 0, bd) ==
            [M.dequantize_one(-3, 9, 0, bd), M.dequantize_one(5, 700, 0, bd), M.dequantize_one(-32768, 700, 0, bd)]).all()   # DC takes dc_q
