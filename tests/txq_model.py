"""An exact model of the encoder half of the block arithmetic: forward 2-D transform, quantiser, dequantiser.

Plain numpy and Python integers.  Nothing here is read from oracle/ or csrc/: the transform is a float64 product of basis matrices
written from their closed forms, the quantiser is the mathematical statement in Python ints, the dequantiser is spec 7.12.3.  The
tests compare the oracle AND the kernels with this file, so that a misreading shared by kernel and oracle shows.

FORWARD TRANSFORM
-----------------
coef = GAIN[size] * Bc^T x Br   (columns first, then rows; a 64-point direction keeps its 32 low frequencies)

with the 1-D bases in the scaling of the spec's inverse processes (7.13.2), B[n, k] = sample n of basis function k:
  DCT-II      cos((2n+1) k pi / 2N), column k = 0 scaled by 1/sqrt(2)
  ADST, N=4   (2 sqrt(2) / 3) sin((n+1)(2k+1) pi / 9)               (the 4-point sine transform of 7.13.2.6, a DST-VII)
  ADST, N=8/16  sin((2n+1)(2k+1) pi / 4N)
  FLIPADST    the ADST on the mirrored input: B[N-1-n, k]
  identity    f(N) * I with f = sqrt(2), 2, 2 sqrt(2), 4 for N = 4, 8, 16, 32
Every one of them is sqrt(N/2) times an orthonormal matrix: B^T B = (N/2) I.

The gain.  It is not read from any forward transform: it is the one number for which the NORMATIVE inverse (spec 7.13.3, pinned to
dav1d in tests/test_av1_blocks.py) gives the residual back.  7.13.3 computes, rounding apart,
    res = 2^-(rs + 4) * r * Bc coef Br^T,     rs = Transform_Row_Shift[size],  r = 1/sqrt(2) when one side is twice the other, else 1
(row pass, shift rs, column pass, shift 4).  With coef = g Bc^T x Br and B B^T = (N/2) I this is
    res = 2^-(rs + 4) * r * g * (H/2)(W/2) * x,
so res = x  <=>  g = 2^(rs + 4) * 4 / (r W H).  (For a 64-point direction B B^T is (N/2) times the projection on the kept band, so
the same g reconstructs every x inside that band, and only those.)  The table, with rs from the spec's Transform_Row_Shift and beside
it the same gain against orthonormal bases, G = g sqrt(W H) / 2 — the familiar 8, 4, 2:

    size   rs  r         g = GAIN       G        size   rs  r         g = GAIN       G
    4x4    0   1         4              8        4x8    0   1/sqrt2   2 sqrt2        8
    8x8    1   1         2              8        8x4    0   1/sqrt2   2 sqrt2        8
    16x16  2   1         1              8        8x16   1   1/sqrt2   sqrt2          8
    32x32  2   1         1/4            4        16x8   1   1/sqrt2   sqrt2          8
    64x64  2   1         1/16           2        16x32  1   1/sqrt2   sqrt2 / 4      4
    4x16   1   1         2              8        32x16  1   1/sqrt2   sqrt2 / 4      4
    16x4   1   1         2              8        32x64  1   1/sqrt2   sqrt2 / 16     2
    8x32   2   1         1              8        64x32  1   1/sqrt2   sqrt2 / 16     2
    32x8   2   1         1              8
    16x64  2   1         1/4            4
    64x16  2   1         1/4            4

tests/test_txq_model.py::test_gain_table_against_the_normative_inverse checks every entry against the inverse.

ERROR BUDGET of a fixed-point forward transform against this model (budget(), in units of the output)
------------------------------------------------------------------------------------------------------
The fixed-point design (libaom's fwd_txfm2d_c, public): x << s0, column pass with a cos table of bc bits, rounding shift s1, row pass
with br bits, rounding shift s2, and for r != 1 a multiplication by 5793 / 4096.  A 1-D pass of length N is a flow graph of add/sub
stages and rotation stages; a rotation computes (w0 a + w1 b + half) >> b with w = round(cos * 2^b).  Let m be the largest number of
rotation (= rounding) stages on a path: DCT log2 N - 1; ADST 1, 3, 4 for N = 4, 8, 16; identity 1 for N = 4, 16 (one multiplication by
5793 or 11586 over 4096) and 0 for N = 8, 32.  Between two rotation stages of a path lies one add/sub stage.
  rounding:  a rotation stage adds at most 0.5 to every value.  Through each later (add/sub, rotation) pair an error e grows to at most
             2 sqrt(2) e in the largest-element norm (add/sub: 2, rotation: |c| + |s| <= sqrt 2) and to sqrt(2) e in the Euclidean norm
             (rotation: 1), where it starts as 0.5 sqrt(N).  Either bound holds, so
                 R(N, m) = 0.5 * sum_{j < m} min((2 sqrt 2)^j, sqrt(N) sqrt(2)^j)
  table:     |w / 2^b - cos| <= 2^-(b+1), so a rotation stage is off by a 2 x 2 matrix of norm <= 2^-b.  The stages before it have
             Euclidean gain g1, those after it g2, with g1 g2 <= sqrt(N) (the add/sub stages of a path, sqrt 2 each, at most
             log2 N of them), and the input has Euclidean norm <= sqrt(N) X for |x| <= X: each stage contributes at most
             2^-b N X, together  m 2^-b N X  — "relative error of the table, times the multiplying stages, times the largest
             intermediate N X".  The 4-point sine table and the identity factors (|5793/4096 - sqrt 2| < 2^-13) are inside it.
  2-D:       E1 = R(H, mc) + mc 2^-bc H X0,  X0 = A 2^s0                                 after the column pass
             E2 = E1 / 2^-s1 + 0.5 [s1 < 0]                                             after the first rounding shift
             E3 = ar E2 + R(W, mr) + mr 2^-br W (ac X0 / 2^-s1 + 0.5 + E2)              the row pass multiplies what comes in by at most
                                                                                        ar = max_k sum_n |Br[n, k]| (ac likewise)
             E4 = E3 / 2^-s2 + 0.5 [s2 < 0]
             E5 = E4 * 5793/4096 + 0.5 + 2^-13 (|coef|max + E4)                         only for r != 1; 5793/4096 against sqrt 2
It is a worst-case bound, so what is observed lies well below it (tests/golden/txq_model_observed.json keeps both).  The s0/s1/s2
and bc/br of DESIGN below enter the budget only; the model's values never see them.  That 2^(s0+s1+s2) / r equals GAIN[size] is what
the comparison checks.

RANGE CLAIMS of the kernels, recomputed from model intermediates (range_claims()) for an input x
-------------------------------------------------------------------------------------------------
  final      |coef| < 2^18                                  ("|v| < 2^18" at the rectangular multiply is a claim about the output)
  pre_sqrt2  r != 1: the value multiplied by 5793 is coef * 4096 / 5793: < 2^18 as claimed, and as a 24-bit operand < 2^23
  sine4      4-point sine transform: its operands are the pass input x_i and x0 + x1 - x3: 3 max|x_i| < 2^23, for the column pass
             (x << s0) and the row pass (C = 2^(s0+s1) Bc^T x, the model's column-pass output after the first shift)
  identity   identity of length 4 / 16: its operand is the pass input (as above) < 2^23
  mad24      the two-multiply-add: its operands are the intermediates of a DCT / 8-, 16-point ADST pass.  Every one is a combination of
             the pass input v with a coefficient vector of Euclidean norm <= sqrt(N) (above), so |operand| <= sqrt(N) |v|_2 < 2^23
  mad32      the same helper accumulates w0 a + w1 b + half in 32 bits: |w0 a + w1 b| <= 2^b sqrt(a^2 + b^2) <= 2^b sqrt(2) sqrt(N) |v|_2,
             which must stay < 2^31 (the kernels' comments do not name it; a 64-bit accumulate in the oracle would hide a wrap)
The inverse 4-point sine transform takes operands clamped to bd + 8 bits: 3 * 2^17 < 2^23 without measuring anything.

QUANTISER (quantize(), Python ints), r = rounding in 1/128 of the step (64 for DC, the caller's for AC), ls = log scale 0..2
-----------------------------------------------------------------------------------------------------------------------
    rnd   = round2((r q) >> 7, ls)
    level = sign(c) min(32767, floor(min(|c| + rnd, 32767) floor(65536 / q) / 2^(16 - ls)))   when |c| 2^(1 + ls) >= q, else 0
    dq    = sign(c) floor(|level| q / 2^ls)            (the encoder's own reconstruction; no 24-bit wrap, no clamp)
Ideal real-valued quantiser L* = (|c| + rnd) 2^ls / q.  While |c| + rnd <= 32767 and outside the zero bin,
    0 <= L* - |level| <= 1 + L* q / 65536.
Proof: with a = |c| + rnd, floor(65536 / q) > 65536 / q - 1 gives a floor(65536/q) / 2^(16-ls) > L* - a 2^ls / 65536 = L* - L* q / 65536,
and floor(65536 / q) <= 65536 / q gives <= L*; the final floor takes away less than 1 more.  (The outer min is idle there:
a <= 32767 and q >= 4 >= 2^ls give L* <= 32767.)
Above |c| + rnd = 32767 the level is that of |c| + rnd = 32767: the int16 clamp of the coefficient, a choice of the design.

DEQUANTISER (dequantize(), spec 7.12.3): dq = ((|level| q) & 0xFFFFFF) >> ls, the sign restored, clipped to [-2^(7+bd), 2^(7+bd) - 1].
"""
import functools
import math

import numpy as np

TX_W = (4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64)
TX_H = (4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16)
N_SIZES, N_TYPES = 19, 16
DCT, ADST, FLIPADST, IDTX = 0, 1, 2, 3
# the 16 regular types as (vertical = column kind, horizontal = row kind), in the order of the spec's tx_type values:
# DCT_DCT ADST_DCT DCT_ADST ADST_ADST FLIPADST_DCT DCT_FLIPADST FLIPADST_FLIPADST ADST_FLIPADST FLIPADST_ADST IDTX V_DCT H_DCT V_ADST
# H_ADST V_FLIPADST H_FLIPADST (a name reads vertical_horizontal; V_x: x vertically, identity horizontally)
TYPE_KINDS = ((DCT, DCT), (ADST, DCT), (DCT, ADST), (ADST, ADST), (FLIPADST, DCT), (DCT, FLIPADST), (FLIPADST, FLIPADST),
              (ADST, FLIPADST), (FLIPADST, ADST), (IDTX, IDTX), (DCT, IDTX), (IDTX, DCT), (ADST, IDTX), (IDTX, ADST),
              (FLIPADST, IDTX), (IDTX, FLIPADST))
SQRT2 = math.sqrt(2.0)
R2 = SQRT2  # shorthand in the table below
# spec Transform_Row_Shift, in the order of TX_W / TX_H
ROW_SHIFT = (0, 1, 2, 2, 2, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2)
# the table of the docstring, written out; test_gain_table_is_the_derivation recomputes it from ROW_SHIFT
GAIN = (4.0, 2.0, 1.0, 1 / 4, 1 / 16, 2 * R2, 2 * R2, R2, R2, R2 / 4, R2 / 4, R2 / 16, R2 / 16, 2.0, 2.0, 1.0, 1.0, 1 / 4, 1 / 4)


def is_rect2(ts):
    return TX_W[ts] == 2 * TX_H[ts] or TX_H[ts] == 2 * TX_W[ts]


def derived_gain(ts):
    """g = 2^(rs + 4) * 4 / (r W H) of the docstring"""
    return 2.0 ** (ROW_SHIFT[ts] + 4) * 4 * (SQRT2 if is_rect2(ts) else 1.0) / (TX_W[ts] * TX_H[ts])


def valid(ts, tt):
    """ADST exists for lengths 4, 8, 16, the identity up to 32 (spec 5.11.47 / get_tx_set)"""
    ck, rk = TYPE_KINDS[tt]
    for kind, n in ((ck, TX_H[ts]), (rk, TX_W[ts])):
        if kind in (ADST, FLIPADST) and n > 16:
            return False
        if kind == IDTX and n > 32:
            return False
    return True


def valid_pairs():
    return [(ts, tt) for ts in range(N_SIZES) for tt in range(N_TYPES) if valid(ts, tt)]


def coef_shape(ts):
    return min(TX_H[ts], 32), min(TX_W[ts], 32)


@functools.lru_cache(maxsize=None)
def basis(kind, n):
    """B[sample, frequency], all n frequencies, in the scaling of the docstring"""
    s, k = np.arange(n)[:, None], np.arange(n)[None, :]
    if kind == DCT:
        b = np.cos((2 * s + 1) * k * np.pi / (2 * n))
        b[:, 0] = 1 / SQRT2
    elif kind in (ADST, FLIPADST):
        if n == 4:
            b = np.sin((s + 1) * (2 * k + 1) * np.pi / 9) * 2 * SQRT2 / 3
        else:
            b = np.sin((2 * s + 1) * (2 * k + 1) * np.pi / (4 * n))
        if kind == FLIPADST:
            b = b[::-1]
    else:
        b = np.eye(n) * {4: SQRT2, 8: 2.0, 16: 2 * SQRT2, 32: 4.0}[n]
    b = np.ascontiguousarray(b, np.float64)
    b.setflags(write=False)
    return b


def bases(ts, tt):
    """(Bc [H, min(H, 32)], Br [W, min(W, 32)]): the kept frequencies only"""
    ck, rk = TYPE_KINDS[tt]
    ch, cw = coef_shape(ts)
    return basis(ck, TX_H[ts])[:, :ch], basis(rk, TX_W[ts])[:, :cw]


def fwd2d(x, ts, tt):
    """float64 coefficients [min(H, 32), min(W, 32)] of the residual x [H, W]"""
    bc, br = bases(ts, tt)
    return GAIN[ts] * (bc.T @ np.asarray(x, np.float64) @ br)


def inv2d(coef, ts, tt):
    """the real-valued inverse of fwd2d on its kept band: x = (4 / (GAIN W H)) Bc coef Br^T"""
    bc, br = bases(ts, tt)
    return 4.0 / (GAIN[ts] * TX_W[ts] * TX_H[ts]) * (bc @ np.asarray(coef, np.float64) @ br.T)


# ---- the fixed-point design, for the budget and the range claims only -----------------------------------------------------------
# (s0, s1, s2) per size and the cos-table bits (column pass, row pass): libaom av1_fwd_txfm_shift_ls, av1_fwd_cos_bit_col / _row
DESIGN = {
    "4x4": ((2, 0, 0), 13, 13), "8x8": ((2, -1, 0), 13, 13), "16x16": ((2, -2, 0), 13, 12), "32x32": ((2, -4, 0), 12, 12),
    "64x64": ((0, -2, -2), 13, 10), "4x8": ((2, -1, 0), 13, 13), "8x4": ((2, -1, 0), 13, 13), "8x16": ((2, -2, 0), 13, 13),
    "16x8": ((2, -2, 0), 13, 13), "16x32": ((2, -4, 0), 12, 13), "32x16": ((2, -4, 0), 13, 13), "32x64": ((0, -2, -2), 13, 11),
    "64x32": ((2, -4, -2), 12, 11), "4x16": ((2, -1, 0), 13, 12), "16x4": ((2, -1, 0), 13, 13), "8x32": ((2, -2, 0), 12, 12),
    "32x8": ((2, -2, 0), 13, 12), "16x64": ((0, -2, 0), 13, 12), "64x16": ((2, -4, 0), 13, 12),
}


def size_name(ts):
    return "%dx%d" % (TX_W[ts], TX_H[ts])


def design(ts):
    return DESIGN[size_name(ts)]


def _mult_stages(kind, n):
    if kind == DCT:
        return int(math.log2(n)) - 1
    if kind in (ADST, FLIPADST):
        return {4: 1, 8: 3, 16: 4}[n]
    return 1 if n in (4, 16) else 0


def _rounding(n, m):
    return 0.5 * sum(min((2 * SQRT2) ** j, math.sqrt(n) * SQRT2 ** j) for j in range(m))


def _abs_gain(b):
    return float(np.abs(b).sum(axis=0).max())


def budget(ts, tt, amp):
    """the docstring's E4 (E5 for r != 1): the most a correct fixed-point forward transform of this design can differ from fwd2d on a
    residual bounded by amp"""
    (s0, s1, s2), bit_c, bit_r = design(ts)
    ck, rk = TYPE_KINDS[tt]
    h, w = TX_H[ts], TX_W[ts]
    bc, br = bases(ts, tt)
    mc, mr = _mult_stages(ck, h), _mult_stages(rk, w)
    if ck == IDTX:
        bit_c = 12
    if rk == IDTX:
        bit_r = 12
    x0 = amp * 2.0 ** s0
    e1 = _rounding(h, mc) + mc * 2.0 ** -bit_c * h * x0
    e2 = e1 * 2.0 ** s1 + (0.5 if s1 < 0 else 0.0)
    x2 = _abs_gain(bc) * x0 * 2.0 ** s1 + 0.5 + e2
    e3 = _abs_gain(br) * e2 + _rounding(w, mr) + mr * 2.0 ** -bit_r * w * x2
    e4 = e3 * 2.0 ** s2 + (0.5 if s2 < 0 else 0.0)
    if not is_rect2(ts):
        return e4
    cmax = GAIN[ts] * _abs_gain(bc) * _abs_gain(br) * amp
    return e4 * 5793 / 4096 + 0.5 + 2.0 ** -13 * (cmax + e4)


# claimed limit of every range claim (docstring)
RANGE_LIMITS = {"final": 1 << 18, "pre_sqrt2": 1 << 18, "sine4": 1 << 23, "identity": 1 << 23, "mad24": 1 << 23, "mad32": 1 << 31}


def range_claims(x, ts, tt):
    """{claim: measured magnitude} for the residual x, from model intermediates (docstring, RANGE CLAIMS); a claim that does not
    apply to this (size, type) is absent"""
    (s0, s1, _), bit_c, bit_r = design(ts)
    ck, rk = TYPE_KINDS[tt]
    h, w = TX_H[ts], TX_W[ts]
    bc, br = bases(ts, tt)
    x = np.asarray(x, np.float64)
    coef = fwd2d(x, ts, tt)
    out = {"final": float(np.abs(coef).max())}
    if is_rect2(ts):
        out["pre_sqrt2"] = out["final"] * 4096 / 5793
    col_in = x * 2.0 ** s0                                         # [h, w]: the column pass transforms along axis 0
    row_in = (basis(ck, h).T @ x) * 2.0 ** (s0 + s1)               # every row of the column-pass output (rows >= 32 are computed too)
    for kind, n, v, axis, bit in ((ck, h, col_in, 0, bit_c), (rk, w, row_in[:coef_shape(ts)[0]], 1, bit_r)):
        if kind in (ADST, FLIPADST) and n == 4:
            out["sine4"] = max(out.get("sine4", 0.0), 3 * float(np.abs(v).max()))
        elif kind == IDTX:
            if n in (4, 16):
                out["identity"] = max(out.get("identity", 0.0), float(np.abs(v).max()))
        else:
            op = math.sqrt(n) * float(np.sqrt((v * v).sum(axis=axis)).max())
            out["mad24"] = max(out.get("mad24", 0.0), op)
            out["mad32"] = max(out.get("mad32", 0.0), op * SQRT2 * 2.0 ** bit)
    return out


# ---- worst-case inputs ----------------------------------------------------------------------------------------------------------
def maximiser_positions(ts, tt):
    """output positions (u, v) whose coefficient the generator maximises: DC, the last kept row, the last kept column, their corner,
    (1, 1) and two seeded random ones"""
    ch, cw = coef_shape(ts)
    rng = np.random.default_rng(1000 * ts + tt)
    pos = [(0, 0), (ch - 1, 0), (0, cw - 1), (ch - 1, cw - 1), (1, 1)]
    pos += [(int(rng.integers(0, ch)), int(rng.integers(0, cw))) for _ in range(2)]
    return pos


def worst_case_inputs(ts, tt, amp):
    """[(name, int16 residual [H, W])]: flat +-amp, checkerboard, an impulse of either sign in each corner, a horizontal and a vertical
    step edge, and for each of maximiser_positions the residual amp * sign(Bc[:, u] (x) Br[:, v]), which maximises |coef[u, v]| over
    all residuals bounded by amp (the coefficient is linear in x, so its maximum over the cube lies at that corner)"""
    h, w = TX_H[ts], TX_W[ts]
    yy, xx = np.mgrid[0:h, 0:w]
    out = [("flat+", np.full((h, w), amp)), ("flat-", np.full((h, w), -amp)), ("checker", np.where((yy + xx) & 1, -amp, amp))]
    for cy, cx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        for s in (1, -1):
            z = np.zeros((h, w), np.int64)
            z[cy, cx] = s * amp
            out.append(("impulse%+d@%d,%d" % (s, cy, cx), z))
    out.append(("hstep", np.where(yy < h // 2, amp, -amp)))
    out.append(("vstep", np.where(xx < w // 2, amp, -amp)))
    bc, br = bases(ts, tt)
    for u, v in maximiser_positions(ts, tt):
        sgn = np.where(np.outer(bc[:, u], br[:, v]) >= 0, 1, -1)
        out.append(("max@%d,%d" % (u, v), amp * sgn))
    return [(name, np.ascontiguousarray(a, np.int16)) for name, a in out]


# ---- quantiser, dequantiser (Python ints) ------------------------------------------------------------------------------------------
def round2(v, n):
    return (v + (1 << (n - 1))) >> n if n else v


def quant_round(q, ls, r=64):
    return round2((r * q) >> 7, ls)


def quantize_one(c, q, ls, r=64):
    """(level, dq) of one coefficient"""
    c = int(c)
    a = abs(c)
    lvl = 0
    if a << (1 + ls) >= q:
        lvl = min(32767, (min(a + quant_round(q, ls, r), 32767) * (65536 // q)) >> (16 - ls))
    dq = (lvl * q) >> ls
    return (-lvl, -dq) if c < 0 else (lvl, dq)


def quantize(coef, dc_q, ac_q, ls, ac_round=64, coef_per_blk=None):
    """a run of coefficients: the first one of every coef_per_blk (default: of the whole run) is DC; returns (levels, dq) as int64
    arrays of coef's shape"""
    flat = [int(v) for v in np.asarray(coef).reshape(-1)]
    per = coef_per_blk or max(len(flat), 1)
    res = [quantize_one(c, dc_q, ls, 64) if i % per == 0 else quantize_one(c, ac_q, ls, ac_round) for i, c in enumerate(flat)]
    shape = np.asarray(coef).shape
    return (np.array([l for l, _ in res], np.int64).reshape(shape), np.array([d for _, d in res], np.int64).reshape(shape))


def ideal_level(c, q, ls, r=64):
    """L* = (|c| + rnd) 2^ls / q, real-valued"""
    return (abs(int(c)) + quant_round(q, ls, r)) * 2.0 ** ls / q


def dequantize_one(level, q, ls, bd):
    level = int(level)
    dq = ((abs(level) * q) & 0xFFFFFF) >> ls
    if level < 0:
        dq = -dq
    return max(-(1 << (7 + bd)), min((1 << (7 + bd)) - 1, dq))


def dequantize(levels, dc_q, ac_q, ls, bd, coef_per_blk=None):
    flat = [int(v) for v in np.asarray(levels).reshape(-1)]
    per = coef_per_blk or max(len(flat), 1)
    out = [dequantize_one(l, dc_q if i % per == 0 else ac_q, ls, bd) for i, l in enumerate(flat)]
    return np.array(out, np.int64).reshape(np.asarray(levels).shape)


@functools.lru_cache(maxsize=None)
def dequantize_all_levels(q, ls, bd):
    """the model over all 65536 int16 levels, every one with step q, in the order -32768 .. 32767"""
    out = np.array([dequantize_one(l, q, ls, bd) for l in range(-32768, 32768)], np.int64)
    out.setflags(write=False)
    return out


def quant_edge_coefs(q, ls, r=64, seed=0, n_random=24):
    """the coefficients at which a quantiser of step q goes wrong if it does: 0, +-1, the +-1 neighbourhood of the zero-bin threshold
    |c| 2^(1+ls) = q and of the clamp |c| + rnd = 32767, |c| around 2^20 and at the ends of int32, and seeded random ones of three
    ranges.  int64, every value inside int32"""
    t = -(-q >> (1 + ls))                       # the smallest |c| outside the zero bin
    k = 32767 - quant_round(q, ls, r)
    mags = [0, 1, t - 1, t, t + 1, k - 1, k, k + 1, 32767, 32768, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 31) - 1]
    rng = np.random.default_rng(seed * 7919 + q * 3 + ls)
    mags += [int(v) for v in rng.integers(0, 4 * q + 2, n_random // 3)]
    mags += [int(v) for v in rng.integers(0, 40000, n_random // 3)]
    mags += [int(v) for v in rng.integers(0, 1 << 31, n_random // 3)]
    out = []
    for m in mags:
        m = max(m, 0)
        out += [m, -m]
    out.append(-(1 << 31))
    return np.array(out, np.int64)


# ---- what the golden file tests/golden/txq_model_observed.json records (tools/gen_txq_observed.py writes it) ----------------------
def random_inputs(ts, tt, amp, n=4):
    rng = np.random.default_rng(77 + 100 * ts + tt + amp)
    return [("random%d" % i, rng.integers(-amp, amp + 1, (TX_H[ts], TX_W[ts])).astype(np.int16)) for i in range(n)]


def observe_size(fwd, ts):
    """fwd(resid, ts, tt) -> integer coefficients of the transform under test.  Over every valid type of the size, the worst-case and
    random inputs: per amplitude the largest |fwd - model| with the budget of the type it occurred at (the type with the largest
    error / budget), the largest |coefficient| of fwd at 10 bit, and for every range claim the largest measured value and its limit"""
    out = {"size": size_name(ts), "forward_error": {}, "claims": {}}
    coef_max = 0
    for amp in (255, 1023):
        worst = None
        for tt in range(N_TYPES):
            if not valid(ts, tt):
                continue
            bud = budget(ts, tt, amp)
            for name, x in worst_case_inputs(ts, tt, amp) + random_inputs(ts, tt, amp):
                got = np.asarray(fwd(x, ts, tt), np.int64)
                err = float(np.abs(got - fwd2d(x, ts, tt)).max())
                if worst is None or err / bud > worst[0] / worst[1]:
                    worst = (err, bud, tt, name)
                if amp == 1023:
                    coef_max = max(coef_max, int(np.abs(got).max()))
                    for k, v in range_claims(x, ts, tt).items():
                        out["claims"][k] = max(out["claims"].get(k, 0.0), v)
        out["forward_error"][str(amp)] = {"observed": round(worst[0], 3), "budget": round(worst[1], 3), "type": worst[2], "input": worst[3]}
    out["coef_max_10bit"] = coef_max
    out["claims"] = {k: {"measured": round(v, 1), "limit": RANGE_LIMITS[k]} for k, v in sorted(out["claims"].items())}
    return out


def check_quantiser_against_ideal(coef, levels, dc_q, ac_q, ls, ac_round=64):
    """the proved bound against the real-valued quantiser wherever |c| + rnd <= 32767, and above that point the behaviour the design
    has chosen.  coef / levels: one run whose first coefficient is DC"""
    for i, (c, lvl) in enumerate(zip((int(v) for v in np.asarray(coef).reshape(-1)), (int(v) for v in np.asarray(levels).reshape(-1)))):
        q, r = (dc_q, 64) if i == 0 else (ac_q, ac_round)
        rnd = quant_round(q, ls, r)
        assert lvl == 0 or (lvl > 0) == (c > 0), (c, lvl)
        if abs(c) << (1 + ls) < q:
            assert lvl == 0, (c, q, ls)
        elif abs(c) + rnd <= 32767:
            ideal = ideal_level(c, q, ls, r)
            assert 0 <= ideal - abs(lvl) <= 1 + ideal * q / 65536, (c, q, ls, r, lvl, ideal)
        else:
            # The int16 clamp of the coefficient: min(|c| + rnd, 32767) in kernel and oracle alike.  Every larger coefficient codes as
            # the one at the clamp, so the reconstruction falls short of the source.  Content that reaches it: a 10-bit 8 x 8 block
            # whose mean residual exceeds +-511 (its DC coefficient is 64 times the mean); 8-bit content never does.
            at_clamp = quantize_one(32767 - rnd, q, ls, r)[0]
            assert abs(lvl) == at_clamp, (c, q, ls, r, lvl, at_clamp)


def dequant_steps(O, bd):
    """the smallest and the largest step of the bit depth, the steps whose product with 32767 lies just below and just above 2^24
    (512 and 513, and the nearest entries of the AC table), and one in between"""
    ac = sorted({O.ac_q(i, bd) for i in range(256)})
    below, above = max(q for q in ac if 32767 * q < 1 << 24), min([q for q in ac if 32767 * q >= 1 << 24] or [513])
    return sorted({ac[0], ac[-1], 512, 513, below, above, 100})


ALL_LEVELS = np.arange(-32768, 32768, dtype=np.int16)
