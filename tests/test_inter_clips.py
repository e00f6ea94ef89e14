"""The clips of tests/inter_clips.py do what they are there for — checked with the CPU oracle alone (no GPU): ties among non-zero
ranks, fractional vectors whose prediction is clamped at 0 and at the top value, scattered vectors, matches at the corners of the
search square, a refinement on the low bits.  The thresholds are the issue's; the counts observed are kept in
tests/golden/inter_content_observed.json (recorded results; `python tests/test_inter_clips.py` rewrites the file)."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import inter_clips as IC
import me_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_content_observed.json")
W, H, Q = IC.W, IC.H, 60
NB = (W // 8) * (H // 8)
DEPTHS = (8, 10)


def _oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from oracle import oracle
    oracle.build()
    return oracle


def sad_table(src_y, ref_y, bd, R):
    """[2R+1 (dy), 2R+1 (dx), h / 8, w / 8]: the integer search's score of every displacement of every block as
    me_ref.integer_vectors computes it — 8-bit views, the block's even rows, reference coordinates clamped into the plane"""
    h, w = src_y.shape
    S8 = me_ref.m8(src_y, bd)
    R8 = np.pad(me_ref.m8(ref_y, bd), R, mode="edge")
    n = 2 * R + 1
    out = np.zeros((n, n, h // 8, w // 8), np.int64)
    for dy in range(n):
        for dx in range(n):
            d = np.abs(S8 - R8[dy:dy + h, dx:dx + w])
            out[dy, dx] = d.reshape(h // 8, 8, w // 8, 8)[:, ::2].sum(axis=(1, 3))
    return out


def final_stats(O, src, ref, bd, R):
    """one frame through the oracle's inter loop: the result, which blocks end on a fractional vector, and whether the luma
    prediction at the final vector holds a 0 / a top sample"""
    r = O.inter_encode_frame(src, ref, bd, Q, R)
    h, w = src[0].shape
    mv = r["mvs"].astype(int)
    frac = ((mv & 7) != 0).any(axis=1)
    lo, hi = np.zeros(len(mv), bool), np.zeros(len(mv), bool)
    for b in range(len(mv)):
        p = O.mc_block(ref[0], bd, (b % (w // 8)) * 8, (b // (w // 8)) * 8, 8, 8, 2 * int(mv[b, 0]), 2 * int(mv[b, 1]))
        lo[b], hi[b] = (p == 0).any(), (p == IC.top_of(bd)).any()
    return r, frac, lo, hi


@functools.lru_cache(maxsize=None)
def observe(bd):
    """the counts each condition below is about, per clip, at one depth (plain ints: what the golden file holds)"""
    O = _oracle()
    out = {}
    # checker_shift: ties among non-zero ranks
    src, ref = IC.checker_shift(W, H, bd)
    T = sad_table(src[0], ref[0], bd, 8)
    at_min = T == T.min(axis=(0, 1))
    tied = (at_min.sum(axis=(0, 1)) > 1) & ~at_min[8, 8]
    out["checker_shift"] = dict(blocks=NB, tied_without_zero_vector=int(tied.sum()), least_ties=int(at_min.sum(axis=(0, 1)).min()))
    # ... of single samples: the two first minima in raster order lie 2 apart in one row of displacements, and both in one of the
    # integer search's groups of four (dx = -8 .. -5, -4 .. -1, ...)
    src, ref = IC.checker_shift(W, H, bd, cell=1)
    T = sad_table(src[0], ref[0], bd, 8)
    at_min = (T == T.min(axis=(0, 1))).reshape(17 * 17, H // 8, W // 8)
    first = at_min.argmax(axis=0)
    second = np.where(np.arange(17 * 17)[:, None, None] > first, at_min, False).argmax(axis=0)
    same_group = (first // 17 == second // 17) & (first % 17 // 4 == second % 17 // 4) & ~at_min[8 * 17 + 8]
    out["checker1_shift"] = dict(blocks=NB, first_two_minima_in_one_group=int(same_group.sum()))
    # half-sample clips: fractional vectors with a prediction clamped at both ends
    for name, clip, R in (("checker_half_x", IC.checker_half(W, H, bd, False), 8), ("checker_half_xy", IC.checker_half(W, H, bd, True), 4),
                          ("binary_half", IC.binary_half(W, H, bd), 8)):
        _, frac, lo, hi = final_stats(O, clip[0], clip[1], bd, R)
        out[name] = dict(blocks=NB, search_range=R, fractional_touching_0_and_top=int((frac & lo & hi).sum()))
    src, ref = IC.noise_vs_noise(W, H, bd)
    r, frac, lo, hi = final_stats(O, src, ref, bd, 8)
    out["noise_vs_noise"] = dict(blocks=NB, distinct_vectors=len({tuple(v) for v in r["mvs"].tolist()}),
                                 fractional_touching_0=int((frac & lo).sum()), fractional_touching_top=int((frac & hi).sum()))
    # noise_corner: the displaced vector exactly, wherever the match lies inside the plane
    nc = {}
    for R in (5, 8, 15):
        for sx, sy in IC.corner_displacements(R):
            src, ref = IC.noise_corner(W, H, bd, sx, sy)
            r = O.inter_encode_frame(src, ref, bd, Q, R)
            by, bx = np.divmod(np.arange(NB), W // 8)
            inside = (bx * 8 + sx >= 0) & (bx * 8 + 8 + sx <= W) & (by * 8 + sy >= 0) & (by * 8 + 8 + sy <= H)
            exact = (r["mvs"][:, 0] == 8 * sx) & (r["mvs"][:, 1] == 8 * sy) & ~r["lev_y"].reshape(NB, -1).any(axis=1)
            nc["R%d(%d,%d)" % (R, sx, sy)] = dict(inside=int(inside.sum()), inside_exact=int((inside & exact).sum()))
    out["noise_corner"] = nc
    if bd == 10:
        src, ref = IC.low_bits(W, H)
        r, frac, _, _ = final_stats(O, src, ref, bd, 8)
        equal8 = all((me_ref.m8(s, bd) == me_ref.m8(f, bd)).all() for s, f in zip(src, ref))
        out["low_bits"] = dict(blocks=NB, views_equal=bool(equal8), fractional=int(frac.sum()),
                               distinct_vectors=len({tuple(v) for v in r["mvs"].tolist()}))
    return out


@pytest.mark.parametrize("bd", DEPTHS)
def test_shapes_types_and_range(bd):
    clips = [IC.checker_shift(W, H, bd), IC.checker_half(W, H, bd, False), IC.checker_half(W, H, bd, True), IC.noise_vs_noise(W, H, bd),
             IC.binary_half(W, H, bd), IC.noise_corner(W, H, bd, -8, 8)] + ([IC.low_bits(W, H)] if bd == 10 else [])
    for src, ref in clips:
        for t in (src, ref):
            assert [a.shape for a in t] == [(H, W), (H // 2, W // 2), (H // 2, W // 2)]
            assert all(a.dtype == (np.uint8 if bd == 8 else np.uint16) and int(a.max()) <= IC.top_of(bd) for a in t)
    for k in (0, 3):      # full range: the extremes are there, in source and reference, luma and chroma
        for t in clips[k]:
            assert all(int(a.min()) == 0 and int(a.max()) == IC.top_of(bd) for a in t)
    S, R = IC.stack(clips[:3])
    assert S[0].shape == (3, H, W) and R[2].shape == (3, H // 2, W // 2) and (S[1][2] == clips[2][0][1]).all()


@pytest.mark.parametrize("bd", DEPTHS)
def test_checker_shift_ties_without_the_zero_vector(bd):
    o = observe(bd)["checker_shift"]
    assert o["tied_without_zero_vector"] >= 0.9 * NB, o
    o = observe(bd)["checker1_shift"]
    assert o["first_two_minima_in_one_group"] >= 0.9 * NB, o


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("clip", ["checker_half_x", "checker_half_xy", "binary_half"])
def test_half_sample_clips_clamp_at_both_ends(bd, clip):
    o = observe(bd)[clip]
    assert o["fractional_touching_0_and_top"] >= 0.9 * NB, o


@pytest.mark.parametrize("bd", DEPTHS)
def test_noise_vs_noise_scatters_and_overshoots(bd):
    o = observe(bd)["noise_vs_noise"]
    assert o["distinct_vectors"] >= 100, o
    assert o["fractional_touching_0"] >= 0.25 * NB and o["fractional_touching_top"] >= 0.25 * NB, o


@pytest.mark.parametrize("bd", DEPTHS)
def test_noise_corner_finds_the_displaced_block(bd):
    for key, o in observe(bd)["noise_corner"].items():
        assert o["inside"] > 0 and o["inside_exact"] == o["inside"], (key, o)


def test_low_bits_leaves_the_refinement_alone():
    o = observe(10)["low_bits"]
    assert o["views_equal"], o
    assert o["fractional"] >= 0.9 * NB and o["distinct_vectors"] >= 20, o


@pytest.mark.parametrize("bd", DEPTHS)
def test_half_sample_frames_fill_every_class_of_vector(bd):
    """what tests/test_gpu_inter_vs_mc.py compares must be there by the oracle alone: per depth at least 16 skipped blocks whose final
    vector has a fraction along x only, 16 along y only, 16 along both, and one whose filter window reaches outside the plane.  (72 x 40
    is 45 blocks, so the three times 16 take three frames.)"""
    O = _oracle()
    w, h, q = IC.HALF_W, IC.HALF_H, IC.HALF_Q
    n = dict(x_only=0, y_only=0, both=0, outside=0)
    for src, ref in IC.half_sample_frames(w, h, bd):
        r = O.inter_encode_frame(src, ref, bd, q, 8)
        for k, m in IC.vector_classes(r["mvs"], r["skip"], w, h).items():
            n[k] += int(m.sum())
    assert n["x_only"] >= 16 and n["y_only"] >= 16 and n["both"] >= 16 and n["outside"] >= 1, n


def test_observed_counts_are_recorded():
    rec = json.load(open(GOLD))
    now = {str(bd): observe(bd) for bd in DEPTHS}
    assert rec == json.loads(json.dumps(now)), "tests/golden/inter_content_observed.json is stale: python tests/test_inter_clips.py"


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "av1-go_amd"))
    with open(GOLD, "w") as f:
        json.dump({str(bd): observe(bd) for bd in DEPTHS}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(GOLD).read())
