"""GPU parity of the inter block pipeline (k_me_int + k_inter_pipe) on the hard content of tests/inter_clips.py: all eight outputs of
Context.inter_encode_arrays — vectors, skip flags, levels and reconstruction of the three planes — equal the oracle's inter loop
(oracle/av1o_pipeline.c av1o_inter_encode_frame) bit for bit, frame by frame.  What tests/test_gpu_inter.py's blurred, limited-range
clip never does happens here in most blocks: ties among non-zero ranks in the integer search and in both refinement rounds,
predictions clamped at 0 and at the top value, samples 0 and 255 under the biased-byte dot products, windows up to R + 4 samples
outside the plane on every side, rows further apart than the plane is wide, frame counts that leave a remainder.
tests/test_inter_clips.py shows (CPU, oracle alone) that the clips do these things."""
import numpy as np
import pytest

import inter_clips as IC
import me_ref

pytestmark = pytest.mark.gpu
KEYS = ("mvs", "skip", "lev_y", "lev_u", "lev_v", "rec_y", "rec_u", "rec_v")
W, H, Q = IC.W, IC.H, 60
DEPTHS = (8, 10)

_clips, _expected = {}, {}


def clip(name, w, h, bd):
    """a clip by name, built once: the generators' names, 'checker_half_x' / '_xy', 'noise_vs_noise#seed', 'corner(sx,sy)',
    'checker1_shift' (the checker of single samples)"""
    key = (name, w, h, bd)
    if key not in _clips:
        if name.startswith("corner("):
            sx, sy = (int(v) for v in name[7:-1].split(","))
            c = IC.noise_corner(w, h, bd, sx, sy)
        elif name.startswith("noise_vs_noise#"):
            c = IC.noise_vs_noise(w, h, bd, seed=int(name.split("#")[1]))
        elif name.startswith("checker_half_"):
            c = IC.checker_half(w, h, bd, name.endswith("_xy"))
        elif name == "low_bits":
            c = IC.low_bits(w, h)
        elif name == "checker1_shift":
            c = IC.checker_shift(w, h, bd, cell=1)
        else:
            c = getattr(IC, name)(w, h, bd)
        _clips[key] = c
    return _clips[key]


def expected(O, name, w, h, bd, q, R):
    """the oracle's result for one clip, computed once and shared by the tests that run the clip with the same settings"""
    key = (name, w, h, bd, q, R)
    if key not in _expected:
        src, ref = clip(name, w, h, bd)
        _expected[key] = O.inter_encode_frame(src, ref, bd, q, R)
    return _expected[key]


def stacked_names(bd, R):
    """the clips that share a range, as frames of one job: 6 at 8 bits, 7 at 10 — no multiple of 8"""
    names = ["checker_shift", "checker_half_x", "checker_half_xy", "noise_vs_noise#1", "binary_half", "corner(%d,%d)" % (-R, R)]
    return names + (["low_bits"] if bd == 10 else [])


def run_and_compare(ctx, O, names, w, h, bd, q, R, **strides):
    S, Rf = IC.stack([clip(n, w, h, bd) for n in names])
    got = ctx.inter_encode_arrays(S, Rf, bd, q, R, **strides)
    for f, name in enumerate(names):
        exp = expected(O, name, w, h, bd, q, R)
        for k in KEYS:
            g, e = got[k][f], exp[k]
            assert g.shape == e.shape and (g == e).all(), (
                "clip %s, %dx%d, %d bit, q %d, range %d, %s: %s of frame %d (of %d) differs from the oracle at %s: got %s, expected %s"
                % (name, w, h, bd, q, R, strides or "compact rows", k, f, len(names), np.argwhere(g != e)[:4].tolist(),
                   g[g != e][:4].tolist(), e[g != e][:4].tolist()))
    return got


@pytest.mark.parametrize("R", [8, 5, 15])
@pytest.mark.parametrize("bd", DEPTHS)
def test_stacked_clips(ctx, O, bd, R):
    """R = 8: the compile-time search with 32 items per block; R = 5: R4 = 8 and 11 rows, the last triple of vertical displacements
    holds two; R = 15: the widest window"""
    run_and_compare(ctx, O, stacked_names(bd, R), W, H, bd, Q, R)


@pytest.mark.parametrize("q", [255, 1])
@pytest.mark.parametrize("bd", DEPTHS)
def test_checker_and_noise_at_the_quantiser_ends(ctx, O, bd, q):
    """... and the checker of single samples, whose tied displacements share a packed QSAD word"""
    run_and_compare(ctx, O, ["checker_shift", "checker_half_x", "checker_half_xy", "noise_vs_noise#1", "checker1_shift"], W, H, bd, q, 8)


@pytest.mark.parametrize("bd", DEPTHS)
def test_refinement_alone(ctx, O, bd):
    """R = 0: one candidate in the integer search, every decision is the refinement's"""
    run_and_compare(ctx, O, ["checker_half_x", "checker_half_xy", "binary_half"] + (["low_bits"] if bd == 10 else []), W, H, bd, Q, 0)


@pytest.mark.parametrize("R", [5, 8, 15])
@pytest.mark.parametrize("bd", DEPTHS)
def test_match_at_corners_and_edges_of_the_search_square(ctx, O, bd, R):
    """the only exact match is rank 1, rank (2R + 1)^2, the ends of a row or of a column of the square; edge blocks search windows up
    to R + 4 samples outside the plane on every side"""
    run_and_compare(ctx, O, ["corner(%d,%d)" % d for d in IC.corner_displacements(R)], W, H, bd, Q, R)


@pytest.mark.parametrize("w,h", [(72, 40), (8, 8)])
@pytest.mark.parametrize("bd", DEPTHS)
def test_small_frames(ctx, O, bd, w, h):
    """72x40: less than a tile down, chroma 36 wide (a 4-tap window row of 12 over a 36-sample plane); 8x8: one block, every window
    mostly outside the plane"""
    run_and_compare(ctx, O, stacked_names(bd, 8), w, h, bd, Q, 8)


@pytest.mark.parametrize("bd", DEPTHS)
def test_noise_200x136(ctx, O, bd):
    """425 blocks a frame: the frames' workgroups end on a partial one, and 3 x 14 workgroups are no multiple of the XCD count"""
    run_and_compare(ctx, O, ["noise_vs_noise#1", "noise_vs_noise#2", "noise_vs_noise#3"], 200, 136, bd, Q, 8)


@pytest.mark.parametrize("bd", DEPTHS)
def test_padded_rows(ctx, O, bd):
    """stride_y = w + 24, stride_uv = w / 2 + 4: the results equal the oracle's on the compact arrays and the reconstruction's padding
    still holds the sentinel it was filled with"""
    names = ["noise_vs_noise#1", "corner(-8,8)", "noise_vs_noise#2"]
    got = run_and_compare(ctx, O, names, W, H, bd, Q, 8, stride_y=W + 24, stride_uv=W // 2 + 4)
    sentinel = 0xA5 if bd == 8 else 0xA5A5
    for p, rows, cols in (("y", H, 24), ("u", H // 2, 4), ("v", H // 2, 4)):
        pad = got["rec_pad_" + p]
        assert pad.shape == (len(names), rows, cols)
        assert (pad == sentinel).all(), ("plane %s, %d bit: the kernel wrote into the row padding at %s" % (p, bd, np.argwhere(pad != sentinel)[:4].tolist()))


def test_bad_strides_are_refused(ctx, av1mi):
    S, Rf = IC.stack([clip("noise_vs_noise#1", 8, 8, 8)])
    for strides in (dict(stride_y=10), dict(stride_y=4), dict(stride_uv=6), dict(stride_uv=0), dict(stride_y=8 + 24, stride_uv=4 + 2)):
        with pytest.raises(av1mi.Av1miError):
            ctx.inter_encode_arrays(S, Rf, 8, Q, 8, **strides)


@pytest.mark.parametrize("R", [8, 5])
@pytest.mark.parametrize("bd", DEPTHS)
def test_search_alone_matches_the_numpy_restatement(ctx, bd, R):
    """the tie order held to the second, independent restatement (tests/me_ref.py): all ties but never the zero vector
    (checker_shift), and all ties with the zero vector among them (low_bits)"""
    names = ["checker_shift"] + (["low_bits"] if bd == 10 else []) + ["checker1_shift"]
    S, Rf = IC.stack([clip(n, W, H, bd) for n in names])
    got = ctx.me_search(S[0], Rf[0], bd, R)["mvs"]
    for f, name in enumerate(names):
        exp = me_ref.search(S[0][f], Rf[0][f], bd, R, 0)["mvs"]
        assert (got[f] == exp).all(), ("clip %s, %d bit, range %d: integer vectors of frame %d differ at blocks %s"
                                       % (name, bd, R, f, np.argwhere(got[f] != exp)[:4].tolist()))
    if bd == 10:
        assert not got[1].any()      # low_bits: every displacement scores 0, rank 0 wins
