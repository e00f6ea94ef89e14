"""Hard content for the inter block pipeline (k_me_int + k_inter_pipe): one frame per clip, built so that what synth.frames never
does happens in most blocks — tied candidates of non-zero rank, predictions clamped at 0 and at the top value, windows far outside
the plane, a refinement that has only the low bits to go by.  Plain numpy, nothing read from disk; test infrastructure only.

Every generator returns (src, ref), each a (Y, U, V) tuple of [h, w] / [h / 2, w / 2] arrays of the depth's sample type.  What each
clip is there for is checked with the oracle alone in tests/test_inter_clips.py; the GPU is held to them in
tests/test_gpu_inter_content.py."""
import numpy as np

W, H = 136, 72      # 2 full tiles + an 8-column tile across, 1 tile + 8 rows down: 153 blocks, 5 workgroups of k_inter_pipe (4.8)


def top_of(bd):
    return (1 << bd) - 1


def _dt(bd):
    return np.uint8 if bd == 8 else np.uint16


def _planes(w, h):
    return ((h, w), (h // 2, w // 2), (h // 2, w // 2))


def _checker(h, w, bd, cell=2):
    """C[y, x] = top * ((x // 2 + y // 2) & 1): period 4 both ways, and C[y + 2, x + 2] = C[y, x] (cell = 1: single samples, period 2)"""
    y, x = np.mgrid[0:h, 0:w]
    return (top_of(bd) * ((x // cell + y // cell) & 1)).astype(np.int32)


def _avg2(a, b):
    return (a + b + 1) >> 1


def checker_shift(w, h, bd, cell=2):
    """ref = the checker, src = the checker one column to the right: every displacement (1 + 4 i + 2 j, 2 j) matches exactly, the
    zero vector does not.  The winner is the first exact match in raster order — never rank 0.  The matches of a row of
    displacements lie 4 apart; with cell = 1 (a checker of single samples) every (dx, dy) with dx + dy odd matches, so tied
    displacements lie 2 apart: inside one group of four horizontal neighbours."""
    src, ref = [], []
    for ph, pw in _planes(w, h):
        C = _checker(ph, pw + 1, bd, cell)
        ref.append(C[:, :pw].astype(_dt(bd)))
        src.append(C[:, 1:pw + 1].astype(_dt(bd)))
    return tuple(src), tuple(ref)


def checker_half(w, h, bd, both):
    """ref = the checker, src = the rounded average of the checker and its right neighbour (both: of the four samples at x, x + 1,
    y, y + 1): the best vector is a half-sample one, where the 8-tap filter overshoots the checker's steps to below 0 and above top"""
    src, ref = [], []
    for ph, pw in _planes(w, h):
        C = _checker(ph + 1, pw + 1, bd)
        ref.append(C[:ph, :pw].astype(_dt(bd)))
        if both:
            s = (C[:ph, :pw] + C[:ph, 1:pw + 1] + C[1:ph + 1, :pw] + C[1:ph + 1, 1:pw + 1] + 2) >> 2
        else:
            s = _avg2(C[:ph, :pw], C[:ph, 1:pw + 1])
        src.append(s.astype(_dt(bd)))
    return tuple(src), tuple(ref)


def noise_vs_noise(w, h, bd, seed=1):
    """independent uniform noise over 0 .. top in all six planes: nothing matches, vectors scatter over the whole search square and
    the sub-sample predictions of noise overshoot both ways"""
    rng = np.random.default_rng([seed, bd, w, h])
    src = tuple(rng.integers(0, top_of(bd) + 1, s).astype(_dt(bd)) for s in _planes(w, h))
    ref = tuple(rng.integers(0, top_of(bd) + 1, s).astype(_dt(bd)) for s in _planes(w, h))
    return src, ref


def binary_half(w, h, bd, seed=2):
    """ref = noise of {0, top}, src = its rounded average with the right neighbour: half-sample vectors on content whose every
    step is the full range"""
    rng = np.random.default_rng([seed, bd, w, h])
    src, ref = [], []
    for ph, pw in _planes(w, h):
        N = top_of(bd) * rng.integers(0, 2, (ph, pw + 1)).astype(np.int32)
        ref.append(N[:, :pw].astype(_dt(bd)))
        src.append(_avg2(N[:, :pw], N[:, 1:pw + 1]).astype(_dt(bd)))
    return tuple(src), tuple(ref)


def noise_corner(w, h, bd, sx, sy, seed=3):
    """ref = a crop of full-range noise, src = the crop displaced by (sx, sy): the block at (x, y) matches the reference at
    (x + sx, y + sy) and nowhere else, so with (sx, sy) a corner or an edge mid-point of the search square the winner is its first or
    last rank, or the first or last of a row.  Chroma is displaced by (sx / 2, sy / 2) where both are whole, else it is independent
    noise.  Blocks whose match lies outside the plane search windows that are mostly edge extension."""
    rng = np.random.default_rng([seed, bd, w, h, sx + 64, sy + 64])
    src, ref = [], []
    for i, (ph, pw) in enumerate(_planes(w, h)):
        dx, dy = (sx, sy) if i == 0 else (sx // 2, sy // 2)
        m = max(abs(dx), abs(dy))
        N = rng.integers(0, top_of(bd) + 1, (ph + 2 * m, pw + 2 * m)).astype(_dt(bd))
        ref.append(N[m:m + ph, m:m + pw].copy())
        if i and ((sx | sy) & 1):
            src.append(rng.integers(0, top_of(bd) + 1, (ph, pw)).astype(_dt(bd)))
        else:
            src.append(N[m + dy:m + dy + ph, m + dx:m + dx + pw].copy())
    return tuple(src), tuple(ref)


def corner_displacements(R):
    """the four corners and the four edge mid-points of the search square [-R, R]^2, as (sx, sy)"""
    return [(-R, -R), (R, -R), (-R, R), (R, R), (-R, 0), (R, 0), (0, -R), (0, R)]


def low_bits(w, h, bd=10, seed=4):
    """10 bit only: src and ref = 512 + independent noise in 0 .. 3.  Their 8-bit views are equal everywhere, so the integer search is
    all ties (rank 0 must win) and the refinement has only the two low bits to go by"""
    assert bd == 10
    rng = np.random.default_rng([seed, w, h])
    src = tuple((512 + rng.integers(0, 4, s)).astype(np.uint16) for s in _planes(w, h))
    ref = tuple((512 + rng.integers(0, 4, s)).astype(np.uint16) for s in _planes(w, h))
    return src, ref


HALF_W, HALF_H, HALF_Q = 72, 40, 255      # half_sample_frames as the tests run them: 45 blocks a frame, the coarsest quantiser


def transposed(clip):
    """a clip of the transposed size with every plane transposed: what a generator does along x happens along y"""
    return tuple(tuple(np.ascontiguousarray(a.T) for a in t) for t in clip)


def half_sample_frames(w, h, bd):
    """three frames whose best vectors are half-sample ones along x only, along y only and along both, on content that a coarse
    quantiser leaves without a residual: checker_half along x, the same transposed, and checker_half both ways at half the
    amplitude (at the full one the 8-tap overshoot is a residual that no quantiser drops)"""
    both = tuple(tuple(a >> 1 for a in t) for t in checker_half(w, h, bd, True))
    return [checker_half(w, h, bd, False), transposed(checker_half(h, w, bd, False)), both]


def vector_classes(mvs, skip, w, h):
    """of the 8x8 blocks of a w x h frame with vectors mvs [n, 2] (1/8 luma samples) and flags skip [n]: boolean arrays for 'skipped
    and the vector has a fraction along x only', '... along y only', '... along both', and 'skipped and the 15 x 15 samples an 8-tap
    filter reads around the displaced block reach outside the plane'"""
    mv, sk = np.asarray(mvs).astype(int), np.asarray(skip).astype(bool)
    fx, fy = (mv[:, 0] & 7) != 0, (mv[:, 1] & 7) != 0
    b = np.arange(len(mv))
    x0, y0 = (b % (w // 8)) * 8 + (mv[:, 0] >> 3) - 3, (b // (w // 8)) * 8 + (mv[:, 1] >> 3) - 3
    outside = (x0 < 0) | (y0 < 0) | (x0 + 15 > w) | (y0 + 15 > h)
    return dict(x_only=sk & fx & ~fy, y_only=sk & ~fx & fy, both=sk & fx & fy, outside=sk & outside)


def stack(clips):
    """clips [(src, ref), ...] of one size -> (src, ref) with [frames, h, w] arrays, the layout of inter_encode_arrays"""
    return (tuple(np.stack([c[0][i] for c in clips]) for i in range(3)),
            tuple(np.stack([c[1][i] for c in clips]) for i in range(3)))
