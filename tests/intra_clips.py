"""Hard content for the fused intra pipeline (k_intra_pipe<8|16|32>, k_intra_modes, intra_fast.hpp): one frame per clip, built so that
what synth.frames never does happens in many blocks — exact ties among the 13 candidates with and without DC among them, upsampled
edges that overshoot 0 and the top value, neighbours that chose a smooth mode (edge filter type 1), reconstructions pinned against
both ends of the range.  Plain numpy, seeded, nothing read from disk; test infrastructure only.

Every generator returns (Y, U, V): [h, w] / [h / 2, w / 2] arrays of the depth's sample type.  What each clip is there for is checked
with the oracle alone in tests/test_intra_clips.py; the GPU is held to them in tests/test_gpu_intra_content.py."""
import numpy as np

# per luma block size the smallest frame whose tiles are partial both ways: 2 full 64x64 tiles + one of bs columns across, 1 tile +
# bs rows down — 6 tiles a frame at every size
SIZES = {8: (136, 72), 16: (144, 80), 32: (160, 96)}


def top_of(bd):
    return (1 << bd) - 1


def _dt(bd):
    return np.uint8 if bd == 8 else np.uint16


def _planes(w, h):
    return ((h, w), (h // 2, w // 2), (h // 2, w // 2))


def _yx(s):
    return np.mgrid[0:s[0], 0:s[1]]


def noise(w, h, bd, seed=1):
    """uniform over 0 .. top in all planes: the smooth modes win in about one block of seven, so many blocks have a smooth neighbour
    (edge filter type 1), and the reconstructed neighbours step across most of the range"""
    rng = np.random.default_rng([seed, bd, w, h])
    return tuple(rng.integers(0, top_of(bd) + 1, s).astype(_dt(bd)) for s in _planes(w, h))


def binary(w, h, bd, seed=2):
    """noise of {0, top}: every step is the full range, the reconstruction sits at 0 and at top in thousands of samples"""
    rng = np.random.default_rng([seed, bd, w, h])
    return tuple((top_of(bd) * rng.integers(0, 2, s)).astype(_dt(bd)) for s in _planes(w, h))


def checker(w, h, bd, cell=2):
    """top * ((x // cell + y // cell) & 1)"""
    out = []
    for s in _planes(w, h):
        y, x = _yx(s)
        out.append((top_of(bd) * ((x // cell + y // cell) & 1)).astype(_dt(bd)))
    return tuple(out)


def stripes(w, h, bd, across=False):
    """vertical stripes of period 6 (three samples of 0, three of top); across: the same along y"""
    out = []
    for s in _planes(w, h):
        y, x = _yx(s)
        out.append((top_of(bd) * (((y if across else x) // 3) & 1)).astype(_dt(bd)))
    return tuple(out)


def diag(w, h, bd):
    """stripes of period 6 along x + y: constant along the direction D45 predicts in"""
    out = []
    for s in _planes(w, h):
        y, x = _yx(s)
        out.append((top_of(bd) * (((x + y) // 3) & 1)).astype(_dt(bd)))
    return tuple(out)


def flat(w, h, bd, level):
    """every sample = level.  The first block of a tile has no neighbour and every candidate predicts a constant near mid-grey (V, D45
    and D67 one below it, H and D203 one above): a tie that DC is not part of.  Every later block's candidates all predict the
    reconstruction's constant: a tie of all 13 that DC wins."""
    return tuple(np.full(s, level, _dt(bd)) for s in _planes(w, h))


def flat0(w, h, bd):
    return flat(w, h, bd, 0)


def flat_top(w, h, bd):
    return flat(w, h, bd, top_of(bd))


def low_bits(w, h, bd=10, seed=4):
    """10 bit only: 512 + noise in 0 .. 3 — a decision on the two low bits, which an 8-bit view of the samples would not see"""
    assert bd == 10
    rng = np.random.default_rng([seed, w, h])
    return tuple((512 + rng.integers(0, 4, s)).astype(np.uint16) for s in _planes(w, h))


def uv_negative(w, h, bd, seed=5):
    """U = blocks of 4x4 noise, V = top - U: whatever a candidate gains on U's pattern it loses on V's negative, so the chroma
    decision is the one over the SUM of both planes' SADs — a sum over one half of the U + V pair decides differently.  Y = the
    same pattern as U at twice the size."""
    rng = np.random.default_rng([seed, bd, w, h])
    cells = rng.integers(0, top_of(bd) + 1, (h // 8 + 1, w // 8 + 1))
    y, x = _yx((h // 2, w // 2))
    ramp = ((x % 4) * 3 + (y % 4) * 5) << (bd - 8)
    u = np.clip(cells[y // 4, x // 4] + ramp, 0, top_of(bd))
    yy, xx = _yx((h, w))
    return (u[yy // 2, xx // 2].astype(_dt(bd)), u.astype(_dt(bd)), (top_of(bd) - u).astype(_dt(bd)))


def quadrants(w, h, bd, levels=(0, 1, 2)):
    """built for ties: every 64x64 luma tile (32x32 chroma) is four flat quadrants, the first of them four flat quarters again —

        b a | a a           a, b, c = the three of (0, mid, top) in the order `levels`
        c b | a a
        ----+----           The quadrant right of the first has no top neighbour inside the tile, so V, D45 and D67 all predict the
        c c | a a           one sample left of its first row (a): they tie, and V wins.  The one below it has no left neighbour: H
        c c | a a           and D203 predict the sample above its first column (c).  The last has a flat top edge (a) and a flat
                            left edge (c), and no top-right inside the tile: V, D45 and D67 tie again.

    This holds at block size 32, where a quadrant is a block; at 16 and 8 every block is flat and so is each of its edges, which ties
    whole families of candidates in most blocks, with DC among them wherever both edges have the same level."""
    vals = (0, 128 << (bd - 8), top_of(bd))
    a, b, c = (vals[i] for i in levels)
    out = []
    for i, s in enumerate(_planes(w, h)):
        T = 64 if i == 0 else 32
        y, x = _yx(s)
        ty, tx = y % T, x % T
        right, low = tx >= T // 2, ty >= T // 2
        first = np.where((tx >= T // 4) == (ty >= T // 4), b, np.where(tx >= T // 4, a, c))
        out.append(np.where(right, a, np.where(low, c, first)).astype(_dt(bd)))
    return tuple(out)


def ramps(w, h, bd, seed=6):
    """smooth content: per 16x16 luma cell a bilinear patch between four random corner levels — what SMOOTH, SMOOTH_V and SMOOTH_H
    predict well, so that their neighbours take edge filter type 1"""
    rng = np.random.default_rng([seed, bd, w, h])
    out = []
    for i, s in enumerate(_planes(w, h)):
        T = 16 if i == 0 else 8
        k = rng.integers(0, top_of(bd) + 1, (s[0] // T + 2, s[1] // T + 2)).astype(np.int64)
        y, x = _yx(s)
        cy, cx, fy, fx = y // T, x // T, y % T, x % T
        v = (k[cy, cx] * (T - fy) * (T - fx) + k[cy, cx + 1] * (T - fy) * fx + k[cy + 1, cx] * fy * (T - fx) + k[cy + 1, cx + 1] * fy * fx) // (T * T)
        out.append(v.astype(_dt(bd)))
    return tuple(out)


_SM_WEIGHTS = {4: (255, 149, 85, 64), 8: (255, 197, 146, 105, 73, 50, 37, 32)}      # AV1 spec 7.11.2.6, Sm_Weights_Tx_4x4 / _8x8


def smooth_steps(w, h, bd, seed=14):
    """built for ties under edge filter type 1 at block size 8: cells of 8x8 luma (4x4 chroma) samples, three to a period across and
    two down, with random levels A and B per period —

        A A B | A' A' B' |         S = what SMOOTH_V predicts from a flat top edge B and a flat left edge A, so SMOOTH_V wins there;
        A A S | A' A' S' |         the flat cell right of it then has a smooth-predicted left neighbour (filter type 1) and a flat
                                   top edge of its own level that goes on over its top-right: V, D45 and D67 tie, and V wins."""
    rng = np.random.default_rng([seed, bd, w, h])
    out = []
    for i, s in enumerate(_planes(w, h)):
        T = 8 if i == 0 else 4
        y, x = _yx(s)
        cy, cx = y // T, x // T
        lv = rng.integers(0, top_of(bd) + 1, (2, s[0] // (2 * T) + 1, s[1] // (3 * T) + 1)).astype(np.int64)
        A, B = lv[0][cy // 2, cx // 3], lv[1][cy // 2, cx // 3]
        wt = np.array(_SM_WEIGHTS[T], np.int64)[y % T]
        S = (wt * B + (256 - wt) * A + 128) >> 8
        out.append(np.where(cx % 3 < 2, A, np.where(cy % 2 == 0, B, S)).astype(_dt(bd)))
    return tuple(out)


NAMES = ("noise", "binary", "checker2", "checker1", "stripes", "stripes_across", "diag", "flat0", "flat_top", "uv_negative",
         "quadrants012", "quadrants201", "ramps", "smooth_steps")


def clip(name, w, h, bd):
    """a clip by name: the generators' names, 'checker1' / 'checker2' (the cell), 'stripes_across', 'quadrantsABC' (the levels),
    'noise#seed'"""
    if name.startswith("noise#"):
        return noise(w, h, bd, seed=int(name.split("#")[1]))
    if name.startswith("checker"):
        return checker(w, h, bd, cell=int(name[7:]))
    if name == "stripes_across":
        return stripes(w, h, bd, across=True)
    if name.startswith("quadrants"):
        return quadrants(w, h, bd, tuple(int(ch) for ch in name[9:]))
    if name == "low_bits":
        return low_bits(w, h)
    return globals()[name](w, h, bd)


def stacked_names(bd):
    """the clips as frames of one job: 14 at 8 bits, 15 at 10.  With 6 tiles a frame that is 84 / 90 tiles — no multiple of the 8, 16
    or 32 tiles of a workgroup: the last workgroup of a job is a partial one at every block size"""
    return list(NAMES) + (["low_bits"] if bd == 10 else [])


def stack(clips):
    """clips [(Y, U, V), ...] of one size -> (Y, U, V) with [frames, h, w] arrays, the layout of intra_encode_arrays"""
    return tuple(np.stack([c[i] for c in clips]) for i in range(3))
