"""The denoise plan (av1-go_amd/host/noiseplan.hpp through av1mi_plan_denoise) == its numpy twin (tests/noise_ref.py) on hand-made
histograms, and the plan on synthetic content: the estimate's error against the true sigma, a clean clip, a clip that pans as a whole.
No GPU."""
import numpy as np
import pytest

import noise_ref as R


def _rec(bins, blocks=None, eligible=None):
    """a record from {bin: count}"""
    r = np.zeros((), R.NOISE_DTYPE)
    for b, n in bins.items():
        r["hist"][b] = n
    r["eligible"] = int(r["hist"].sum()) if eligible is None else eligible
    r["blocks"] = int(r["eligible"]) if blocks is None else blocks
    return r


def _both(recs):
    """the plan from C and from numpy, which must agree: (strength, levels, s16)"""
    import av1stream
    recs = np.array(recs, R.NOISE_DTYPE) if len(recs) else np.zeros(0, R.NOISE_DTYPE)
    k, q, s16 = av1stream.plan_denoise(recs)
    want = R.plan(recs)
    assert (k, q.tolist(), s16) == want, ((k, q.tolist(), s16), want)
    return want


def test_quartile_index():
    """the smallest bin whose cumulative count reaches ceil(counted / 4): counted 1, 4 and 5"""
    assert _both([_rec({40: 1})])[1] == [40]
    assert _both([_rec({10: 1, 20: 1, 30: 1, 40: 1})])[1] == [10]          # ceil(4 / 4) = 1: the first block
    assert _both([_rec({10: 1, 20: 1, 30: 1, 40: 1, 50: 1})])[1] == [20]   # ceil(5 / 4) = 2: the second
    assert _both([_rec({10: 1, 20: 4})])[1] == [20]
    assert _both([_rec({0: 3, 254: 9})])[1] == [0] and _both([_rec({0: 2, 254: 7})])[1] == [254]
    # bin 255 is no part of the percentile: 5 counted, the second of them
    assert _both([_rec({10: 1, 20: 1, 30: 3, 255: 15})])[1] == [20]


def test_pair_validity():
    assert _both([_rec({30: 25, 255: 75})])[1] == [30]      # 4 x 25 >= 100
    assert _both([_rec({30: 24, 255: 76})])[1] == [-1]      # 4 x 24 < 100: moving
    assert _both([_rec({30: 6}, blocks=96)])[1] == [30]     # eligible 6 >= floor(96 / 16)
    assert _both([_rec({30: 6}, blocks=112)])[1] == [-1]    # 6 < 7: almost everything is outside the range
    assert _both([_rec({}, blocks=8)])[1] == [-1]           # nothing counted, though 0 >= floor(8 / 16)
    assert _both([_rec({}, blocks=1000)])[1] == [-1]        # the all-zero histogram
    assert _both([_rec({255: 1000})]) == (0, [-1], -1)      # everything moved


def test_no_valid_pair_plans_0():
    assert _both([]) == (0, [], -1)
    assert _both([_rec({255: 50}), _rec({100: 1, 255: 50})]) == (0, [-1, -1], -1)


def test_file_level_index():
    """the valid pairs' levels sorted ascending, index floor((n - 1) / 4): n = 1, 4, 5, 16, and invalid pairs do not count"""
    def levels(qs):
        return [_rec({q: 10}) if q >= 0 else _rec({255: 10}) for q in qs]
    s = lambda q: R.sigma16(q)
    assert _both(levels([90]))[2] == s(90)
    assert _both(levels([90, 50, 70, 60]))[2] == s(50)               # index 0
    assert _both(levels([90, 50, 70, 60, 80]))[2] == s(60)           # index 1
    assert _both(levels(list(range(100, 100 + 16))[::-1]))[2] == s(103)      # index 3
    assert _both(levels([-1, 90, -1, 50, 70, -1, 60, 80, -1]))[2] == s(60)


def test_floor_and_cap():
    """s16 = 7 plans 0 and 8 plans 1; ceil(1.5 sigma); the cap at 16"""
    q7, q8 = 8, 9
    assert (R.sigma16(q7), R.sigma16(q8)) == (7, 8)
    assert _both([_rec({q7: 10})]) == (0, [q7], 7)
    assert _both([_rec({q8: 10})]) == (1, [q8], 8)
    assert [R.strength(v) for v in (0, 7, 8, 10, 11, 16, 21, 22, 32, 64, 128, 160, 170, 171, 225)] == [0, 0, 1, 1, 2, 2, 2, 3, 3, 6, 12, 15, 16, 16, 16]
    assert _both([_rec({254: 10})]) == (16, [254], 225)
    for q in range(255):
        assert _both([_rec({q: 3})])[0] == R.strength(R.sigma16(q))


W, H, PAIRS = 192, 128, 4


def _estimate(sigma, pan=(0, 0), half=False, seed=7):
    Y = R.clip(W, H, 2 * PAIRS, sigma, seed, pan)
    if half:      # the right half of the picture stands still
        Y[:, :, W // 2:] = R.clip(W, H, 2 * PAIRS, sigma, seed + 1)[:, :, W // 2:]
    return _both(R.records(R.sample(Y), 8, W, H))


@pytest.mark.parametrize("sigma", [1, 2, 4, 8])
def test_still_texture_under_noise(sigma):
    """the estimate lies within -15 % .. +5 % of the true sigma (the low side: the lower quartile's bias on pure noise)"""
    k, levels, s16 = _estimate(sigma)
    assert all(q >= 0 for q in levels)
    print("sigma %g: estimate %.3f, strength %d" % (sigma, s16 / 16, k))
    assert 0.85 * sigma <= s16 / 16 <= 1.05 * sigma, (sigma, s16 / 16)
    assert k == R.strength(s16) and int(np.ceil(1.5 * 0.85 * sigma)) <= k <= int(np.ceil(1.5 * 1.05 * sigma))


@pytest.mark.parametrize("sigma", [2, 8])
def test_half_the_picture_panning(sigma):
    """motion in half the picture only adds to S: the still half carries the quartile"""
    k, levels, s16 = _estimate(sigma, pan=(5, 3), half=True)
    assert all(q >= 0 for q in levels) and 0.85 * sigma <= s16 / 16 <= 1.05 * sigma, (sigma, s16 / 16)


def test_clean_still_clip_plans_0():
    k, levels, s16 = _estimate(0)
    assert (k, s16) == (0, 0) and levels == [0] * PAIRS


@pytest.mark.parametrize("sigma", [0, 4])
def test_clip_panning_as_a_whole_plans_0(sigma):
    """every block lands in bin 255: no pair is valid.  (Without the `counted` rule a clean panning clip would plan strength 16.)"""
    k, levels, s16 = _estimate(sigma, pan=(5, 3))
    assert (k, levels, s16) == (0, [-1] * PAIRS, -1)
