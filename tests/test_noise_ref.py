"""tests/noise_ref.py on built cases (include/av1mi.h "noise records"): the eligibility bounds, the bins' edges, the blocks of a true size
that is no multiple of 8, and the depths.  No GPU: the kernel is pinned against the same file in tests/test_gpu_noise.py."""
import numpy as np

import noise_ref as R


def _pair_with_block(level_sum=None, diff_sum=0, bd=8):
    """one 8x8 pair: A's samples sum to level_sum, |A - B| sums to diff_sum (8-bit terms)"""
    a = np.full(64, level_sum // 64, np.int64)
    a[:level_sum - a.sum()] += 1
    assert a.sum() == level_sum
    d = np.full(64, diff_sum // 64, np.int64)
    d[:diff_sum - d.sum()] += 1
    b = np.where(a + d <= 255, a + d, a - d)
    assert np.abs(a - b).sum() == diff_sum
    dt = np.uint8 if bd == 8 else np.uint16
    return (a.reshape(8, 8) << (bd - 8)).astype(dt), (b.reshape(8, 8) << (bd - 8)).astype(dt)


def test_eligibility_bounds_are_inclusive():
    for m, ok in ((16 * 64, 1), (16 * 64 - 1, 0), (235 * 64, 1), (235 * 64 + 1, 0), (0, 0), (255 * 64, 0), (128 * 64, 1)):
        a, b = _pair_with_block(m)
        r = R.pair_record(a, b, 8, 8, 8)
        assert (int(r["eligible"]), int(r["blocks"]), int(r["hist"].sum()), int(r["hist"][0])) == (ok, 1, ok, ok), m


def test_bin_edges():
    """S8 >> 2 of exactly 254, 255 and 300 land in bins 254, 255, 255; the last S of a bin and the first of the next"""
    for s, b in ((254 * 4, 254), (254 * 4 + 3, 254), (255 * 4, 255), (300 * 4, 255), (0, 0), (3, 0), (4, 1), (64 * 100, 255)):
        a, bb = _pair_with_block(100 * 64, s)
        r = R.pair_record(a, bb, 8, 8, 8)
        assert int(r["hist"][b]) == 1 and int(r["hist"].sum()) == 1, (s, b)


def test_true_size_that_is_no_multiple_of_8():
    """90 x 70 in 96 x 72 counts 11 x 8 blocks; garbage in the padding and in the partial blocks changes nothing"""
    Y = R.clip(96, 72, 2, 2.0, 3)
    base = R.pair_record(Y[0], Y[1], 8, 90, 70)
    assert int(base["blocks"]) == 11 * 8 and int(base["eligible"]) == 11 * 8 == int(base["hist"].sum())
    G = Y.copy()
    G[:, 64:, :] = 255      # the partial row of blocks and the padding rows
    G[:, :, 88:] = 0        # the partial column of blocks and the padding columns
    got = R.pair_record(G[0], G[1], 8, 90, 70)
    assert got.tobytes() == base.tobytes()
    assert int(R.pair_record(Y[0], Y[1], 8, 7, 70)["blocks"]) == 0


def test_depths_shifted_left_give_the_8_bit_record():
    Y = R.clip(64, 48, 4, 3.0, 4)
    Y[2:, :16] = 4      # below the range
    Y[2:, 48:] = 250    # above it
    want = R.records(Y, 8, 64, 48)
    assert 0 < int(want[1]["eligible"]) < int(want[1]["blocks"])
    for bd in (10, 12):
        assert R.records(Y.astype(np.uint16) << (bd - 8), bd, 64, 48).tobytes() == want.tobytes(), bd


def test_low_bits_of_a_deep_sample():
    """S is formed on native samples and shifted once: 64 differences of 3 at 10 bits are S = 192, S8 = 48, bin 12 — not 64 x (3 >> 2) = 0"""
    a = np.full((8, 8), 400, np.uint16)
    r = R.pair_record(a, a + 3, 10, 8, 8)
    assert int(r["hist"][12]) == 1
    # M on the m8 view of EACH sample: 32 x (63 >> 2) + 32 x (67 >> 2) = 992 is below the range, though (32 x 63 + 32 x 67) >> 2 = 1040 is not
    lo = np.full((8, 8), 63, np.uint16)
    lo[4:] = 67
    assert int(R.pair_record(lo, lo, 10, 8, 8)["eligible"]) == 0
    lo[:] = 64
    assert int(R.pair_record(lo, lo, 10, 8, 8)["eligible"]) == 1


def test_pair_slots():
    assert R.pair_slots(0) == [] and R.pair_slots(1) == [] and R.pair_slots(2) == [0] and R.pair_slots(3) == [0] and R.pair_slots(5) == [0, 1]
    assert R.pair_slots(32) == list(range(16)) and R.pair_slots(33) == list(range(16))
    s = R.pair_slots(1000)
    assert len(s) == 16 and s[0] == 0 and s[-1] == 499 and s == sorted(set(s))
    import av1stream
    for n in (0, 1, 2, 3, 4, 5, 8, 31, 32, 33, 34, 100, 1000, 100001):
        assert av1stream.noise_pair_slots(n) == R.pair_slots(n), n
