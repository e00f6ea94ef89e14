"""The CDEF search's candidate sets (include/av1mi.h "CDEF search") against their restatement (cdef_search_ref.py), and the
restatement's pick: the tie rule and the all-skipped rule.  CPU only."""
import numpy as np
import pytest

import cdef_search_ref as R


def test_sets_equal_the_restatement_for_every_quantiser(av1mi):
    for bd in (8, 10):
        for ft in (0, 1):
            for q in list(range(0, 256, 5)) + [255]:
                p = av1mi.policy_frame_params(q, bd, ft)
                for bits in (1, 2, 3):
                    y, uv = av1mi.cdef_search_sets(p, bits)
                    assert (y, uv) == R.sets(p, bits), (bd, ft, q, bits)
                    # set 0 is the policy's, set 1 is zero, nothing behind the last set, every byte inside the syntax's 4 + 2 bits
                    assert y[0] == p.cdef_y and uv[0] == p.cdef_uv and y[1] == uv[1] == 0
                    assert not any(y[1 << bits:]) and not any(uv[1 << bits:]) and max(y + uv) < 64


def test_bits_outside_1_to_3_are_refused(av1mi):
    p = av1mi.policy_frame_params(100, 8, 0)
    for bits in (0, 4, -1):
        with pytest.raises(ValueError):
            av1mi.cdef_search_sets(p, bits)


def test_the_arithmetic_of_the_sets():
    assert [R.dbl(x) for x in (0, 1, 7, 8, 15)] == [1, 2, 14, 15, 15] and [R.up(x) for x in range(4)] == [1, 2, 3, 3]
    # P = 2, S = 1: (2,1) (0,0) (1,1) (4,1) (2,2) (2,0) (4,2) (8,2)
    assert R.sets_of((2 << 2) | 1, 3) == [9, 0, 5, 17, 10, 8, 18, 34]
    # a policy set of zero: candidates 0, 1, 2 and 5 are the same set, and stay in place
    assert R.sets_of(0, 3) == [0, 0, 0, 4, 1, 0, 5, 9]


def test_pick_takes_the_lowest_sum_and_the_lowest_index_on_a_tie():
    t = np.array([[100, 90, 90, 500, 90, 90, 90, 90], [10, 10, 10, 10, 10, 10, 10, 10], [7, 5, 3, 3, 0, 0, 0, 0]], np.uint64)
    assert R.pick(t, 3).tolist() == [1, 0, 4]
    assert R.pick(t, 2).tolist() == [1, 0, 2]      # columns from 1 << bits on hold 0 and do not take part
    assert R.pick(t, 1).tolist() == [1, 0, 1]


@pytest.mark.parametrize("bd", [8, 10])
def test_an_all_skipped_superblock_gets_index_0(av1mi, O, bd):
    """skipped blocks are left unfiltered, so every candidate leaves an all-skipped superblock as it is: all sums tie, index 0"""
    w, h, bits = 128, 64, 3
    p = av1mi.policy_frame_params(128, bd, 1)
    src, dbl = R.content(np.random.default_rng(3), w, h, bd)
    y, uv = R.sets(p, bits)
    skip = np.zeros((h // 8, w // 8), np.uint8)
    free = R.pick(R.table(O, dbl, src, bd, p.cdef_damping, y, uv, bits, skip), bits)
    assert free[0] != 0                             # (the ringing superblock wants a filter)
    skip[:, :8] = 1
    t = R.table(O, dbl, src, bd, p.cdef_damping, y, uv, bits, skip)
    assert len(set(t[0].tolist())) == 1 and R.pick(t, bits)[0] == 0 and R.pick(t, bits)[1] == free[1]
