"""The deblocking search's candidate levels (include/av1mi.h "deblocking search") against their restatement (lf_search_ref.py), the two
refusals, and the restatement itself: a flat frame picks (0, 0), and the inputs the GPU test shares make it choose differently.  CPU only."""
import numpy as np
import pytest

import lf_search_ref as R


def _params(av1mi, levels, bd=8):
    p = av1mi.policy_frame_params(100, bd, 0)
    for i, v in enumerate(levels):
        p.lf_level[i] = v
    return p


def test_candidate_tables():
    want = {0: ([0, 1, 1, 1, 1, 1, 1, 1], [0] * 8),
            1: ([1, 1, 1, 1, 1, 2, 2, 3], [1, 0, 1, 1, 1, 2, 2, 3]),
            6: ([6, 1, 3, 5, 8, 9, 12, 18], [6, 0, 3, 5, 8, 9, 12, 18]),
            31: ([31, 1, 16, 23, 39, 47, 62, 63], [31, 0, 16, 23, 39, 47, 62, 63]),
            63: ([63, 1, 32, 47, 63, 63, 63, 63], [63, 0, 32, 47, 63, 63, 63, 63])}
    for L, (luma, chroma) in want.items():
        assert [R.level(L, c, False) for c in range(8)] == luma, L
        assert [R.level(L, c, True) for c in range(8)] == chroma, L


@pytest.mark.parametrize("L", [0, 1, 6, 31, 63])
def test_library_levels_equal_the_restatement(av1mi, L):
    for P in ((L, L, L, L), (L, max(L - 1, 0) if L else 0, L // 2, L // 2), (L, L, 0, 0)):
        p = _params(av1mi, P)
        for c in range(8):
            assert av1mi.lf_search_levels(p, c) == R.levels(P, c), (P, c)
    assert av1mi.lf_search_levels(_params(av1mi, (L, L, L, L)), 0) == [L] * 4
    assert av1mi.LF_SEARCH_CANDIDATES == len(R.M) == 8


def test_the_two_refusals_and_the_range(av1mi):
    for P in ((10, 10, 5, 6), (0, 0, 3, 3)):
        with pytest.raises(ValueError):
            R.levels(P, 0)
        with pytest.raises(ValueError):
            av1mi.lf_search_levels(_params(av1mi, P), 0)
    ok = _params(av1mi, (10, 10, 5, 5))
    for c in (-1, 8):
        with pytest.raises(ValueError):
            av1mi.lf_search_levels(ok, c)
    assert av1mi.lf_search_levels(_params(av1mi, (0, 3, 3, 3)), 0) == [0, 3, 3, 3]      # one luma level is enough to carry chroma
    assert av1mi.lf_search_scratch_bytes(136, 72, 3) == 3 * 3 * 2 * 16 * 8 and av1mi.lf_search_scratch_bytes(0, 72, 3) == 0


def test_patch_holds_the_words_that_carry_bit_24():
    mi = np.array([[3 | 3 << 4 | 9 << 8 | 7 << 16 | 3 << 25, 3 | 3 << 4 | 1 << 24, 0xFFFFFFFF]], np.uint32)
    assert R.patched(mi, 20, 14).tolist() == [[3 | 3 << 4 | 20 << 8 | 14 << 16 | 3 << 25, 3 | 3 << 4 | 1 << 24, 0xFFFFFFFF]]


@pytest.mark.parametrize("bd", [8, 10])
def test_a_flat_frame_picks_0_0(O, bd):
    w, h = 64, 64
    flat = [np.full((h >> (p > 0), w >> (p > 0)), 77 << (bd - 8), np.uint8 if bd == 8 else np.uint16) for p in range(3)]
    mi_y, mi_c = R.base_maps(w, h)
    sse, choice, lv, _ = R.search(O, flat, flat, bd, R.POLICY, 0, mi_y, mi_c)
    assert not sse.any() and choice == [0, 0] and lv == list(R.POLICY)


@pytest.mark.parametrize("bd", [8, 10])
def test_the_shared_inputs_make_the_reference_choose_differently(O, bd):
    """what keeps the GPU test from passing on "always 0": over the frames of its inputs at least three luma and two chroma indices"""
    luma, chroma = set(), set()
    for w, h, true_size in R.SIZES:
        src, rec = R.frames(w, h, bd)
        for key32 in (False, True):
            mi_y, mi_c = R.base_maps(w, h, true_size, key32)
            for f in range(3):
                _, choice, _, _ = R.search(O, [a[f] for a in rec], [a[f] for a in src], bd, R.POLICY, 0, mi_y, mi_c, true_size)
                luma.add(choice[0]); chroma.add(choice[1])
    assert len(luma) >= 3 and len(chroma) >= 2, (sorted(luma), sorted(chroma))
