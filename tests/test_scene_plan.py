"""CPU tests of the scene-cut option's host side: the GOP planner (av1mi_plan_gops, host/sceneplan.hpp), the product's default
sensitivity on the two clips it was chosen on (tests/scene_clips.py through tests/scene_ref.py), and the command line's argument rules."""
import numpy as np
import pytest

import scene_clips as K
import scene_ref as R


@pytest.fixture(scope="module")
def A():
    import av1stream
    return av1stream


def check_plan(n, G, S, cut, min_len, K_, start, ln):
    m = min_len if min_len > 0 else max(1, G // 4)
    assert K_ == -(-n // G)
    assert start[0] == 0 and int(ln[:K_].sum()) == n
    for k in range(K_):
        assert ln[k] >= 1
        if k + 1 < K_:
            assert start[k + 1] == start[k] + ln[k]                 # a partition, in order
            assert m <= ln[k] <= G + G // 2
            assert abs(int(start[k + 1]) - (k + 1) * G) <= G // 2
        else:
            assert ln[k] <= G + G // 2                              # the last may be cut short by the end of the input
    assert (start[K_:] == n).all() and (ln[K_:] == 0).all()


def test_random_cut_patterns_give_ordered_partitions_within_the_bounds(A):
    rng = np.random.default_rng(20)
    for i in range(400):
        G, S = int(rng.integers(1, 33)), int(rng.integers(1, 7))
        n = int(rng.integers(1, S * G + 1))
        min_len = 0 if i % 3 else int(rng.integers(1, G - G // 2 + 1))
        cut = rng.random(n) < rng.choice([0.0, 0.05, 0.2, 0.6])
        K_, start, ln = A.plan_gops(n, G, S, cut, min_len)
        check_plan(n, G, S, cut, min_len, K_, start, ln)
        # every boundary that is not on its grid position is a cut
        for k in range(1, K_):
            assert start[k] == k * G or cut[start[k]]


def test_no_cuts_is_the_fixed_layout(A):
    for n, G, S in ((24, 8, 3), (20, 8, 3), (5, 8, 3), (12, 4, 4), (1, 1, 1), (31, 30, 2)):
        K_, start, ln = A.plan_gops(n, G, S, np.zeros(n, bool))
        assert list(start[:K_]) == [k * G for k in range(K_)]
        assert list(ln[:K_]) == [min(G, n - k * G) for k in range(K_)]


def test_a_single_cut_within_reach_becomes_a_start(A):
    G, S, n = 8, 3, 24
    for f in range(1, n):
        cut = np.zeros(n, bool)
        cut[f] = True
        K_, start, ln = A.plan_gops(n, G, S, cut)
        near = [k for k in (1, 2) if abs(f - k * G) <= G // 2]
        # frames 4 and 20 are in reach of one boundary, 12 of two: the first boundary asked takes it (12 is then too near for the second)
        want = [0, 8, 16]
        if near:
            want[near[0]] = f
        assert list(start[:K_]) == want, f
        check_plan(n, G, S, cut, 0, K_, start, ln)


def test_the_nearer_of_two_cuts_wins_and_ties_go_to_the_earlier(A):
    G, S, n = 8, 3, 24
    cut = np.zeros(n, bool)
    cut[[6, 9]] = True                    # 9 is nearer to 8 than 6
    assert list(A.plan_gops(n, G, S, cut)[1]) == [0, 9, 16]
    cut[:] = False
    cut[[5, 9]] = True
    assert list(A.plan_gops(n, G, S, cut)[1]) == [0, 9, 16]
    cut[:] = False
    cut[[7, 9]] = True                    # a tie: the earlier
    assert list(A.plan_gops(n, G, S, cut)[1]) == [0, 7, 16]
    cut[:] = False
    cut[[6, 17]] = True                   # the test clip of the GPU tests
    K_, start, ln = A.plan_gops(n, G, S, cut)
    assert list(start) == [0, 6, 17] and list(ln) == [6, 11, 7]


def test_min_len_keeps_cuts_near_the_previous_start_out(A):
    G, S, n = 8, 3, 24
    cut = np.zeros(n, bool)
    cut[[4, 5]] = True
    assert list(A.plan_gops(n, G, S, cut, 2)[1]) == [0, 5, 16]
    cut[:] = False
    cut[[12, 13]] = True                  # 12 goes to the first boundary; 13 is one frame later: too short a GOP at min_len 2
    assert list(A.plan_gops(n, G, S, cut, 2)[1]) == [0, 12, 16]
    assert list(A.plan_gops(n, G, S, cut, 1)[1]) == [0, 12, 13]
    # a GOP that started early does not also end late: 4 + 8 + 4 = 16 would be 12 frames
    cut[:] = False
    cut[[4, 20]] = True
    K_, start, ln = A.plan_gops(n, G, S, cut)
    assert list(start) == [0, 4, 16] and max(ln) <= G + G // 2


def test_windows_shorter_than_the_grid(A):
    K_, start, ln = A.plan_gops(5, 8, 3, np.array([0, 0, 0, 1, 0], bool))           # n < G: one GOP, a cut inside changes nothing
    assert K_ == 1 and list(start) == [0, 5, 5] and list(ln) == [5, 0, 0]
    cut = np.zeros(19, bool)
    cut[18] = True                                                                # n not a multiple of G; the last frame is a cut in reach of 16
    K_, start, ln = A.plan_gops(19, 8, 3, cut)
    assert K_ == 3 and list(start) == [0, 8, 18] and list(ln) == [8, 10, 1]


def test_bad_arguments_are_refused(A):
    for n, G, S, m in ((0, 8, 3, 0), (25, 8, 3, 0), (8, 0, 3, 0), (8, 8, 0, 0), (24, 8, 3, 5)):
        with pytest.raises(ValueError):
            A.plan_gops(n, G, S, np.zeros(max(n, 1), bool), m)


def test_cut_rule_matches_the_reference(A):
    import av1mi
    rec = np.zeros(1, av1mi.SCENE_DTYPE)
    for inter, intra in ((0, 0), (10, 0), (85, 100), (84, 100), (1, 1), (2 ** 40, 2 ** 40 + 5), (30, 100), (69, 100), (70, 100)):
        rec[0] = (inter, intra, 1, 0)
        for sc in (1, 15, 30, 50, 99):
            assert A.scene_is_cut(rec[0], sc) == R.is_cut(rec[0], sc)


def test_default_finds_every_built_cut_and_no_false_one(A):
    """pins AV1MI_SCENECUT_DEFAULT: the middle of the range of sensitivities that are right on both clips"""
    c = K.DEFAULT_CLIPS
    ranges = []
    for bd in (8, 10):
        Y = K.cut_clip(c["w"], c["h"], c["cut"]["n"], bd, c["cut"]["cuts"])[0]
        recs = R.records(Y, bd)
        assert R.cuts(recs, A.SCENECUT_DEFAULT) == list(c["cut"]["cuts"])
        assert recs["inter_sad"][0] == 0 and (recs["blocks"] == (c["w"] // 32) * (c["h"] // 32)).all()
        calm = dict(c["calm"])
        Y = K.calm_clip(c["w"], c["h"], calm.pop("n"), bd, **calm)[0]
        calm_recs = R.records(Y, bd)
        assert R.cuts(calm_recs, A.SCENECUT_DEFAULT) == []
        lo = max(R.cut_range(recs, c["cut"]["cuts"])[0], R.cut_range(calm_recs, [])[0])
        hi = min(R.cut_range(recs, c["cut"]["cuts"])[1], R.cut_range(calm_recs, [])[1])
        ranges.append((lo, hi))
    print("ranges of scenecut that are right on both clips (8 bit, 10 bit):", ranges)
    assert ranges[0] == (1, 30) and A.SCENECUT_DEFAULT == (ranges[0][0] + ranges[0][1]) // 2


def test_command_line_argument_rules(A, tmp_path):
    """the argument errors come before anything is opened; a valid line goes on to fail (or run) as any job does"""
    base = ["-i", tmp_path / "missing.y4m", "-g", 8]
    out = tmp_path / "o.ivf"
    for extra, text in ((["-av1mi_scenecut", "100"], "-av1mi_scenecut takes a sensitivity 1 .. 99"),
                        (["-av1mi_scenecut", "x"], "-av1mi_scenecut takes a sensitivity 1 .. 99"),
                        (["-av1mi_scenecut", "-3"], "-av1mi_scenecut takes a sensitivity 1 .. 99"),
                        (["-av1mi_scenecut", "15", "-av1mi_pack10", "1"], "not together with -av1mi_pack10 1"),
                        (["-av1mi_min_gop", "2"], "-av1mi_min_gop needs -av1mi_scenecut"),
                        (["-av1mi_scenecut", "15", "-av1mi_min_gop", "0"], "-av1mi_min_gop takes a length"),
                        (["-av1mi_scenecut", "15", "-av1mi_min_gop", "5"], "-av1mi_min_gop 5 above gop - gop / 2 = 4")):
        code, err = A.run_transcode(base + extra + [out])
        assert code == 1 and "Invalid argument" in err and text in err, (extra, err)
        assert not out.exists()
    # accepted: the failure is then the job's own (no device here, or no such input), never an argument error
    for extra in (["-av1mi_scenecut", "0"], ["-av1mi_scenecut", "15"], ["-av1mi_scenecut", "99", "-av1mi_min_gop", "4"], ["-av1mi_scenecut", "0", "-av1mi_pack10", "1"]):
        code, err = A.run_transcode(base + extra + [out])
        assert code != 0 and "Invalid argument" not in err, (extra, err)
