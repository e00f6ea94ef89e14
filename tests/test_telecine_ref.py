"""CPU tests of inverse telecine (-av1mi_ivtc, av1mi_gop_config.telecine): the definition of include/av1mi.h as tests/telecine_ref.py
restates it gives the film back from its pulldown — both field orders, every phase, with and without noise; the host's planner
(host/telecineplan.hpp through av1mi_plan_telecine) is that plan, whole or cut into runs with context; the output's rate and count
(host/fieldrate.hpp) and the command line's argument rules."""
import numpy as np
import pytest

import telecine_ref as T

W, H = 64, 48
FILM = 8                    # film frames of a case = 10 video frames
V0 = 10                     # the cases are cut from an endless pulldown: own frames start at V0 + phase, one context frame on either side
CASES = [(order, phase) for order in ("tff", "bff") for phase in range(5)]


@pytest.fixture(scope="module")
def A():
    import av1stream
    return av1stream


def _run(order, first, n, noise=None):
    """luma of video frames first .. first + n - 1, optionally with independent noise of +-2 codes on every video frame"""
    Y = np.stack([T.video_frame(v, order, W, H)[0] for v in range(first, first + n)]).astype(np.int64)
    if noise is not None:
        Y = np.clip(Y + noise.integers(-2, 3, Y.shape), 0, 255)
    return Y.astype(np.uint8)


def _expected_film(order, first, n):
    """the film frames n own video frames starting at `first` carry, in order: the film frame of every bottom field, repeats dropped"""
    out = []
    for v in range(first, first + n):
        b = T.video_sources(v, order)[1]
        if b != T.video_sources(v - 1, order)[1]:
            out.append(b)
    return out


@pytest.mark.parametrize("order, phase", CASES)
@pytest.mark.parametrize("noisy", [False, True])
def test_the_plan_gives_the_film_back(A, order, phase, noisy):
    first, n = V0 + phase, FILM * 5 // 4
    clean = _run(order, first - 1, n + 2)
    Y = _run(order, first - 1, n + 2, np.random.default_rng(100 + phase)) if noisy else clean
    rec = T.records(Y, 8, W, H)
    top, bottom = T.plan(rec, 1, 1)
    want = _expected_film(order, first, n)
    assert len(want) == FILM and want == list(range(want[0], want[0] + FILM))      # none repeated, none missing
    assert len(top) == FILM == T.outputs(n)
    for k in range(FILM):
        film = T.film_frame(want[k], W, H)[0]
        woven = T.weave_plane(clean[top[k]], clean[bottom[k]], W, H)
        assert (woven == film).all(), (order, phase, k, int(top[k]), int(bottom[k]))
    # the host's planner is the same plan
    ht, hb = A.plan_telecine(rec, 1, 1)
    assert ht.tolist() == top.tolist() and hb.tolist() == bottom.tolist()


@pytest.mark.parametrize("order, phase", CASES)
def test_the_margins_hold_under_noise(order, phase):
    """what the plan decides on has room: under +-2 codes of noise the right candidate's comb stays below a quarter of every wrong one's,
    and a repeated bottom field's bdiff below a quarter of every other's"""
    first, n = V0 + phase, 10
    rec = T.records(_run(order, first - 1, n + 2, np.random.default_rng(7 + phase)), 8, W, H)
    for i in range(1, n + 1):
        v = first - 1 + i
        t, b = T.video_sources(v, order)
        cands = [T.video_sources(v + d, order)[0] for d in (-1, 0, 1)]
        right = [j for j in range(3) if cands[j] == b]
        wrong = [j for j in range(3) if cands[j] != b]
        assert right
        for j in wrong:
            assert 4 * max(int(rec["comb"][i][r]) for r in right) < int(rec["comb"][i][j])
    rep = [i for i in range(1, n + 1) if T.video_sources(first - 1 + i, order)[1] == T.video_sources(first - 2 + i, order)[1]]
    other = [i for i in range(1, n + 1) if i not in rep]
    assert len(rep) == 2 and 4 * max(int(rec["bdiff"][i]) for i in rep) < min(int(rec["bdiff"][i]) for i in other)


@pytest.mark.parametrize("run", [5, 10, 20])
@pytest.mark.parametrize("order, phase", [("tff", 1), ("tff", 3), ("bff", 2), ("bff", 4)])
def test_cut_into_runs_with_context_is_the_plan_of_one_run(A, run, order, phase):
    n = 40
    Y = _run(order, phase, n, np.random.default_rng(3))
    top, bottom = A.plan_telecine(T.records(Y, 8, W, H), 0, 0)
    assert len(top) == T.outputs(n)
    got_t, got_b = [], []
    for a in range(0, n, run):
        front, back = int(a > 0), int(a + run < n)
        rec = T.records(Y[a - front: a + run + back], 8, W, H)
        t, b = A.plan_telecine(rec, front, back)
        rt, rb = T.plan(rec, front, back)
        assert t.tolist() == rt.tolist() and b.tolist() == rb.tolist()
        got_t += (t + a - front).tolist()
        got_b += (b + a - front).tolist()
    assert got_t == top.tolist() and got_b == bottom.tolist()


def test_without_context_the_ends_clamp():
    """a run cut without its context codes a combed frame where the film frame's top field lies across the cut: the reason for the context"""
    Y = _run("tff", 0, 15)
    whole_t, whole_b = T.plan(T.records(Y, 8, W, H))
    cut_t, cut_b = T.plan(T.records(Y[:3], 8, W, H))      # video frame 2 holds film 1's top and film 2's bottom; film 2's top is in frame 3
    assert whole_t[2] == 3 and cut_t[2] == 2 and cut_b[2] == whole_b[2] == 2


@pytest.mark.parametrize("tail", [1, 2, 3, 4])
def test_a_tail_drops_none(A, tail):
    n = 10 + tail
    rec = T.records(_run("bff", 2, n), 8, W, H)
    top, bottom = A.plan_telecine(rec)
    rt, rb = T.plan(rec)
    assert top.tolist() == rt.tolist() and bottom.tolist() == rb.tolist()
    assert len(top) == T.outputs(n) == 8 + tail and bottom[-tail:].tolist() == list(range(10, n))
    only = T.records(_run("bff", 2, tail), 8, W, H)
    assert A.plan_telecine(only)[1].tolist() == list(range(tail))


def test_a_still_sequence_matches_c_and_drops_the_first_of_each_cycle(A):
    Y = np.repeat(T.film_frame(3, W, H)[0][None], 12, axis=0)
    rec = T.records(Y, 8, W, H)
    assert (rec["comb"] == rec["comb"][:, :1]).all() and (rec["bdiff"][1:] == 0).all() and int(rec["bdiff"][0]) == T.NO_PREDECESSOR
    for planner in (T.plan, A.plan_telecine):
        top, bottom = planner(rec, 1, 1)                   # own frames 1 .. 10: frames 1 and 6 are dropped
        assert top.tolist() == bottom.tolist() == [2, 3, 4, 5, 7, 8, 9, 10]
        top, bottom = planner(rec[:10], 0, 0)              # frame 0 of a run has no predecessor: the first cycle's first tie is frame 1
        assert top.tolist() == bottom.tolist() == [0, 2, 3, 4, 6, 7, 8, 9]


def test_the_planner_refuses_bad_arguments(A):
    rec = np.zeros(3, T.TELECINE_DTYPE)
    for front, back in ((2, 0), (0, 2), (-1, 0)):
        with pytest.raises(ValueError):
            A.plan_telecine(rec, front, back)
    with pytest.raises(ValueError):
        A.plan_telecine(rec[:1], 1, 1)
    assert A.plan_telecine(rec[:2], 1, 1)[0].size == 0


def test_small_heights():
    """h <= 3 has no eligible line (y = 2 needs line 3): comb = 0; h = 4 has one"""
    rng = np.random.default_rng(1)
    Y = rng.integers(0, 256, (3, 8, 16)).astype(np.uint8)
    for h in (2, 3):
        assert (T.records(Y, 8, 16, h)["comb"] == 0).all()
    r = T.records(Y, 8, 16, 4)
    m = Y.astype(np.int64)
    want = np.maximum(0, np.abs(2 * m[0, 2] - m[1, 1] - m[1, 3]) - np.abs(m[1, 1] - m[1, 3]) - 8).sum()
    assert int(r["comb"][1][0]) == int(want) and int(r["bdiff"][1]) == int(np.abs(m[1, 1::2][:2] - m[0, 1::2][:2]).sum())


# ---------------------------------------------------------------------------------------------- rate, count, argv
BASE = ["-i", "in.y4m", "-global_quality:v:0", 110]
IVTC = ["-av1mi_ivtc", 1, "-g", 8]


def test_the_jobs_output_rate_and_count(A):
    for interlace in "ptbm":
        for n, want in ((0, 0), (4, 4), (5, 4), (9, 8), (10, 8), (-1, -1)):
            per, rate, frames, ratio = A.job_output_ratio(BASE + IVTC + ["out.ivf"], interlace, (30000, 1001), n)
            assert (per, rate, frames, ratio) == (1, (24000, 1001), want, (4, 5))
            assert A.job_output(BASE + IVTC + ["out.ivf"], interlace, (30000, 1001), n) == (1, (24000, 1001), want)
    assert A.job_output_ratio(BASE + IVTC + ["out.ivf"], "p", (30, 1), 10)[1] == (24, 1)
    assert A.job_output_ratio(BASE + IVTC + ["out.ivf"], "p", (25, 1), 10)[1] == (20, 1)
    # without the option: as ever, with the ratio said
    assert A.job_output_ratio(BASE + ["out.ivf"], "t", (30000, 1001), 9) == (1, (30000, 1001), 9, (1, 1))
    assert A.job_output_ratio(BASE + ["-av1mi_ivtc", 0, "out.ivf"], "m", (30000, 1001), 9) == (1, (30000, 1001), 9, (1, 1))
    assert A.job_output_ratio(BASE + ["-av1mi_deinterlace", "auto", "-av1mi_deinterlace_rate", "field", "out.ivf"], "t", (30000, 1001), 9) == (2, (60000, 1001), 18, (2, 1))


@pytest.mark.parametrize("extra, want", [([], 0), (["-av1mi_ivtc", 0], 0), (IVTC, 1), (["-av1mi_ivtc", 1, "-g", 4], 1), (["-g", 256, "-av1mi_ivtc", 1], 1),
                                         (IVTC + ["-av1mi_crop", "32:32:0:0"], 1), (IVTC + ["-av1mi_depth", 8], 1), (["-av1mi_ivtc", 0, "-g", 7, "-av1mi_scenecut", 15], 0)])
def test_argv_accepted(A, extra, want):
    assert A.parse_ivtc_option(BASE + extra + ["out.ivf"]) == want


@pytest.mark.parametrize("extra, names", [
    (["-av1mi_ivtc", 2], "-av1mi_ivtc"), (["-av1mi_ivtc", "on"], "on"),
    (["-av1mi_ivtc", 1], "-g 30"), (["-av1mi_ivtc", 1, "-g", 6], "-g 6"), (["-av1mi_ivtc", 1, "-g", 7], "multiple of 4"),
    (IVTC + ["-av1mi_deinterlace", "auto"], "-av1mi_deinterlace"), (IVTC + ["-av1mi_deinterlace", "tff"], "-av1mi_deinterlace"),
    (IVTC + ["-vf:v:0", "yadif"], "-av1mi_deinterlace"),
    (IVTC + ["-av1mi_denoise", 4], "-av1mi_denoise"), (IVTC + ["-av1mi_pack10", 1], "-av1mi_pack10 1"), (IVTC + ["-av1mi_scenecut", 15], "-av1mi_scenecut"),
    (IVTC + ["-vf:v:0", "fieldmatch"], "fieldmatch"), (IVTC + ["-vf:v:0", "fieldmatch,decimate"], "fieldmatch"), (IVTC + ["-vf:v:0", "decimate"], "decimate"),
    (IVTC + ["-vf:v:0", "pullup"], "pullup"), (IVTC + ["-vf:v:0", "detelecine"], "detelecine"), (["-vf:v:0", "pullup"], "pullup"),
])
def test_argv_refused_with_a_message_that_names_the_argument(A, extra, names):
    with pytest.raises(ValueError) as e:
        A.parse_ivtc_option(BASE + extra + ["out.ivf"])
    assert "Invalid argument" in str(e.value) and names in str(e.value)
    code, text = A.run_transcode([str(a) for a in BASE + extra] + ["out.ivf"])      # the job says the same and runs nothing
    assert code == 1 and names in text
