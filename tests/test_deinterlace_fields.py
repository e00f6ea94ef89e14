"""CPU tests of field-rate deinterlacing (-av1mi_deinterlace_rate field, av1mi_gop_config.deinterlace_fields): the numpy reference
(tests/deinterlace_fields_ref.py) has the properties include/av1mi.h states ("FIELD-RATE OUTPUT"), and the host's pure functions
(host/fieldrate.hpp) and argument parser behave as av1-go_amd/host/transcode.hpp says."""
import numpy as np
import pytest

import deint_clips as K
import deinterlace_fields_ref as F
import deinterlace_ref as R


def _planes(name, bd, k, n=None):
    """(plane [n, H, W], true w, true h) for the three planes of a case"""
    return [(a, w, h) for a, (w, h) in zip(K.case_clip(name, bd, k, n=n), K.case_true_sizes(name))]


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("name", list(K.CASES))
def test_first_fields_are_the_same_rate_filter_and_second_fields_its_time_reversal(name, bd, k):
    """(a) output 2 f is deinterlace_ref.run's frame f; (b) output 2 f + 1 is the same-rate filter on the reversed triple (N, C, P) with
    the opposite parity"""
    for a, w, h in _planes(name, bd, k):
        n = a.shape[0]
        out = F.fields(a, w, h, k)
        assert out.shape == (2 * n,) + a.shape[1:] and out.dtype == a.dtype
        assert (out[0::2] == R.run(a, w, h, k)).all(), name
        for f in range(n):
            P, N = a[max(f - 1, 0)], a[min(f + 1, n - 1)]
            assert (out[2 * f + 1] == R.plane(N, a[f], P, w, h, 1 - k)).all(), (name, f)
        assert (out[1::2, 1 - k:h:2, :w] == a[:, 1 - k:h:2, :w]).all(), "a second field's own lines are not kept"
        assert (out[1::2] != out[0::2]).any()


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("bd", [8, 10])
def test_a_still_clip_gives_the_weave_in_both_phases(bd, k):
    rng = np.random.default_rng(bd + k)
    for w, h in ((8, 8), (13, 7), (40, 1), (5, 2)):
        f = rng.integers(0, 1 << bd, (h, w)).astype(np.uint16)
        still = np.stack([f] * 3)
        assert (F.fields(still, w, h, k) == np.stack([f] * 6)).all(), "%dx%d: a still run changes" % (w, h)


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("bd", [8, 10])
def test_second_fields_lie_at_their_own_field_time(bd, k):
    """(d) the pan clip is sampled at field times: every output 2 f + 1 is nearer (SAD over the true size) to the progressive picture at
    field time 2 f + 1 than to the one at 2 f — and every output 2 f nearer to 2 f than to 2 f + 1"""
    w, h, n, seed = 192, 128, 6, 7
    Y = K.pan_plane(w, h, n, bd, k, seed)
    tex = K._canvas(w, h, 2 * n, bd, seed).astype(np.int64)      # the generator's canvas, from the same arguments
    at = lambda t: tex[K.PAN[1] * t:K.PAN[1] * t + h, K.PAN[0] * t:K.PAN[0] * t + w]
    out = F.fields(Y, w, h, k).astype(np.int64)
    sad = lambda o, t: int(np.abs(out[o] - at(t)).sum())
    for f in range(n):
        assert sad(2 * f + 1, 2 * f + 1) < sad(2 * f + 1, 2 * f), "frame %d: the second field's output lies at the first field's time" % f
        assert sad(2 * f, 2 * f) < sad(2 * f, 2 * f + 1), "frame %d: the first field's output lies at the second field's time" % f


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("bd", [8, 10])
def test_runs_of_one_and_two_frames(n, bd):
    """(e) the ends of a run are their own neighbours: a one-frame run has P = C = N, so m = 0 and both phases return the weave; the last
    frame of a longer run sees t0 = t1 = C in its second field"""
    for k in (0, 1):
        for a, w, h in _planes("8x8", bd, k, n=n):
            out = F.fields(a, w, h, k)
            assert out.shape[0] == 2 * n
            assert (out[0::2] == R.run(a, w, h, k)).all()
            for f in range(n):
                assert (out[2 * f + 1] == R.plane(a[min(f + 1, n - 1)], a[f], a[max(f - 1, 0)], w, h, 1 - k)).all()
            if n == 1:
                assert (out == np.stack([a[0]] * 2)).all(), "a one-frame run is the weave in both phases"
            else:
                last = F.field(a[0], a[1], a[1], w, h, k, 1)      # the last frame's second field: t0 = t1 = C
                assert (out[3] == last).all()


# ---------------------------------------------------------------------------------------------- rate, count, cuts
BASE = ["-i", "in.y4m", "-global_quality:v:0", 110]
FIELD = ["-av1mi_deinterlace_rate", "field"]


@pytest.mark.parametrize("extra, interlace, want", [
    (["-av1mi_deinterlace", "auto"] + FIELD, "t", 2), (["-av1mi_deinterlace", "auto"] + FIELD, "b", 2), (["-av1mi_deinterlace", "tff"] + FIELD, "p", 2),
    (["-av1mi_deinterlace", "bff"] + FIELD, "t", 2), (["-vf:v:0", "yadif"] + FIELD, "t", 2),
    (["-av1mi_deinterlace", "auto"] + FIELD, "p", 1),                                  # a progressive source under auto: as ever
    (FIELD, "t", 1), (["-av1mi_deinterlace", "off"] + FIELD, "t", 1),                  # nothing is deinterlaced
    (["-av1mi_deinterlace", "auto"], "t", 1), (["-av1mi_deinterlace", "auto", "-av1mi_deinterlace_rate", "frame"], "t", 1), ([], "p", 1),
])
def test_the_jobs_output_rate_and_count(extra, interlace, want):
    """(f) one function gives the output's frame rate and count"""
    import av1stream
    for fps, n in (((30000, 1001), 17), ((25, 1), 1), ((30, 1), 0), ((24000, 1001), -1)):
        per, rate, frames = av1stream.job_output(BASE + extra + ["out.ivf"], interlace, fps, n)
        assert per == want and rate == (fps[0] * want, fps[1]) and frames == (n * want if n >= 0 else -1)
    if want == 2:
        assert av1stream.job_output(BASE + extra + ["out.ivf"], interlace, (30000, 1001), 5)[1:] == ((60000, 1001), 10)


def test_the_cut_mapping():
    """(g) output 2 f is a cut iff source f is; output 2 f + 1 never is"""
    import av1stream
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 48):
        cut = rng.integers(0, 2, n).astype(np.uint8) * rng.integers(1, 255, n).astype(np.uint8)      # any non-zero value marks a cut
        out = av1stream.field_rate_cuts(cut)
        assert out.shape == (2 * n,) and (out[0::2] == (cut != 0)).all() and (out[1::2] == 0).all()
    assert av1stream.field_rate_cuts(np.zeros(0, np.uint8)).size == 0
    # the planner then works in output positions: a cut at source frame 5 starts a GOP at output frame 10
    K_, start, ln = av1stream.plan_gops(24, 8, 3, av1stream.field_rate_cuts([0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]))
    assert K_ == 3 and start.tolist() == [0, 10, 16] and ln.tolist() == [10, 6, 8]


# ---------------------------------------------------------------------------------------------- argv
@pytest.mark.parametrize("extra, want", [
    ([], "frame"), (["-av1mi_deinterlace_rate", "frame"], "frame"), (["-av1mi_deinterlace", "auto", "-av1mi_deinterlace_rate", "frame"], "frame"),
    (["-av1mi_deinterlace", "auto"] + FIELD, "field"), (["-av1mi_deinterlace", "tff"] + FIELD, "field"), (["-av1mi_deinterlace", "bff"] + FIELD, "field"),
    (FIELD + ["-av1mi_deinterlace", "auto", "-g", 8], "field"), (["-av1mi_deinterlace", "auto", "-av1mi_scenecut", 15] + FIELD, "field"),
    (FIELD + ["-g", 5], "field"),      # nothing is deinterlaced: -g keeps counting source frames
])
def test_argv_accepted(extra, want):
    import av1stream
    assert av1stream.parse_deinterlace_rate(BASE + extra + ["out.ivf"]) == want


def test_frame_explicit_parses_like_absent():
    import av1stream
    for extra in ([], ["-av1mi_deinterlace", "auto"], ["-av1mi_deinterlace", "bff", "-g", 7], ["-vf:v:0", "yadif"]):
        a, b = BASE + extra + ["out.ivf"], BASE + extra + ["-av1mi_deinterlace_rate", "frame", "out.ivf"]
        assert av1stream.parse_deinterlace_rate(a) == av1stream.parse_deinterlace_rate(b) == "frame"
        assert av1stream.parse_deinterlace_option(a) == av1stream.parse_deinterlace_option(b)
        for interlace in "ptb":
            assert av1stream.job_output(a, interlace, (30, 1), 9) == av1stream.job_output(b, interlace, (30, 1), 9) == (1, (30, 1), 9)


@pytest.mark.parametrize("extra, names", [
    (["-av1mi_deinterlace_rate", "bob"], "bob"), (["-av1mi_deinterlace_rate", "1"], "-av1mi_deinterlace_rate"),
    (["-av1mi_deinterlace", "auto", "-g", 5] + FIELD, "-g"), (["-av1mi_deinterlace", "tff"] + FIELD + ["-g", 31], "-g 31"),
    (["-vf:v:0", "yadif", "-g", 3] + FIELD, "-g"),
    (["-av1mi_deinterlace", "auto", "-av1mi_pack10", 1] + FIELD, "-av1mi_pack10 1"),
    (["-av1mi_deinterlace", "auto", "-av1mi_denoise", 4] + FIELD, "-av1mi_denoise"),
    (["-vf:v:0", "yadif=mode=1"] + FIELD, "yadif=mode=1"), (["-vf:v:0", "bwdif=mode=send_field"] + FIELD, "bwdif=mode=send_field"),
])
def test_argv_refused_with_a_message_that_names_the_argument(extra, names):
    import av1stream
    with pytest.raises(ValueError) as e:
        av1stream.parse_deinterlace_rate(BASE + extra + ["out.ivf"])
    assert "Invalid argument" in str(e.value) and names in str(e.value)
