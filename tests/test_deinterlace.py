"""CPU tests of the deinterlacing option: the numpy reference (tests/deinterlace_ref.py) has the properties include/av1mi.h states, the
clips of the GPU tests exercise both of its paths, and the host reads the Y4M header's I parameter and the argument vector as
av1-go_amd/host/transcode.hpp says."""
import numpy as np
import pytest

import deint_clips as K
import deinterlace_ref as R


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("k", [0, 1])
def test_a_still_run_and_a_one_frame_run_return_their_input(bd, k):
    rng = np.random.default_rng(bd + k)
    for w, h in ((8, 8), (13, 7), (40, 1), (5, 2)):
        f = rng.integers(0, 1 << bd, (h, w)).astype(np.uint16)
        still = np.stack([f] * 3)
        assert (R.run(still, w, h, k) == still).all(), "%dx%d: a still run changes" % (w, h)
        assert (R.run(f[None], w, h, k) == f[None]).all(), "%dx%d: a one-frame run changes" % (w, h)


@pytest.mark.parametrize("k", [0, 1])
def test_kept_lines_are_the_inputs(k):
    for name in K.CASES:
        for plane, (w, h) in zip(K.case_clip(name, 8, k), K.case_true_sizes(name)):
            out = R.run(plane, w, h, k)
            assert (out[:, k:h:2, :w] == plane[:, k:h:2, :w]).all(), name
            assert out.dtype == plane.dtype and out.shape == plane.shape


def test_swapping_parity_on_a_flipped_clip_flips_the_output():
    """A vertical flip swaps the lines above and below a missing line, so score(d) becomes score(-d): the output flips with the clip
    except where the ORDER of the directions decides between two mirror directions of equal score (-1 is tried before +1).  So: flipped
    exactly wherever no such tie exists, and exactly everywhere when the clip is turned by 180 degrees (which maps d to itself)."""
    n, h, w = 4, 24, 40
    Y = K.pan_plane(w, h, n, 10, 0, 3)
    for k in (0, 1):
        a = R.run(Y, w, h, k)
        assert (R.run(Y[:, ::-1, ::-1], w, h, 1 - k)[:, ::-1, ::-1] == a).all()
        b = R.run(Y[:, ::-1], w, h, 1 - k)[:, ::-1]
        tie = np.zeros(a.shape, bool)
        for f in range(n):
            p = R._parts(Y[max(f - 1, 0)], Y[f], Y[min(f + 1, n - 1)], w, h, k)
            tie[f, p["rows"]] = (p["scores"][-1] == p["scores"][1]) | (p["scores"][-2] == p["scores"][2])
        assert (b == a)[~tie].all()
        assert (b == a).mean() > 0.9


def test_the_outputs_padding_replicates_its_edge():
    rng = np.random.default_rng(4)
    Y = K.pan_plane(40, 24, 3, 8, 1, 5)
    dirty = Y.copy()
    dirty[:, 22:, :] = rng.integers(0, 256, dirty[:, 22:, :].shape)      # the input's padding is undefined
    dirty[:, :, 38:] = rng.integers(0, 256, dirty[:, :, 38:].shape)
    out = R.run(dirty, 38, 22, 1)
    assert (out == R.run(Y, 38, 22, 1)).all(), "the input's padding was used"
    assert (out[:, 22:, :] == out[:, 21:22, :]).all() and (out[:, :, 38:] == out[:, :, 37:38]).all()
    assert (out[:, :22, :38] == R.run(np.ascontiguousarray(Y[:, :22, :38]), 38, 22, 1)).all()


# ---------------------------------------------------------------------------------------------- the clips
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("name", list(K.CASES) + ["session"])
def test_the_clips_exercise_both_paths(name, bd, k):
    """conditions on the clips, not measurements: among the missing luma samples of the middle frames at least 10 % leave the output
    different from t, at least 10 % pick a direction other than 0, at least 1 % are clamped at t +- m"""
    if name == "session":
        Y, (w, h) = K.pan_clip(192, 128, 12, bd, k)[0], (192, 128)
    else:
        Y, (w, h) = K.case_clip(name, bd, k)[0], K.case_true_sizes(name)[0]
    off_t, dirs, clamped = R.shares(Y, w, h, k)
    assert off_t >= 0.10 and dirs >= 0.10 and clamped >= 0.01, (off_t, dirs, clamped)
    woven = R.run(Y, w, h, k)
    assert (woven != Y).any()


# ---------------------------------------------------------------------------------------------- header and argv
@pytest.mark.parametrize("tag, want", [("t", "t"), ("b", "b"), ("p", "p"), ("m", "m"), ("?", "p"), (None, "p")])
def test_the_y4m_reader_reports_the_interlace_parameter(tmp_path, tag, want):
    import av1stream
    K.write_y4m(tmp_path / "a.y4m", K.pan_clip(16, 16, 2, 8, 0), 8, interlace=tag)
    assert av1stream.y4m_interlace(tmp_path / "a.y4m") == want


BASE = ["-i", "in.y4m", "-global_quality:v:0", 110]


@pytest.mark.parametrize("extra, want", [
    ([], "off"), (["-av1mi_deinterlace", "off"], "off"), (["-av1mi_deinterlace", "auto"], "auto"), (["-av1mi_deinterlace", "tff"], "tff"),
    (["-av1mi_deinterlace", "bff"], "bff"),
    (["-vf:v:0", "yadif"], "auto"), (["-vf:v:0", "bwdif=mode=0,format=nv12"], "auto"), (["-vf:v:0", "hwupload,deinterlace_vaapi,scale_vaapi=w=64:h=48"], "auto"),
    (["-vf:v:0", "yadif=mode=send_frame"], "auto"), (["-vf", "bwdif=mode=send_frame"], "auto"), (["-vf:v:0", "format=nv12"], "off"),
    (["-vf:v:0", "yadif", "-av1mi_deinterlace", "bff"], "bff"), (["-av1mi_deinterlace", "off", "-vf:v:0", "yadif"], "off"),
    (["-av1mi_deinterlace", "auto", "-av1mi_scenecut", 15], "auto"),
])
def test_argv_accepted(extra, want):
    import av1stream
    assert av1stream.parse_deinterlace_option(BASE + extra + ["out.ivf"]) == want


@pytest.mark.parametrize("extra, names", [
    (["-av1mi_deinterlace", "bob"], "bob"), (["-av1mi_deinterlace", "1"], "-av1mi_deinterlace"),
    (["-vf:v:0", "yadif=mode=1"], "yadif=mode=1"), (["-vf:v:0", "yadif=1"], "yadif=1"), (["-vf:v:0", "bwdif=mode=send_field"], "bwdif=mode=send_field"),
    (["-vf:v:0", "deinterlace_vaapi=rate=field"], "deinterlace_vaapi=rate=field"), (["-vf:v:0", "yadif=mode=0:parity=tff"], "parity=tff"),
    (["-vf:v:0", "kerndeint"], "kerndeint"),
    (["-av1mi_deinterlace", "auto", "-av1mi_pack10", 1], "-av1mi_pack10 1"), (["-vf:v:0", "yadif", "-av1mi_pack10", 1], "-av1mi_pack10 1"),
])
def test_argv_refused_with_a_message_that_names_the_argument(extra, names):
    import av1stream
    with pytest.raises(ValueError) as e:
        av1stream.parse_deinterlace_option(BASE + extra + ["out.ivf"])
    assert "Invalid argument" in str(e.value) and names in str(e.value)
