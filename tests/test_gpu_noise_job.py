"""GPU tests of -av1mi_denoise auto through av1mi_run_transcode: the job samples the file's frame pairs, measures them on the GPU, plans a
strength (tests/noise_ref.py is the expectation, on the same sampled pairs) and IS the job -av1mi_denoise N from there on — byte for
byte; planned 0 is the job without the option.  192 x 128, gop 4.  Every comparison is equality."""
import numpy as np
import pytest

import noise_ref as R

pytestmark = pytest.mark.gpu

W, H, Q, G, S = 192, 128, 110, 4, 2


def _clip(frames, sigma, bd=8, seed=7):
    Y = R.clip(W, H, frames, sigma, seed, bit_depth=bd)
    grey = np.full((frames, H // 2, W // 2), 1 << (bd - 1), Y.dtype)
    return [Y, grey, grey]


def _planned(clip, bd):
    """the strength the reference plans on the pairs the job samples"""
    Y = clip[0]
    assert len(R.pair_slots(len(Y))) == min(16, len(Y) // 2)
    return R.plan(R.records(R.sample(Y), bd, W, H))[0]


def _job(d, name, source, extra):
    import av1stream
    out, stats = d / (name + ".obu"), d / (name + ".stats")
    code, err, planned = av1stream.run_transcode_report(["-i", source, "-global_quality:v:0", Q, "-g", G, "-av1mi_segments", S, "-av1mi_stats", stats] + extra + [out])
    assert code == 0, (name, err)
    return out.read_bytes(), stats.read_text().splitlines(), planned


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """every clip once, every job once: name -> (bytes, stats lines, reported strength); "N:<clip>" -> the reference's strength"""
    import deint_clips as K
    d = tmp_path_factory.mktemp("noise_job")
    out = {}
    for name, frames, sigma, bd, extra in (("clean", 8, 0, 8, []), ("noisy", 8, 4.0, 8, []), ("range", 8, 4.0, 8, ["-av1mi_denoise_range", 4]), ("deep", 8, 4.0, 10, []),
                                           ("short", 3, 4.0, 8, [])):
        clip = _clip(frames, sigma, bd)
        K.write_y4m(d / (name + ".y4m"), clip, bd, interlace="p")
        n = out["N:" + name] = _planned(clip, bd)
        out[name + ":auto"] = _job(d, name + "_auto", d / (name + ".y4m"), ["-av1mi_denoise", "auto"] + extra)
        out[name + ":fixed"] = _job(d, name + "_fixed", d / (name + ".y4m"), (["-av1mi_denoise", n] + extra) if n else [])
    return out


def _tags(lines):
    return [l for l in lines if " denoise:auto>" in l]


def test_clean_clip_is_the_job_without_the_option(jobs):
    assert jobs["N:clean"] == 0
    auto, plain = jobs["clean:auto"], jobs["clean:fixed"]
    assert auto[0] == plain[0] and auto[2] == 0 and plain[2] == -1
    assert auto[1][0].startswith("n:0 ") and " denoise:auto>0" in auto[1][0] and _tags(auto[1]) == [auto[1][0]] and not _tags(plain[1])
    assert not any(" grain:" in l for l in auto[1])      # no frame store, no denoiser
    # the lines are the plain job's but for the tag
    assert [l.replace(" denoise:auto>0", "") for l in auto[1]] == plain[1]


def test_noisy_clip_is_the_job_with_the_planned_strength(jobs):
    import dav1d_ref as D
    n = jobs["N:noisy"]
    assert n == 6      # sigma 4: ceil(1.5 x 3.69)
    auto, fixed = jobs["noisy:auto"], jobs["noisy:fixed"]
    assert auto[0] == fixed[0] and auto[2] == n and fixed[2] == -1
    assert " denoise:auto>%d" % n in auto[1][0] and _tags(auto[1]) == [auto[1][0]] and not _tags(fixed[1])
    assert [l.replace(" denoise:auto>%d" % n, "") for l in auto[1]] == fixed[1] and all(" grain:" in l for l in auto[1] if l.startswith("n:"))
    assert auto[0] != jobs["clean:auto"][0]
    if D.available():
        assert len(D.decode(auto[0])) == 8


def test_with_a_search_range(jobs):
    n = jobs["N:range"]
    auto, fixed = jobs["range:auto"], jobs["range:fixed"]
    assert n == jobs["N:noisy"] and auto[0] == fixed[0] and auto[2] == n and " denoise:auto>%d" % n in auto[1][0]


def test_10_bit_clip(jobs):
    n = jobs["N:deep"]
    auto, fixed = jobs["deep:auto"], jobs["deep:fixed"]
    assert n >= 1 and auto[0] == fixed[0] and auto[2] == n and " denoise:auto>%d" % n in auto[1][0]


def test_three_frames_make_one_pair_at_slot_0(jobs):
    assert R.pair_slots(3) == [0]
    n = jobs["N:short"]
    auto, fixed = jobs["short:auto"], jobs["short:fixed"]
    assert n >= 1 and auto[0] == fixed[0] and auto[2] == n and " denoise:auto>%d" % n in auto[1][0]
    assert len([l for l in auto[1] if l.startswith("n:")]) == 3


def test_planned_0_drops_what_shapes_the_denoiser(tmp_path):
    """a clean clip with -av1mi_denoise_range, -av1mi_film_grain and -av1mi_grain_lag beside auto: they go with the denoiser, nothing is refused"""
    import deint_clips as K
    K.write_y4m(tmp_path / "clean.y4m", _clip(8, 0), 8, interlace="p")
    auto = _job(tmp_path, "auto", tmp_path / "clean.y4m", ["-av1mi_denoise", "auto", "-av1mi_denoise_range", 8, "-av1mi_film_grain", 1, "-av1mi_grain_lag", 2])
    plain = _job(tmp_path, "plain", tmp_path / "clean.y4m", [])
    assert auto[0] == plain[0] and auto[2] == 0 and not any(" grain:" in l or " ar:" in l for l in auto[1])


def test_a_file_of_one_frame_plans_0(tmp_path):
    import deint_clips as K
    K.write_y4m(tmp_path / "one.y4m", _clip(1, 4.0), 8, interlace="p")
    auto = _job(tmp_path, "auto", tmp_path / "one.y4m", ["-av1mi_denoise", "auto"])
    assert auto[2] == 0 and " denoise:auto>0" in auto[1][0] and auto[0] == _job(tmp_path, "plain", tmp_path / "one.y4m", [])[0]
