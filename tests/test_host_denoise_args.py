"""-av1mi_denoise / -av1mi_film_grain through av1mi_run_transcode: what is accepted (which without a GPU ends in the `no usable HIP
device` result, code -1, after the arguments passed) and what ParseBackendJob refuses (`Invalid argument`, exit code 1).  No GPU."""
import pytest


def _run(tmp_path, extra):
    import av1stream
    return av1stream.run_transcode(["-i", tmp_path / "missing.y4m"] + extra + [tmp_path / "out.mkv"])


@pytest.mark.parametrize("good", [["-av1mi_denoise", "4"], ["-av1mi_denoise", "16", "-av1mi_film_grain", "0"], ["-av1mi_denoise", "1", "-av1mi_film_grain", "1"],
                                  ["-av1mi_denoise", "0"], ["-av1mi_denoise", "4", "-av1mi_scenecut", "15"], ["-av1mi_denoise", "4", "-av1mi_deinterlace", "off"],
                                  ["-av1mi_denoise", "4", "-av1mi_stats", "s.txt"]])
def test_accepted(av1mi, tmp_path, good):
    code, text = _run(tmp_path, good)
    assert "Invalid argument" not in text and code != 0, (good, text)
    if av1mi.load().av1mi_device_count() == 0:
        assert code == -1 and "no usable HIP device" in text


@pytest.mark.parametrize("bad,why", [(["-av1mi_denoise", "17"], "-av1mi_denoise takes a strength 1 .. 16"), (["-av1mi_denoise", "-1"], "-av1mi_denoise takes"),
                                     (["-av1mi_denoise", "x"], "-av1mi_denoise takes"), (["-av1mi_film_grain", "2", "-av1mi_denoise", "4"], "-av1mi_film_grain takes 0 or 1"),
                                     (["-av1mi_film_grain", "1"], "-av1mi_film_grain needs -av1mi_denoise"), (["-av1mi_film_grain", "0"], "-av1mi_film_grain needs -av1mi_denoise"),
                                     (["-av1mi_film_grain", "1", "-av1mi_denoise", "0"], "-av1mi_film_grain needs -av1mi_denoise"),
                                     (["-av1mi_denoise", "4", "-av1mi_pack10", "1"], "-av1mi_denoise keeps the group's frames in a planar store on the GPU: not together with -av1mi_pack10 1"),
                                     (["-av1mi_denoise", "4", "-av1mi_deinterlace", "auto"], "not together with -av1mi_deinterlace"),
                                     (["-av1mi_denoise", "4", "-vf:v:0", "yadif"], "not together with -av1mi_deinterlace")])
def test_refused(tmp_path, bad, why):
    code, text = _run(tmp_path, bad)
    assert code == 1 and "Invalid argument: " in text and why in text, (bad, text)
