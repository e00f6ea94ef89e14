"""GPU tests of -av1mi_tonemap_peak auto in a transcode job (av1mi_run_transcode): the job measures its source, plans the peak and is from
there on the job -av1mi_tonemap_peak N, byte for byte; the stats file says what was planned; jobs without auto are what they were."""
import numpy as np
import pytest

import peak_ref as R

pytestmark = pytest.mark.gpu

W = H = 64
Q, G, SEGS, N = 128, 2, 2, 8
TM = ["-av1mi_tonemap", "bt2390"]


def _clip():
    """8 frames of 10-bit PQ: dim ramps, and in frame 5 a ramp up to luma 675 (code 714, about 600 cd/m2) with a patch of luma 810 (code 871,
    about 2500 cd/m2) of 12 x 12 pixels: more than skip (0 at 64 x 64)"""
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:H, 0:W]
    Y = np.stack([64 + (xx * 5 + yy * 2 + 3 * t) + rng.integers(0, 5, (H, W)) for t in range(N)])
    Y[5] = 64 + (xx * 611 // (W - 1))
    Y[5, 20:32, 30:42] = 810
    U = np.stack([500 + xx[::2, ::2] // 2 + t for t in range(N)])
    V = np.stack([530 - yy[::2, ::2] // 2 for t in range(N)])
    U[5] = V[5] = 512
    return [a.astype(np.uint16) for a in (Y, U, V)]


def _write(path, clip):
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420p10\n" % (W, H)).encode())
        for t in range(N):
            f.write(b"FRAME\n")
            for p in clip:
                f.write(np.ascontiguousarray(p[t]).astype("<u2").tobytes())


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    import av1stream
    d = tmp_path_factory.mktemp("peak")
    clip = _clip()
    _write(d / "hdr.y4m", clip)
    slots = av1stream.peak_sample_slots(N)
    planned, codes = R.plan(R.records(*[a[slots] for a in clip], W, H))
    runs = dict(auto=TM + ["-av1mi_tonemap_peak", "auto", "-av1mi_stats", d / "auto.stats"], number=TM + ["-av1mi_tonemap_peak", planned, "-av1mi_stats", d / "number.stats"],
                tm=TM, tm_4000=TM + ["-av1mi_tonemap_peak", 4000], plain=[], auto_crop=TM + ["-av1mi_tonemap_peak", "auto", "-av1mi_crop", "auto"],
                number_crop=TM + ["-av1mi_tonemap_peak", planned, "-av1mi_crop", "auto"])
    out = {"dir": d, "planned": planned, "codes": codes, "slots": slots}
    for name, extra in runs.items():
        path = d / (name + ".obu")
        code, err = av1stream.run_transcode(["-i", d / "hdr.y4m", "-global_quality:v:0", Q, "-g", G, "-av1mi_segments", SEGS] + extra + [path])
        out[name] = (code, err, path.read_bytes() if code == 0 else b"")
    return out


def test_the_plan_of_the_clip(jobs):
    """what the reference plans for the sampled frames: every frame of so short a file, the bright patch's code, a peak that is not 1000"""
    assert jobs["slots"] == list(range(N))
    assert max(jobs["codes"]) == jobs["codes"][5] == (19133 * (810 - 64) + 8192) >> 14 == 871
    assert 2000 < jobs["planned"] < 3000 and jobs["planned"] != 1000


def test_auto_is_the_job_with_the_planned_number(jobs):
    for name in ("auto", "number", "tm", "tm_4000", "plain"):
        assert jobs[name][0] == 0, (name, jobs[name][1])
    assert jobs["auto"][2] == jobs["number"][2] and len(jobs["auto"][2]) > 0
    assert jobs["auto"][2] != jobs["tm"][2] and jobs["auto"][2] != jobs["tm_4000"][2]      # not the job without the option (1000), not another number's
    assert jobs["tm"][2] != jobs["tm_4000"][2] and jobs["plain"][2] not in (jobs["tm"][2], jobs["auto"][2])


def test_the_stats_say_what_was_planned(jobs):
    auto, number = [(jobs["dir"] / (n + ".stats")).read_text().splitlines() for n in ("auto", "number")]
    tag = " peak:auto>%d" % jobs["planned"]
    assert tag in auto[0] and "peak:" not in "".join(auto[1:]) and "peak:" not in "".join(number)
    assert auto[0].replace(tag, "") == number[0] and auto[1:] == number[1:]


def test_the_measurement_is_in_front_of_the_crop(jobs):
    """with -av1mi_crop auto the file is sampled twice, and the plan is the whole frame's"""
    assert jobs["auto_crop"][0] == 0 and jobs["number_crop"][0] == 0, (jobs["auto_crop"][1], jobs["number_crop"][1])
    assert jobs["auto_crop"][2] == jobs["number_crop"][2]
