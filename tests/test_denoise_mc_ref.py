"""Properties of motion-compensated denoising as defined (tests/denoise_mc_ref.py = include/av1mi.h "motion-compensated denoising"), and
-av1mi_denoise_range through the transcode job's argument parser; no GPU."""
import numpy as np
import pytest

import denoise_mc_clips as K
import denoise_mc_ref as M
import denoise_ref as R


def _sizes(w, h):
    return [(w, h), (w // 2, h // 2), (w // 2, h // 2)]


@pytest.mark.parametrize("bd", [8, 10])
def test_zero_vectors_give_the_plain_filter(bd):
    sizes, true = _sizes(72, 40), (70, 38)
    ts = K.true_sizes(sizes, true)
    nb = M.grid(*true)[0] * M.grid(*true)[1]
    for step in ((0, 0), K.STEP):      # standing still: samples are counted; moving: the weights fall
        planes = K.translating(sizes, 4, bd, 7, 2, step=step, true=true)
        outs, recs, vec = M.run(planes, ts, bd, 6, 8, force=np.zeros((4, nb), M.VEC_DTYPE))
        assert not vec.view(np.int8).any()
        for a, (w, h), o, r in zip(planes, ts, outs, recs):
            want, want_rec = R.run(a, w, h, bd, 6)
            assert (o == want).all() and r.tobytes() == want_rec.tobytes()
        assert (sum(int(r["count"].sum()) for r in recs) > 0) == (step == (0, 0))


@pytest.mark.parametrize("bd", [8, 10])
def test_equal_frames_do_not_move_and_come_back(bd):
    sizes, true = _sizes(72, 40), (70, 38)
    ts = K.true_sizes(sizes, true)
    planes = [np.repeat(a[:1], 4, axis=0) for a in K.translating(sizes, 1, bd, 9, 3, true=true)]
    outs, recs, vec = M.run(planes, ts, bd, 4, 8)
    assert not vec.view(np.int8).any()      # the tie rule: the zero vector
    for a, (w, h), o in zip(planes, ts, outs):
        assert (o[:, :h, :w] == a[:, :h, :w]).all()


@pytest.mark.parametrize("sigma", [1, 2, 4, 8])
def test_still_grainy_grey_stays_at_the_zero_vector(sigma):
    """128 x 128 flat grey under independent grain, strength 2 sigma, range 8: at most 1 block in 64 moves (the bias's purpose)"""
    rng = np.random.default_rng(100 + sigma)
    Y = np.clip(128 + np.rint(rng.normal(0, sigma, (3, 128, 128))), 0, 255).astype(np.uint8)
    vec = M.vectors(Y[0], Y[1], Y[2], 128, 128, 8, 2 * sigma, 8)
    moved = int((vec.view(np.int8).reshape(-1, 4) != 0).any(axis=1).sum())
    unbiased = sum(int(M.search(Y[1], F, 128, 128, 8, 2 * sigma, 8, bias=False)[0].any(axis=2).sum()) for F in (Y[0], Y[2]))
    print("sigma %d: %d of 64 blocks moved; without the bias %d of 128 searches" % (sigma, moved, unbiased))
    assert vec.shape == (64,) and moved <= 1


def _interior(w0, h0, rng):
    nbx, nby = M.grid(w0, h0)
    return np.array([[bx * 16 - rng >= 0 and bx * 16 + 16 + rng <= w0 and by * 16 - rng >= 0 and by * 16 + 16 + rng <= h0 for bx in range(nbx)] for by in range(nby)])


def test_translating_content_is_followed():
    w = h = 128
    sigma, strength, rng = 2, 4, 8
    moving = K.translating([(w, h)], 3, 8, 11, sigma)[0]
    still = K.translating([(w, h)], 3, 8, 11, sigma, step=(0, 0))[0]
    vec = M.vectors(moving[0], moving[1], moving[2], w, h, 8, strength, rng).reshape(8, 8)
    inside = _interior(w, h, rng)
    assert inside.sum() == 36
    for k, v in (("dx_p", -K.STEP[0]), ("dy_p", -K.STEP[1]), ("dx_n", K.STEP[0]), ("dy_n", K.STEP[1])):
        assert (vec[k][inside] == v).all(), (k, vec[k])
    # the share of counted samples in those blocks: the moving picture through the search against the picture standing still at range 0
    px = np.kron(inside, np.ones((16, 16), bool))
    def counted(P, C, N, vxp, vyp, vxn, vyn):
        T = R.threshold(strength, 8)
        return ((R.weight(M.sad3(C, P, w, h, vxp, vyp), T) + R.weight(M.sad3(C, N, w, h, vxn, vyn), T)) >= R.COUNTED_FROM)[px].mean()
    full = lambda k: np.kron(vec[k].astype(np.int64), np.ones((16, 16), np.int64))
    got = counted(moving[0], moving[1], moving[2], full("dx_p"), full("dy_p"), full("dx_n"), full("dy_n"))
    ref = counted(still[0], still[1], still[2], 0, 0, 0, 0)
    zero = counted(moving[0], moving[1], moving[2], 0, 0, 0, 0)
    print("counted share: %.3f moving at range 8, %.3f standing still at range 0, %.3f moving at range 0" % (got, ref, zero))
    assert ref > 0.5 and got >= ref / 2 and zero < ref / 2


def test_chroma_vectors_are_halved_downwards():
    """dx = -3 with ssx = 1 reads column x - 2 (floor), not x - 1: P and N are C two columns to the left of where C has it"""
    w, h = 40, 16
    rng = np.random.default_rng(5)
    C = rng.integers(0, 256, (h, w)).astype(np.uint8)
    F = np.roll(C, -2, axis=1)      # F(x - 2) = C(x)
    vec = np.zeros(5, M.VEC_DTYPE)
    vec["dx_p"] = vec["dx_n"] = -3
    out, rec = M.plane(F, C, F, w, h, 8, 4, vec, 5, ss=(1, 0))
    assert (out == C).all()
    assert int(rec["count"].sum()) >= (w - 4) * h      # every sample whose neighbourhood stays clear of the clamp and the roll's seam
    for wrong in (-2, -4):      # (-2 >> 1 = -1, -4 >> 1 = -2 ... in luma terms -4 is the even vector that reads x - 2 too)
        vec["dx_p"] = vec["dx_n"] = wrong
        n = int(M.plane(F, C, F, w, h, 8, 4, vec, 5, ss=(1, 0))[1]["count"].sum())
        assert (n >= (w - 4) * h) == (wrong == -4)
    vec["dx_p"] = vec["dx_n"] = -3
    assert int(M.plane(F, C, F, w, h, 8, 4, vec, 3, ss=(0, 0))[1]["count"].sum()) < w      # the same vector in a plane that is not subsampled reads x - 3


# ---------------------------------------------------------------------------------------------- the transcode job's arguments
def _run(tmp_path, extra):
    import av1stream
    return av1stream.run_transcode(["-i", tmp_path / "missing.y4m"] + extra + [tmp_path / "out.mkv"])


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    """ParseBackendJob of the host library (host/transcode.hpp) behind a small program: arguments -> (ok, denoise, denoise_range, error text)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "av1-go_amd", "host")
    d = tmp_path_factory.mktemp("parse")
    src = d / "parse.cpp"
    src.write_text('#include "transcode.hpp"\n#include <cstdio>\nint main(int argc, char **argv) {\n  std::vector<std::string> a(argv + 1, argv + argc);\n'
                   '  av1mi_host::BackendJob job; std::string err;\n  const bool ok = av1mi_host::ParseBackendJob(a, &job, &err);\n'
                   '  std::printf("%d %d %d %s", (int)ok, job.denoise, job.denoise_range, err.c_str());\n  return 0;\n}\n')
    exe = str(d / "parse")
    subprocess.check_call(["g++", "-std=c++17", "-I", host, str(src), "-o", exe, "-L", host, "-lav1mi_host", "-Wl,-rpath," + host, "-Wl,-rpath," + os.path.dirname(host)])
    def run(extra):
        ok, denoise, rng, err = subprocess.check_output([exe, "-i", "in.y4m"] + extra + ["out.mkv"]).decode().split(" ", 3)
        return bool(int(ok)), int(denoise), int(rng), err
    return run


@pytest.mark.parametrize("good,want", [(["-av1mi_denoise", "4", "-av1mi_denoise_range", "8"], (4, 8)), (["-av1mi_denoise", "4", "-av1mi_denoise_range", "4"], (4, 4)),
                                       (["-av1mi_denoise", "4", "-av1mi_denoise_range", "0"], (4, 0)), (["-av1mi_denoise_range", "0"], (0, 0)), (["-av1mi_denoise", "4"], (4, 0)),
                                       (["-av1mi_denoise_range", "8", "-av1mi_denoise", "16", "-av1mi_film_grain", "0"], (16, 8))])
def test_range_is_parsed_into_the_job(parse, good, want):
    ok, denoise, rng, err = parse(good)
    assert ok and (denoise, rng) == want, (good, err)


def test_range_refusals_come_from_the_parser(parse):
    for bad, why in ((["-av1mi_denoise_range", "8"], "-av1mi_denoise_range needs -av1mi_denoise"), (["-av1mi_denoise", "4", "-av1mi_denoise_range", "3"], "-av1mi_denoise_range takes 0 (off), 4 or 8")):
        ok, _, _, err = parse(bad)
        assert not ok and err.startswith("Invalid argument: ") and why in err, (bad, err)


@pytest.mark.parametrize("good", [["-av1mi_denoise", "4", "-av1mi_denoise_range", "8"], ["-av1mi_denoise", "4", "-av1mi_denoise_range", "4"],
                                  ["-av1mi_denoise", "4", "-av1mi_denoise_range", "0"], ["-av1mi_denoise_range", "0"],
                                  ["-av1mi_denoise_range", "8", "-av1mi_denoise", "16", "-av1mi_film_grain", "0"]])
def test_range_passes_through_the_transcode_entry(av1mi, tmp_path, good):
    """the same through av1mi_run_transcode, which without a GPU ends in `no usable HIP device` after the arguments passed (that the
    values arrive in the job is test_range_is_parsed_into_the_job's business)"""
    code, text = _run(tmp_path, good)
    assert "Invalid argument" not in text and code != 0, (good, text)
    if av1mi.load().av1mi_device_count() == 0:
        assert code == -1 and "no usable HIP device" in text


@pytest.mark.parametrize("bad,why", [(["-av1mi_denoise_range", "8"], "-av1mi_denoise_range needs -av1mi_denoise"),
                                     (["-av1mi_denoise_range", "4", "-av1mi_denoise", "0"], "-av1mi_denoise_range needs -av1mi_denoise"),
                                     (["-av1mi_denoise", "4", "-av1mi_denoise_range", "3"], "-av1mi_denoise_range takes 0 (off), 4 or 8"),
                                     (["-av1mi_denoise", "4", "-av1mi_denoise_range", "16"], "-av1mi_denoise_range takes"),
                                     (["-av1mi_denoise", "4", "-av1mi_denoise_range", "-4"], "-av1mi_denoise_range takes"),
                                     (["-av1mi_denoise", "4", "-av1mi_denoise_range", "x"], "-av1mi_denoise_range takes"),
                                     (["-av1mi_denoise", "17", "-av1mi_denoise_range", "8"], "-av1mi_denoise takes a strength 1 .. 16"),
                                     (["-av1mi_denoise", "4", "-av1mi_denoise_range", "8", "-av1mi_pack10", "1"], "not together with -av1mi_pack10 1"),
                                     (["-av1mi_denoise", "4", "-av1mi_denoise_range", "8", "-av1mi_deinterlace", "auto"], "not together with -av1mi_deinterlace"),
                                     (["-av1mi_denoise", "4", "-av1mi_denoise_range", "8", "-vf:v:0", "yadif"], "not together with -av1mi_deinterlace")])
def test_range_refused(tmp_path, bad, why):
    code, text = _run(tmp_path, bad)
    assert code == 1 and "Invalid argument: " in text and why in text, (bad, text)
