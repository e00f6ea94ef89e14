"""Properties of the denoiser's definition (tests/denoise_ref.py = include/av1mi.h "denoising" / "grain records"); no GPU."""
import numpy as np
import pytest

import denoise_ref as R

W, H = 64, 48


def _picture(bd, shift=0):
    """a ramp with a bright square whose left edge is at 8 + shift"""
    y, x = np.mgrid[0:H, 0:W]
    a = (40 + x + y) << (bd - 8)
    a[12:36, 8 + shift:16 + shift] = 200 << (bd - 8)
    return a.astype(np.uint8 if bd == 8 else np.uint16)


def _psnr(a, b, bd):
    mse = ((a.astype(np.float64) - b) ** 2).mean()
    return 10 * np.log10(((1 << bd) - 1) ** 2 / mse)


def test_the_reciprocal_is_the_floor_division_for_every_sum_and_threshold():
    for bd in (8, 10, 12):
        D = np.arange(9 * ((1 << bd) - 1) + 1, dtype=np.int64)
        for s in range(1, 17):
            T = R.threshold(s, bd)
            assert (R.weight(D, T) == np.maximum(0, 16 - (16 * D) // (27 * T))).all()
            assert 16 * D.max() * R.reciprocal(T) < 1 << 63 and 16 * 27 * T < 1 << 32 and R.reciprocal(T) < 1 << 32
    assert R.K[0] == 4096 and R.K[32] == 1365 and len(R.K) == 33
    assert all(k == round(65536 / den) for k, den in zip(R.K, range(16, 49)))


@pytest.mark.parametrize("bd", [8, 10])
def test_a_still_clean_clip_is_returned_unchanged(bd):
    clip = np.stack([_picture(bd)] * 4)
    out, rec = R.run(clip, W, H, bd, 4)
    assert (out == clip).all()
    assert (rec["sum_sq"] == 0).all()
    assert rec["count"][0].sum() == 0 and rec["count"][3].sum() == 0 and (rec["count"][1:3].sum(axis=1) == W * H).all()


@pytest.mark.parametrize("bd", [8, 10])
def test_noise_on_a_still_clip_is_reduced_and_motion_is_left_alone(bd):
    rng = np.random.default_rng(5)
    clean = np.stack([_picture(bd)] * 5)
    noisy = np.clip(clean + np.rint(rng.normal(0, 2 << (bd - 8), clean.shape)), 0, (1 << bd) - 1).astype(clean.dtype)
    out, rec = R.run(noisy, W, H, bd, 8)
    for f in range(1, 4):
        assert _psnr(out[f], clean[f], bd) > _psnr(noisy[f], clean[f], bd) + 2.0
    assert rec["count"][1:4].sum() > 0.9 * 3 * W * H and rec["sum_sq"][1:4].sum() > 0
    # the square moves 8 samples per frame over a still ramp: where both sums exceed the cut-off the output IS C, and nothing is lost
    # against C anywhere on the moving edges
    moving = np.stack([_picture(bd, 8 * f) for f in range(4)])
    for f in (1, 2):
        q = R.parts(moving[f - 1], moving[f], moving[f + 1], W, H, bd, 8)
        cut_off = (q["dp"] >= q["cut"]) & (q["dn"] >= q["cut"])
        assert cut_off.sum() > 100
        assert (q["out"][cut_off] == q["c"][cut_off]).all()
    grainy = np.clip(moving + np.rint(rng.normal(0, 2 << (bd - 8), moving.shape)), 0, (1 << bd) - 1).astype(moving.dtype)
    out, _ = R.run(grainy, W, H, bd, 8)
    for f in (1, 2):
        assert _psnr(out[f], moving[f], bd) >= _psnr(grainy[f], moving[f], bd)


def test_the_ends_of_a_run_return_c_and_count_nothing():
    rng = np.random.default_rng(6)
    clip = rng.integers(90, 110, (4, H, W)).astype(np.uint8)
    out, rec = R.run(clip, W, H, 8, 16)
    assert (out[0] == clip[0]).all() and (out[3] == clip[3]).all()
    assert (out[1] != clip[1]).any()
    for f in (0, 3):
        assert (rec["count"][f] == 0).all() and (rec["sum_sq"][f] == 0).all()
    assert rec["count"][1].sum() > 0
    one, rec1 = R.run(clip[:1], W, H, 8, 16)
    assert (one == clip[:1]).all() and rec1["count"].sum() == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_padding_replicates_the_output_and_the_inputs_padding_does_not_matter(bd):
    rng = np.random.default_rng(7)
    w, h, Wb, Hb = 70, 38, 72, 40
    dt = np.uint8 if bd == 8 else np.uint16
    base = (rng.integers(100, 116, (4, Hb, Wb)) << (bd - 8)).astype(dt)
    a, b = base.copy(), base.copy()
    a[:, h:, :] = 0
    a[:, :, w:] = 0
    b[:, h:, :] = (1 << bd) - 1
    b[:, :, w:] = rng.integers(0, 1 << bd, (4, Hb, Wb - w))
    oa, ra = R.run(a, w, h, bd, 6)
    ob, rb = R.run(b, w, h, bd, 6)
    assert (oa == ob).all() and (ra == rb).all()
    assert (oa[:, :, w:] == oa[:, :, w - 1:w]).all() and (oa[:, h:, :] == oa[:, h - 1:h, :]).all()
    assert ra["count"][1].sum() <= w * h
