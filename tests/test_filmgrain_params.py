"""av1mi_film_grain_from_records (host/filmgrain.hpp): the rules from records to parameters, and the writer's refusal of parameters in a
stream whose sequence header does not announce them.  No GPU."""
import numpy as np
import pytest

import denoise_ref as R


def _records(luma=None, cb=None, cr=None):
    """[3, 16] records; per plane a dict bin -> (rms, count)"""
    rec = np.zeros((3, R.BINS), R.RECORD_DTYPE)
    for p, bins in enumerate((luma, cb, cr)):
        for b, (rms, count) in (bins or {}).items():
            rec[p, b]["sum_sq"], rec[p, b]["count"] = int(round(rms * rms * count)), count
    return rec


def _points(g):
    return [(g.point_y_value[i], g.point_y_scaling[i]) for i in range(g.num_y_points)]


def test_empty_records_give_no_grain():
    import av1stream
    for bd in (8, 10):
        g = av1stream.film_grain_from_records(_records(), bd, 0)
        assert g.apply_grain == 0 and g.num_y_points == 0 and g.num_cb_points == 0 and g.num_cr_points == 0
        assert av1stream.film_grain_mid_grey(g) == 0
    few = av1stream.film_grain_from_records(_records(luma={5: (3.0, 255)}), 8, 0)      # below the minimum count of 256
    assert few.apply_grain == 0
    with pytest.raises(ValueError):
        av1stream.film_grain_from_records(_records(), 12, 0)


def test_no_chroma_points_without_luma_points():
    import av1stream
    g = av1stream.film_grain_from_records(_records(cb={8: (3.0, 5000)}, cr={8: (3.0, 5000)}), 8, 3)
    assert g.apply_grain == 0 and g.num_cb_points == 0 and g.num_cr_points == 0
    g = av1stream.film_grain_from_records(_records(luma={8: (3.0, 5000)}, cb={7: (2.0, 4000), 8: (2.0, 1000)}), 8, 3)
    assert g.apply_grain == 1 and g.num_cb_points == 2 and g.num_cr_points == 0
    assert (g.point_cb_value[0], g.point_cb_value[1]) == (0, 255) and g.point_cb_scaling[0] == g.point_cb_scaling[1] == round(2.0 * 1.5 ** 0.5 / 0.0650)
    assert (g.cb_mult, g.cb_luma_mult, g.cb_offset) == (192, 128, 256)


def test_points_are_strictly_increasing_and_follow_the_bins():
    import av1stream
    luma = {b: (1.0 + 0.25 * b, 1000 + 10 * b) for b in range(16)}      # all 16 bins hold enough: the two with the fewest samples go
    g = av1stream.film_grain_from_records(_records(luma=luma), 8, 9)
    pts = _points(g)
    assert len(pts) == 14 and [v for v, _ in pts] == [16 * b + 8 for b in range(2, 16)]
    assert all(a[0] < b[0] for a, b in zip(pts, pts[1:]))
    assert [s for _, s in pts] == [int(np.floor((1.0 + 0.25 * b) * 1.5 ** 0.5 / 0.0619 + 0.5)) for b in range(2, 16)]
    g10 = av1stream.film_grain_from_records(_records(luma={b: (4 * r, c) for b, (r, c) in luma.items()}), 10, 9)
    assert _points(g10) == pts                                           # the same grain at 10 bits: the same 8-bit scaling
    gap = av1stream.film_grain_from_records(_records(luma={3: (2.0, 300), 12: (4.0, 300)}), 8, 9)
    assert _points(gap) == [(56, 40), (200, 79)] and av1stream.film_grain_mid_grey(gap) == 60      # empty bins lie on the line between their neighbours
    assert (g.ar_coeff_lag, g.overlap_flag, g.chroma_scaling_from_luma, g.clip_to_restricted_range, g.grain_scaling_minus_8) == (0, 1, 0, 0, 1)
    loud = av1stream.film_grain_from_records(_records(luma={3: (40.0, 300)}), 8, 9)
    assert _points(loud) == [(56, 255)]


def test_the_seed_follows_the_frame_index():
    import av1stream
    rec = _records(luma={8: (3.0, 5000)})
    seeds = [av1stream.film_grain_from_records(rec, 8, i).grain_seed for i in range(300)]
    assert len(set(seeds)) == 300 and all(0 <= s <= 65535 for s in seeds)
    assert seeds == [av1stream.film_grain_from_records(rec, 8, i).grain_seed for i in range(300)]


def test_parameters_without_the_sequence_flag_are_refused():
    import av1stream
    g = av1stream.film_grain_from_records(_records(luma={8: (3.0, 5000)}), 8, 0)
    nb = 64
    sym = dict(y_mode=np.zeros(nb, np.uint8), uv_mode=np.zeros(nb, np.uint8), lev_y=np.zeros((nb, 64), np.int16), lev_u=np.zeros((nb, 16), np.int16),
               lev_v=np.zeros((nb, 16), np.int16))
    assert av1stream.temporal_unit(64, 64, 8, 100, film_grain=g, **sym) != av1stream.temporal_unit(64, 64, 8, 100, **sym)
    with pytest.raises(ValueError) as e:
        av1stream.temporal_unit(64, 64, 8, 100, film_grain=g, film_grain_present=0, **sym)
    assert "film_grain_params_present = 0" in str(e.value)
