"""Film grain parameters in the frame header (av1mi_obu_frame.film_grain, spec 5.9.30) against dav1d: with the grain switched off the
stream decodes to exactly the frames the same symbols give without parameters (which pins the header's length and the sequence bit);
with it on, the decoder adds grain that follows the seed.  No GPU."""
import numpy as np
import pytest

import dav1d_grain as DG

pytestmark = pytest.mark.skipif(not DG.available(), reason="dav1d is not in this image")


def film_grain(av1stream, seed, scaling=40, apply=1, chroma=True):
    """white grain with a constant scaling function on every plane"""
    g = av1stream.FilmGrain()
    g.apply_grain, g.grain_seed, g.num_y_points = apply, seed, 2
    for i, v in enumerate((0, 255)):
        g.point_y_value[i], g.point_y_scaling[i] = v, scaling
        g.point_cb_value[i], g.point_cb_scaling[i] = v, scaling
        g.point_cr_value[i], g.point_cr_scaling[i] = v, scaling
    g.num_cb_points = g.num_cr_points = 2 if chroma else 0
    g.grain_scaling_minus_8, g.ar_coeff_lag, g.ar_coeff_shift_minus_6, g.grain_scale_shift = 3, 0, 0, 0
    g.ar_coeffs_cb_plus_128[0] = g.ar_coeffs_cr_plus_128[0] = 128      # the one chroma coefficient (the luma grain's share): 0
    g.cb_mult, g.cb_luma_mult, g.cb_offset = 192, 128, 256             # the chroma index is the chroma sample itself
    g.cr_mult, g.cr_luma_mult, g.cr_offset = 192, 128, 256
    g.overlap_flag, g.clip_to_restricted_range = 1, 0
    return g


@pytest.fixture(scope="module")
def gops(O):
    """per (true size, bit depth): the symbols of a key frame and a P frame, as keyword sets for av1stream.temporal_unit"""
    import pipeline as P
    import synth
    import test_av1_conformance as TC
    out = {}
    for (vw, vh) in ((64, 64), (70, 38)):
        for bd in (8, 10):
            w, h, q = (vw + 7) // 8 * 8, (vh + 7) // 8 * 8, 120
            Yc, Uc, Vc = synth.frames(w + 8, h + 8, 2, bd, 3)
            units, ref = [], None
            for t in range(2):
                src = (TC._pad(Yc[t][:vh, :vw], h, w), TC._pad(Uc[t][:(vh + 1) // 2, :(vw + 1) // 2], h // 2, w // 2), TC._pad(Vc[t][:(vh + 1) // 2, :(vw + 1) // 2], h // 2, w // 2))
                if t == 0:
                    r = O.intra_encode_frame(src[0], src[1], src[2], bd, 8, q)
                    hdr, st = TC._filters(O, P, r, bd, q, 0, w, h, np.zeros((h // 8, w // 8), np.uint8), src, (vw, vh))
                    units.append(dict(hdr, y_mode=r["modes_y"], uv_mode=r["modes_uv"], lev_y=r["lev_y"], lev_u=r["lev_u"], lev_v=r["lev_v"]))
                else:
                    r = O.inter_encode_frame(src, ref, bd, q, 8)
                    hdr, st = TC._filters(O, P, r, bd, q, 1, w, h, r["skip"].reshape(h // 8, w // 8), src, (vw, vh))
                    units.append(dict(hdr, frame_type=1, with_sequence_header=False, mv=r["mvs"], skip=r["skip"], lev_y=r["lev_y"], lev_u=r["lev_u"], lev_v=r["lev_v"]))
                ref = st[2]
            out[(vw, vh, bd)] = (w, h, q, units)
    return out


def _units(av1stream, key, gop, opstream, grains=(None, None), present=None):
    w, h, q, units = gop
    return b"".join(av1stream.temporal_unit(w, h, key[2], q, opstream=opstream, film_grain=g, film_grain_present=present, **u) for u, g in zip(units, grains))


def _same(a, b):
    return len(a) == len(b) and all((x == y).all() for fa, fb in zip(a, b) for x, y in zip(fa, fb))


@pytest.mark.parametrize("opstream", [False, True])      # the symbol writer, and the writer around tile payloads coded elsewhere
@pytest.mark.parametrize("key", [(64, 64, 8), (64, 64, 10), (70, 38, 8), (70, 38, 10)])
def test_parameters_change_nothing_with_the_grain_off_and_add_seeded_grain_with_it_on(gops, key, opstream):
    import av1stream
    gop = gops[key]
    plain = _units(av1stream, key, gop, opstream)
    a = _units(av1stream, key, gop, opstream, (film_grain(av1stream, 1234), film_grain(av1stream, 77)))
    b = _units(av1stream, key, gop, opstream, (film_grain(av1stream, 4321), film_grain(av1stream, 78)))
    none = _units(av1stream, key, gop, opstream, (film_grain(av1stream, 1234, apply=0), None), present=1)
    assert a != plain and len(a) > len(plain)
    want = DG.decode(plain, False)
    assert len(want) == 2 and want[0][0].shape == (key[1], key[0])
    assert _same(DG.decode(plain, True), want)                      # no parameters: nothing to apply
    for s in (a, b, none):
        assert _same(DG.decode(s, False), want), "the parameters changed what the symbols decode to"
    ga, gb = DG.decode(a, True), DG.decode(b, True)
    for t in range(2):
        for i in range(3):
            assert (ga[t][i] != want[t][i]).any(), "frame %d plane %d: no grain was added" % (t, i)
            assert (ga[t][i] != gb[t][i]).any(), "frame %d plane %d: another seed, the same grain" % (t, i)
    assert _same(DG.decode(a, True), ga)                            # the same seed: the same grain
    assert _same(DG.decode(none, True), want)                       # apply_grain = 0, and a frame without parameters in a sequence that has them


def test_luma_only_parameters_and_the_refusals(gops):
    import av1stream
    key = (64, 64, 8)
    gop = gops[key]
    want = DG.decode(_units(av1stream, key, gop, False), False)
    luma = _units(av1stream, key, gop, False, (film_grain(av1stream, 5, chroma=False),) * 2)
    got = DG.decode(luma, True)
    assert _same(DG.decode(luma, False), want)
    assert (got[0][0] != want[0][0]).any() and (got[0][1] == want[0][1]).all() and (got[0][2] == want[0][2]).all()
    with pytest.raises(ValueError) as e:
        _units(av1stream, key, gop, False, (film_grain(av1stream, 5), None), present=0)
    assert "film_grain" in str(e.value) and "sequence" in str(e.value)
    g = film_grain(av1stream, 5)
    g.num_y_points = 0
    with pytest.raises(ValueError) as e:
        _units(av1stream, key, gop, False, (g, None))
    assert "chroma points without luma points" in str(e.value)
    g = film_grain(av1stream, 5)
    g.point_y_value[1] = 0
    with pytest.raises(ValueError) as e:
        _units(av1stream, key, gop, False, (g, None))
    assert "strictly increasing" in str(e.value)


# ---------------------------------------------------------------------------------------------- the closed loop
# The ratio (regenerated / injected standard deviation) the reference path reaches, measured on the CPU with tests/filmgrain_loop.py
# (mean over the three regions and three noise seeds): it is not 1 because 8-bit rounding of the source adds 1/12 to
# the variance (visible at sigma 2), and because at sigma 8 the weights of the counted samples fall to about 13 of 16, where the residual
# holds less than the 2/3 of the variance the model assumes.
MEASURED = {(8, 2): 1.051, (8, 4): 1.013, (8, 8): 0.948, (10, 2): 1.008, (10, 4): 0.992, (10, 8): 0.948}
GAIN = 0.0619                                  # host/filmgrain.hpp kGainLuma: standard deviation per unit of scaling, 8-bit terms


@pytest.mark.parametrize("bd", [8, 10])
def test_closed_loop_regenerates_the_injected_grain(O, bd):
    """inject sigma -> denoise_ref -> records -> av1mi_film_grain_from_records -> stream -> dav1d: per region the standard deviation of
    (grain on - grain off) against the injected one.  The band around the measured ratio is one step of the scaling value at that sigma
    (GAIN / sigma) plus three standard errors of a standard deviation over the region's 20 480 samples (3 / sqrt(2 N)), nothing else.
    The regenerated standard deviation must rise with sigma."""
    import filmgrain_loop as L
    import pipeline as P
    n = (L.ROWS[0][1] - L.ROWS[0][0]) * L.W
    out = {}
    for sigma in (2, 4, 8):
        r = L.loop(O, P, sigma, bd, seed=11)
        g = r["grain"]
        print("bit depth %d sigma %d: ratio per region %s, chroma %s, luma points %s" % (bd, sigma, np.round(r["ratio"], 4), np.round(r["chroma_ratio"], 4),
              [(g.point_y_value[i], g.point_y_scaling[i]) for i in range(g.num_y_points)]))
        assert g.apply_grain == 1 and g.num_y_points >= 3 and g.num_cb_points == 2 and g.num_cr_points == 2
        band = GAIN / sigma + 3 / np.sqrt(2 * n)
        for region, ratio in enumerate(r["ratio"]):
            assert abs(ratio - MEASURED[(bd, sigma)]) <= band, "sigma %d region %d: ratio %.4f, measured %.3f +- %.4f" % (sigma, region, ratio, MEASURED[(bd, sigma)], band)
        out[sigma] = [ratio * sigma for ratio in r["ratio"]]
    for region in range(3):
        assert out[2][region] < out[4][region] < out[8][region]
