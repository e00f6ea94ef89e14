"""The clips of tests/intra_clips.py do what they are there for — checked with the CPU oracle alone (no GPU).  First the mode decision
restated in tests/intra_ref.py on the dav1d-pinned predictor agrees with the oracle's loop on every clip, closed and open loop; then
its by-products are counted over the stacked clips at q index 60: which modes win, how many minima are tied with and without DC, how
many blocks take edge filter type 1, how many upsampled edge values overshoot the range before the clip, how much of the
reconstruction is pinned at 0 and at the top value.  The floors are the issue's; the counts observed are in the docstrings
(`python tests/test_intra_clips.py` prints them)."""
import functools
import os
import sys

import numpy as np
import pytest

import intra_clips as IC
import intra_ref

Q = 60
DEPTHS = (8, 10)
SIZES = (8, 16, 32)


def _oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from oracle import oracle
    oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def coded(bd, bs, open_loop=False):
    """per stacked clip at this depth and block size: (name, source, the oracle's result, the restatement's decisions)"""
    O = _oracle()
    w, h = IC.SIZES[bs]
    out = []
    try:
        for name in IC.stacked_names(bd):
            src = IC.clip(name, w, h, bd)
            r = O.intra_encode_frame(src[0], src[1], src[2], bd, bs, Q, open_loop=open_loop)
            d = intra_ref.frame_decisions(O, src, (r["rec_y"], r["rec_u"], r["rec_v"]), bd, bs, open_loop=open_loop)
            out.append((name, src, r, d))
    finally:
        O.set_intra_open_loop(False)
    return out


@functools.lru_cache(maxsize=None)
def observe(bd, bs):
    """the counts the floors below are about, over the stack (plain ints)"""
    o = dict(modes_y=set(), modes_uv=set(), ft1_y=0, ft1_uv=0, ft1_tied_y=0, ft1_tied_uv=0, tied_not_dc=0, tied_dc_wins=0,
             clip_lo_y=0, clip_hi_y=0, clip_lo_uv=0, clip_hi_uv=0, rec_at_0=0, rec_at_top=0)
    for name, src, r, d in coded(bd, bs):
        for kind in ("y", "uv"):
            k = d[kind]
            o["modes_" + kind] |= set(k["mode"].tolist())
            o["ft1_" + kind] += int((k["ft"] == 1).sum())
            o["ft1_tied_" + kind] += int(((k["ft"] == 1) & k["tied"]).sum())
            o["tied_not_dc"] += int((k["tied"] & (k["mode"] != intra_ref.DC)).sum())
            o["tied_dc_wins"] += int((k["dc_tied"] & (k["mode"] == intra_ref.DC)).sum())
            o["clip_lo_" + kind] += int(k["lo"].sum())
            o["clip_hi_" + kind] += int(k["hi"].sum())
        for p in ("rec_y", "rec_u", "rec_v"):
            o["rec_at_0"] += int((r[p] == 0).sum())
            o["rec_at_top"] += int((r[p] == IC.top_of(bd)).sum())
    o["modes_y"], o["modes_uv"] = sorted(o["modes_y"]), sorted(o["modes_uv"])
    return o


@pytest.mark.parametrize("bd", DEPTHS)
def test_shapes_types_range_and_stack(bd):
    for bs, (w, h) in IC.SIZES.items():
        assert w % 64 == bs and h % 64 == bs and w > 128 and h > 64      # partial tiles both ways, more than one full tile across
        names = IC.stacked_names(bd)
        clips = [IC.clip(n, w, h, bd) for n in names]
        for c in clips:
            assert [a.shape for a in c] == [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
            assert all(a.dtype == (np.uint8 if bd == 8 else np.uint16) and int(a.max()) <= IC.top_of(bd) for a in c)
        for n in ("binary", "checker2", "checker1", "stripes", "diag", "quadrants012"):      # both ends of the range in every plane
            assert all(int(a.min()) == 0 and int(a.max()) == IC.top_of(bd) for a in clips[names.index(n)]), n
        u, v = clips[names.index("uv_negative")][1:]
        assert (u.astype(int) + v == IC.top_of(bd)).all()
        S = IC.stack(clips)
        assert S[0].shape == (len(names), h, w) and S[2].shape == (len(names), h // 2, w // 2) and (S[1][3] == clips[3][1]).all()
    tiles = 6 * len(IC.stacked_names(bd))
    assert any(tiles % (256 // bs) for bs in SIZES), "every block size ends the stacked job on a full workgroup"


@pytest.mark.parametrize("open_loop", [False, True])
@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_restatement_agrees_with_the_oracles_loop(bd, bs, open_loop):
    """two statements of one decision: the loop of oracle/av1o_pipeline.c and tests/intra_ref.py choose the same mode in every block
    of every clip — closed loop from the reconstruction with the neighbours' filter type, open loop from the source with type 0"""
    for name, src, r, d in coded(bd, bs, open_loop):
        for kind, key in (("y", "modes_y"), ("uv", "modes_uv")):
            bad = np.flatnonzero(d[kind]["mode"] != r[key])
            assert bad.size == 0, ("clip %s, %d bit, block size %d, %s loop, %s: blocks %s: restated %s, the oracle's loop %s"
                                   % (name, bd, bs, "open" if open_loop else "closed", key, bad[:4].tolist(),
                                      d[kind]["mode"][bad[:4]].tolist(), r[key][bad[:4]].tolist()))


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_every_mode_is_chosen(bd, bs):
    """every one of the 13 modes wins somewhere, in luma and in chroma, at block sizes 8 and 16; at 32 (15 blocks a frame) at least 10 of
    them in luma.  Observed: all 13 in luma and chroma at 8 and 16 at both depths; at 32 12 in luma (all but D67) and 13 in chroma at
    8 bits, 13 and 13 at 10 bits."""
    o = observe(bd, bs)
    if bs == 32:
        assert len(o["modes_y"]) >= 10, o
    else:
        assert o["modes_y"] == list(range(13)) and o["modes_uv"] == list(range(13)), o


@pytest.mark.parametrize("bd", DEPTHS)
def test_filter_type_1_is_reached(bd):
    """at block size 8 at least 10 luma and 10 chroma blocks have both a smooth-predicted neighbour (edge filter type 1) and a tied
    minimum.  Observed: 8 bits 169 luma and 137 chroma blocks of filter type 1, 30 and 14 of them tied; 10 bits 186 and 164, 36 and 17
    tied (most of the tied ones are smooth_steps')."""
    o = observe(bd, 8)
    assert o["ft1_y"] >= 10 and o["ft1_uv"] >= 10, o
    assert o["ft1_tied_y"] >= 10 and o["ft1_tied_uv"] >= 10, o


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_tied_minima_with_and_without_dc(bd, bs):
    """at least 40 blocks (luma and chroma blocks together) have a tied minimum that DC does not win, at least 20 a tie with DC in it,
    which DC wins.  Observed (not DC / DC wins): 8 bits 973 / 1387 at block size 8, 301 / 377 at 16, 144 / 75 at 32; 10 bits
    954 / 1617, 297 / 402, 160 / 73."""
    o = observe(bd, bs)
    assert o["tied_not_dc"] >= 40 and o["tied_dc_wins"] >= 20, o


@pytest.mark.parametrize("bd", DEPTHS)
def test_upsampled_edges_overshoot_both_ends(bd):
    """at block size 8 at least 50 blocks have a candidate's upsampled edge value below 0 before the clip and at least 50 one above the
    top value; in the 8x8 chroma blocks of block size 16 at least 10 each.  Observed (below 0 / above top): block size 8, 8 bits
    815 / 759 luma blocks and 883 / 807 chroma blocks, 10 bits 801 / 766 and 878 / 826; the chroma of block size 16: 249 / 228 at
    8 bits, 228 / 213 at 10."""
    o = observe(bd, 8)
    assert o["clip_lo_y"] + o["clip_lo_uv"] >= 50 and o["clip_hi_y"] + o["clip_hi_uv"] >= 50, o
    o = observe(bd, 16)
    assert o["clip_lo_y"] == 0 and o["clip_hi_y"] == 0, o       # 16x16 luma blocks upsample nothing
    assert o["clip_lo_uv"] >= 10 and o["clip_hi_uv"] >= 10, o


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_reconstruction_is_pinned_at_both_ends(bd, bs):
    """at least 1000 samples of the oracle's reconstruction equal 0 and at least 1000 the top value.  Observed (at 0 / at top): 8 bits
    52522 / 55409 at block size 8, 62425 / 67227 at 16, 78512 / 85425 at 32; 10 bits 38441 / 50141, 40622 / 45352, 38539 / 45224."""
    o = observe(bd, bs)
    assert o["rec_at_0"] >= 1000 and o["rec_at_top"] >= 1000, o


if __name__ == "__main__":
    import time
    for bd in DEPTHS:
        for bs in SIZES:
            t = time.time()
            print(bd, bs, observe(bd, bs), "%.1f s" % (time.time() - t), flush=True)
