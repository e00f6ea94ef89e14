"""The motion search's numpy reference (tests/me_ref.py) on the CPU: pinned to the oracle's integer search where the two overlap, then
shown to follow motion the +-8 search cannot; and the boundary of the new option (exported entry, struct sizes, refused values)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import me_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "av1-go_amd", "host", "libav1mi_host.so")


def test_integer_vectors_are_the_oracles_integer_stage(O):
    """Centres 0, range 8 = today's policy.  Frame 4 of the slow clip against frame 0 moves by exactly (5, 3) samples, so most blocks
    end the oracle's sub-sample refinement where its integer stage left them; the refinement moves a vector by 2, 4 or 6 eighths per
    component, never by 8, so a vector whose components are both multiples of 8 IS the integer stage's."""
    import synth
    for bd in (8, 10):
        Y, U, V = synth.frames(192, 136, 5, bd)
        r = O.inter_encode_frame((Y[4], U[4], V[4]), (Y[0], U[0], V[0]), bd, 120, 8)
        got = M.integer_vectors(Y[4], Y[0], bd, np.zeros((3, 3, 2), np.int16), 8).reshape(-1, 2)
        whole = (r["mvs"] % 8 == 0).all(axis=1)
        assert whole.mean() > 0.5, "too few whole-sample vectors to compare (%.2f)" % whole.mean()
        assert (got[whole] == r["mvs"][whole]).all()
        # ... and the others lie within the refinement's reach of the integer stage
        assert (np.abs(got.astype(int) - r["mvs"]) <= 6).all()


def _interior(a):
    return a[1:-1, 1:-1]


def _follows(cen, vx, vy, tol=8):
    """centres within `tol` samples of (vx, vy) per component: the +-8 integer search around them then covers the true vector"""
    return (np.abs(cen[..., 0].astype(int) - vx) <= tol) & (np.abs(cen[..., 1].astype(int) - vy) <= tol)


W, H, BD, SCALE = 640, 384, 8, 20      # (25, 15) samples per frame


def test_centres_follow_a_fast_pan():
    """640x384, 8 bit, the texture at 20 times its speed: frame 1 against frame 0 moves by (25, 15).  A centre is a multiple of 4, so
    the best one lies within 4 of the pan; 8 = the integer search's range is allowed, because that is what the centre is for.  At most
    10 % of the interior tiles may miss.  Reached on this clip by me_ref alone: 0 of 32 interior tiles miss (0 %) with coarse_range 32
    and 64; with the centres at 0 the integer vectors are off the pan in nearly every block."""
    Y, _, _ = M.pan_clip(W, H, 2, BD, SCALE)
    for cr in (32, 64):
        cen = M.coarse_centres(M.quarter_plane(Y[1], BD), M.quarter_plane(Y[0], BD), cr).reshape(H // 64, W // 64, 2)
        miss = 1.0 - _follows(_interior(cen), 25, 15).mean()
        print("coarse_range %d: %.1f %% of the interior tiles miss the pan" % (cr, 100 * miss))
        assert miss <= 0.10
        mv = M.integer_vectors(Y[1], Y[0], BD, cen, 8)
        inner = mv[8:-8, 8:-8]
        hit = ((inner[..., 0] == 200) & (inner[..., 1] == 120)).mean()
        print("coarse_range %d: %.1f %% of the interior blocks find (25, 15)" % (cr, 100 * hit))
        assert hit >= 0.90
    mv0 = M.integer_vectors(Y[1], Y[0], BD, np.zeros((H // 64, W // 64, 2), np.int16), 8)[8:-8, 8:-8]
    assert ((mv0[..., 0] == 200) & (mv0[..., 1] == 120)).mean() == 0      # out of the +-8 window's reach


def test_centres_follow_each_half_of_a_split_scene():
    """the left half pans by (25, 15), the right half by (-25, -15).  Interior = not on the picture's edge and not next to the seam
    (a tile beside it predicts from across it).  Reached by me_ref alone: 0 of 24 tiles miss (0 %)."""
    Y, _, _ = M.split_clip(W, H, 2, BD, SCALE)
    cen = M.coarse_centres(M.quarter_plane(Y[1], BD), M.quarter_plane(Y[0], BD), 64).reshape(H // 64, W // 64, 2)
    half = W // 128
    left, right = cen[1:-1, 1:half - 1], cen[1:-1, half + 1:-1]
    ok = np.concatenate([_follows(left, 25, 15).ravel(), _follows(right, -25, -15).ravel()])
    print("split scene: %.1f %% of %d interior tiles miss" % (100 * (1 - ok.mean()), ok.size))
    assert 1.0 - ok.mean() <= 0.10


def test_static_frame_and_tie_rule():
    """a frame against itself: every SAD at (0, 0) is 0 and rank 0 wins the ties a flat area produces"""
    Y, _, _ = M.pan_clip(200, 136, 1, 10, 1.0)
    Y[0][:, :64] = 512                      # a flat area: every displacement inside it ties
    r = M.search(Y[0], Y[0], 10, 8, 64)
    assert (r["centres"] == 0).all() and (r["mvs"] == 0).all()
    assert r["q_src"].shape == (34, 50) and r["centres"].shape == (3 * 4, 2)


# ---- the boundary -------------------------------------------------------------------------------------------------------------

def test_me_search_is_exported_and_the_structs_match_the_header(av1mi):
    lib = av1mi.load()
    assert hasattr(lib, "av1mi_me_search") and "av1mi_me_search" in av1mi.exported_symbols()
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "sz.c")
        open(src, "w").write('#include "av1mi.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu", sizeof(av1mi_inter_job), '
                             'sizeof(av1mi_gop_config), offsetof(av1mi_inter_job, coarse_range), offsetof(av1mi_gop_config, coarse_range));return 0;}\n')
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", os.path.join(d, "sz")])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(d, "sz")]).split()]
    assert sizes == [C.sizeof(av1mi.InterJob), C.sizeof(av1mi.GopConfig), av1mi.InterJob.coarse_range.offset, av1mi.GopConfig.coarse_range.offset]
    # appended: the fields that were there keep their places
    assert av1mi.InterJob.coarse_range.offset > av1mi.InterJob.d_ref_sel.offset and av1mi.GopConfig.coarse_range.offset > av1mi.GopConfig.quality_stats.offset


def _transcode(argv):
    host = C.CDLL(HOST)
    host.av1mi_host_run_transcode.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(2048)
    return host.av1mi_host_run_transcode("\n".join(str(a) for a in argv).encode(), buf, 2048), buf.value.decode()


@pytest.mark.parametrize("bad", ["6", "68", "-4", "x"])
def test_me_range_outside_the_rule_is_refused(bad):
    code, err = _transcode(["-i", "in.y4m", "-av1mi_me_range", bad, "out.obu"])
    assert code == 1 and "-av1mi_me_range" in err
