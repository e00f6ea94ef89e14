"""The two users of csrc/subpel.hpp held to each other, with no oracle in between: where k_inter_pipe codes no residual (skip flag 1)
its reconstruction IS its prediction — luma from the candidate path of the quarter-sample round (mc_h16 + mc_rows7 + mc_v7), chroma
from mc_row<4, ., 2, 6> — and that must equal, bit for bit, what k_mc's general path (Context.mc_list, regular filter) predicts at the
final vector from the same reference plane.

The frames are tests/inter_clips.py half_sample_frames at 72 x 40 and the coarsest quantiser.  One such frame is 45 blocks and cannot
hold 16 blocks in each of three classes of vector, so a depth's job is the three frames, one launch.  The test fails unless at least
16 compared blocks per depth have a fraction along x only, 16 along y only, 16 along both, and one has a window that reaches outside
the plane; tests/test_inter_clips.py shows with the oracle alone that the frames provide them.

What this does not see: the content is the checker, so every fractional vector is a half-sample one and only phase 8 of the tap tables
is compared, no quarter phase; and at 8 bits the horizontal pass of both kernels is the same subpel.hpp fir8_u8, so an error in it
shows on both sides alike (the 10-bit horizontal passes and all vertical passes are separate code).  The oracle tests
(test_gpu_inter_content.py, test_gpu_mc.py) cover both."""
import numpy as np
import pytest

import inter_clips as IC

pytestmark = pytest.mark.gpu
W, H, Q = IC.HALF_W, IC.HALF_H, IC.HALF_Q


def mc_blocks(ctx, av1mi, ref, bd, size_id, bs, xs, ys, mvx, mvy):
    """k_mc's prediction of the bs x bs blocks at (xs, ys) displaced by (mvx, mvy) 1/16 samples, regular filter: [n, bs, bs]"""
    dt = ref.dtype
    h, w = ref.shape
    lst = np.zeros(len(xs), av1mi.MC_BLK_DTYPE)
    lst["x"], lst["y"], lst["mvx"], lst["mvy"] = xs, ys, mvx, mvy
    d_ref, d_lst, d_dst = ctx.to_device(ref), ctx.to_device(lst), ctx.to_device(np.zeros((h, w), dt))
    ctx.mc_list(size_id, d_ref, w, w, h, d_dst, w, bd, d_lst, len(lst))
    got = d_dst.download((h, w), dt)
    d_ref.free(); d_lst.free(); d_dst.free()
    return np.stack([got[y:y + bs, x:x + bs] for x, y in zip(xs, ys)])


@pytest.mark.parametrize("bd", [8, 10])
def test_skipped_blocks_equal_k_mc_at_the_final_vector(ctx, av1mi, bd):
    S, R = IC.stack(IC.half_sample_frames(W, H, bd))
    got = ctx.inter_encode_arrays(S, R, bd, Q, 8)
    count = dict(x_only=0, y_only=0, both=0, outside=0)
    for f in range(S[0].shape[0]):
        mvs, skip = got["mvs"][f].astype(int), got["skip"][f]
        for k, m in IC.vector_classes(mvs, skip, W, H).items():
            count[k] += int(m.sum())
        b = np.flatnonzero(skip)
        if not len(b):
            continue
        bx, by = b % (W // 8), b // (W // 8)
        # luma: 8x8 (size id 1), the vector of 1/8 samples doubled to k_mc's 1/16; chroma: 4x4 (size id 0) at half the position, the
        # same numbers being the vector in 1/16 chroma samples
        planes = (("rec_y", 0, 1, 8, 2), ("rec_u", 1, 0, 4, 1), ("rec_v", 2, 0, 4, 1))
        for key, p, size_id, bs, scale in planes:
            exp = mc_blocks(ctx, av1mi, R[p][f], bd, size_id, bs, bx * bs, by * bs, mvs[b, 0] * scale, mvs[b, 1] * scale)
            rec = np.stack([got[key][f][y:y + bs, x:x + bs] for x, y in zip(bx * bs, by * bs)])
            bad = np.flatnonzero((rec != exp).any(axis=(1, 2)))
            assert not len(bad), ("%d bit, frame %d, %s: k_inter_pipe's prediction differs from k_mc's in blocks %s (vectors %s)"
                                  % (bd, f, key, b[bad][:6].tolist(), mvs[b[bad][:6]].tolist()))
    print("%d bit: compared blocks by class %s" % (bd, count))
    assert count["x_only"] >= 16 and count["y_only"] >= 16 and count["both"] >= 16 and count["outside"] >= 1, count
