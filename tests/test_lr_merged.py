"""av1mi_lr_yuv_decide runs the three planes of 4:2:0 frames in ONE k_lr launch per pass (csrc/lr_kernel.hip k_lr_yuv: the planes' grids
end to end, a workgroup takes its plane and its stripe height from its index), and its decision kernel leaves the sums it has read
zero, so a session's scratch needs no zeroing launch per batch (csrc/capi.hip lr_yuv_decide_with: the rule).

Against the oracle's lr_plane / lr_select: 192x136 x 3 frames (the last stripe partial, chroma height 68) and 64x72 x 1 frame (one
column band, two luma stripes of which the second holds 16 rows), 8 and 10 bit, the kernel with and without the self-guided path; an
input where restoration cannot help (the source IS the CDEF planes: every flag 0) and a noisy one where it helps (the restored planes
plus noise of one step); calls in a row on one scratch, which must be all zero after each.  Planes this small lie whole in the
decision's sample, so the restored planes are complete whatever the decision."""
import numpy as np
import pytest

from lf_util import test_image as make_image

pytestmark = pytest.mark.gpu

UNIT = 64
LR_Y, LR_UV = [1, 3, -7, 15, 3, -7, 15, 0], [1, 0, -7, 15, 0, -7, 15, 0]      # the session's Wiener taps (csrc/gop_session.hip frame_params)
_REF = {}


def _dims(w, h):
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


def _units(O, w, h):
    return [np.tile(np.array(t, np.int8), (O.lr_units(UNIT, hh), O.lr_units(UNIT, ww), 1)) for t, (hh, ww) in zip((LR_Y, LR_UV, LR_UV), _dims(w, h))]


def _case(O, w, h, nf, bd, kind):
    """planes [plane][frame], and the oracle's restored planes, flags and selected planes: computed once per case, left unchanged"""
    key = (w, h, nf, bd, kind)
    if key not in _REF:
        rng = np.random.default_rng(w * 31 + h + bd + len(kind))
        mx = (1 << bd) - 1
        cdef = [np.stack([make_image(rng, hh, ww, bd) for _ in range(nf)]) for hh, ww in _dims(w, h)]
        dbl = [np.clip(c.astype(int) + rng.integers(-1, 2, c.shape), 0, mx).astype(c.dtype) for c in cdef]      # differs from cdef: the halo rows
        units = _units(O, w, h)
        lr = [np.stack([O.lr_plane(cdef[p][f], dbl[p][f], bd, int(p > 0), UNIT, units[p]) for f in range(nf)]) for p in range(3)]
        if kind == "same":        # restoration cannot help: nothing is closer to the source than the CDEF planes themselves
            src = cdef
        else:                     # a noisy source that lies nearer the restored planes than the CDEF planes: restoration helps
            src = [np.clip(a.astype(int) + rng.integers(-1, 2, a.shape), 0, mx).astype(a.dtype) for a in lr]
        sel = [O.lr_select([src[p][f] for p in range(3)], [cdef[p][f] for p in range(3)], [lr[p][f] for p in range(3)], bd) for f in range(nf)]
        on = [s[1] for s in sel]
        for a in cdef + dbl + src + lr:
            a.setflags(write=False)
        _REF[key] = dict(cdef=cdef, dbl=dbl, src=src, units=units, lr=lr, on=on, ref=[s[0] for s in sel])
    return _REF[key]


def _decide(ctx, av1mi, w, h, nf, bd, case, scr, no_sgr):
    d = {k: [ctx.to_device(a) for a in case[k]] for k in ("cdef", "dbl", "src", "units")}
    out = [ctx.to_device(np.full(a.shape, 3, a.dtype)) for a in case["cdef"]]
    on = ctx.to_device(np.full(3 * nf + 4, 9, np.uint8))
    try:
        ctx.lr_yuv_decide(av1mi.LrDecideJob(w, h, bd, nf, UNIT, w, w // 2, *[b.ptr for b in d["cdef"] + d["dbl"] + out + d["src"]], d["units"][0].ptr, d["units"][1].ptr,
                                            0, 0, scr.ptr, on.ptr, no_sgr))
        ctx.sync()
        return on.download((3 * nf + 4,), np.uint8), [o.download(a.shape, a.dtype) for o, a in zip(out, case["cdef"])]
    finally:
        for b in sum(d.values(), []) + out + [on]:
            b.free()


def _check(case, nf, on, out):
    assert on[:3 * nf].reshape(nf, 3).tolist() == case["on"] and (on[3 * nf:] == 9).all()
    for p in range(3):
        assert (out[p] == case["lr"][p]).all(), "plane %d: the restored plane differs from the oracle" % p
        for f in range(nf):      # what the next frame predicts from
            assert ((out[p][f] if on[3 * f + p] else case["cdef"][p][f]) == case["ref"][f][p]).all()


@pytest.mark.parametrize("no_sgr", [1, 0])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h,nf", [(192, 136, 3), (64, 72, 1)])
def test_merged_launch_equals_the_oracle_and_leaves_the_scratch_zero(ctx, av1mi, O, w, h, nf, bd, no_sgr):
    same, noisy = _case(O, w, h, nf, bd, "same"), _case(O, w, h, nf, bd, "noisy")
    assert all(v == [0, 0, 0] for v in same["on"]), "the input where restoration cannot help keeps a flag"
    assert any(any(v) for v in noisy["on"]), "the noisy input keeps no restoration: it does not test the ON side"
    nbytes = ctx.lr_yuv_decide_scratch_bytes(h, nf)
    scr = ctx.to_device(np.full(nbytes, 0xA5, np.uint8))      # a caller's scratch may hold anything before the first call
    try:
        # two calls in a row on the same scratch: the sums of the noisy call are large, and the decision kernel must have left them zero
        for case in (noisy, same, noisy):
            on, out = _decide(ctx, av1mi, w, h, nf, bd, case, scr, no_sgr)
            _check(case, nf, on, out)
            assert not scr.download((nbytes,), np.uint8).any(), "the decision left sums behind in the scratch"
    finally:
        scr.free()
