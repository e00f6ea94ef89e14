"""GPU parity of the in-loop filters on the hard content of tests/filter_clips.py: av1mi_deblock_frames, av1mi_cdef_frames, the fused
av1mi_deblock_cdef_frames, av1mi_lr_frames / av1mi_lr_frames_decide and the error sums of av1mi_cdef_search / av1mi_lf_search against the
CPU oracle (oracle/av1o_deblock.c, av1o_cdef.c, av1o_lr.c), bit for bit, every clip a frame of one job.  What lf_util.test_image and
the searches' mild generators never do happens here on many lines and blocks: deblocking edges at and one above every mask threshold,
narrow-filter clamps next to 0 and the top value, CDEF blocks whose directions tie, variance 0 and at its cap, the 0xFFFF mark beside
samples at the top value, Wiener intermediates beyond their range, self-guided boxes of two-level content, squared errors of the full
range.  tests/test_filter_clips.py shows (CPU) that the clips do these things and that dav1d filters them as the oracle does."""
import numpy as np
import pytest

import cdef_search_ref
import filter_clips as FC
import lf_search_ref
from lf_util import random_mi
from test_gpu_deblock_cdef import lr_rows

pytestmark = pytest.mark.gpu
DEPTHS = (8, 10)
NAMES = FC.NAMES

_clips, _expected = {}, {}


def clip(name, w, h, bd):
    key = (name, w, h, bd)
    if key not in _clips:
        _clips[key] = FC.clip(name, w, h, bd)
    return _clips[key]


def cached(key, make):
    """an oracle result, computed once and shared by the tests that run the same clip with the same parameters; never changed"""
    if key not in _expected:
        _expected[key] = make()
    return _expected[key]


def sentinel(bd):
    return 0xA5 if bd == 8 else 0xA5A5


def stacked(w, h, bd):
    return FC.stack([clip(n, w, h, bd) for n in NAMES])


def differs(got, exp):
    return "at %s: got %s, expected %s" % (np.argwhere(got != exp)[:4].tolist(), got[got != exp][:4].tolist(), exp[got != exp][:4].tolist())


# ---- deblocking maps: (luma, chroma), [1 or frames, units down, units across]
def lf_maps(O, kind, w, h, lv, nf):
    if kind == "random":
        rng = np.random.default_rng([w, h, lv[0]])
        return (np.stack([random_mi(rng, O, h, w, 0) for _ in range(nf)]), np.stack([random_mi(rng, O, h // 2, w // 2, 1) for _ in range(nf)]))
    y = np.full((1, h // 4, w // 4), int(O.lf_mi(3, 3, lv[0], lv[1], 0, 1, 1)), np.uint32)
    c = np.full((1, h // 8, w // 8), int(O.lf_mi(2, 2, lv[2], lv[2], 0, 1, 1)), np.uint32)
    if kind == "key32":      # 32x32 luma / 16x16 chroma transforms over the complete superblock rows, as the session's key frames have them
        rows = h // 64 * 64
        y[:, :rows // 4] = int(O.lf_mi(5, 5, lv[0], lv[1], 0, 1, 1))
        c[:, :rows // 8] = int(O.lf_mi(4, 4, lv[2], lv[2], 0, 1, 1))
    return y, c


def oracle_deblocked(O, name, w, h, bd, kind, k, f, mi, sharp):
    """the three deblocked planes of clip `name` as frame f of the job under map kind / level set k"""
    def make():
        planes = clip(name, w, h, bd)
        return [O.deblock_plane(planes[p], bd, int(p > 0), mi[int(p > 0)][f % len(mi[int(p > 0)])], sharp) for p in range(3)]
    return cached(("dbl", name, w, h, bd, kind, k, f if kind == "random" else 0), make)


# (map kind, index into FC.LF_SETS): the uniform map shared by the frames (frame stride 0) with every level set; the key map with a high
# level and with sharpness 5; random transform sizes, levels, skip and edge flags per 64x64 with a map per frame
LF_CASES = [("uniform", k) for k in range(len(FC.LF_SETS))] + [("key32", 1), ("key32", 2), ("random", 0), ("random", 3)]


@pytest.mark.parametrize("kind,k", LF_CASES)
@pytest.mark.parametrize("w,h", FC.SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_deblock_frames(ctx, O, bd, w, h, kind, k):
    """the 12 clips as frames of one job per plane; the output buffer is 8 rows longer than the job, and those rows keep their sentinel"""
    lv, sharp = FC.LF_SETS[k]
    nf = len(NAMES)
    src = stacked(w, h, bd)
    mi = lf_maps(O, kind, w, h, lv, nf)
    d_mi = [ctx.to_device(m) for m in mi]
    for p in range(3):
        c = int(p > 0)
        ph, pw = h >> c, w >> c
        d_src = ctx.to_device(src[p])
        d_dst = ctx.to_device(np.full((nf * ph + 8, pw), sentinel(bd), src[p].dtype))
        ctx.deblock_frames(d_src, pw, d_dst, pw, pw, ph, bd, c, d_mi[c], pw // 4, 0 if len(mi[c]) == 1 else (ph // 4) * (pw // 4), sharp, nf)
        got = d_dst.download((nf * ph + 8, pw), src[p].dtype)
        d_src.free(), d_dst.free()
        assert (got[nf * ph:] == sentinel(bd)).all(), "plane %d: rows beyond the job were written" % p
        for f, name in enumerate(NAMES):
            exp = oracle_deblocked(O, name, w, h, bd, kind, k, f, mi, sharp)[p]
            g = got[f * ph:(f + 1) * ph]
            assert (g == exp).all(), "clip %s, plane %d, %dx%d, %d bit, %s map, levels %s sharpness %d: %s" % (name, p, w, h, bd, kind, lv, sharp, differs(g, exp))
    for b in d_mi:
        b.free()


# ---- CDEF
ALL_STRENGTHS = np.array(FC.CDEF_SETS + (FC.CDEF_OFF, (7, 1, 6, 2)), np.uint8)


def cdef_maps(w, h, nf, damping, per_frame):
    """strength records [frames or 1, superblocks, 4] in turn — every set meets every superblock position over the frames and dampings,
    255 (off) among them — and skip flags [frames or 1, h / 8, w / 8]: a quarter of the blocks, and the first superblock whole in frame 0"""
    nsb = ((w + 63) // 64) * ((h + 63) // 64)
    n = nf if per_frame else 1
    st = np.stack([ALL_STRENGTHS[(np.arange(nsb) + f + 2 * damping) % len(ALL_STRENGTHS)] for f in range(n)])
    skip = (np.random.default_rng([w, h, damping]).random((n, h // 8, w // 8)) < 0.25).astype(np.uint8)
    skip[0, :8, :8] = 1
    return st, skip


def oracle_cdef(O, key, planes, bd, damping, st, skip):
    return cached(("cdef",) + key + (damping, st.tobytes(), skip.tobytes()), lambda: O.cdef_frame(planes[0], planes[1], planes[2], bd, damping, st, skip))


@pytest.mark.parametrize("damping", [3, 4, 5, 6])
@pytest.mark.parametrize("w,h", FC.SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_cdef_frames(ctx, O, bd, w, h, damping):
    """damping 3 and 5 with strength and skip maps per frame, 4 and 6 with shared ones; at 136x136 superblock (1, 1) takes the interior
    route and the eight around it the one with marks"""
    nf = len(NAMES)
    st, skip = cdef_maps(w, h, nf, damping, per_frame=damping % 2 == 1)
    got = ctx.cdef_arrays(*stacked(w, h, bd), bd, damping, st, skip)
    for f, name in enumerate(NAMES):
        exp = oracle_cdef(O, (name, w, h, bd), clip(name, w, h, bd), bd, damping, st[f % len(st)], skip[f % len(skip)])
        for p in range(3):
            assert (got[p][f] == exp[p]).all(), "clip %s, plane %d, %dx%d, %d bit, damping %d: %s" % (name, p, w, h, bd, damping, differs(got[p][f], exp[p]))


# ---- the fused kernel against the ORACLE's deblocking then CDEF
@pytest.mark.parametrize("kind,k,damping", [("uniform", 0, 3), ("uniform", 1, 6), ("key32", 3, 4), ("random", 2, 5)])
@pytest.mark.parametrize("w,h", FC.SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_deblock_cdef_frames(ctx, av1mi, O, bd, w, h, kind, k, damping):
    """av1mi_deblock_cdef_frames: the CDEF output everywhere, the deblocked planes on the rows restoration reads (lr_rows), the sentinel
    on every other row"""
    lv, sharp = FC.LF_SETS[k]
    nf = len(NAMES)
    rec = stacked(w, h, bd)
    mi = lf_maps(O, kind, w, h, lv, nf)
    st, skip = cdef_maps(w, h, nf, damping, per_frame=kind == "random")
    dt = rec[0].dtype
    d_rec = [ctx.to_device(a) for a in rec]
    d_dbl = [ctx.to_device(np.full(a.shape, sentinel(bd), dt)) for a in rec]
    d_dst = [ctx.to_device(np.zeros_like(a)) for a in rec]
    d_mi = [ctx.to_device(m) for m in mi]
    d_st, d_skip = ctx.to_device(st), ctx.to_device(skip)
    mfs = [0 if len(m) == 1 else m.shape[1] * m.shape[2] for m in mi]
    ctx.deblock_cdef_frames(av1mi.DeblockCdefJob(w, h, bd, nf, damping, sharp, w, w // 2, w, w // 2, w, w // 2, *[b.ptr for b in d_rec + d_dbl + d_dst],
                                                 d_mi[0].ptr, d_mi[1].ptr, w // 4, w // 8, mfs[0], mfs[1], d_st.ptr, 0 if len(st) == 1 else st.shape[1],
                                                 d_skip.ptr, 0 if len(skip) == 1 else skip.shape[1] * skip.shape[2]))
    dbl = [b.download(a.shape, dt) for b, a in zip(d_dbl, rec)]
    dst = [b.download(a.shape, dt) for b, a in zip(d_dst, rec)]
    for b in d_rec + d_dbl + d_dst + d_mi + [d_st, d_skip]:
        b.free()
    for f, name in enumerate(NAMES):
        e_dbl = oracle_deblocked(O, name, w, h, bd, kind, k, f, mi, sharp)
        e_cdef = oracle_cdef(O, (name, w, h, bd, kind, k, f if kind == "random" else 0), e_dbl, bd, damping, st[f % len(st)], skip[f % len(skip)])
        what = "clip %s, %dx%d, %d bit, %s map, levels %s sharpness %d, damping %d" % (name, w, h, bd, kind, lv, sharp, damping)
        for p in range(3):
            assert (dst[p][f] == e_cdef[p]).all(), "%s: CDEF output, plane %d: %s" % (what, p, differs(dst[p][f], e_cdef[p]))
            rows = lr_rows(h >> int(p > 0), int(p > 0))
            assert (dbl[p][f][rows] == e_dbl[p][rows]).all(), "%s: deblocked rows, plane %d: %s" % (what, p, differs(dbl[p][f][rows], e_dbl[p][rows]))
            others = np.setdiff1d(np.arange(h >> int(p > 0)), rows)
            assert (dbl[p][f][others] == sentinel(bd)).all(), "%s: plane %d: a row restoration does not read was written" % (what, p)


# ---- restoration, with the decision and its sums
KINDS = ("wiener", "sgr", "mixed")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ss", [0, 1])
@pytest.mark.parametrize("w,h", FC.LR_SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_lr_frames_and_decide(ctx, O, bd, w, h, ss, kind):
    """every clip's plane with Wiener units at the tap ends / the self-guided sets 0, 9, 10, 14, 15 with their weights at the ends / both
    and no filter in turn; units of 64, and of 32 where the plane is a chroma one; rows w, w + 2 or w + 8 apart (each width meets each
    over the three kinds), the padding columns keep their sentinel.  The deblocked plane is the inverse of the CDEF plane, so a wrong row
    at a stripe boundary is wrong by the full range.  The decision's source is the inverse of the restored plane: its sums are those of
    full-swing errors, equal to exact Python-int sums per frame and stripe, and the flags are O.lr_select's."""
    nf, top = len(NAMES), FC.top_of(bd)
    unit = 32 if ss else 64
    stride = w + (0, 2, 8)[(KINDS.index(kind) + FC.LR_SIZES.index((w, h))) % 3]
    dt = np.uint8 if bd == 8 else np.uint16
    cdef = np.full((nf, h, stride), sentinel(bd), dt)
    for f, name in enumerate(NAMES):
        cdef[f, :, :w] = FC.plane(name, w, h, bd)
    dbl = (top - cdef.astype(np.int64)).astype(dt)
    units = np.stack([FC.lr_unit_map(O, w, h, unit, kind, shift=FC.lr_shift(f)) for f in range(nf)])
    lr = np.stack([cached(("lr", NAMES[f], w, h, bd, ss, kind), lambda: O.lr_plane(cdef[f, :, :w], dbl[f, :, :w], bd, ss, unit, units[f])) for f in range(nf)])
    src = np.full_like(cdef, sentinel(bd))
    src[:, :, :w] = top - lr.astype(np.int64)
    d_c, d_d, d_u, d_s = ctx.to_device(cdef), ctx.to_device(dbl), ctx.to_device(units), ctx.to_device(src)
    ufs = units.shape[1] * units.shape[2]
    # av1mi_lr_frames
    d_o = ctx.to_device(np.full_like(cdef, sentinel(bd)))
    ctx.lr_frames(d_c, d_d, d_o, stride, w, h, bd, ss, unit, d_u, ufs, nf)
    plain = d_o.download(cdef.shape, dt)
    d_o.free()
    # av1mi_lr_frames_decide
    d_o, d_on = ctx.to_device(np.full_like(cdef, sentinel(bd))), ctx.to_device(np.full(nf, 7, np.uint8))
    nbytes = ctx.lr_decide_scratch_bytes(h, ss, nf)
    d_scr = ctx.alloc(nbytes)
    ctx.lr_frames_decide(d_c, d_d, d_o, stride, w, h, bd, ss, unit, d_u, ufs, nf, d_s, d_scr, d_on)
    got, on = d_o.download(cdef.shape, dt), d_on.download((nf,), np.uint8)
    sums = d_scr.download((nf, nbytes // (16 * nf), 2), np.uint64)      # [frame, stripe, (restored, CDEF)]
    for b in (d_c, d_d, d_u, d_s, d_o, d_on, d_scr):
        b.free()
    what = "%dx%d rows %d apart, %d bit, ss %d, %s units of %d" % (w, h, stride, bd, ss, kind, unit)
    SH, off = 64 >> ss, 8 >> ss
    stripes = [slice(max(0, k * SH - off), min(h, (k + 1) * SH - off)) for k in range((h + off + SH - 1) // SH)]
    assert sums.shape[1] == len(stripes)
    for name, out in (("av1mi_lr_frames", plain), ("av1mi_lr_frames_decide", got)):
        for f in range(nf):
            assert (out[f, :, :w] == lr[f]).all(), "%s, clip %s, %s: %s" % (name, NAMES[f], what, differs(out[f, :, :w], lr[f]))
        assert (out[:, :, w:] == sentinel(bd)).all(), "%s, %s: the padding columns of the output were written" % (name, what)
    sq = lambda a, f, r: int(((a[f, r].astype(np.int64) - src[f, r, :w].astype(np.int64)) ** 2).sum())
    exp = [[[sq(lr, f, r), sq(cdef[:, :, :w], f, r)] for r in stripes] for f in range(nf)]
    assert sums.tolist() == exp, what
    assert on.tolist() == [O.lr_select((src[f, :, :w],), (cdef[f, :, :w],), (lr[f],), bd, ss)[1][0] for f in range(nf)], what


# ---- the searches' error sums at full swing
SEARCH_CLIPS = ("binary", "full_swing_blocks", "big_steps")
SEARCH_CASES = [(136, 72, (130, 70)), (64, 64, None)]


def search_frames(w, h, bd):
    """(reconstruction, source): the clips of SEARCH_CLIPS as frames, the source the inverse — every sample of the binary frame errs by the
    top value under a candidate that filters nothing: 6144 x 1023^2 a superblock at 10 bits, beyond 2^32
    (tests/test_filter_clips.py test_full_swing_sums_need_64_bits has the partial sums per lane and per wave)"""
    rec = FC.stack([clip(n, w, h, bd) for n in SEARCH_CLIPS])
    return list(rec), [FC.top_of(bd) - a for a in rec]


@pytest.mark.parametrize("w,h,true_size", SEARCH_CASES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_cdef_search_sums_at_full_swing(ctx, av1mi, O, bd, w, h, true_size):
    """the cost table is cdef_search_ref.table's, the picks the first of equal minima, the tails past the arrays untouched (_search)"""
    from test_gpu_cdef_search import _search
    R, bits = cdef_search_ref, 3
    rec, src = search_frames(w, h, bd)
    nf = len(SEARCH_CLIPS)
    skip = (np.random.default_rng([w, bd]).random((nf, h // 8, w // 8)) < 0.1).astype(np.uint8)
    params = av1mi.policy_frame_params(128, bd, 1)
    y, uv = R.sets(params, bits)
    table, records, idx = _search(ctx, av1mi, rec, src, skip, bd, bits, params, true_size)
    for f in range(nf):
        exp = cached(("cdef_search", w, h, bd, f), lambda: R.table(O, [a[f] for a in rec], [a[f] for a in src], bd, params.cdef_damping, y, uv, bits, skip[f], true_size))
        assert (table[f] == exp).all(), ("cost table", SEARCH_CLIPS[f], differs(table[f], exp))
        want = R.pick(exp, bits)
        assert idx[f].tolist() == want.tolist() and records[f].tolist() == R.records(y, uv, want).tolist(), ("picks", SEARCH_CLIPS[f])
    if bd == 10:
        assert int(table[0].max()) > 1 << 32


@pytest.mark.parametrize("w,h,true_size", SEARCH_CASES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_lf_search_sums_at_full_swing(ctx, av1mi, O, bd, w, h, true_size):
    """the sums, the choice and the header levels are lf_search_ref.search's; the tails past the arrays untouched (_search)"""
    from test_gpu_lf_search import _params, _search
    R = lf_search_ref
    rec, src = search_frames(w, h, bd)
    maps = [R.base_maps(w, h, true_size)]
    sse, choice, lv, _ = _search(ctx, av1mi, rec, src, bd, _params(av1mi, R.POLICY, bd), maps, False, true_size)
    for f in range(len(SEARCH_CLIPS)):
        e_sse, e_choice, e_lv, _ = cached(("lf_search", w, h, bd, f), lambda: R.search(O, [a[f] for a in rec], [a[f] for a in src], bd, R.POLICY, 0, maps[0][0], maps[0][1], true_size))
        assert (sse[f] == e_sse).all(), ("sums", SEARCH_CLIPS[f], sse[f].tolist(), e_sse.tolist())
        assert choice[f].tolist() == e_choice and lv[f].tolist() == e_lv, (SEARCH_CLIPS[f], choice[f], e_choice, lv[f], e_lv)
    if bd == 10:
        assert int(sse[0].max()) > 1 << 31
