"""The fused deblocking + CDEF kernel (av1mi_deblock_cdef_frames) against the two kernels it replaces, bit for bit: the CDEF output
everywhere, the deblocked planes on exactly the rows loop restoration reads, and loop restoration run on both results; and a small
GOP session against what the commit before the fusion produced (tests/golden/deblock_cdef_session.json)."""
import json
import os
import sys

import numpy as np
import pytest

from lf_util import random_mi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


def lr_rows(h, ss):
    """the rows of a deblocked plane of h rows that k_lr stages (lr_kernel.hip): per stripe the three rows above its first written row
    and below its last, clamped into the plane, then — where they lie beyond the stripe — clamped to two rows from its boundary"""
    SH, off, rows = 64 >> ss, 8 >> ss, set()
    for stripe in range((h + off + SH - 1) // SH):
        sstart = stripe * SH - off
        send = sstart + SH - 1
        y0, y1 = max(sstart, 0), min(send, h - 1)
        if y0 > y1:
            continue
        for y in list(range(y0 - 3, y0)) + list(range(y1 + 1, y1 + 4)):
            y = min(max(y, 0), h - 1)
            if y < sstart:
                rows.add(max(sstart - 2, y))
            elif y > send:
                rows.add(min(send + 2, y))
    return sorted(rows)


def test_lr_rows_are_four_at_every_stripe_boundary():
    """the rule above in closed form, as deblock_cdef_kernel.hip states it: rows 64k - 10 .. 64k - 7 (32k - 6 .. 32k - 3 in chroma) for
    every k >= 1 whose stripe exists (64k - 8 < h), for every plane height the coded sizes give"""
    for ss in (0, 1):
        SH, off = 64 >> ss, 8 >> ss
        for h in range(4, 400, 4):
            exp = [k * SH - off - 2 + i for k in range(1, h // SH + 2) if k * SH - off < h for i in range(4)]
            assert lr_rows(h, ss) == exp and (not exp or exp[-1] < h), (h, ss)


def _planes(rng, nf, h, w, bd):
    """noise, a little smooth structure, and hard edges at the superblock boundaries +- 0 .. 3 samples (so that filters across a
    superblock boundary fire, and so do the flat ones next to them)"""
    mx = (1 << bd) - 1
    out = []
    for hh, ww, sb in ((h, w, 64), (h // 2, w // 2, 32), (h // 2, w // 2, 32)):
        a = np.empty((nf, hh, ww), np.int64)
        for f in range(nf):
            yy, xx = np.mgrid[0:hh, 0:ww]
            img = (mx * 0.45 + mx * 0.1 * np.sin(xx / 19.0 + f) + mx * 0.08 * np.cos(yy / 13.0)).astype(np.int64)
            img += rng.integers(-2, 3, (hh, ww)) << (bd - 8)
            step = mx // 14      # small enough for the masks of a high level, large enough to be seen
            for e in range(sb, ww, sb):
                img[:, e + int(rng.integers(-3, 4)):] += int(rng.choice([-1, 1])) * step
            for e in range(sb, hh, sb):
                img[e + int(rng.integers(-3, 4)):, :] += int(rng.choice([-1, 1])) * step
            img[hh // 3:hh // 3 + 6] += rng.integers(-mx // 6, mx // 6, (6, ww))      # a noisy band
            a[f] = img
        out.append(np.clip(a, 0, mx).astype(np.uint8 if bd == 8 else np.uint16))
    return out


def _maps(rng, O, kind, nf, h, w, lvl):
    """(mi_y, mi_uv) [frames or 1, h/4, w/4] as the GOP session builds them (gop_session.hip), or random per frame"""
    if kind == "random":
        return (np.stack([random_mi(rng, O, h, w, 0) for _ in range(nf)]), np.stack([random_mi(rng, O, h // 2, w // 2, 1) for _ in range(nf)]))
    ty, tc = (5, 4) if kind == "key32" else (3, 2)      # log2 transform size: 32x32 / 16x16, or 8x8 / 4x4
    lv, lh, lc = lvl
    return (np.full((1, h // 4, w // 4), O.lf_mi(ty, ty, lv, lh, 0, 1, 1), np.uint32),
            np.full((1, h // 8, w // 8), O.lf_mi(tc, tc, lc, lc, 0, 1, 1), np.uint32))


def _strengths(rng, nf, nsb, per_frame):
    """CDEF strength sets per superblock: random, with primary 0, secondary 0, both, and 'off' (255) among them"""
    sb = np.stack([rng.integers(0, 16, (nf, nsb)), rng.integers(0, 4, (nf, nsb)), rng.integers(0, 16, (nf, nsb)), rng.integers(0, 4, (nf, nsb))], -1).astype(np.uint8)
    fixed = [(0, 2, 0, 1), (9, 0, 5, 0), (0, 0, 0, 0), (15, 3, 15, 3), (255, 0, 0, 0), (4, 3, 0, 2)]
    for i in range(nsb):
        if i % 2 == 0 or nsb == 1:
            sb[:, i] = fixed[(i // 2) % len(fixed)]
    if nsb == 1 and nf == 1:
        sb[0, 0] = (7, 1, 6, 2)
    return sb if per_frame else sb[:1]


def _random_units(rng, O, unit, h, w):
    u = np.zeros((O.lr_units(unit, h), O.lr_units(unit, w), 8), np.int8)
    for r in range(u.shape[0]):
        for c in range(u.shape[1]):
            t = int(rng.integers(0, 3))
            if t == 1:
                u[r, c] = O.lr_unit_wiener((rng.integers(-5, 11), rng.integers(-23, 9), rng.integers(-17, 47)),
                                           (rng.integers(-5, 11), rng.integers(-23, 9), rng.integers(-17, 47)))
            elif t == 2:
                u[r, c] = O.lr_unit_sgr(int(rng.integers(0, 16)), int(rng.integers(-96, 32)), int(rng.integers(-32, 96)))
    if u.shape[0] * u.shape[1] > 1:
        u[0, 0] = O.lr_unit_wiener((3, -7, 15), (2, -5, 20))      # at least one unit filters across a stripe boundary
    return u


def _both_ways(ctx, av1mi, O, rng, w, h, nf, bd, kind, lvl, sharp):
    """runs the two kernels and the fused one, then loop restoration on both; returns what the assertions need"""
    rec = _planes(rng, nf, h, w, bd)
    mi_y, mi_c = _maps(rng, O, kind, nf, h, w, lvl)
    nsb = ((w + 63) // 64) * ((h + 63) // 64)
    sb = _strengths(rng, nf, nsb, per_frame=kind != "key8")
    if kind in ("key8", "key32"):
        skip8 = np.zeros((1, h // 8, w // 8), np.uint8)
    else:       # inter: random skip flags per frame, and one superblock with every block skipped
        skip8 = (rng.random((nf, h // 8, w // 8)) < 0.35).astype(np.uint8)
        skip8[:, :8, :8] = 1
    damping = 3 + int(rng.integers(0, 4))
    dt = rec[0].dtype
    d_rec = [ctx.to_device(a) for a in rec]
    d_mi = [ctx.to_device(mi_y), ctx.to_device(mi_c)]
    d_sb, d_skip = ctx.to_device(sb), ctx.to_device(skip8)
    mfs = [0 if m.shape[0] == 1 else m.shape[1] * m.shape[2] for m in (mi_y, mi_c)]
    sbs = 0 if sb.shape[0] == 1 else nsb
    sks = 0 if skip8.shape[0] == 1 else skip8.shape[1] * skip8.shape[2]
    # the two kernels: deblocking of each plane, CDEF
    dbl_a = [ctx.to_device(np.zeros_like(a)) for a in rec]
    cdef_a = [ctx.to_device(np.zeros_like(a)) for a in rec]
    for p in range(3):
        ww, hh, c = (w, h, 0) if p == 0 else (w // 2, h // 2, 1)
        ctx.deblock_frames(d_rec[p], ww, dbl_a[p], ww, ww, hh, bd, c, d_mi[c], ww // 4, mfs[c], sharp, nf)
    ctx.cdef_frames(av1mi.CdefJob(w, h, bd, nf, damping, w, w // 2, *[b.ptr for b in dbl_a + cdef_a], d_sb.ptr, sbs, d_skip.ptr, sks))
    # the fused kernel: the deblocked planes pre-filled with a sentinel
    dbl_b = [ctx.to_device(np.full(a.shape, SENTINEL * 0x0101 if bd > 8 else SENTINEL, dt)) for a in rec]
    cdef_b = [ctx.to_device(np.zeros_like(a)) for a in rec]
    ctx.deblock_cdef_frames(av1mi.DeblockCdefJob(w, h, bd, nf, damping, sharp, w, w // 2, w, w // 2, w, w // 2, *[b.ptr for b in d_rec + dbl_b + cdef_b],
                                                 d_mi[0].ptr, d_mi[1].ptr, w // 4, w // 8, mfs[0], mfs[1], d_sb.ptr, sbs, d_skip.ptr, sks))
    # loop restoration + decision on both
    unit = 64
    uy, uc = _random_units(rng, O, unit, h, w), _random_units(rng, O, unit, h // 2, w // 2)
    mx = (1 << bd) - 1
    src = [np.clip(a.astype(int) + rng.integers(-3, 4, a.shape), 0, mx).astype(dt) for a in rec]
    d_src, d_uy, d_uc = [ctx.to_device(a) for a in src], ctx.to_device(uy), ctx.to_device(uc)
    res = {}
    for name, dbl, cdef in (("a", dbl_a, cdef_a), ("b", dbl_b, cdef_b)):
        out = [ctx.to_device(np.zeros_like(a)) for a in rec]
        on = ctx.to_device(np.full(3 * nf, 9, np.uint8))
        scr = ctx.alloc(ctx.lr_yuv_decide_scratch_bytes(h, nf))
        ctx.lr_yuv_decide(av1mi.LrDecideJob(w, h, bd, nf, unit, w, w // 2, *[b.ptr for b in cdef + dbl + out + d_src], d_uy.ptr, d_uc.ptr, 0, 0, scr.ptr, on.ptr))
        res[name] = dict(dbl=[b.download(a.shape, dt) for b, a in zip(dbl, rec)], cdef=[b.download(a.shape, dt) for b, a in zip(cdef, rec)],
                         lr=[b.download(a.shape, dt) for b, a in zip(out, rec)], on=on.download((3 * nf,), np.uint8))
        for b in out + [on, scr]:
            b.free()
    for b in d_rec + d_mi + [d_sb, d_skip, d_uy, d_uc] + d_src + dbl_a + dbl_b + cdef_a + cdef_b:
        b.free()
    return rec, res


def _check(rec, res, h, bd, what):
    a, b = res["a"], res["b"]
    sent = SENTINEL * 0x0101 if bd > 8 else SENTINEL
    changed = 0
    for p in range(3):
        assert (a["cdef"][p] == b["cdef"][p]).all(), (what, "CDEF output", p, np.argwhere(a["cdef"][p] != b["cdef"][p])[:4])
        rows = lr_rows(h if p == 0 else h // 2, int(p > 0))
        assert (a["dbl"][p][:, rows] == b["dbl"][p][:, rows]).all(), (what, "deblocked rows", p)
        others = np.setdiff1d(np.arange(a["dbl"][p].shape[1]), rows)
        assert (b["dbl"][p][:, others] == sent).all(), (what, "the fused kernel wrote a row loop restoration does not read", p)
        assert (a["lr"][p] == b["lr"][p]).all(), (what, "loop restoration", p)
        changed += int((a["dbl"][p] != rec[p]).sum()) + int((a["cdef"][p] != a["dbl"][p]).sum())
    assert a["on"].tolist() == b["on"].tolist() and set(a["on"].tolist()) <= {0, 1}, (what, a["on"], b["on"])
    return changed


# 192x128: interior superblocks, all four picture borders, corners; 136x88: partial superblocks at the right and bottom, a chroma
# block narrower than 32; 64x64: a single superblock with every side a picture border.  The 32x32 key map needs width % 32 == 0.
SHAPES = [(192, 128, 2), (136, 88, 2), (64, 64, 1)]
CASES = [(w, h, nf, bd, kind) for (w, h, nf) in SHAPES for bd in (8, 10) for kind in ("key8", "key32", "inter", "random")
         if not (kind == "key32" and w % 32)]


@pytest.mark.parametrize("w,h,nf,bd,kind", CASES)
def test_fused_equals_deblock_then_cdef(ctx, av1mi, O, w, h, nf, bd, kind):
    rng = np.random.default_rng(w * 131 + h * 7 + bd + len(kind))
    changed = 0
    # two filter levels, one low and one near the maximum; sharpness 0 and a non-zero value
    for lvl, sharp in (((4, 3, 5), 0), ((60, 63, 58), 0), ((6, 5, 4), 5), ((61, 57, 63), 2)):
        rec, res = _both_ways(ctx, av1mi, O, rng, w, h, nf, bd, kind, lvl, sharp)
        changed += _check(rec, res, h, bd, (w, h, bd, kind, lvl, sharp))
    assert changed > 0      # the filters did something


def test_argument_checks(ctx, av1mi):
    d = ctx.alloc(64 * 64 * 2)
    ok = lambda **kw: av1mi.DeblockCdefJob(**dict(dict(width=64, height=64, bit_depth=8, nframes=0, damping=3, sharpness=0, rec_stride_y=64, rec_stride_uv=32,
                                                    dbl_stride_y=64, dbl_stride_uv=32, dst_stride_y=64, dst_stride_uv=32, mi_stride_y=16, mi_stride_uv=8,
                                                    d_mi_y=d.ptr, d_mi_uv=d.ptr, d_sb_strength=d.ptr, d_skip8=d.ptr,
                                                    **{"d_%s_%s" % (a, p): d.ptr + 1024 * i for i, (a, p) in enumerate((a, p) for a in ("rec", "dbl", "dst") for p in "yuv")}), **kw))
    ctx.deblock_cdef_frames(ok())      # nframes 0: checked, nothing launched
    for bad in (dict(width=68), dict(damping=7), dict(sharpness=8), dict(rec_stride_y=60), dict(mi_stride_uv=7), dict(d_mi_y=None), dict(d_dbl_u=d.ptr),
                dict(d_dst_v=d.ptr + 1028), dict(bit_depth=12)):
        with pytest.raises(av1mi.Av1miError):
            ctx.deblock_cdef_frames(ok(**bad))
    d.free()


@pytest.mark.parametrize("case", ["192x136", "200x136_true_197x131"])
def test_session_equals_the_record_of_the_commit_before(ctx, av1mi, case):
    """tile payloads, restoration flags and reference planes of one GOP of a small session — a size that takes the fused kernel, and a
    true size that is no multiple of 8 and keeps the two kernels — against the record taken at the commit named in the fixture"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_filter_session as R
    with open(R.GOLDEN) as f:
        golden = json.load(f)
    assert len(golden["recorded_from_commit"]) >= 7
    got = R.run_case(av1mi, ctx, R.CASES[case])
    exp = golden["cases"][case]
    assert len(got) == len(exp) == R.FRAMES
    for t, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (case, "batch", t, {k: (g[k], e[k]) for k in e if g[k] != e[k]})
