"""GPU: av1mi_lf_search (k_lf_search, k_lf_pick, k_mi_levels_frames) against its restatement (lf_search_ref.py: the oracle's deblocking
of the whole plane per candidate) — the sums, the choice and the header levels bit for bit —, and av1mi_deblock_frames /
av1mi_deblock_cdef_frames fed the written maps against the reference's deblocked planes of the chosen candidates."""
import ctypes as C

import numpy as np
import pytest

import lf_search_ref as R

pytestmark = pytest.mark.gpu

TAIL = 16
NF = 3


def _params(av1mi, levels, bd):
    p = av1mi.policy_frame_params(128, bd, 0)
    for i, v in enumerate(levels):
        p.lf_level[i] = v
    return p


def _search(ctx, av1mi, rec, src, bd, params, maps, per_frame, true_size, want_maps=True):
    """maps: per frame (luma, chroma) base maps; per_frame False: the first pair is shared (frame stride 0).  Returns sse [f][2][8],
    choice [f][2], levels [f][4], the output maps [f][...] (luma, chroma)"""
    nf, h, w = rec[0].shape
    ny, ncw = (h // 4) * (w // 4), (h // 8) * (w // 8)
    d = [ctx.to_device(a) for a in rec + src]
    use = maps if per_frame else maps[:1]
    d_mi = [ctx.to_device(np.stack([m[k] for m in use])) for k in range(2)]
    nsb = ((w + 63) // 64) * ((h + 63) // 64)
    assert av1mi.lf_search_scratch_bytes(w, h, nf) == nf * nsb * 128
    d_scr = ctx.alloc(nf * nsb * 128)
    d_sse = ctx.to_device(np.full(nf * 128 + TAIL, 0xA5, np.uint8))
    d_choice = ctx.to_device(np.full(nf * 2 + TAIL, 0xEE, np.uint8))
    d_lv = ctx.to_device(np.full(nf * 4 + TAIL, 0x55, np.uint8))
    d_out = [ctx.to_device(np.full(nf * n * 4 + TAIL, 0x77, np.uint8)) for n in (ny, ncw)]
    tw, th = true_size if true_size else (0, 0)
    ctx.lf_search(av1mi.LfSearchJob(w, h, bd, nf, w, w // 2, *[b.ptr for b in d], tw, th, d_mi[0].ptr, d_mi[1].ptr, w // 4, w // 8,
                                    ny if per_frame else 0, ncw if per_frame else 0, C.addressof(params), d_scr.ptr, d_sse.ptr, d_choice.ptr, d_lv.ptr,
                                    d_out[0].ptr if want_maps else None, d_out[1].ptr if want_maps else None))
    sse, choice, lv = d_sse.download((nf * 128 + TAIL,), np.uint8), d_choice.download((nf * 2 + TAIL,), np.uint8), d_lv.download((nf * 4 + TAIL,), np.uint8)
    out = [b.download((nf * n * 4 + TAIL,), np.uint8) for b, n in zip(d_out, (ny, ncw))]
    for b in d + d_mi + d_out + [d_scr, d_sse, d_choice, d_lv]:
        b.free()
    # the tails past the arrays are untouched
    assert (sse[-TAIL:] == 0xA5).all() and (choice[-TAIL:] == 0xEE).all() and (lv[-TAIL:] == 0x55).all() and all((o[-TAIL:] == 0x77).all() for o in out)
    if not want_maps:
        assert all((o == 0x77).all() for o in out)
    out = [o[:-TAIL].view(np.uint32).reshape(nf, h // s, w // s) for o, s in zip(out, (4, 8))]
    return sse[:-TAIL].view(np.uint64).reshape(nf, 2, 8), choice[:-TAIL].reshape(nf, 2), lv[:-TAIL].reshape(nf, 4), out


def _deblock_with(ctx, av1mi, rec, bd, out_maps):
    """the three planes through av1mi_deblock_frames, and the rows av1mi_deblock_cdef_frames writes, both with the per-frame maps"""
    nf, h, w = rec[0].shape
    d_mi = [ctx.to_device(m) for m in out_maps]
    d_rec = [ctx.to_device(a) for a in rec]
    d_dbl = [ctx.to_device(np.zeros_like(a)) for a in rec]
    for p in range(3):
        ss = int(p > 0)
        ctx.deblock_frames(d_rec[p], w >> ss, d_dbl[p], w >> ss, w >> ss, h >> ss, bd, ss, d_mi[ss], (w >> ss) // 4, ((h >> ss) // 4) * ((w >> ss) // 4), 0, nf)
    plain = [b.download(a.shape, a.dtype) for b, a in zip(d_dbl, rec)]
    # the fused kernel: CDEF switched off (primary strength 255), so d_dst receives the deblocked planes whole
    nsb = ((w + 63) // 64) * ((h + 63) // 64)
    d_rows = [ctx.to_device(np.zeros_like(a)) for a in rec]
    d_dst = [ctx.to_device(np.zeros_like(a)) for a in rec]
    d_sb, d_skip = ctx.to_device(np.tile(np.array([255, 0, 255, 0], np.uint8), nsb)), ctx.to_device(np.zeros((h // 8) * (w // 8), np.uint8))
    ctx.deblock_cdef_frames(av1mi.DeblockCdefJob(w, h, bd, nf, 3, 0, w, w // 2, w, w // 2, w, w // 2, *[b.ptr for b in d_rec + d_rows + d_dst],
                                                 d_mi[0].ptr, d_mi[1].ptr, w // 4, w // 8, (h // 4) * (w // 4), (h // 8) * (w // 8), d_sb.ptr, 0, d_skip.ptr, 0))
    fused = [b.download(a.shape, a.dtype) for b, a in zip(d_dst, rec)]
    for b in d_mi + d_rec + d_dbl + d_rows + d_dst + [d_sb, d_skip]:
        b.free()
    return plain, fused


@pytest.fixture(scope="module")
def expected(O):
    """the reference per (size case, bit depth, key32, per-frame maps), computed once and shared"""
    cache = {}

    def get(case, bd, key32, per_frame):
        k = (case, bd, key32, per_frame)
        if k not in cache:
            w, h, true_size = R.SIZES[case]
            src, rec = R.frames(w, h, bd)
            # per-frame base maps: frame 1 gets the other form, and every map other level bytes (which the search must not read)
            maps = [R.base_maps(w, h, true_size, key32 != (per_frame and f == 1), level_bytes=7 * f + 3) for f in range(NF)]
            use = maps if per_frame else maps[:1] * NF
            ref = [R.search(O, [a[f] for a in rec], [a[f] for a in src], bd, R.POLICY, 0, use[f][0], use[f][1], true_size) for f in range(NF)]
            cache[k] = (src, rec, maps, use, ref)
        return cache[k]
    return get


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("key32", [False, True])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("case", range(len(R.SIZES)))
def test_search_equals_the_restatement_and_deblocking_takes_its_maps(ctx, av1mi, expected, case, bd, key32, per_frame):
    w, h, true_size = R.SIZES[case]
    src, rec, maps, use, ref = expected(case, bd, key32, per_frame)
    params = _params(av1mi, R.POLICY, bd)
    sse, choice, lv, out = _search(ctx, av1mi, rec, src, bd, params, maps, per_frame, true_size)
    for f in range(NF):
        e_sse, e_choice, e_lv, _ = ref[f]
        assert (sse[f] == e_sse).all(), ("sums", f, sse[f].tolist(), e_sse.tolist())
        assert choice[f].tolist() == e_choice and lv[f].tolist() == e_lv, (f, choice[f], e_choice, lv[f], e_lv)
        assert (out[0][f] == R.patched(use[f][0], e_lv[0], e_lv[1])).all() and (out[1][f] == R.patched(use[f][1], e_lv[2], e_lv[2])).all(), ("maps", f)
    plain, fused = _deblock_with(ctx, av1mi, rec, bd, out)
    for f in range(NF):
        for p in range(3):
            assert (plain[p][f] == ref[f][3][p]).all(), ("av1mi_deblock_frames", f, p)
            assert (fused[p][f] == ref[f][3][p]).all(), ("av1mi_deblock_cdef_frames", f, p)


def test_the_maps_are_optional(ctx, av1mi, expected):
    src, rec, maps, use, ref = expected(1, 8, False, False)
    sse, choice, lv, _ = _search(ctx, av1mi, rec, src, 8, _params(av1mi, R.POLICY, 8), maps, False, None, want_maps=False)
    for f in range(NF):
        assert (sse[f] == ref[f][0]).all() and choice[f].tolist() == ref[f][1] and lv[f].tolist() == ref[f][2]


@pytest.mark.parametrize("P", [(1, 1, 1, 1), (2, 0, 0, 0)])
def test_duplicate_candidates_never_win_a_tie(ctx, av1mi, O, P):
    """small levels: several candidates are one level; whatever they cost, a later twin is never chosen, and its sum is its twin's"""
    w, h, bd = 136, 72, 8
    src, rec = R.frames(w, h, bd, seed=5)
    maps = [R.base_maps(w, h)]
    params = _params(av1mi, P, bd)
    twins = [c for c in range(8) if any(R.levels(P, e)[:2] == R.levels(P, c)[:2] for e in range(c))]
    twins_c = [c for c in range(8) if any(R.levels(P, e)[2] == R.levels(P, c)[2] for e in range(c))]
    assert len(twins) >= 2 and len(twins_c) >= 3      # (1, 1, 1, 1): luma 1 .. 4, chroma 2 .. 4; (2, 0, 0, 0): luma 2 and 5, every chroma
    sse, choice, lv, _ = _search(ctx, av1mi, rec, src, bd, params, maps, False, None)
    for f in range(NF):
        e_sse, e_choice, e_lv, _ = R.search(O, [a[f] for a in rec], [a[f] for a in src], bd, P, 0, maps[0][0], maps[0][1])
        assert (sse[f] == e_sse).all() and choice[f].tolist() == e_choice and lv[f].tolist() == e_lv
        assert choice[f][0] not in twins and choice[f][1] not in twins_c


def test_search_refuses_what_it_does_not_support(ctx, av1mi):
    z = ctx.alloc(1 << 16)
    good = _params(av1mi, (20, 14, 12, 12), 8)
    fields = [name for name, _ in av1mi.LfSearchJob._fields_]

    def job(params=good, **kw):
        a = dict(width=64, height=64, bit_depth=8, nframes=1, stride_y=64, stride_uv=32, true_width=0, true_height=0, mi_stride_y=16, mi_stride_uv=8,
                 mi_frame_stride_y=0, mi_frame_stride_uv=0, params=None if params is None else C.addressof(params))
        a.update({k: z.ptr + 4096 * i for i, k in enumerate(f for f in fields if f.startswith("d_"))})
        a.update(kw)
        return av1mi.LfSearchJob(*[a[f] for f in fields])
    for P in ((20, 14, 12, 11), (0, 0, 3, 3), (64, 14, 12, 12)):
        with pytest.raises(av1mi.Av1miError) as e:
            ctx.lf_search(job(_params(av1mi, P, 8)))
        assert "deblocking search" in str(e.value)
    for kw in (dict(width=60), dict(bit_depth=12), dict(stride_y=32), dict(true_width=56), dict(true_height=70), dict(mi_stride_y=8), dict(params=None),
               dict(d_rec_y=None), dict(d_orig_v=None), dict(d_scratch=None), dict(d_sse=None), dict(d_choice=None), dict(d_levels=z.ptr + 2),
               dict(d_mi_uv=None), dict(d_mi_uv_out=None), dict(nframes=-1)):
        with pytest.raises(av1mi.Av1miError):
            ctx.lf_search(job(**kw))
    z.free()
