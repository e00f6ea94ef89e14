"""GPU: av1mi_cdef_search (k_cdef_search) against its restatement (cdef_search_ref.py: the oracle's CDEF of the whole frame per
candidate, summed per superblock over the true size) — the cost table, the indices and the strength records bit for bit —, CDEF
with the written records, and the GPU coder with an index per superblock against the CPU op stream."""
import ctypes as C

import numpy as np
import pytest

import cdef_search_ref as R
from test_av1_opstream_cdef import cdef_header, p_frame_source
from test_gpu_chains_order import EntropyJob, _key_symbols

pytestmark = pytest.mark.gpu

TAIL = 16


def _dims(h, w):
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


def _case(w, h, bd, nf):
    """nf frames of different content and their skip maps: superblock f of frame f is all skipped, and a few single blocks elsewhere"""
    rng = np.random.default_rng(w + h + bd)
    frames = [R.content(rng, w, h, bd, shift=5 * f) for f in range(nf)]
    src = [np.stack([fr[0][p] for fr in frames]) for p in range(3)]
    dbl = [np.stack([fr[1][p] for fr in frames]) for p in range(3)]
    skip = (rng.random((nf, h // 8, w // 8)) < 0.1).astype(np.uint8)
    sbw = (w + 63) // 64
    for f in range(nf):
        r, c = divmod(f, sbw)
        skip[f, r * 8:r * 8 + 8, c * 8:c * 8 + 8] = 1
    return src, dbl, skip


def _search(ctx, av1mi, dbl, src, skip, bd, bits, params, true_size):
    nf, h, w = dbl[0].shape
    nsb = ((w + 63) // 64) * ((h + 63) // 64)
    d = [ctx.to_device(a) for a in dbl + src]
    d_skip = ctx.to_device(skip)
    nbytes = av1mi.cdef_search_table_bytes(w, h, nf)
    assert nbytes == nf * nsb * 64
    d_sse = ctx.to_device(np.full(nbytes + TAIL, 0xA5, np.uint8))
    d_rec = ctx.to_device(np.full(nf * nsb * 4 + TAIL, 0x55, np.uint8))
    d_idx = ctx.to_device(np.full(nf * nsb + TAIL, 0xEE, np.uint8))
    tw, th = true_size if true_size else (0, 0)
    ctx.cdef_search(av1mi.CdefSearchJob(w, h, bd, nf, w, w // 2, *[b.ptr for b in d], d_skip.ptr, (h // 8) * (w // 8), tw, th, bits,
                                        C.addressof(params), d_sse.ptr, d_rec.ptr, d_idx.ptr))
    sse, rec, idx = d_sse.download((nbytes + TAIL,), np.uint8), d_rec.download((nf * nsb * 4 + TAIL,), np.uint8), d_idx.download((nf * nsb + TAIL,), np.uint8)
    for b in d + [d_skip, d_sse, d_rec, d_idx]:
        b.free()
    # the tails past the arrays are untouched
    assert (sse[nbytes:] == 0xA5).all() and (rec[-TAIL:] == 0x55).all() and (idx[-TAIL:] == 0xEE).all()
    return sse[:nbytes].view(np.uint64).reshape(nf, nsb, 8), rec[:-TAIL].reshape(nf, nsb, 4), idx[:-TAIL].reshape(nf, nsb)


#                  w    h    true size
CASES = [(192, 128, None), (136, 72, (130, 70))]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("bits", [1, 2, 3])
@pytest.mark.parametrize("w,h,true_size", CASES)
def test_search_equals_the_restatement_and_cdef_takes_its_records(ctx, av1mi, O, w, h, true_size, bits, bd):
    nf, q = 2, 128
    src, dbl, skip = _case(w, h, bd, nf)
    params = av1mi.policy_frame_params(q, bd, 1)
    y, uv = R.sets(params, bits)
    table, rec, idx = _search(ctx, av1mi, dbl, src, skip, bd, bits, params, true_size)
    for f in range(nf):
        exp = R.table(O, [a[f] for a in dbl], [a[f] for a in src], bd, params.cdef_damping, y, uv, bits, skip[f], true_size)
        assert (table[f] == exp).all(), ("cost table", f, np.argwhere(table[f] != exp)[:4], table[f][table[f] != exp][:4], exp[table[f] != exp][:4])
        want = R.pick(exp, bits)
        # the content does its job on the CPU already: the restatement alone picks different sets (three where there are that many)
        assert len(set(want.tolist())) >= min(3, 1 << bits), want
        assert want[f] == 0 and len(set(exp[f].tolist()[:1 << bits])) == 1, "the all-skipped superblock ties and takes index 0"
        assert idx[f].tolist() == want.tolist(), ("indices", f)
        assert rec[f].tolist() == R.records(y, uv, want).tolist(), ("strength records", f)
        chosen = table[f][np.arange(len(want)), idx[f]]
        assert (chosen <= table[f][:, 0]).all()
    # av1mi_cdef_frames with the written records = the oracle's CDEF with per-superblock strengths
    nsb = rec.shape[1]
    d = [ctx.to_device(a) for a in dbl]
    out = [ctx.to_device(np.zeros_like(a)) for a in dbl]
    d_rec, d_skip = ctx.to_device(rec), ctx.to_device(skip)
    ctx.cdef_frames(av1mi.CdefJob(w, h, bd, nf, params.cdef_damping, w, w // 2, *[b.ptr for b in d + out], d_rec.ptr, nsb, d_skip.ptr, (h // 8) * (w // 8)))
    got = [o.download(a.shape, a.dtype) for o, a in zip(out, dbl)]
    for b in d + out + [d_rec, d_skip]:
        b.free()
    for f in range(nf):
        exp = R.cdef_with(O, [a[f] for a in dbl], bd, params.cdef_damping, rec[f], skip[f])
        for p in range(3):
            assert (got[p][f] == exp[p]).all(), (f, p)


def test_duplicate_sets_never_win_a_tie(ctx, av1mi, O):
    """q 30: the policy's set is zero, so candidates 0, 1, 2 and 5 are one set; whatever they cost, 1, 2 and 5 are never chosen"""
    w, h, bd, bits = 192, 128, 8, 3
    src, dbl, skip = _case(w, h, bd, 1)
    params = av1mi.policy_frame_params(30, bd, 0)
    y, uv = R.sets(params, bits)
    assert y[0] == y[1] == y[2] == y[5] and uv[0] == uv[1] == uv[2] == uv[5]
    table, rec, idx = _search(ctx, av1mi, dbl, src, skip, bd, bits, params, None)
    exp = R.table(O, [a[0] for a in dbl], [a[0] for a in src], bd, params.cdef_damping, y, uv, bits, skip[0])
    assert (table[0] == exp).all() and idx[0].tolist() == R.pick(exp, bits).tolist() and not set(idx[0].tolist()) & {1, 2, 5}


def test_search_refuses_what_it_does_not_support(ctx, av1mi):
    z = ctx.alloc(4096)
    params = av1mi.policy_frame_params(100, 8, 0)
    ok = [64, 64, 8, 1, 64, 32] + [z.ptr] * 7 + [64, 0, 0, 2, C.addressof(params), z.ptr, z.ptr, z.ptr]
    for field, value in ((0, 60), (2, 12), (4, 32), (16, 0), (16, 4), (17, 0), (14, 56), (15, 70), (18, 0), (6, 0)):
        a = list(ok)
        a[field] = value
        with pytest.raises(av1mi.Av1miError):
            ctx.cdef_search(av1mi.CdefSearchJob(*a))
    z.free()


def _gpu_units(ctx, av1mi, w, h, bd, q, key, sym, hdr, key_rows32=0):
    """one frame's symbols through av1mi_av1_entropy_encode_sides with the header's cdef_bits and indices; returns the temporal unit"""
    import av1stream
    tiles = ((w + 63) // 64) * ((h + 63) // 64)
    names = ("lev_y", "lev_u", "lev_v") + (("y_mode", "uv_mode") if key else ("mv", "skip"))
    dtypes = dict(lev_y=np.int16, lev_u=np.int16, lev_v=np.int16, y_mode=np.uint8, uv_mode=np.uint8, mv=np.int16, skip=np.uint8)
    dev = {k: ctx.to_device(np.ascontiguousarray(sym[k], dtypes[k]).reshape(-1)) for k in names}
    cap = tiles * (1 << 16)
    d_out, d_size, d_total = ctx.alloc(cap), ctx.alloc(tiles * 4), ctx.alloc(16)
    d_idx = ctx.to_device(np.ascontiguousarray(hdr["cdef_idx"], np.uint8))
    j = EntropyJob()
    j.width, j.height, j.nframes, j.key, j.base_q_idx, j.key_rows32 = w, h, 1, int(key), q, key_rows32
    j.d_lev_y, j.d_lev_u, j.d_lev_v = dev["lev_y"].ptr, dev["lev_u"].ptr, dev["lev_v"].ptr
    if key:
        j.d_modes_y, j.d_modes_uv = dev["y_mode"].ptr, dev["uv_mode"].ptr
    else:
        j.d_mvs, j.d_skip = dev["mv"].ptr, dev["skip"].ptr
    j.d_out, j.out_cap, j.d_tile_size, j.d_total = d_out.ptr, cap, d_size.ptr, d_total.ptr
    side = av1mi.EntropyCdef(hdr["cdef_bits"], d_idx.ptr, tiles)
    try:
        ctx.lib.av1mi_av1_entropy_encode_sides.argtypes = [C.c_void_p, C.POINTER(EntropyJob), C.c_void_p, C.POINTER(av1mi.EntropyCdef), C.c_void_p]
        ctx._chk(ctx.lib.av1mi_av1_entropy_encode_sides(ctx.h, C.byref(j), None, C.byref(side), None))
        ctx.sync()
        total, status = (int(v) for v in d_total.download((2,), np.uint64))
        assert status == 0, "the GPU coder reports status %d" % status
        sizes = d_size.download((tiles,), np.uint32)
        pay = d_out.download((total,), np.uint8)
    finally:
        for b in list(dev.values()) + [d_out, d_size, d_total, d_idx]:
            b.free()
    h2 = {k: v for k, v in hdr.items() if k != "cdef_idx"}
    return av1stream.assemble_temporal_unit(w, h, bd, q, pay, sizes, with_sequence_header=bool(key), **h2)


@pytest.mark.parametrize("bits,bd", [(1, 8), (2, 10), (3, 8)])
def test_gpu_coder_with_indices_equals_the_cpu_op_stream(ctx, av1mi, O, bits, bd):
    """key frame in 8x8 blocks, key frame in 32x32 blocks, P frame whose skip map holds an all-skipped tile, a tile whose first block
    in z-order is skipped and a tile whose only coded block is its last; random indices; 192x128"""
    import av1stream
    import synth
    w, h, q = 192, 128, 90
    rng = np.random.default_rng(bits + bd)
    nsb = 6
    Y, U, V = (a[0] for a in synth.frames(w, h, 1, bd, 5))
    for rows32 in (0, h):
        sym = _key_symbols(O, Y, U, V, w, h, bd, q, rows32)
        _, _, _, hdr = cdef_header(av1mi, q, bd, 0, bits, rng.integers(0, 1 << bits, nsb))
        twin = av1stream.temporal_unit(w, h, bd, q, with_sequence_header=True, opstream=True, key_rows32=rows32, **sym, **hdr)
        assert _gpu_units(ctx, av1mi, w, h, bd, q, True, sym, hdr, rows32) == twin, "key frame, 32x32 rows %d" % rows32
    r = O.intra_encode_frame(Y, U, V, bd, 8, q)
    ref = [r["rec_y"], r["rec_u"], r["rec_v"]]
    src, _ = p_frame_source(rng, ref, w, h, bd)
    r = O.inter_encode_frame(src, ref, bd, q, 8)
    skip8 = r["skip"].reshape(h // 8, w // 8)
    assert skip8[:8, :8].all() and skip8[0, 8] == 1 and not skip8[:8, 8:16].all() and skip8[7, 23] == 0 and skip8[:8, 16:24].sum() == 63
    sym = dict(mv=r["mvs"], skip=r["skip"], lev_y=r["lev_y"], lev_u=r["lev_u"], lev_v=r["lev_v"])
    _, _, _, hdr = cdef_header(av1mi, q, bd, 1, bits, rng.integers(1, 1 << bits, nsb))
    twin = av1stream.temporal_unit(w, h, bd, q, with_sequence_header=False, opstream=True, **sym, **hdr)
    assert _gpu_units(ctx, av1mi, w, h, bd, q, False, sym, hdr) == twin, "P frame"
