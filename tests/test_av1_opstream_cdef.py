"""cdef_bits 1, 2, 3 with an index per superblock through the CPU twin of the GPU coder (host/av1_opstream.cpp): its temporal unit
equals the host writer's byte for byte, and dav1d decodes it to the oracle's reconstruction filtered with those per-superblock
strengths.  Key frames in 8x8 blocks, key frames in 32x32 blocks, P frames whose skip maps hold an all-skipped tile, a tile whose
first block in z-order is skipped and a tile whose only coded block is its last.  192x128, and 200x136 with partial superblocks at
both edges (not the 32x32 blocks: they need a width that is a multiple of 32).  CPU only."""
import numpy as np
import pytest

import cdef_search_ref as R

SIZES = [(192, 128), (200, 136)]


def cdef_header(av1mi, q, bd, frame_type, bits, idx):
    p = av1mi.policy_frame_params(q, bd, frame_type)
    y, uv = R.sets(p, bits)
    n = 1 << bits
    return p, y, uv, dict(frame_type=frame_type, lf_level=tuple(p.lf_level), lf_sharpness=p.lf_sharpness, cdef_damping=p.cdef_damping, cdef_bits=bits,
                          cdef_y=tuple(y[:n]), cdef_uv=tuple(uv[:n]), cdef_idx=np.asarray(idx, np.uint8))


def filtered(O, pa, rec, bd, p, y, uv, idx, skip8, mi=None):
    mi_y, mi_c = mi if mi is not None else (pa["mi_y"], pa["mi_c"])
    dbl = [O.deblock_plane(rec[0], bd, 0, mi_y), O.deblock_plane(rec[1], bd, 1, mi_c), O.deblock_plane(rec[2], bd, 1, mi_c)]
    return list(R.cdef_with(O, dbl, bd, p.cdef_damping, R.records(y, uv, idx), skip8))


def p_frame_source(rng, ref, w, h, bd):
    """the reference itself (every block predicts exactly: skipped), with new content in chosen 8x8 blocks: tile 0 keeps none (all
    skipped), tile 1 all but its first block in z-order, tile 2 only its last, every other tile a random half"""
    change = rng.random((h // 8, w // 8)) < 0.5
    change[:8, :8] = False
    change[:8, 8:16] = True
    change[0, 8] = False
    change[:8, 16:24] = False
    change[7, 23] = True
    src = [a.copy() for a in ref]
    for r, c in zip(*np.nonzero(change)):
        src[0][r * 8:r * 8 + 8, c * 8:c * 8 + 8] = rng.integers(0, 1 << bd, (8, 8))
        for p in (1, 2):
            src[p][r * 4:r * 4 + 4, c * 4:c * 4 + 4] = rng.integers(0, 1 << bd, (4, 4))
    return src, change


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("bits,bd", [(1, 8), (2, 10), (3, 8)])
def test_key_and_p_frames_in_8x8_blocks(av1mi, O, w, h, bits, bd):
    import av1stream
    import dav1d_ref as D
    import pipeline
    import synth
    q = 90
    rng = np.random.default_rng(100 * bits + w)
    nsb = ((w + 63) // 64) * ((h + 63) // 64)
    Y, U, V = synth.frames(w, h, 1, bd, 5)
    stream, expect = b"", []
    # the key frame
    idx = rng.integers(0, 1 << bits, nsb)
    p, y, uv, hdr = cdef_header(av1mi, q, bd, 0, bits, idx)
    r = O.intra_encode_frame(Y[0], U[0], V[0], bd, 8, q)
    skip8 = np.zeros((h // 8, w // 8), np.uint8)
    ref = filtered(O, pipeline.policy_arrays(q, bd, 0, w, h), [r["rec_y"], r["rec_u"], r["rec_v"]], bd, p, y, uv, idx, skip8)
    sym = dict(y_mode=r["modes_y"], uv_mode=r["modes_uv"], lev_y=r["lev_y"], lev_u=r["lev_u"], lev_v=r["lev_v"])
    tu = av1stream.temporal_unit(w, h, bd, q, with_sequence_header=True, **sym, **hdr)
    assert av1stream.temporal_unit(w, h, bd, q, with_sequence_header=True, opstream=True, **sym, **hdr) == tu, "key frame: the twin and the host writer disagree"
    no_idx = dict(hdr, cdef_idx=None)       # a null index array is index 0 everywhere, in the writers and in the twin
    assert av1stream.temporal_unit(w, h, bd, q, opstream=True, **sym, **no_idx) == av1stream.temporal_unit(w, h, bd, q, **sym, **no_idx)
    stream += tu
    expect.append(ref)
    # the P frame
    src, change = p_frame_source(rng, ref, w, h, bd)
    r = O.inter_encode_frame(src, ref, bd, q, 8)
    skip8 = r["skip"].reshape(h // 8, w // 8)
    assert skip8[:8, :8].all(), "tile 0 must be all skipped"
    assert skip8[0, 8] == 1 and not skip8[:8, 8:16].all(), "tile 1: its first block skipped, others coded"
    assert skip8[7, 23] == 0 and skip8[:8, 16:24].sum() == 63, "tile 2: only its last block coded"
    idx = rng.integers(0, 1 << bits, nsb)
    idx[:3] = (1 << bits) - 1                # (the index of the all-skipped tile is coded nowhere; the decoder leaves that superblock alone)
    p, y, uv, hdr = cdef_header(av1mi, q, bd, 1, bits, idx)
    ref = filtered(O, pipeline.policy_arrays(q, bd, 1, w, h), [r["rec_y"], r["rec_u"], r["rec_v"]], bd, p, y, uv, idx, skip8)
    sym = dict(mv=r["mvs"], skip=r["skip"], lev_y=r["lev_y"], lev_u=r["lev_u"], lev_v=r["lev_v"])
    tu = av1stream.temporal_unit(w, h, bd, q, with_sequence_header=False, **sym, **hdr)
    assert av1stream.temporal_unit(w, h, bd, q, with_sequence_header=False, opstream=True, **sym, **hdr) == tu, "P frame: the twin and the host writer disagree"
    stream += tu
    expect.append(ref)
    if D.available():
        got = D.decode(stream)
        assert len(got) == 2
        for t in range(2):
            for pl in range(3):
                assert (np.asarray(got[t][pl]) == expect[t][pl]).all(), (t, pl)


@pytest.mark.parametrize("bits,bd", [(1, 10), (2, 8), (3, 10)])
def test_key_frames_in_32x32_blocks(av1mi, O, bits, bd):
    import av1stream
    import av1_blocks as B
    import dav1d_ref as D
    import pipeline
    import synth
    w, h, q = 192, 128, 90
    rng = np.random.default_rng(7 + bits)
    nsb = (w // 64) * (h // 64)
    Y, U, V = (a[0] for a in synth.frames(w, h, 1, bd, 3))
    a = O.intra_encode_frame(Y, U, V, bd, 32, q)
    idx = rng.integers(0, 1 << bits, nsb)
    p, y, uv, hdr = cdef_header(av1mi, q, bd, 0, bits, idx)
    hdr.pop("frame_type")
    lay = B.Layout(w, h)
    parts, tree = B.build_tree(lay, B.uniform_chooser(9))
    w32 = w // 32
    blocks = []
    for r, c, bsize, tb in tree:
        i = (r // 8) * w32 + c // 8
        blocks.append(dict(r=r, c=c, bsize=bsize, tile=tb, skip=0, is_inter=0, y_mode=int(a["modes_y"][i]), uv_mode=int(a["modes_uv"][i]), angle_y=0, angle_uv=0,
                           cfl=(0, 0), tx_depth=0, filt=0, mv=(0, 0), tx=B.max_tx_rect(bsize), tx_types=[0], levels=[[a["lev_y"][i]], [a["lev_u"][i]], [a["lev_v"][i]]]))
    ref = B.encode(lay, bd, q, parts, blocks, **hdr)
    nb = (h // 8) * (w // 8)
    ym, uvm = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
    n32 = (h // 32) * w32
    ym[:n32], uvm[:n32] = a["modes_y"], a["modes_uv"]
    twin = av1stream.temporal_unit(w, h, bd, q, opstream=True, key_rows32=h, y_mode=ym, uv_mode=uvm, lev_y=a["lev_y"].reshape(-1), lev_u=a["lev_u"].reshape(-1),
                                   lev_v=a["lev_v"].reshape(-1), **hdr)
    assert twin == ref, "the twin and the block writer disagree"
    if D.available():
        pa = pipeline.policy_arrays(q, bd, 0, w, h)
        mi_y = (pa["mi_y"] & ~np.uint32(0xFF)) | np.uint32(5 | (5 << 4))       # 32x32 luma transforms, 16x16 chroma
        mi_c = (pa["mi_c"] & ~np.uint32(0xFF)) | np.uint32(4 | (4 << 4))
        want = filtered(O, pa, [a["rec_y"], a["rec_u"], a["rec_v"]], bd, p, y, uv, idx, np.zeros((h // 8, w // 8), np.uint8), mi=(mi_y, mi_c))
        pic = D.decode(twin)[0]
        for pl in range(3):
            assert np.array_equal(np.asarray(pic[pl]), want[pl]), pl
