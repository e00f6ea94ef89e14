"""The restoration search's tables (include/av1mi.h "restoration search") against their restatement (lr_search_ref.py), the restatement's
bits against what the op-stream twin of the GPU coder emits for the record, and its unit map against the oracle.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import lr_search_ref as R
from lf_util import test_image as make_image


def test_candidates_bits_and_lambda_equal_the_restatement(av1mi, O):
    assert av1mi.LR_SEARCH_CANDIDATES == R.CANDIDATES == 9
    for chroma in (0, 1):
        for c in range(R.CANDIDATES):
            assert av1mi.lr_search_candidate(chroma, c) == R.record(chroma, c), (chroma, c)
            assert av1mi.lr_search_bits(chroma, c) == R.bits(chroma, c), (chroma, c)
        # every record stays inside the syntax's ranges, a chroma record codes no tap0, and (I, I) is not among them
        recs = [R.record(chroma, c) for c in range(1, R.CANDIDATES)]
        assert len({tuple(r) for r in recs}) == 8 and [1, 0, 0, 0, 0, 0, 0, 0] not in recs
        for r in recs:
            for ps in range(2):
                assert all(R.TAP_MIN[j] <= r[1 + 3 * ps + j] <= R.TAP_MAX[j] for j in range(3)) and (not chroma or r[1 + 3 * ps] == 0)
    with pytest.raises(ValueError):
        av1mi.lr_search_candidate(0, 9)
    assert av1mi.lr_search_bits(0, 9) == -1 and av1mi.lr_search_bits(1, -1) == -1
    # the policy's record is candidate 4 of its class, and it is the cheapest Wiener record: every tap equals its reference
    p = av1mi.policy_frame_params(128, 8, 0)
    assert list(p.lr_unit_y) == R.record(0, R.POLICY) and list(p.lr_unit_uv) == R.record(1, R.POLICY)
    assert R.bits(0, 0) == 1 and R.bits(0, R.POLICY) == min(R.bits(0, c) for c in range(1, 9))
    for bd in (8, 10):
        for q in (0, 23, 128, 200, 255):
            assert av1mi.lr_search_lambda(q, bd) == R.lam(O, q, bd) == (3 * O.dc_q(q, bd) ** 2) >> 7


def _literal_bits_of_a_tile(plane, rec):
    """the literal bits in the list of a 64 x 64 key frame's only tile (all levels zero) through the op-stream twin, restoration on in
    `plane` with the one unit record rec, or off (rec None)"""
    import av1stream
    L = av1stream.lib()
    L.av1mi_host_opstream_slots.restype = C.c_int
    L.av1mi_host_opstream_tile8.restype = C.c_int
    L.av1mi_host_opstream_tile8.argtypes = [C.POINTER(av1stream.ObuFrame), C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 4
    ns, cap, nb = L.av1mi_host_opstream_slots(), 1 << 14, 64
    f = av1stream.ObuFrame()
    f.width, f.height, f.bit_depth, f.frame_type, f.base_q_idx = 64, 64, 8, 0, 100
    f.tile_cols_log2 = f.tile_rows_log2 = -1
    keep = dict(y_mode=np.zeros(nb, np.uint8), uv_mode=np.zeros(nb, np.uint8), lev_y=np.zeros(nb * 64, np.int16), lev_u=np.zeros(nb * 16, np.int16),
                lev_v=np.zeros(nb * 16, np.int16))
    for k, v in keep.items():
        setattr(f, k, v.ctypes.data)
    if rec is not None:
        units = np.array(rec, np.int8)
        f.lr_type[plane] = 1
        f.lr_units[plane] = units.ctypes.data
    lst, grp = np.zeros(cap, np.uint32), np.zeros(cap + 4 * ns, np.uint32)
    tot, base = np.zeros(ns, np.uint16), np.zeros(ns, np.uint16)
    n = L.av1mi_host_opstream_tile8(C.byref(f), 0, 0, cap, *[a.ctypes.data for a in (lst, grp, tot, base)])
    assert n > 0
    literal = np.ones(n, bool)                           # the words the chains fill in later are not literals
    for b, t in zip(base, tot):
        if t:
            literal[grp[int(b):int(b) + int(t)] >> 4] = False
    words = lst[:n][literal]
    assert (words >> 31 == 1).all()
    return int(((words >> 27) & 15).sum()), int((~literal).sum())


@pytest.mark.parametrize("chroma", [0, 1], ids=["luma", "chroma"])
def test_bits_equal_the_literals_the_opstream_twin_emits(chroma):
    """bits_c = 1 (use_wiener, the one adaptive symbol a unit adds) + the literal bits of the record in the tile's list"""
    off_bits, off_syms = _literal_bits_of_a_tile(chroma, None)
    for c in range(R.CANDIDATES):
        bits, syms = _literal_bits_of_a_tile(chroma, R.record(chroma, c))
        assert syms == off_syms + 1 and 1 + bits - off_bits == R.bits(chroma, c), (chroma, c, bits, off_bits)


@pytest.mark.parametrize("bd,ss,h,w", [(8, 0, 136, 200), (10, 1, 72, 100), (10, 0, 300, 260), (8, 1, 40, 24)])
def test_unit_map_of_the_restatement_is_the_oracles(O, bd, ss, h, w):
    """a plane restored with a random candidate per unit equals, inside every unit of the map, the plane restored with that candidate
    everywhere: the map the per-unit sums run over is the oracle's assignment of samples to units"""
    rng = np.random.default_rng(h + w + bd)
    cdef, dbl = make_image(rng, h, w, bd), make_image(rng, h, w, bd)
    umap, n = R.unit_map(O, h, w, ss)
    rows, cols = O.lr_units(64, h), O.lr_units(64, w)
    assert n == rows * cols and umap.max() == n - 1
    choice = rng.integers(0, R.CANDIDATES, n)
    mixed = O.lr_plane(cdef, dbl, bd, ss, 64, np.array([R.record(ss, c) for c in choice], np.int8).reshape(rows, cols, 8))
    differ = 0
    for c in sorted(set(choice.tolist())):
        whole = O.lr_plane(cdef, dbl, bd, ss, 64, np.tile(np.array(R.record(ss, c), np.int8), (rows, cols, 1)))
        inside = np.isin(umap, np.flatnonzero(choice == c))
        assert (mixed[inside] == whole[inside]).all(), c
        differ += int((mixed[~inside] != whole[~inside]).sum())
    assert n == 1 or differ > 0


def test_pick_takes_the_lowest_cost_and_the_lowest_index_on_a_tie():
    t = np.array([[100, 90, 90, 500, 90, 90, 90, 90, 90], [10, 0, 0, 0, 0, 0, 0, 0, 0]], np.int64)
    idx, j = R.pick(t, 0, 0)
    assert idx.tolist() == [1, 1]
    idx, j = R.pick(t, 0, 5)      # the cheapest luma Wiener record costs 18 bits more than "none": 90 against a gain of 10
    assert idx.tolist() == [0, 0] and j[0, 0] == 105


@pytest.mark.parametrize("bd", [8, 10])
def test_per_unit_records_in_the_stream(av1mi, O, bd):
    """a key frame and a P frame, 192 x 136, every unit of every plane with a random candidate, "none" included: the op-stream twin of
    the GPU coder (per-unit records through FrameView::lr_units) produces the host writer's bytes, dav1d decodes the stream to the
    oracle's chain restored with those units, and units that are all alike give the bytes of the shared-record path"""
    import av1stream
    import dav1d_ref as D
    import pipeline
    import synth
    w, h, q = 192, 136, 90
    rng = np.random.default_rng(17 + bd)
    Y, U, V = synth.frames(w, h, 2, bd, 5)
    dims = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    stream, ref, expect = b"", None, []
    for t in range(2):
        pa = pipeline.policy_arrays(q, bd, t, w, h)
        if t == 0:
            r = O.intra_encode_frame(Y[0], U[0], V[0], bd, 8, q)
            skip8 = np.zeros((h // 8, w // 8), np.uint8)
            sym = dict(y_mode=r["modes_y"], uv_mode=r["modes_uv"])
        else:
            r = O.inter_encode_frame((Y[1], U[1], V[1]), ref, bd, q, 8)
            skip8 = r["skip"].reshape(h // 8, w // 8)
            sym = dict(mv=r["mvs"], skip=r["skip"])
        units = [np.array([R.record(int(p > 0), c) for c in rng.integers(0, R.CANDIDATES, O.lr_units(64, hh) * O.lr_units(64, ww))], np.int8)
                 .reshape(O.lr_units(64, hh), O.lr_units(64, ww), 8) for p, (hh, ww) in enumerate(dims)]
        units[0][0, 0] = units[2][-1, -1] = 0                   # "none" at least in the first luma unit and the last unit of V
        assert len({tuple(x) for u in units for x in u.reshape(-1, 8).tolist()}) > 4
        dbl = [O.deblock_plane(r["rec_y"], bd, 0, pa["mi_y"]), O.deblock_plane(r["rec_u"], bd, 1, pa["mi_c"]), O.deblock_plane(r["rec_v"], bd, 1, pa["mi_c"])]
        cdef = O.cdef_frame(dbl[0], dbl[1], dbl[2], bd, pa["cdef_damping"], pa["cdef_sb"], skip8)
        ref = [O.lr_plane(cdef[p], dbl[p], bd, int(p > 0), 64, units[p]) for p in range(3)]
        expect.append(ref)
        hdr = av1stream.header_from_params(av1mi.policy_frame_params(q, bd, t), w, h, [1, 1, 1], None)
        lev = dict(lev_y=r["lev_y"], lev_u=r["lev_u"], lev_v=r["lev_v"])
        args = dict(with_sequence_header=(t == 0), **lev, **sym)
        per_unit = dict(hdr, lr_units=tuple(units))
        tu = av1stream.temporal_unit(w, h, bd, q, **args, **per_unit)
        assert av1stream.temporal_unit(w, h, bd, q, opstream=True, **args, **per_unit) == tu, "frame %d: the twin and the host writer disagree" % t
        assert av1stream.temporal_unit(w, h, bd, q, opstream=True, **args, **hdr) == av1stream.temporal_unit(w, h, bd, q, **args, **hdr)
        stream += tu
    if D.available():
        got = D.decode(stream)
        assert len(got) == 2
        for t in range(2):
            for p in range(3):
                assert (np.asarray(got[t][p]) == expect[t][p]).all(), (t, p)
