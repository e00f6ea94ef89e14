"""The tile tokenizer of 8x8 blocks (av1-go_amd/csrc/av1_ops8.hpp tok_tile8): one wave per tile, a lane per block; the neighbours' level
summaries are the tile's own, the records are replayed once through positions sized by the slots the tile uses (twice only for a tile
that uses more than half of all slots).  The CPU twin (host/av1_opstream.cpp) runs the same source as a loop over the lanes; its bytes
must equal the block-sequential writer's (host/av1_bitstream.cpp) on content chosen to hit that logic, and dav1d (when present) must
decode them.  One tile through av1mi_host_opstream_tile8 checks the areas it writes and what it does at its capacities.  CPU only."""
import ctypes as C

import numpy as np
import pytest


def _scan(n):
    """Default_Scan_NxN (zig-zag, odd diagonals downwards): scan index -> position"""
    pos = np.zeros(n * n, np.int64)
    k = 0
    for d in range(2 * n - 1):
        rows = range(max(0, d - n + 1), min(d, n - 1) + 1)
        for r in (rows if d & 1 else reversed(rows)):
            pos[k] = r * n + d - r
            k += 1
    return pos


SCAN = {4: _scan(4), 8: _scan(8)}


def _levels(rng, n, eob, density=0.5, big=(), lo=1, hi=5):
    """an n x n transform block whose last non-zero level is at scan index eob - 1; big: scan indices of levels above 14 (Golomb)"""
    a = np.zeros(n * n, np.int16)
    if eob:
        pos = SCAN[n][:eob]
        m = rng.random(eob) < density
        a[pos[m]] = rng.integers(lo, hi, int(m.sum())) * rng.choice([-1, 1], int(m.sum()))
        a[pos[eob - 1]] = rng.choice([-2, -1, 1, 3])
        for c in big:
            if c < eob:
                a[pos[c]] = int(rng.integers(15, 4000)) * int(rng.choice([-1, 1]))
    return a


def _frame(rng, w, h, eobs_y, eobs_c, density=0.5, big_y=(), big_c=(), hi=5):
    """block i (raster) takes eobs_y[i % len] / eobs_c[i % len] (U) / eobs_c[(i + 1) % len] (V); eobs_* may be a function of (row, column)"""
    w8, nb = w // 8, (w // 8) * (h // 8)
    ey = eobs_y if callable(eobs_y) else (lambda r, c: eobs_y[(r * w8 + c) % len(eobs_y)])
    ec = eobs_c if callable(eobs_c) else (lambda r, c, v=0: eobs_c[(r * w8 + c + v) % len(eobs_c)])
    ly = np.stack([_levels(rng, 8, ey(i // w8, i % w8), density, big_y, hi=hi) for i in range(nb)])
    lu = np.stack([_levels(rng, 4, ec(i // w8, i % w8), density, big_c, hi=hi) for i in range(nb)])
    lv = np.stack([_levels(rng, 4, ec(i // w8, i % w8, 1), density, big_c, hi=hi) for i in range(nb)])
    return dict(lev_y=ly, lev_u=lu, lev_v=lv)


def _step_totals(rng, w, h):
    """scan positions per tile exactly on, one below and one above 64 and 128 (tile t takes variant t % 6): luma eob 1 (2) in every
    block, the tile's first block one less / the same / one more; chroma empty"""
    sbc = (w + 63) // 64

    def ey(r, c):
        v = ((r // 8) * sbc + c // 8) % 6
        return (1 if v < 3 else 2) + ((v % 3) - 1 if (r % 8, c % 8) == (0, 0) else 0)
    return _frame(rng, w, h, ey, [0], density=1.0)


def _one_among(a, b):
    """block 21 of every 64 takes a, the others b"""
    return [a if i == 21 else b for i in range(64)]


CASES = {
    "all_zero": lambda rng, w, h: _frame(rng, w, h, [0], [0]),
    "eob_1_everywhere": lambda rng, w, h: _frame(rng, w, h, [1], [1]),
    "eob_full_everywhere": lambda rng, w, h: _frame(rng, w, h, [64], [16], density=0.4),
    "one_dense_block_among_empty": lambda rng, w, h: _frame(rng, w, h, _one_among(64, 0), _one_among(16, 0), density=0.9, hi=14),
    "one_empty_block_among_dense": lambda rng, w, h: _frame(rng, w, h, _one_among(0, 64), _one_among(0, 16), density=0.9, hi=14),
    "scan_positions_at_multiples_of_64": _step_totals,
    "golomb_at_the_first_and_last_position": lambda rng, w, h: _frame(rng, w, h, [64, 57, 3, 1], [16, 14, 2, 1], density=0.2, big_y=(0, 1, 2, 56, 63),
                                                                      big_c=(0, 1, 13, 15)),
    "zero_luma_nonzero_chroma": lambda rng, w, h: _frame(rng, w, h, [0], [5, 16, 1, 3]),
    "nonzero_luma_zero_chroma": lambda rng, w, h: _frame(rng, w, h, [17, 64, 1, 30], [0]),
    "mixed_zero_blocks": lambda rng, w, h: _frame(rng, w, h, [0, 40, 0, 0, 64, 3], [0, 0, 9, 16, 0, 1]),
}
SKIP_SHARE = {"all_zero": 0.0, "eob_full_everywhere": 0.0, "mixed_zero_blocks": 0.5}      # inter frames; 0.25 elsewhere


def _vectors(rng, nb):
    """a few clusters (NEARESTMV / NEARMV of the neighbours), zeros (GLOBALMV), far outliers (NEWMV with large differences)"""
    base = rng.integers(-6, 7, (4, 2)) * 2
    mv = base[rng.integers(0, 4, nb)].astype(np.int16)
    far = rng.random(nb) < 0.2
    mv[far] = (rng.integers(-1000, 1001, (int(far.sum()), 2)) * 2).astype(np.int16)
    mv[rng.random(nb) < 0.15] = 0
    return mv


def _lr_header(w, h):
    ur = lambda n: max(1, (n + 32) // 64)
    uy = np.tile(np.array([1, 3, -7, 15, 3, -7, 15, 0], np.int8), (ur(h), ur(w), 1))
    uc = np.tile(np.array([1, 0, -7, 15, 0, -7, 15, 0], np.int8), (ur(h // 2), ur(w // 2), 1))
    return dict(lr_type=(1, 0, 1), lr_units=(uy, uc, uc), lf_level=(9, 7, 5, 5), cdef_y=(5,), cdef_uv=(4,), cdef_damping=4)


def _symbols(rng, case, w, h, key):
    nb = (w // 8) * (h // 8)
    sym = CASES[case](rng, w, h)
    if key:
        sym.update(y_mode=rng.integers(0, 13, nb).astype(np.uint8), uv_mode=rng.integers(0, 13, nb).astype(np.uint8))
    else:
        sym.update(mv=_vectors(rng, nb), skip=(rng.random(nb) < SKIP_SHARE.get(case, 0.25)).astype(np.uint8))
    return sym


@pytest.mark.parametrize("bd,lr", [(8, False), (10, True), (8, True), (10, False)], ids=["8bit_lr_off", "10bit_lr_on", "8bit_lr_on", "10bit_lr_off"])
@pytest.mark.parametrize("key", [True, False], ids=["key", "inter"])
@pytest.mark.parametrize("w,h", [(64, 64), (136, 72), (200, 64)], ids=["64x64", "136x72_partial_tiles", "200x64"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_twin_equals_the_sequential_writer(case, w, h, key, bd, lr):
    import av1stream
    import dav1d_ref as D
    rng = np.random.default_rng(sorted(CASES).index(case) * 11 + w + (0 if key else 1000))
    q = 100
    sym = _symbols(rng, case, w, h, key)
    hdr = _lr_header(w, h) if lr else {}
    if not key:
        hdr = dict(hdr, frame_type=1, with_sequence_header=False)
    ref = av1stream.temporal_unit(w, h, bd, q, **sym, **hdr)
    twin = av1stream.temporal_unit(w, h, bd, q, opstream=True, **sym, **hdr)
    assert twin == ref
    if D.available():
        if not key:      # a P frame predicts from a key frame: an empty one in front of it
            nb = (w // 8) * (h // 8)
            z = dict(y_mode=np.zeros(nb, np.uint8), uv_mode=np.zeros(nb, np.uint8), lev_y=np.zeros((nb, 64), np.int16), lev_u=np.zeros((nb, 16), np.int16),
                     lev_v=np.zeros((nb, 16), np.int16))
            twin = av1stream.temporal_unit(w, h, bd, q, opstream=True, **z) + twin
        pics = D.decode(twin, inloop_filters=0)
        assert len(pics) == (1 if key else 2) and np.asarray(pics[-1][0]).shape == (h, w)


def test_a_tile_that_uses_more_than_half_of_the_slots_takes_two_replay_passes():
    """dense, varied content and vectors of every class: the tile uses more slots than one pass has rows for (the second pass's rows
    start at a non-zero row); a sparse tile beside the same code path uses far fewer"""
    import av1stream
    rng = np.random.default_rng(77)
    w, h = 64, 64
    for key in (True, False):
        sym = _symbols(rng, "eob_full_everywhere", w, h, key)
        sym.update(_frame(rng, w, h, [64, 33, 9, 2, 50], [16, 7, 3, 1, 12], density=0.6, big_y=(0, 5), big_c=(1,), hi=12))
        hdr = {} if key else dict(frame_type=1, with_sequence_header=False)
        n, lst, grp, tot, base, fill = _tile8((w, h, 10, 60), sym, key, 0, 0, 1 << 16)
        assert n > 0 and int((tot > 0).sum()) > (len(tot) + 1) // 2, "the content does not reach the second pass"
        assert av1stream.temporal_unit(w, h, 10, 60, opstream=True, **sym, **hdr) == av1stream.temporal_unit(w, h, 10, 60, **sym, **hdr)


def _tile8(f_args, sym, key, sbr, sbc, ops_cap, guard=64):
    """one tile through av1mi_host_opstream_tile8 into areas with guard words around them; returns (words, list, grouped, totals, bases,
    fill) after checking the guards"""
    import av1stream
    L = av1stream.lib()
    L.av1mi_host_opstream_slots.restype = C.c_int
    L.av1mi_host_opstream_tile8.restype = C.c_int
    L.av1mi_host_opstream_tile8.argtypes = [C.POINTER(av1stream.ObuFrame), C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 4
    ns = L.av1mi_host_opstream_slots()
    w, h, bd, q = f_args
    f = av1stream.ObuFrame()
    f.width, f.height, f.bit_depth, f.frame_type, f.base_q_idx = w, h, bd, 0 if key else 1, q
    f.tile_cols_log2 = f.tile_rows_log2 = -1
    keep = {k: np.ascontiguousarray(v.reshape(-1)) for k, v in sym.items()}
    for k, v in keep.items():
        setattr(f, k, v.ctypes.data)
    FILL32, FILL16 = 0xA5A5A5A5, 0x5A5A
    areas = [np.full(ops_cap + 2 * guard, FILL32, np.uint32), np.full(ops_cap + 4 * ns + 2 * guard, FILL32, np.uint32), np.full(ns + 2 * guard, FILL16, np.uint16),
             np.full(ns + 2 * guard, FILL16, np.uint16)]
    n = L.av1mi_host_opstream_tile8(C.byref(f), sbr, sbc, ops_cap, *[a.ctypes.data + guard * a.itemsize for a in areas])
    for a, fill in zip(areas, (FILL32, FILL32, FILL16, FILL16)):
        assert (a[:guard] == fill).all() and (a[-guard:] == fill).all(), "written outside the tile's areas"
    return (n,) + tuple(a[guard:-guard] for a in areas) + (FILL32,)


@pytest.mark.parametrize("key", [True, False], ids=["key", "inter"])
def test_a_tile_past_the_list_capacity_reports_overflow_and_writes_nothing(key):
    """the capacity of the list is the caller's: one word short of what the tile needs, the tile must report overflow (-1 -> the GPU kernel's
    status bit 0 and nops = 0), leave every slot total 0 and write neither list nor entries; with exactly enough it is coded"""
    rng = np.random.default_rng(3)
    w, h = 136, 72
    sym = _symbols(rng, "golomb_at_the_first_and_last_position", w, h, key)
    n, lst, grp, tot, base, fill = _tile8((w, h, 10, 60), sym, key, 0, 1, 1 << 14)
    assert n > 1000 and 0 < int(tot.sum()) <= n
    assert (lst[n:] == fill).all()                       # nothing beyond the tile's words
    last = int(base.argmax())
    assert (grp[int(base[last]) + int(tot[last]):] == fill).all()
    assert (base % 4 == 0).all() and (np.diff(base[tot > 0].astype(int)) > 0).all()
    # every entry names a list word the tokenizer left for the chains, each exactly once; the others are literals
    idx = np.concatenate([grp[int(b):int(b) + int(t)] >> 4 for b, t in zip(base, tot) if t])
    assert len(np.unique(idx)) == len(idx) == int(tot.sum()) and (lst[idx] == fill).all()
    rest = np.ones(n, bool)
    rest[idx] = False
    assert (lst[:n][rest] >> 31 == 1).all()
    n2, lst2, grp2, tot2, base2, _ = _tile8((w, h, 10, 60), sym, key, 0, 1, n)       # exactly enough
    assert n2 == n and (lst2 == lst[:n]).all() and (tot2 == tot).all() and (base2 == base).all()
    for cap in (n - 1, 100, 0):
        m, lst3, grp3, tot3, base3, _ = _tile8((w, h, 10, 60), sym, key, 0, 1, cap)
        assert m == -1
        assert (tot3 == 0).all()
        assert (lst3 == fill).all() and (grp3 == fill).all()


def test_a_block_with_more_than_255_symbols_of_one_slot():
    """The counts per (slot, block) are bytes.  A slot of one block reaches 255 only through the range symbols of large levels in one
    context: 64 luma levels of 15 or more give 4 range symbols each, of which the 2-D class of the positions away from the top-left
    corner holds up to 4 x 60 = 240 in one context — the largest count the 8x8 syntax can produce stays below 255, so the tile is CODED,
    as by the tokenizer before this one (whose counters were the same bytes, refusing a tile at the 256th symbol of a slot in a block)."""
    import av1stream
    w, h = 64, 64
    nb = 64
    sym = dict(y_mode=np.zeros(nb, np.uint8), uv_mode=np.zeros(nb, np.uint8), lev_y=np.full((nb, 64), 300, np.int16), lev_u=np.full((nb, 16), -300, np.int16),
               lev_v=np.full((nb, 16), 300, np.int16))
    n, lst, grp, tot, base, fill = _tile8((w, h, 10, 30), sym, True, 0, 0, 1 << 16)
    assert n > 0 and int(tot.max()) > 255 * 32          # slots with far more than 255 symbols in the TILE
    assert av1stream.temporal_unit(w, h, 10, 30, opstream=True, **sym) == av1stream.temporal_unit(w, h, 10, 30, **sym)
