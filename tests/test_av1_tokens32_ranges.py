"""The tile tokenizer of key frames in 32x32 blocks (av1-go_amd/csrc/av1_ops32.hpp tok_tile32): one wave per tile, the lanes over scan
ranges of a transform block (16 scan positions of a 32x32 luma block, 4 of a 16x16 chroma block).  The CPU twin (host/av1_opstream.cpp)
runs the same source as a loop over the lanes; its bytes must equal the general block writer's (host/av1_blockstream.cpp) on content
chosen to hit the range logic, and dav1d (when present) must decode them.  CPU only."""
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


SCAN = {16: _scan(16), 32: _scan(32)}


def _levels(rng, n, eob, density=0.5, big=()):
    """an n x n transform block whose last non-zero level is at scan index eob - 1; big: scan indices of levels above 14 (Golomb)"""
    a = np.zeros(n * n, np.int16)
    if eob:
        pos = SCAN[n][:eob]
        m = rng.random(eob) < density
        a[pos[m]] = rng.integers(1, 5, int(m.sum())) * rng.choice([-1, 1], int(m.sum()))
        a[pos[eob - 1]] = rng.choice([-2, -1, 1, 3])
        for c in big:
            if c < eob:
                a[pos[c]] = int(rng.integers(15, 4000)) * int(rng.choice([-1, 1]))
    return a


def _frame(rng, w, h, eobs_y, eobs_c, density=0.5, big_y=(), big_c=()):
    """a key frame of 32x32 blocks: block i takes eobs_y[i % len] / eobs_c[i % len] (U) / eobs_c[(i + 1) % len] (V)"""
    nblk = (w // 32) * (h // 32)
    ym, uvm = rng.integers(0, 13, nblk).astype(np.uint8), rng.integers(0, 13, nblk).astype(np.uint8)
    ly = np.stack([_levels(rng, 32, eobs_y[i % len(eobs_y)], density, big_y) for i in range(nblk)])
    lu = np.stack([_levels(rng, 16, eobs_c[i % len(eobs_c)], density, big_c) for i in range(nblk)])
    lv = np.stack([_levels(rng, 16, eobs_c[(i + 1) % len(eobs_c)], density, big_c) for i in range(nblk)])
    return dict(y_mode=ym, uv_mode=uvm, lev_y=ly, lev_u=lu, lev_v=lv)


def _lr_header(w, h):
    ur = lambda n: max(1, (n + 32) // 64)
    uy = np.tile(np.array([1, 3, -7, 15, 3, -7, 15, 0], np.int8), (ur(h), ur(w), 1))
    uc = np.tile(np.array([1, 0, -7, 15, 0, -7, 15, 0], np.int8), (ur(h // 2), ur(w // 2), 1))
    return dict(lr_type=(1, 0, 1), lr_units=(uy, uc, uc), lf_level=(9, 7, 5, 5), cdef_y=(5,), cdef_uv=(4,), cdef_damping=4)


def _both_writers(w, h, bd, q, sym, lr):
    """the frame through the general block writer and through the twin; a tile the twin cannot place raises (no case may overflow)"""
    import av1stream
    import av1_blocks as B
    lay = B.Layout(w, h)
    parts, tree = B.build_tree(lay, B.uniform_chooser(9))
    w32 = w // 32
    blocks = []
    for r, c, bsize, tb in tree:
        i = (r // 8) * w32 + c // 8
        blocks.append(dict(r=r, c=c, bsize=bsize, tile=tb, skip=0, is_inter=0, y_mode=int(sym["y_mode"][i]), uv_mode=int(sym["uv_mode"][i]), angle_y=0,
                           angle_uv=0, cfl=(0, 0), tx_depth=0, filt=0, mv=(0, 0), tx=B.max_tx_rect(bsize), tx_types=[0],
                           levels=[[sym["lev_y"][i]], [sym["lev_u"][i]], [sym["lev_v"][i]]]))
    hdr = _lr_header(w, h) if lr else {}
    ref = B.encode(lay, bd, q, parts, blocks, **hdr)
    nb = (h // 8) * (w // 8)
    ym, uvm = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
    ym[:len(sym["y_mode"])], uvm[:len(sym["uv_mode"])] = sym["y_mode"], sym["uv_mode"]
    twin = av1stream.temporal_unit(w, h, bd, q, opstream=True, key_rows32=h, y_mode=ym, uv_mode=uvm, lev_y=sym["lev_y"].reshape(-1),
                                   lev_u=sym["lev_u"].reshape(-1), lev_v=sym["lev_v"].reshape(-1), **hdr)
    return ref, twin


def _check(w, h, bd, q, sym, lr):
    import dav1d_ref as D
    ref, twin = _both_writers(w, h, bd, q, sym, lr)
    assert twin == ref
    if D.available():
        pics = D.decode(twin, inloop_filters=0)
        assert len(pics) == 1 and np.asarray(pics[0][0]).shape == (h, w)


# eob exactly at, one below and one above a range boundary (16 luma / 4 chroma scan positions per lane), eob = 1 and eob = N^2
EOBS_Y = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 511, 512, 513, 1007, 1008, 1009, 1023, 1024]
EOBS_C = [1, 3, 4, 5, 7, 8, 9, 127, 128, 129, 251, 252, 253, 255, 256, 2]
CASES = {
    "eob_at_range_boundaries": lambda rng, w, h: _frame(rng, w, h, EOBS_Y, EOBS_C),
    "eob_at_range_boundaries_sparse": lambda rng, w, h: _frame(rng, w, h, EOBS_Y[::-1], EOBS_C[::-1], density=0.05),
    "eob_1_everywhere": lambda rng, w, h: _frame(rng, w, h, [1], [1]),
    "eob_full_everywhere": lambda rng, w, h: _frame(rng, w, h, [1024], [256], density=0.3),
    "zero_luma_nonzero_chroma": lambda rng, w, h: _frame(rng, w, h, [0], [5, 256, 1, 64]),
    "nonzero_luma_zero_chroma": lambda rng, w, h: _frame(rng, w, h, [17, 1024, 1, 300], [0]),
    "mixed_zero_blocks": lambda rng, w, h: _frame(rng, w, h, [0, 40, 0, 0, 1024], [0, 0, 9, 256, 0, 1]),
    "all_zero": lambda rng, w, h: _frame(rng, w, h, [0], [0]),
    "golomb_in_the_first_and_last_range": lambda rng, w, h: _frame(rng, w, h, [1024, 1017, 16, 3], [256, 254, 4, 2], density=0.2, big_y=(0, 1, 7, 15, 1008, 1016, 1023),
                                                                  big_c=(0, 3, 252, 253, 255)),
}


@pytest.mark.parametrize("lr", [False, True], ids=["lr_off", "lr_on"])
@pytest.mark.parametrize("w,h", [(128, 128), (160, 64), (96, 128)], ids=["128x128", "160x64_half_sb", "96x128_half_sb"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_range_logic_twin_equals_the_block_writer(case, w, h, lr):
    """width % 64 == 32: a last column of half superblocks (blocks 1 and 3 of the tile are not coded)"""
    rng = np.random.default_rng(sorted(CASES).index(case) * 7 + w)
    _check(w, h, 10, 100, CASES[case](rng, w, h), lr)


@pytest.mark.parametrize("w,h,lr", [(128, 128, True), (160, 128, False)])
def test_dense_noise_at_q23(O, w, h, lr):
    """noise through the 32x32 block pipeline of the oracle at the reference's quality: every range of every block is full"""
    rng = np.random.default_rng(23)
    bd = 10
    Y, U, V = (rng.integers(0, 1 << bd, (h // d, w // d)).astype(np.uint16) for d in (1, 2, 2))
    a = O.intra_encode_frame(Y, U, V, bd, 32, 23)
    n = (w // 32) * (h // 32)
    sym = dict(y_mode=a["modes_y"], uv_mode=a["modes_uv"], lev_y=a["lev_y"].reshape(n, 1024), lev_u=a["lev_u"].reshape(n, 256), lev_v=a["lev_v"].reshape(n, 256))
    assert (sym["lev_y"] != 0).mean() > 0.5
    _check(w, h, bd, 23, sym, lr)


def _tile32(f_args, sym, sbr, sbc, ops_cap, guard=64):
    """one tile through av1mi_host_opstream_tile32 into areas with guard words around them; returns (words, list, grouped, totals, bases)
    after checking the guards"""
    import av1stream
    L = av1stream.lib()
    L.av1mi_host_opstream_slots.restype = C.c_int
    L.av1mi_host_opstream_tile32.restype = C.c_int
    L.av1mi_host_opstream_tile32.argtypes = [C.POINTER(av1stream.ObuFrame), C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 4
    ns = L.av1mi_host_opstream_slots()
    w, h, bd, q = f_args
    f = av1stream.ObuFrame()
    f.width, f.height, f.bit_depth, f.frame_type, f.base_q_idx = w, h, bd, 0, q
    f.tile_cols_log2 = f.tile_rows_log2 = -1
    keep = {k: np.ascontiguousarray(v.reshape(-1)) for k, v in sym.items()}
    for k, v in keep.items():
        setattr(f, k, v.ctypes.data)
    FILL32, FILL16 = 0xA5A5A5A5, 0x5A5A
    areas = [np.full(ops_cap + 2 * guard, FILL32, np.uint32), np.full(ops_cap + 4 * ns + 2 * guard, FILL32, np.uint32), np.full(ns + 2 * guard, FILL16, np.uint16),
             np.full(ns + 2 * guard, FILL16, np.uint16)]
    n = L.av1mi_host_opstream_tile32(C.byref(f), sbr, sbc, ops_cap, *[a.ctypes.data + guard * a.itemsize for a in areas])
    for a, fill in zip(areas, (FILL32, FILL32, FILL16, FILL16)):
        assert (a[:guard] == fill).all() and (a[-guard:] == fill).all(), "written outside the tile's areas"
    return (n,) + tuple(a[guard:-guard] for a in areas) + (FILL32,)


def test_a_tile_past_the_list_capacity_reports_overflow_and_writes_nothing():
    """the capacity of the list is the caller's: one word short of what the tile needs, the tile must report overflow (-1 -> the GPU kernel's
    status bit 0 and nops = 0), leave every slot total 0 and write neither list nor entries; with exactly enough it is coded"""
    rng = np.random.default_rng(3)
    w, h = 128, 64
    sym = _frame(rng, w, h, [1024, 700], [256, 100], density=0.6, big_y=(0, 1023), big_c=(1,))
    n, lst, grp, tot, base, fill = _tile32((w, h, 10, 60), sym, 0, 1, 1 << 16)
    assert n > 4000 and int(tot.sum()) > 0 and int(tot.sum()) <= n
    assert (lst[n:] == fill).all()                       # nothing beyond the tile's words
    assert (grp[int(base.max()) + int(tot[int(base.argmax())]):] == fill).all()
    n2, lst2, grp2, tot2, base2, _ = _tile32((w, h, 10, 60), sym, 0, 1, n)       # exactly enough
    assert n2 == n and (lst2 == lst[:n]).all() and (tot2 == tot).all() and (base2 == base).all()
    for cap in (n - 1, 100, 0):
        m, lst3, grp3, tot3, base3, _ = _tile32((w, h, 10, 60), sym, 0, 1, cap)
        assert m == -1
        assert (tot3 == 0).all()
        assert (lst3 == fill).all() and (grp3 == fill).all()
