"""GPU tests of inverse telecine's two kernels on their own (av1-go_amd/csrc/telecine_kernels.hip): the field-match records
(av1mi_telecine_analyse) and the weave gather (av1mi_telecine_gather), bit exact against tests/telecine_ref.py."""
import numpy as np
import pytest

import telecine_ref as T

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- records
def _content(kind, n, hb, wb, bd, seed):
    top = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, top + 1, (n, hb, wb)).astype(dt)
    # the extremes: 0 / max alternating lines, the phase flipping from frame to frame: every term of every sum is at its largest
    Y = np.zeros((n, hb, wb), dt)
    for f in range(n):
        Y[f, (f & 1)::2] = top
    return Y


def _check_records(ctx, Y, bd, w, h):
    got = ctx.telecine_analyse(Y, bd, (w, h))
    want = T.records(Y, bd, w, h)
    assert got["comb"].tolist() == want["comb"].tolist() and got["bdiff"].tolist() == want["bdiff"].tolist(), (Y.shape, bd, w, h)


# buffer (w, h), true (w, h): odd height (the last line is a top-field line), odd width, heights without / with one eligible line
SIZES = [((16, 8), (16, 8)), ((24, 16), (18, 10)), ((24, 16), (17, 9)), ((16, 8), (16, 3)), ((16, 8), (16, 2)), ((16, 8), (13, 4)),
         ((24, 40), (20, 37))]      # ... and three tiles of rows (16 a tile)


@pytest.mark.parametrize("kind", ["random", "extreme"])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("n", [1, 2, 7])
def test_records_are_the_reference(ctx, n, bd, kind):
    for (wb, hb), (w, h) in SIZES:
        _check_records(ctx, _content(kind, n, hb, wb, bd, 11 * n + bd), bd, w, h)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_records_of_a_run_longer_than_a_chunk_and_wider_than_a_tile(ctx, bd):
    """a workgroup walks 16 frames: 18 frames are two chunks, the second starting from frames 15 and 16; 64 cells a tile: 66 cells are two"""
    _check_records(ctx, _content("random", 18, 16, 24, bd, 5), bd, 19, 11)
    _check_records(ctx, _content("extreme", 33, 8, 16, bd, 5), bd, 16, 8)
    wb = 66 * (16 if bd == 8 else 8)
    _check_records(ctx, _content("random", 3, 8, wb, bd, 6), bd, wb - 5, 7)


def test_records_ignore_the_padding(ctx):
    Y = _content("random", 4, 16, 24, 10, 9)
    Z = Y.copy()
    Z[:, 9:, :] = 1023 - Z[:, 9:, :]
    Z[:, :, 17:] = 777
    a, b = ctx.telecine_analyse(Y, 10, (17, 9)), ctx.telecine_analyse(Z, 10, (17, 9))
    assert a.tobytes() == b.tobytes()


def test_records_of_a_pulldown_plan_to_the_film(ctx):
    import av1stream
    Y = np.stack([T.pad8(T.video_frame(v, "tff", 70, 50)[0], True) for v in range(6, 18)])
    rec = ctx.telecine_analyse(Y, 8, (70, 50))
    assert rec.tobytes() == T.records(Y, 8, 70, 50).tobytes()
    top, bottom = av1stream.plan_telecine(rec, 1, 1)
    for k in range(8):
        woven = T.weave_plane(Y[top[k]], Y[bottom[k]], 70, 50)
        assert (woven[:50, :70] == T.film_frame(T.video_sources(7, "tff")[1] + k, 70, 50)[0]).all()


def test_analyse_refuses_bad_arguments(ctx, av1mi):
    for Y, bd, true in ((np.zeros((1, 16, 24), np.uint8), 9, (24, 16)), (np.zeros((1, 16, 24), np.uint8), 8, (16, 16)), (np.zeros((1, 16, 24), np.uint8), 8, (24, 0)),
                        (np.zeros((1, 16, 20), np.uint8), 8, (20, 16))):
        with pytest.raises(av1mi.Av1miError) as e:
            ctx.telecine_analyse(Y, bd, true)
        assert "av1mi_telecine_analyse" in str(e.value)


# ---------------------------------------------------------------------------------------------- the weave
def _weave_against_reference(ctx, planes, sizes, true_sizes, bd, pairs):
    """planes[p]: [frames, PH, PW] (None = no such plane); pairs[s] = (top frame, bottom frame), top -1 = a flat slot.  Checks every
    destination plane against the reference and that nothing beyond it is written"""
    S = len(pairs)
    dt = np.uint8 if bd == 8 else np.uint16
    have = [p for p in range(3) if planes[p] is not None]
    planes = [np.ascontiguousarray(planes[p], dt) if p in have else None for p in range(3)]
    nbytes = [planes[p][0].nbytes if p in have else 0 for p in range(3)]
    d_store = [ctx.to_device(planes[p]) if p in have else None for p in range(3)]
    table = np.zeros((S, 3, 2), np.uint64)
    for s, (t, b) in enumerate(pairs):
        for p in have:
            if t >= 0:
                table[s, p] = (d_store[p].ptr + t * nbytes[p], d_store[p].ptr + b * nbytes[p])
    d_table = ctx.to_device(table)
    guard = 64
    d_dst = [ctx.to_device(np.full(S * nbytes[p] + guard, 0xA5, np.uint8)) if p in have else None for p in range(3)]
    try:
        ctx.telecine_gather(bd, sizes, true_sizes, S, d_table, d_dst)
        for p in have:
            raw = d_dst[p].download((S * nbytes[p] + guard,), np.uint8)
            assert (raw[S * nbytes[p]:] == 0xA5).all(), "plane %d: written beyond its end" % p
            got = raw[:S * nbytes[p]].view(dt).reshape((S,) + planes[p].shape[1:])
            for s, (t, b) in enumerate(pairs):
                want = T.weave_plane(planes[p][t] if t >= 0 else None, planes[p][b], *true_sizes[p])
                bad = np.argwhere(got[s] != want)
                assert bad.size == 0, "plane %d segment %d (%d / %d): %d samples differ, the first at (y, x) = %s" % (p, s, t, b, len(bad), bad[0])
    finally:
        for b in d_store + d_dst + [d_table]:
            if b is not None:
                b.free()


def _planes(sizes, n, bd, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, (n, h, w)).astype(np.uint8 if bd == 8 else np.uint16) if w else None for w, h in sizes]


PAIRS = [(0, 1), (2, 2), (-1, 0), (3, 1), (1, 0)]      # a null slot among real ones, top == bottom


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_weave_of_a_420_frame_with_odd_chroma_height(ctx, bd):
    """true 18x10 in 24x16: chroma 9x5 in 12x8; at 8 bits the luma rows are 24 bytes and the chroma rows 12: both dword paths, at 16 bits
    48 and 24 bytes: luma in 16-byte units"""
    sizes, true = [(24, 16), (12, 8), (12, 8)], [(18, 10), (9, 5), (9, 5)]
    _weave_against_reference(ctx, _planes(sizes, 4, bd, bd), sizes, true, bd, PAIRS)


@pytest.mark.parametrize("bd", [8, 10])
def test_weave_rows_of_8_bytes_and_of_whole_units(ctx, bd):
    w8 = 8 if bd == 8 else 4                       # rows of 8 bytes: the dword path
    sizes, true = [(w8, 8), (0, 0), (0, 0)], [(w8 - 1, 5), (1, 1), (1, 1)]
    _weave_against_reference(ctx, _planes(sizes, 4, bd, 3), sizes, true, bd, PAIRS)
    w16 = 32 if bd == 8 else 16                    # rows of two whole 16-byte units; true sizes that are no multiple of 8
    sizes, true = [(w16, 24), (w16 // 2, 12), (w16 // 2, 12)], [(w16 - 3, 19), (w16 // 2 - 1, 10), (w16 // 2 - 1, 10)]
    _weave_against_reference(ctx, _planes(sizes, 4, bd, 4), sizes, true, bd, PAIRS)


def test_weave_a_plane_of_one_line_is_the_top_source(ctx):
    sizes, true = [(40, 8), (20, 4), (20, 4)], [(40, 1), (20, 1), (20, 1)]
    planes = _planes(sizes, 3, 8, 8)
    _weave_against_reference(ctx, planes, sizes, true, 8, [(0, 1), (2, 0), (1, 1)])
    assert (T.weave_plane(planes[0][0], planes[0][1], 40, 1) == planes[0][0][:1]).all()


def test_weave_more_than_a_group_of_cells_more_than_a_band_and_a_cell_in_the_padding(ctx):
    """66 cells a row (a wave owns 64), 40 rows (a band is 16); and rows of 20 samples with 13 true ones, whose second cell lies wholly
    beyond the true width"""
    sizes, true = [(66 * 16, 40), (0, 0), (0, 0)], [(66 * 16 - 3, 35), (1, 1), (1, 1)]
    _weave_against_reference(ctx, _planes(sizes, 3, 8, 2), sizes, true, 8, [(0, 1), (2, 1)])
    sizes, true = [(20, 8), (0, 0), (0, 0)], [(13, 6), (1, 1), (1, 1)]
    _weave_against_reference(ctx, _planes(sizes, 3, 8, 2), sizes, true, 8, [(0, 1), (2, 1), (-1, 0)])


def test_weave_of_equal_sources_is_that_source(ctx):
    sizes, true = [(24, 16), (12, 8), (12, 8)], [(24, 16), (12, 8), (12, 8)]
    planes = _planes(sizes, 2, 10, 1)
    _weave_against_reference(ctx, planes, sizes, true, 10, [(1, 1), (0, 0)])
    assert (T.weave_plane(planes[0][1], planes[0][1], 24, 16) == planes[0][1]).all()


def test_gather_refuses_bad_arguments(ctx, av1mi):
    d, d_table = ctx.to_device(np.zeros(4096, np.uint8)), ctx.to_device(np.zeros(6, np.uint64))
    ok = dict(bit_depth=8, plane_sizes=[(24, 16), (12, 8), (12, 8)], true_sizes=[(18, 10), (9, 5), (9, 5)], segments=1, d_table=d_table, d_dst=[d, d, d])
    ctx.telecine_gather(**ok)      # (a table of zeros: flat slots)
    for bad in (dict(bit_depth=9), dict(segments=0), dict(true_sizes=[(8, 10), (9, 5), (9, 5)]), dict(plane_sizes=[(22, 16), (12, 8), (12, 8)])):
        with pytest.raises(av1mi.Av1miError) as e:
            ctx.telecine_gather(**dict(ok, **bad))
        assert "av1mi_telecine_gather" in str(e.value)
    ctx.sync()
    d.free()
    d_table.free()
