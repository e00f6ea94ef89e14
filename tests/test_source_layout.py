"""The source layout without a GPU (include/av1mi.h av1mi_source_layout): av1mi_gop_source_layout against formulas written here from
the header's text — the fed size, the true size, the depth, every plane's size and bytes — over a table that crosses input formats,
chroma layouts, depths, scaling, cropped sizes and segment counts, and the refusals it shares with av1mi_gop_open."""
import ctypes as C
import itertools

import pytest

FORMATS, LAYOUTS = (0, 1, 2, 3), (0, 1, 2, 3)                    # enum av1mi_input_format, enum av1mi_source_chroma
DEPTHS = ((8, 8), (10, 10), (12, 10), (0, 8), (0, 10))           # (source_bit_depth, bit_depth): the pairs av1mi_gop_open accepts; 0 = bit_depth
CODED = (((8, 8), None), ((72, 40), (70, 38)), ((136, 72), (130, 70)))      # coded size, and a visible size inside it
SOURCES = (None, (35, 21), (100, 50), (136, 72))                 # scaling: the true size of the fed frames (odd; padded; a multiple of 8)


def _r8(n):
    return (n + 7) & ~7


def _cfg(av1mi, coded, visible=None, fmt=0, chroma=0, src_bd=0, bd=8, source=None, segments=1, **kw):
    d = dict(width=coded[0], height=coded[1], bit_depth=bd, base_q_idx=100, gop_length=2, segments=segments, search_range=8, input_format=fmt,
             source_chroma=chroma, source_bit_depth=src_bd)
    if visible:
        d.update(visible_width=visible[0], visible_height=visible[1])
    if source:
        d.update(source_width=source[0], source_height=source[1])
    d.update(kw)
    return av1mi.GopConfig(**d)


def _accepted(coded, visible, fmt, chroma, src_bd, bd, source):
    """the rules of av1mi_gop_open that the table's axes can break, from the header: a wire format is 4:2:0 at its own depth; a scaler's
    source and target are at least 16 x 16 and within a factor of 4 of each other"""
    if (fmt in (1, 2) and bd != 10) or (fmt == 3 and bd != 8):
        return False
    if fmt != 0 and (chroma != 0 or (src_bd or bd) != bd):
        return False
    if source:
        tw, th = visible or coded
        if min(source + (tw, th)) < 16 or source[0] > 4 * tw or tw > 4 * source[0] or source[1] > 4 * th or th > 4 * source[1]:
            return False
    return True


def _expected(av1mi, coded, visible, fmt, chroma, src_bd, bd, source):
    """(width, height, true_width, true_height, bit_depth, [(width, height, frame_bytes)] * 3) by the header's text"""
    W, H = (_r8(source[0]), _r8(source[1])) if source else coded
    true = source or visible or coded
    depth = src_bd or bd
    item = 1 if depth == 8 else 2
    if fmt == 0:          # a planar source in its chroma layout
        planes = [(s[1], s[0], s[0] * s[1] * item) if s else (0, 0, 0) for s in av1mi.source_plane_shapes(chroma, W, H)]
    elif fmt == 1:        # 10 bits per sample, no padding
        planes = [(W, H, W * H * 10 // 8)] + [(W // 2, H // 2, (W // 2) * (H // 2) * 10 // 8)] * 2
    else:                 # P010 / NV12: the luma plane, then one plane of interleaved pairs
        planes = [(W, H, W * H * item), (W, H // 2, W * (H // 2) * item), (0, 0, 0)]
    return (W, H) + tuple(true) + (depth, planes)


def _got(L):
    return (L.width, L.height, L.true_width, L.true_height, L.bit_depth, [(P.width, P.height, P.frame_bytes) for P in L.plane])


def test_layout_of_every_configuration(av1mi):
    accepted = refused = 0
    for (coded, crop), cropped, fmt, chroma, (src_bd, bd), source, S in itertools.product(CODED, (False, True), FORMATS, LAYOUTS, DEPTHS, SOURCES, (1, 3)):
        if cropped and not crop:
            continue
        visible = crop if cropped else None
        axes = (coded, visible, fmt, chroma, src_bd, bd, source)
        cfg = _cfg(av1mi, coded, visible, fmt, chroma, src_bd, bd, source, S)
        if not _accepted(*axes):
            with pytest.raises(av1mi.Av1miError) as e:
                av1mi.gop_source_layout(cfg)
            assert e.value.code == -1, axes
            refused += 1
            continue
        L = av1mi.gop_source_layout(cfg)
        want = _expected(av1mi, *axes)
        assert _got(L) == want, axes
        W, H = want[0], want[1]
        for p, (pw, ph, fb) in enumerate(want[5]):
            # a batch's plane is `segments` frames: what today's two functions give for rows = segments * height
            if fmt == 0:
                assert S * fb == av1mi.source_plane_bytes(chroma, src_bd or bd, p, W, S * H), (axes, p)
            if chroma == 0 and (src_bd or bd) == bd:
                assert S * fb == av1mi.input_plane_bytes(fmt, bd, p, W, S * H), (axes, p)
            assert (fb == 0) == (pw == 0 and ph == 0) == (p > 0 and (chroma == 3 or (p == 2 and fmt in (2, 3)))), (axes, p)
        accepted += 1
    assert accepted > 300 and refused > 300      # the table is not vacuous on either side


BASE = dict(coded=(72, 40), bd=10)
REFUSED = [      # one per refusal of av1mi_gop_open's argument rules
    dict(coded=(0, 40)), dict(coded=(72, -8)), dict(coded=(70, 40)), dict(coded=(72, 38)), dict(coded=(16392, 40)),
    dict(visible=(80, 40)), dict(visible=(64, 40)), dict(visible=(72, 32)), dict(visible_width=-1), dict(visible_height=-1),
    dict(bd=9), dict(bd=12), dict(base_q_idx=0), dict(base_q_idx=256), dict(gop_length=0), dict(segments=0), dict(segments=4097),
    dict(search_range=-1), dict(search_range=16), dict(gpu_entropy=3), dict(gpu_entropy=-1), dict(coder_streams=4), dict(coder_streams=-1),
    dict(fmt=-1), dict(fmt=4), dict(fmt=1, bd=8), dict(fmt=2, bd=8), dict(fmt=3, bd=10),
    dict(chroma=-1), dict(chroma=4), dict(src_bd=9), dict(src_bd=16), dict(src_bd=12, bd=8), dict(src_bd=10, bd=8), dict(src_bd=8, bd=10),
    dict(fmt=2, chroma=2), dict(fmt=3, bd=8, chroma=1), dict(fmt=1, src_bd=12),
    dict(source_width=64), dict(source_height=64), dict(source=(-64, -64)), dict(source=(8, 64)), dict(source=(600, 64)), dict(source=(64, 600)),
    dict(source=(4104, 2048)), dict(key_block_size=16), dict(key_block_size=32), dict(gpu_entropy=1, coded=(4104, 40)),
    dict(coded=(72, 16384), segments=33), dict(coarse_range=-4), dict(coarse_range=68), dict(coarse_range=6),
    dict(quality_stats=1, coded=(72, 8)), dict(quality_stats=1, coded=(16, 16), visible=(15, 16)),
    dict(store_frames=-1), dict(store_frames=65536), dict(store_frames=4, fmt=1), dict(deinterlace=3, store_frames=4), dict(deinterlace=-1, store_frames=4),
    dict(deinterlace=1),
]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()).replace(" ", ""))
def test_what_open_refuses_has_no_layout(av1mi, bad):
    L = av1mi.gop_source_layout(_cfg(av1mi, **BASE))
    assert (L.width, L.height, L.bit_depth) == (72, 40, 10)
    with pytest.raises(av1mi.Av1miError) as e:
        av1mi.gop_source_layout(_cfg(av1mi, **dict(BASE, **bad)))
    assert e.value.code == -1


def test_null_pointers_are_refused_and_the_output_is_untouched(av1mi):
    lib = av1mi.load()
    lib.av1mi_gop_source_layout.argtypes = [C.c_void_p] * 2
    cfg, out = _cfg(av1mi, **BASE), av1mi.SourceLayout()
    assert lib.av1mi_gop_source_layout(None, C.addressof(out)) == -1 and lib.av1mi_gop_source_layout(C.addressof(cfg), None) == -1
    assert lib.av1mi_gop_source_layout(C.addressof(cfg), C.addressof(out)) == 0 and out.plane[1].frame_bytes == 36 * 20 * 2
    bad = _cfg(av1mi, **dict(BASE, bd=9))
    assert lib.av1mi_gop_source_layout(C.addressof(bad), C.addressof(out)) == -1 and out.plane[1].frame_bytes == 36 * 20 * 2
