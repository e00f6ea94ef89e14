"""CPU tests of the colour description and the HDR10 static metadata (include/av1mi_host.h av1mi_colour): the sequence header's color_config read
back by a bit reader written from spec 5.5, the metadata OBUs (5.8.3 / 5.8.4), the Matroska Colour element, the job's options."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import av1stream
import dav1d_ref as D

MDCV = ((45875, 19661), (11141, 52233), (8585, 3015), (20493, 21561), 10000 << 8, 1)      # BT.2020 primaries, D65, the extremes of the luminances
HDR10 = dict(primaries=9, transfer=16, matrix=9, full_range=0, mdcv=MDCV, cll=(65535, 400))
CASES = [dict(primaries=9, transfer=16, matrix=9, full_range=0), dict(primaries=1, transfer=1, matrix=1, full_range=0),
         dict(primaries=9, transfer=18, matrix=9, full_range=1), dict(full_range=1)]


@functools.lru_cache(maxsize=None)
def _key_symbols(w, h, bd):
    """a key frame coded by the oracle, as the writer tests use them (tests/test_av1_conformance.py)"""
    import synth
    from oracle import oracle as O
    O.build()
    Y, U, V = synth.frames(w, h, 1, bd, 3)
    r = O.intra_encode_frame(Y[0], U[0], V[0], bd, 8, 100)
    return dict(y_mode=r["modes_y"], uv_mode=r["modes_uv"], lev_y=r["lev_y"], lev_u=r["lev_u"], lev_v=r["lev_v"])


def _unit(w, h, bd, visible, key, seq, colour):
    """the 8x8 writer: an oracle-coded key frame, or a P frame of zero vectors and no residual behind it"""
    nb = (w // 8) * (h // 8)
    z = lambda n, dt: np.zeros(n, dt)
    if key:
        kw = _key_symbols(w, h, bd)
    else:
        kw = dict(y_mode=z(nb, np.uint8), uv_mode=z(nb, np.uint8), skip=np.ones(nb, np.uint8), lev_y=z(nb * 64, np.int16), lev_u=z(nb * 16, np.int16), lev_v=z(nb * 16, np.int16),
                  mv=z(nb * 2, np.int16), is_inter=np.ones(nb, np.uint8))
    return av1stream.temporal_unit(w, h, bd, 100, frame_type=0 if key else 1, with_sequence_header=seq, visible=visible, colour=colour, **kw)


@functools.lru_cache(maxsize=None)
def _block_symbols(w, h, bd):
    """a key frame of a random partition tree with oracle-made levels, as the block writer tests use them (tests/test_av1_blocks.py)"""
    import av1_blocks as B
    from oracle import oracle as O
    O.build()
    lay = B.Layout(w, h)
    return (lay,) + tuple(B.random_frame(O, np.random.default_rng(5), lay, bd, 100))


def _block_unit(colour, seq=True, w=64, h=64, visible=None, bd=8):
    import av1_blocks as B
    lay, parts, blocks = _block_symbols(w, h, bd)
    return B.encode(lay, bd, 100, parts, blocks, with_sequence_header=seq, colour=colour, visible=visible)


def _obus(b):
    out, p = [], 0
    while p < len(b):
        hdr = b[p]; p += 1
        assert hdr & 2      # obu_has_size_field
        n = sh = 0
        while True:
            c = b[p]; p += 1
            n |= (c & 0x7F) << sh; sh += 7
            if not c & 0x80:
                break
        out.append(((hdr >> 3) & 15, b[p:p + n])); p += n
    return out


class Bits:
    def __init__(self, b):
        self.b, self.p = b, 0

    def f(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.b[self.p >> 3] >> (7 - (self.p & 7))) & 1); self.p += 1
        return v


def _color_config(seq):
    """sequence_header_obu (5.5.1) as this writer's streams use it, down to color_config (5.5.2): (primaries, transfer, matrix, range)"""
    r = Bits(seq)
    assert r.f(3) == 0 and r.f(1) == 0 and r.f(1) == 0      # profile 0, not a still picture, full header
    assert r.f(1) == 0 and r.f(1) == 0                      # timing_info_present_flag, initial_display_delay_present_flag
    assert r.f(5) == 0                                      # operating_points_cnt_minus_1
    r.f(12); lvl = r.f(5)
    if lvl > 7:
        r.f(1)                                              # seq_tier
    wb, hb = r.f(4) + 1, r.f(4) + 1
    r.f(wb); r.f(hb)
    assert r.f(1) == 0                                      # frame_id_numbers_present_flag
    r.f(1); r.f(1); r.f(1)                                  # use_128x128_superblock, enable_filter_intra, enable_intra_edge_filter
    r.f(1); r.f(1); r.f(1); r.f(1)                          # interintra, masked compound, warped motion, dual filter
    assert r.f(1) == 0                                      # enable_order_hint (so no jnt_comp / ref_frame_mvs)
    assert r.f(1) == 0                                      # seq_choose_screen_content_tools
    if r.f(1) > 0:                                          # seq_force_screen_content_tools
        if r.f(1) == 0:
            r.f(1)
    r.f(1); r.f(1); r.f(1)                                  # enable_superres, enable_cdef, enable_restoration
    r.f(1)                                                  # high_bitdepth (profile 0: no twelve_bit)
    assert r.f(1) == 0                                      # mono_chrome
    p, t, m = (r.f(8), r.f(8), r.f(8)) if r.f(1) else (2, 2, 2)
    assert not (p == 1 and t == 13 and m == 0)
    return p, t, m, r.f(1)


@pytest.mark.parametrize("w,h,visible", [(64, 64, None), (24, 40, (20, 38))])
@pytest.mark.parametrize("case", CASES)
def test_description_in_the_sequence_header(w, h, visible, case):
    c = av1stream.Colour(**case)
    tu = _unit(w, h, 10, visible, True, True, c)
    seq = [p for t, p in _obus(tu) if t == 1]
    assert len(seq) == 1
    assert _color_config(seq[0]) == (case.get("primaries", 2), case.get("transfer", 2), case.get("matrix", 2), case.get("full_range", 0))
    blk = [p for t, p in _obus(_block_unit(c, w=w, h=h, visible=visible, bd=10)) if t == 1]
    assert len(blk) == 1 and blk[0] == seq[0] and _color_config(blk[0]) == _color_config(seq[0])
    assert not [t for t, _ in _obus(tu) if t == 5]


def test_null_and_unspecified_change_no_byte():
    for w, h, visible in ((64, 64, None), (24, 40, (20, 38))):
        for key, seq in ((True, True), (False, False)):
            assert _unit(w, h, 8, visible, key, seq, None) == _unit(w, h, 8, visible, key, seq, av1stream.Colour())
    assert _block_unit(None) == _block_unit(av1stream.Colour()) and _block_unit(None, w=24, h=40, visible=(20, 38)) == _block_unit(av1stream.Colour(), w=24, h=40, visible=(20, 38))


def test_metadata_obus_follow_the_sequence_header_and_parse_back():
    c = av1stream.Colour(**HDR10)
    for tu in (_unit(64, 64, 10, None, True, True, c), _block_unit(c)):
        obus = _obus(tu)
        assert [t for t, _ in obus] == [2, 1, 5, 5, 6]
        cll, mdcv = obus[2][1], obus[3][1]
        assert cll[0] == 1 and struct.unpack(">HH", cll[1:5]) == (65535, 400) and cll[5:] == b"\x80"
        assert mdcv[0] == 2 and mdcv[25:] == b"\x80"
        v = struct.unpack(">8HII", mdcv[1:25])
        assert v[:6] == (45875, 19661, 11141, 52233, 8585, 3015) and v[6:8] == (20493, 21561) and v[8:] == (10000 << 8, 1)
    # no sequence header, no metadata
    assert [t for t, _ in _obus(_unit(64, 64, 10, None, False, False, c))] == [2, 6]
    assert [t for t, _ in _obus(_block_unit(c, seq=False))] == [2, 6]


@pytest.mark.skipif(not D.available(), reason="dav1d is not installed")
def test_dav1d_decodes_the_same_frames():
    c = av1stream.Colour(**HDR10)
    for w, h, visible in ((64, 64, None), (24, 40, (20, 38))):
        a = D.decode(_unit(w, h, 10, visible, True, True, c) + _unit(w, h, 10, visible, False, False, c))
        b = D.decode(_unit(w, h, 10, visible, True, True, None) + _unit(w, h, 10, visible, False, False, None))
        assert len(a) == len(b) == 2 and all((x == y).all() for fa, fb in zip(a, b) for x, y in zip(fa, fb))
        assert a[0][0].shape == ((visible or (w, h))[1], (visible or (w, h))[0]) and a[0][0].std() > 0
        a, b = D.decode(_block_unit(c, w=w, h=h, visible=visible, bd=10)), D.decode(_block_unit(None, w=w, h=h, visible=visible, bd=10))
        assert len(a) == len(b) == 1 and all((x == y).all() for x, y in zip(a[0], b[0])) and a[0][0].std() > 0


def test_refusals():
    for bad in (dict(matrix=0), dict(primaries=256), dict(transfer=-1), dict(matrix=300)):
        with pytest.raises(ValueError):
            _unit(64, 64, 8, None, True, True, av1stream.Colour(**bad))


def _ebml(b, p, end):
    """(id, payload) of the elements in b[p:end]"""
    out = []
    while p < end:
        n = 1
        while not b[p] & (0x80 >> (n - 1)):
            n += 1
        eid = int.from_bytes(b[p:p + n], "big"); p += n
        k = 1
        while not b[p] & (0x80 >> (k - 1)):
            k += 1
        size = int.from_bytes(b[p:p + k], "big") & ((1 << (7 * k)) - 1); p += k
        if size == (1 << (7 * k)) - 1:
            size = end - p
        out.append((eid, b[p:p + size])); p += size
    return out


def _find(b, path):
    for eid in path:
        b = dict(_ebml(b, 0, len(b)))[eid]
    return b


def _mux(tmp_path, name, colour, fn):
    tu = _unit(64, 64, 10, None, True, True, colour)
    L = av1stream.lib()
    sizes, keys = (C.c_longlong * 1)(len(tu)), (C.c_uint8 * 1)(1)
    path = str(tmp_path / name)
    if fn == "colour":
        L.av1mi_host_mux_units_colour.argtypes = [C.c_char_p] + [C.c_int] * 5 + [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        assert L.av1mi_host_mux_units_colour(path.encode(), 64, 64, 10, 30, 1, tu, sizes, keys, 1, C.addressof(colour) if colour is not None else None) == 0
    else:
        L.av1mi_host_mux_units.argtypes = [C.c_char_p] + [C.c_int] * 5 + [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int]
        assert L.av1mi_host_mux_units(path.encode(), 64, 64, 10, 30, 1, tu, sizes, keys, 1) == 0
    return open(path, "rb").read()


def test_matroska_colour_element(tmp_path):
    c = av1stream.Colour(**HDR10)
    f = _mux(tmp_path, "hdr.mkv", c, "colour")
    video = _find(f, [0x18538067, 0x1654AE6B, 0xAE, 0xE0])
    col = dict(_ebml(_find(video, [0x55B0]), 0, len(_find(video, [0x55B0]))))
    u = lambda eid: int.from_bytes(col[eid], "big")
    assert (u(0x55B1), u(0x55B2), u(0x55B3), u(0x55B4), u(0x55B9), u(0x55BA), u(0x55BB), u(0x55BC), u(0x55BD)) == (9, 10, 1, 1, 1, 16, 9, 65535, 400)
    mm = dict(_ebml(col[0x55D0], 0, len(col[0x55D0])))
    got = [struct.unpack(">d", mm[0x55D1 + i])[0] for i in range(10)]
    want = [45875 / 65536, 19661 / 65536, 11141 / 65536, 52233 / 65536, 8585 / 65536, 3015 / 65536, 20493 / 65536, 21561 / 65536, 10000.0, 1 / 16384]
    assert all(abs(g - w) <= 1e-6 * w for g, w in zip(got, want))
    # without a description: the muxer's output as it was
    plain = _mux(tmp_path, "a.mkv", None, "plain")
    assert _mux(tmp_path, "b.mkv", None, "colour") == plain and _mux(tmp_path, "c.mkv", av1stream.Colour(), "colour") == plain
    video = _find(plain, [0x18538067, 0x1654AE6B, 0xAE, 0xE0])
    assert 0x55B0 not in dict(_ebml(video, 0, len(video)))


def _parse(argv, y4m_range=-1):
    L = av1stream.lib()
    L.av1mi_host_parse_colour_options.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    c, tone, err = av1stream.Colour(), (C.c_int * 2)(), C.create_string_buffer(1024)
    rc = L.av1mi_host_parse_colour_options("\n".join(["-i", "in.y4m"] + argv + ["out.obu"]).encode(), y4m_range, C.addressof(c), tone, err, 1024)
    return rc, c, list(tone), err.value.decode()


def test_job_options():
    rc, c, tone, _ = _parse(["-color_primaries", "bt2020", "-color_trc:v", "smpte2084", "-colorspace:v:0", "bt2020nc", "-color_range", "tv",
                             "-av1mi_master_display", "G(8500,39850)B(6550,2300)R(35400,14600)WP(15635,16450)L(10000000,1)", "-av1mi_max_cll", "1000,400"])
    assert rc == 0 and (c.primaries, c.transfer, c.matrix, c.full_range, c.have_mdcv, c.have_cll, c.max_cll, c.max_fall) == (9, 16, 9, 0, 1, 1, 1000, 400)
    assert (c.primary_x[0], c.primary_y[0]) == (round(35400 * 65536 / 50000), round(14600 * 65536 / 50000)) and c.luminance_max == 1000 << 8 and c.luminance_min == 2
    assert tone == [0, 0]
    for name, val, want in (("-color_primaries", "bt709", 1), ("-color_primaries", "bt470bg", 5), ("-color_primaries", "smpte170m", 6), ("-color_primaries", "12", 12)):
        assert _parse([name, val])[1].primaries == want
    assert _parse(["-color_trc", "arib-std-b67"])[1].transfer == 18 and _parse(["-colorspace", "bt2020c"])[1].matrix == 10
    for val, want in (("pc", 1), ("jpeg", 1), ("tv", 0), ("mpeg", 0)):
        assert _parse(["-color_range", val])[1].full_range == want
    # the Y4M header's range where the option is absent
    assert _parse([], 1)[1].full_range == 1 and _parse(["-color_range", "tv"], 1)[1].full_range == 0 and _parse([], -1)[1].full_range == 0
    for bad in (["-color_primaries", "nonsense"], ["-color_trc", "256"], ["-colorspace", "rgb"], ["-color_range", "2"], ["-av1mi_master_display", "G(1,2)"],
                ["-av1mi_max_cll", "70000,1"], ["-av1mi_max_cll", "1000"], ["-av1mi_tonemap", "hable"], ["-av1mi_tonemap_peak", "1000"],
                ["-av1mi_tonemap", "bt2390", "-av1mi_tonemap_peak", "50"], ["-av1mi_tonemap", "bt2390", "-color_trc", "bt709"],
                ["-av1mi_tonemap", "bt2390", "-av1mi_denoise", "4"], ["-vf", "tonemap_vaapi=format=nv12:t=bt2020"], ["-vf", "tonemap=hable"], ["-vf", "zscale=t=linear"]):
        rc, _, _, err = _parse(bad)
        assert rc == -1 and "Invalid argument" in err, (bad, err)


def test_tone_mapped_job_says_bt709():
    for argv in (["-av1mi_tonemap", "bt2390"], ["-vf:v:0", "tonemap_vaapi"], ["-vf:v:0", "tonemap_vaapi=format=p010:t=bt709:m=bt709:p=bt709,hwdownload"],
                 ["-av1mi_tonemap", "bt2390", "-color_primaries", "bt2020", "-color_trc", "smpte2084", "-colorspace", "bt2020nc", "-color_range", "tv",
                  "-av1mi_max_cll", "1000,400", "-av1mi_tonemap_peak", "4000"]):
        rc, c, tone, err = _parse(argv)
        assert rc == 0, err
        assert (c.primaries, c.transfer, c.matrix, c.full_range, c.have_mdcv, c.have_cll) == (1, 1, 1, 0, 0, 0) and tone[0] == 1


def test_y4m_colour_range(tmp_path):
    L = av1stream.lib()
    for tag, want in ((" XCOLORRANGE=FULL", 1), (" XCOLORRANGE=LIMITED", 0), ("", -1), (" XCOLORRANGE=WIDE", -2)):
        p = tmp_path / "r.y4m"
        p.write_bytes(("YUV4MPEG2 W16 H16 F30:1 C420jpeg%s\n" % tag).encode() + b"FRAME\n" + bytes(16 * 16 * 3 // 2))
        assert L.av1mi_host_y4m_colour_range(str(p).encode()) == want
