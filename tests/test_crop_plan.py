"""The crop plan (av1-go_amd/host/cropplan.hpp via av1mi_host_crop_plan), the crop-aware chain parse (ChainTarget via av1mi_host_chain_target)
and the windows av1mi_gop_source_layout describes and refuses.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import crop_ref as R

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "av1-go_amd", "host", "libav1mi_host.so")
PLAIN_CHAIN = "scale_vaapi=w=ceil(iw/2)*2:h=ceil(ih/2)*2,hwdownload,format=nv12,setsar=1,format=nv12,hwupload"
WEBRIP_CHAIN = "scale_vaapi=w='if(gt(iw,iw*sar),iw,iw*sar)':h='if(gt(iw,iw*sar),iw/sar,ih)'," + PLAIN_CHAIN


@pytest.fixture(scope="module")
def host():
    return C.CDLL(HOST)


def _rec(rows):
    a = np.zeros(len(rows), R.CROP_DTYPE)
    for i, r in enumerate(rows):
        a[i] = r
    return a


def _plan(host, rec, w, h):
    win = (C.c_int * 4)()
    host.av1mi_host_crop_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    rc = host.av1mi_host_crop_plan(rec.ctypes.data if len(rec) else None, len(rec), w, h, win)
    assert rc in (0, 1) and (rc == 1 or list(win) == [0, 0, 0, 0])
    return tuple(win) if rc else None


W, H = 1920, 1080
CASES = {
    "letterbox": (W, H, [(140, 140, 0, 0)] * 3, (0, 140, 1920, 800)),
    "letterbox_odd_margins": (W, H, [(139, 141, 0, 0), (141, 139, 0, 0)], (0, 138, 1920, 804)),
    "pillarbox": (W, H, [(0, 0, 240, 240), (0, 0, 242, 250)], (240, 0, 1440, 1080)),
    "both": (W, H, [(20, 22, 100, 90), (24, 20, 96, 94)], (96, 20, 1734, 1040)),
    "subtitle_in_the_lower_bar": (W, H, [(140, 140, 0, 0), (140, 36, 0, 0), (140, 140, 0, 0)], (0, 140, 1920, 904)),
    "all_dark_frames_mixed_in": (W, H, [(H, H, W, W), (140, 140, 0, 0), (H, H, W, W), (138, 140, 0, 0)], (0, 138, 1920, 802)),
    "a_single_usable_frame": (W, H, [(H, H, W, W), (140, 140, 0, 0), (H, H, W, W)], None),
    "no_frames": (W, H, [], None),
    "margins_of_7_lines": (W, H, [(4, 3, 0, 0), (5, 3, 0, 0)], (0, 0, 1920, 1080)),            # 4 + 2 < 8: nothing is cut
    "margins_of_8_lines": (W, H, [(4, 4, 3, 5), (4, 5, 3, 5)], (0, 4, 1920, 1072)),            # 4 + 4 = 8 is cut; L + R = 2 + 4 = 6 < 8 is not
    "odd_true_size": (1919, 1079, [(140, 139, 0, 0), (140, 139, 1, 1)], (0, 140, 1918, 800)),
    "odd_true_size_no_bars": (91, 71, [(0, 0, 0, 0)] * 2, (0, 0, 90, 70)),
    "too_small": (64, 64, [(26, 26, 0, 0)] * 2, None),
    "exactly_16": (64, 64, [(24, 24, 0, 0)] * 2, (0, 24, 64, 16)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_on_hand_built_records(host, name):
    w, h, rows, want = CASES[name]
    rec = _rec(rows)
    assert R.plan(rec, w, h) == want, "the reference disagrees with the hand-worked window"
    assert _plan(host, rec, w, h) == want


def test_plan_equals_the_reference_on_random_records(host):
    rng = np.random.default_rng(11)
    seen = {None: 0, "window": 0}
    for i in range(400):
        w, h = int(rng.integers(16, 400)), int(rng.integers(16, 400))
        n = int(rng.integers(0, 9))
        rows = []
        for _ in range(n):
            if rng.integers(0, 5) == 0:
                rows.append((h, h, w, w))
            else:
                small = rng.integers(0, 2)
                rows.append(tuple(int(rng.integers(0, (12 if small else m // 2) + 1)) for m in (h, h, w, w)))
        rec = _rec(rows)
        want = R.plan(rec, w, h)
        seen[None if want is None else "window"] += 1
        assert _plan(host, rec, w, h) == want, (w, h, rows)
    assert seen[None] > 20 and seen["window"] > 20


# ---- the chain ---------------------------------------------------------------------------------------------------------------------

def _chain(host, iw, ih, chain, sar=(1, 1)):
    w, h, win, err = C.c_int(), C.c_int(), (C.c_int * 4)(), C.create_string_buffer(512)
    rc = host.av1mi_host_chain_target(iw, ih, sar[0], sar[1], chain.encode(), C.byref(w), C.byref(h), win, err, 512)
    return ((w.value, h.value), tuple(win)) if rc == 0 else err.value.decode()


def test_chain_with_crop_accepted_forms(host):
    assert _chain(host, 1920, 1080, "crop=1920:800:0:140") == ((1920, 800), (0, 140, 1920, 800))
    assert _chain(host, 1920, 1080, "crop=1920:800") == ((1920, 800), (0, 140, 1920, 800))                     # y = (1080 - 800) / 2
    assert _chain(host, 1920, 1080, "crop=w=1440:h=1080:x=240:y=0") == ((1440, 1080), (240, 0, 1440, 1080))
    assert _chain(host, 1920, 1080, "crop=out_w=1440:out_h=1080") == ((1440, 1080), (240, 0, 1440, 1080))
    assert _chain(host, 1920, 1080, "crop=y=140:h=800:w=1920:x=0:exact=0:keep_aspect=0") == ((1920, 800), (0, 140, 1920, 800))
    assert _chain(host, 1920, 1080, "crop=1920:800:x=0:y=140") == ((1920, 800), (0, 140, 1920, 800))
    # all four values rounded down to even; the centre is taken of the rounded size: (1920 - 1436) / 2 = 242, (1080 - 802) / 2 = 139 -> 138
    assert _chain(host, 1920, 1080, "crop=1437:803:241:139") == ((1436, 802), (240, 138, 1436, 802))
    assert _chain(host, 1920, 1080, "crop=1437:803") == ((1436, 802), (242, 138, 1436, 802))
    # the window touches the far edges
    assert _chain(host, 90, 70, "crop=64:48:26:22") == ((64, 48), (26, 22, 64, 48))
    # the reference's own chains behind a crop: they see the window's size (even: nothing to round; sar 4:3 widens the WINDOW)
    assert _chain(host, 1920, 1080, "crop=1920:800:0:140," + PLAIN_CHAIN) == ((1920, 800), (0, 140, 1920, 800))
    assert _chain(host, 1440, 1080, "crop=1440:800:0:140," + WEBRIP_CHAIN, (4, 3)) == ((1920, 800), (0, 140, 1440, 800))
    assert _chain(host, 1920, 1080, "crop=1920:800:0:140,scale=1280:534") == ((1280, 534), (0, 140, 1920, 800))
    # a second crop composes with the first, in source samples
    assert _chain(host, 1920, 1080, "crop=1920:800:0:140,crop=1000:400:100:50") == ((1000, 400), (100, 190, 1000, 400))
    # a chain without a crop: no window, the size as av1mi_host_scale_target gives it
    assert _chain(host, 853, 479, PLAIN_CHAIN) == ((854, 480), (0, 0, 0, 0))


@pytest.mark.parametrize("chain,why", [
    ("crop=iw:ih-280", "no expressions"), ("crop=1920:800:0:(ih-800)/2", "no expressions"), ("crop=w=iw/2:h=800", "no expressions"),
    ("crop=1920:800:0:140:exact=1", "exact=1"), ("crop=1920:800:0:140:0:1", "exact=1"), ("crop=1920:800:keep_aspect=1", "keep_aspect"),
    ("crop=1920:800:0:140:1", "keep_aspect"), ("scale=1280:720,crop=1280:534", "after a scale filter"),
    (PLAIN_CHAIN + ",crop=1920:800", "after a scale filter"), ("crop=1920:800:0:300", "outside"), ("crop=1922:800", "outside"),
    ("crop=1920:800:2:140", "outside"), ("crop=8:8", "16x16"), ("crop=1920", "width and height"), ("crop=h=800", "width and height"),
    ("crop=1920:800:0:140:0:0:7", "too many"), ("crop=1920:800:z=3", "unknown option"), ("crop=1920:-800", "no expressions"),
])
def test_chain_with_crop_refused_forms(host, chain, why):
    got = _chain(host, 1920, 1080, chain)
    assert isinstance(got, str) and got.startswith("Invalid argument: unsupported filter argument crop=") and why in got, got


def test_scale_target_still_refuses_crop(host):
    """av1mi_host_scale_target (ScaleTarget) keeps its meaning: a chain with crop= is not its business"""
    w, h = C.c_int(), C.c_int()
    assert host.av1mi_host_scale_target(1920, 1080, 1, 1, b"crop=1920:800:0:140", C.byref(w), C.byref(h)) == -1
    assert host.av1mi_host_scale_target(1920, 1080, 1, 1, PLAIN_CHAIN.encode(), C.byref(w), C.byref(h)) == 0 and (w.value, h.value) == (1920, 1080)


def _run(host, tmp_path, extra, inp=None):
    err = C.create_string_buffer(1024)
    argv = ["-i", inp or str(tmp_path / "missing.y4m")] + extra + [str(tmp_path / "out.obu")]
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    return host.av1mi_run_transcode(len(argv), arr, err, 1024), err.value.decode()


def test_crop_options_are_parsed_without_a_gpu(host, tmp_path):
    for good in (["-av1mi_crop", "off"], ["-av1mi_crop", "auto"], ["-av1mi_crop", "1920:800:0:140"], ["-av1mi_crop", "auto", "-av1mi_crop_limit", "16"],
                 ["-vf:v:0", "crop=1920:800:0:140," + PLAIN_CHAIN], ["-av1mi_crop", "auto", "-vf:v:0", PLAIN_CHAIN]):
        code, text = _run(host, tmp_path, good)
        assert "Invalid argument" not in text and code != 0, (good, text)
    for bad, why in ((["-av1mi_crop", "on"], "-av1mi_crop takes"), (["-av1mi_crop", "1920:800"], "-av1mi_crop takes"), (["-av1mi_crop", "w=1920:h=800:x=0:y=0"], "-av1mi_crop takes"),
                     (["-av1mi_crop", "8:8:0:0"], "-av1mi_crop takes"), (["-av1mi_crop_limit", "256"], "-av1mi_crop_limit"), (["-av1mi_crop_limit", "x"], "-av1mi_crop_limit"),
                     (["-av1mi_crop", "auto", "-vf:v:0", "crop=1920:800"], "give one"), (["-av1mi_crop", "64:48:0:0", "-vf:v:0", "crop=64:48"], "give one"),
                     (["-av1mi_crop", "auto", "-av1mi_pack10", "1"], "-av1mi_pack10"), (["-vf:v:0", "crop=64:48", "-av1mi_pack10", "1"], "-av1mi_pack10"),
                     (["-vf:v:0", "crop=iw:800"], "no expressions"), (["-vf:v:0", "crop=64:48:exact=1"], "exact=1")):
        code, text = _run(host, tmp_path, bad)
        assert code == 1 and text.startswith("av1mi failed with exit code 1: Invalid argument") and why in text, (bad, code, text)


# ---- the layout ----------------------------------------------------------------------------------------------------------------------

def _cfg(av1mi, w, h, bd=8, source=None, crop=None, visible=None, **kw):
    vw, vh = visible or (0, 0)
    sw, sh = source or (0, 0)
    c = av1mi.GopConfig(w, h, bd, 100, 3, 2, 8, 1, vw, vh, source_width=sw, source_height=sh, **kw)
    if crop:
        c.crop_x, c.crop_y, c.crop_width, c.crop_height = crop
    return c


def test_source_layout_describes_a_windowed_session(av1mi):
    """fed whole frames at the source size rounded up to 8, whatever the window: the layout of the scaling session of that source"""
    for source, crop, coded, visible in (((96, 80), (18, 22, 64, 48), (64, 48), None), ((90, 70), (26, 22, 64, 48), (64, 48), None),
                                         ((96, 80), (18, 22, 52, 38), (56, 40), (52, 38)), ((160, 120), (40, 30, 64, 48), (32, 24), None)):
        for bd in (8, 10):
            L = av1mi.gop_source_layout(_cfg(av1mi, coded[0], coded[1], bd, source, crop, visible))
            S = av1mi.gop_source_layout(_cfg(av1mi, (source[0] + 7) & ~7, (source[1] + 7) & ~7, bd, source))      # that source scaled to itself
            W8, H8, b = (source[0] + 7) & ~7, (source[1] + 7) & ~7, bd // 8 if bd == 8 else 2
            assert (L.width, L.height, L.true_width, L.true_height, L.bit_depth) == (W8, H8, source[0], source[1], bd)
            assert [(P.width, P.height, P.frame_bytes) for P in L.plane] == [(W8, H8, W8 * H8 * b), (W8 // 2, H8 // 2, W8 * H8 * b // 4)] * 1 + [(W8 // 2, H8 // 2, W8 * H8 * b // 4)]
            assert [(P.width, P.height, P.frame_bytes) for P in L.plane] == [(P.width, P.height, P.frame_bytes) for P in S.plane]
    # a 4:4:4 source and a wire format: the window changes nothing about what is fed
    L = av1mi.gop_source_layout(_cfg(av1mi, 64, 48, 10, (96, 80), (18, 22, 64, 48), source_chroma=av1mi.CHROMA_444, source_bit_depth=10))
    assert [(P.width, P.height) for P in L.plane] == [(96, 80)] * 3
    L = av1mi.gop_source_layout(_cfg(av1mi, 64, 48, 8, (96, 80), (18, 22, 64, 48), input_format=av1mi.INPUT_NV12))
    assert [(P.width, P.height) for P in L.plane] == [(96, 80), (96, 40), (0, 0)]
    # no window: exactly the layout it was
    L = av1mi.gop_source_layout(_cfg(av1mi, 64, 48))
    assert (L.width, L.height, L.true_width, L.true_height) == (64, 48, 64, 48)


@pytest.mark.parametrize("source,crop,coded,visible", [
    (None, (18, 22, 64, 48), (64, 48), None),             # no source size
    ((96, 80), (17, 22, 64, 48), (64, 48), None),         # odd x
    ((96, 80), (18, 21, 64, 48), (64, 48), None),         # odd y
    ((96, 80), (18, 22, 63, 48), (64, 48), (63, 48)),     # odd width
    ((96, 80), (18, 22, 64, 47), (64, 48), (64, 47)),     # odd height
    ((96, 80), (34, 22, 64, 48), (64, 48), None),         # beyond the right edge
    ((96, 80), (18, 34, 64, 48), (64, 48), None),         # beyond the bottom edge
    ((90, 70), (28, 22, 64, 48), (64, 48), None),         # inside the buffer (96 x 72) but outside the TRUE size
    ((96, 80), (18, 22, 14, 48), (16, 48), (14, 48)),     # narrower than 16
    ((96, 80), (18, 22, 64, 14), (64, 16), (64, 14)),     # lower than 16
    ((96, 80), (-2, 22, 64, 48), (64, 48), None),         # negative
    ((96, 80), (0, 0, 64, 0), (64, 48), None),            # half a window
    ((400, 300), (0, 0, 320, 240), (64, 48), None),       # window -> target beyond 4:1
])
def test_source_layout_refuses_bad_windows(av1mi, source, crop, coded, visible):
    with pytest.raises(av1mi.Av1miError):
        av1mi.gop_source_layout(_cfg(av1mi, coded[0], coded[1], 8, source, crop, visible))


def test_crop_ref_margins_by_hand():
    """the reference itself on a frame small enough to work out by hand: limit 2, w x h = 6 x 5 inside an 8 x 8 buffer full of 255"""
    a = np.full((8, 8), 255, np.uint8)
    a[:5, :6] = [[2, 2, 2, 2, 2, 2],       # 12 = 2 * 6: dark
                 [2, 2, 3, 2, 2, 2],       # 13: not dark
                 [0, 0, 9, 0, 0, 0],
                 [2, 2, 2, 2, 2, 2],
                 [0, 0, 0, 0, 0, 0]]
    # columns: 6, 6, 16, 6, 6, 6 against 2 * 5 = 10
    assert R.margins(a, 8, 6, 5, 2) == (1, 3, 2, 3)          # rows 12, 13, 9, 12, 0 against 12: row 1 alone is not dark
    assert R.margins(a, 8, 6, 5, 255) == (5, 5, 6, 6)      # all dark
    assert R.margins(a, 8, 6, 5, 0) == (0, 1, 0, 0)
    b = a.astype(np.uint16) << 2                             # 10 bits: the same picture through m8
    b[:5, :6] |= 3
    assert R.margins(b, 10, 6, 5, 2) == (1, 3, 2, 3)


def test_auto_crop_on_a_pipe_is_refused(host, tmp_path):
    """-av1mi_crop auto samples frames from all over the file: stdin and a FIFO are refused before anything is opened"""
    fifo = tmp_path / "in.y4m"
    os.mkfifo(fifo)
    for inp in ("-", "pipe:0", str(fifo)):
        code, text = _run(host, tmp_path, ["-av1mi_crop", "auto"], inp=inp)
        assert code == 1 and "Invalid argument: -av1mi_crop auto needs a seekable file" in text, (inp, code, text)
