"""Depth reduction without a GPU: the arithmetic of include/av1mi.h "depth reduction" as tests/depth_ref.py restates it, the session's argument
rules through av1mi_gop_source_layout, and the job's argument handling: what -av1mi_depth / -av1mi_dither refuse (before a device is opened) and
the session config a job makes of them."""
import ctypes as C
import os

import numpy as np
import pytest

import depth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the arithmetic
def test_every_aligned_cell_of_a_constant_sums_to_it():
    """the property that makes the dither mean-preserving: the four outputs of an aligned 2x2 cell of constant v sum to exactly v, for
    every v that hits no clamp and in all three planes"""
    for p in range(3):
        for v in range(1021):
            o = R.reduce_plane(np.full((4, 6), v, np.uint16), p, R.ORDERED).astype(np.int64)
            cells = o[0::2, 0::2] + o[0::2, 1::2] + o[1::2, 0::2] + o[1::2, 1::2]
            assert (cells == v).all(), (p, v)


def test_limited_range_maps_onto_limited_range():
    for mode in (R.ROUND, R.ORDERED):
        for p in range(3):
            for v, want in ((64, 16), (940, 235), (1023, 255), (0, 0)):
                assert (R.reduce_plane(np.full((2, 4), v, np.uint16), p, mode) == want).all(), (mode, p, v)


def test_round_is_the_plain_formula():
    v = np.arange(1024, dtype=np.uint16).reshape(16, 64)
    for p in range(3):
        assert np.array_equal(R.reduce_plane(v, p, R.ROUND), np.minimum((v.astype(np.int64) + 2) >> 2, 255))


def test_a_planes_pattern_is_plane_zeros_shifted_by_p_columns():
    t0 = R.thresholds((6, 12), 0, R.ORDERED)
    assert t0[:2, :2].tolist() == [[0, 2], [3, 1]]
    for p in (1, 2):
        assert np.array_equal(R.thresholds((6, 10), p, R.ORDERED), t0[:, p:p + 10])
    # ... and it does not know the frame: a batch of stacked frames of even height repeats it
    assert np.array_equal(R.thresholds((12, 12), 1, R.ORDERED)[6:], R.thresholds((6, 12), 1, R.ORDERED))


# ---------------------------------------------------------------------------------------------- the session's rules
def _cfg(av1mi, bd=10, **kw):
    c = av1mi.GopConfig(72, 40, bd, 60, 3, 2)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _layout_tuple(L):
    return (L.width, L.height, L.true_width, L.true_height, L.bit_depth) + tuple((P.width, P.height, P.frame_bytes) for P in L.plane)


def test_config_refusals(av1mi):
    def refused(**kw):
        with pytest.raises(av1mi.Av1miError) as e:
            av1mi.gop_source_layout(_cfg(av1mi, **kw))
        assert e.value.code == -1
    refused(coded_bit_depth=9)
    refused(coded_bit_depth=12)
    refused(bd=8, coded_bit_depth=10)                      # 8 -> 10 bits is not built
    refused(bd=8, coded_bit_depth=8)                       # nothing to do
    refused(depth_dither=1)                                # the dither without the reduction
    refused(coded_bit_depth=10, depth_dither=1)
    refused(coded_bit_depth=8, depth_dither=2)
    refused(coded_bit_depth=8, depth_dither=-1)
    refused(coded_bit_depth=8, denoise=4, store_frames=4)
    av1mi.gop_source_layout(_cfg(av1mi, denoise=4, store_frames=4))      # (the pair is what is refused, not denoise)
    # the pairs the chroma stage refuses stay refused: the reduction is a field of its own, not a new pair of the old ones
    refused(bd=8, source_bit_depth=10)
    refused(bd=8, source_bit_depth=12)


def test_the_fed_layout_does_not_know_the_coded_depth(av1mi):
    """coded_bit_depth 0 yields the layout it always did, and 8 feeds the same buffers: bit_depth stays the depth of the input side"""
    plain = _layout_tuple(av1mi.gop_source_layout(_cfg(av1mi)))
    assert plain == (72, 40, 72, 40, 10, (72, 40, 72 * 40 * 2), (36, 20, 36 * 20 * 2), (36, 20, 36 * 20 * 2))
    assert _layout_tuple(av1mi.gop_source_layout(_cfg(av1mi, coded_bit_depth=0, depth_dither=0))) == plain
    assert _layout_tuple(av1mi.gop_source_layout(_cfg(av1mi, coded_bit_depth=10))) == plain
    for dither in (0, 1):
        assert _layout_tuple(av1mi.gop_source_layout(_cfg(av1mi, coded_bit_depth=8, depth_dither=dither))) == plain
    twelve = _layout_tuple(av1mi.gop_source_layout(_cfg(av1mi, source_bit_depth=12, source_chroma=av1mi.CHROMA_444)))
    assert _layout_tuple(av1mi.gop_source_layout(_cfg(av1mi, source_bit_depth=12, source_chroma=av1mi.CHROMA_444, coded_bit_depth=8))) == twelve


def test_the_c_struct_has_the_mirrors_size(av1mi, tmp_path):
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text('#include "av1mi.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu", sizeof(av1mi_gop_config), '
                   'offsetof(av1mi_gop_config, coded_bit_depth), offsetof(av1mi_gop_config, depth_dither), sizeof(av1mi_gop_frame), '
                   'offsetof(av1mi_gop_frame, bit_depth));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert sizes == [C.sizeof(av1mi.GopConfig), av1mi.GopConfig.coded_bit_depth.offset, av1mi.GopConfig.depth_dither.offset, C.sizeof(av1mi.GopFrame),
                     av1mi.GopFrame.bit_depth.offset]


# ---------------------------------------------------------------------------------------------- the job's arguments
def _y4m(path, bd, w=64, h=48, frames=2):
    n = w * h * 3 // 2 * (1 if bd == 8 else 2)
    path.write_bytes(("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s\n" % (w, h, "420jpeg" if bd == 8 else "420p%d" % bd)).encode() + (b"FRAME\n" + bytes(n)) * frames)
    return str(path)


def _plan(av1mi, argv):
    """SessionConfig for an argv (av1mi_host_session_config: the Y4M header is read, no device is opened): the session's config, or the text"""
    import av1stream
    host = av1stream.lib()
    host.av1mi_host_session_config.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(av1mi.GopConfig), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    cfg, target, switches, err = av1mi.GopConfig(), (C.c_int * 3)(), (C.c_int * 5)(), C.create_string_buffer(1024)
    code = host.av1mi_host_session_config("\n".join(["av1mi"] + [str(a) for a in argv]).encode(), None, C.byref(cfg), target, switches, err, 1024)
    return cfg if code == 0 else err.value.decode()


CHAIN = "scale_vaapi=w=ceil(iw/2)*2:h=ceil(ih/2)*2,hwdownload,format=nv12,setsar=1,format=nv12,hwupload"


def test_job_arguments_are_refused_before_anything_runs(av1mi, tmp_path):
    """through av1mi_run_transcode itself: the input does not even exist, and the refusal is the arguments'"""
    import av1stream
    run = lambda extra: av1stream.run_transcode(["-i", tmp_path / "missing.y4m"] + extra + [tmp_path / "out.obu"])
    for bad, why in ((["-av1mi_depth", "9"], "-av1mi_depth takes 8, 10, source or chain, not 9"), (["-av1mi_depth", "nv12"], "-av1mi_depth takes"),
                     (["-av1mi_dither", "ordered"], "-av1mi_dither needs -av1mi_depth"), (["-av1mi_dither", "round", "-vf:v:0", CHAIN], "-av1mi_dither needs -av1mi_depth"),
                     (["-av1mi_depth", "8", "-av1mi_dither", "bayer"], "-av1mi_dither takes ordered or round, not bayer"),
                     (["-av1mi_depth", "chain", "-vf:v:0", CHAIN.replace("format=nv12,hwupload", "format=yuv444p,hwupload")], "unsupported filter format=yuv444p")):
        code, text = run(bad)
        assert code == 1 and text.startswith("av1mi failed with exit code 1: Invalid argument") and why in text, (bad, code, text)
    for good in (["-av1mi_depth", "8"], ["-av1mi_depth", "source", "-av1mi_dither", "round"], ["-av1mi_depth", "chain", "-vf:v:0", CHAIN], ["-av1mi_depth", "10"]):
        code, text = run(good)
        assert code != 0 and "Invalid argument" not in text, (good, text)


def test_what_the_job_opens_the_session_with(av1mi, tmp_path):
    s8, s10 = _y4m(tmp_path / "a8.y4m", 8), _y4m(tmp_path / "a10.y4m", 10)
    plan = lambda src, *extra: _plan(av1mi, ["-i", src] + list(extra) + [src + ".obu"])
    depth = lambda c: (c.bit_depth, c.coded_bit_depth, c.depth_dither)
    # the default, `source`, and a chain nobody asked: the config a job has always made
    base = plan(s10, "-vf:v:0", CHAIN)
    assert depth(base) == (10, 0, 0)
    for extra in (["-av1mi_depth", "source"], ["-av1mi_depth", "10"], ["-av1mi_depth", "source", "-av1mi_dither", "round"]):
        assert bytes(plan(s10, "-vf:v:0", CHAIN, *extra)) == bytes(base), extra
    # 8, and the chain's LAST format=
    assert depth(plan(s10, "-av1mi_depth", "8")) == (10, 8, 1)
    assert depth(plan(s10, "-av1mi_depth", "8", "-av1mi_dither", "round")) == (10, 8, 0)
    assert depth(plan(s10, "-av1mi_depth", "chain", "-vf:v:0", CHAIN)) == (10, 8, 1)
    assert depth(plan(s10, "-av1mi_depth", "chain", "-vf:v:0", "format=nv12,format=p010")) == (10, 0, 0)
    assert depth(plan(s10, "-av1mi_depth", "chain", "-vf:v:0", "format=yuv420p10le,format=yuv420p")) == (10, 8, 1)
    assert depth(plan(s10, "-av1mi_depth", "chain", "-vf:v:0", "scale=64:48")) == (10, 0, 0)      # no format=: the source's
    assert depth(plan(s10, "-av1mi_depth", "chain")) == (10, 0, 0)
    # an 8-bit source: 8 is a no-op, 10 is refused — by name, or by what the chain names
    assert depth(plan(s8, "-av1mi_depth", "8")) == depth(plan(s8)) == (8, 0, 0)
    assert depth(plan(s8, "-av1mi_depth", "chain", "-vf:v:0", CHAIN)) == (8, 0, 0)
    for extra in (["-av1mi_depth", "10"], ["-av1mi_depth", "chain", "-vf:v:0", "format=p010"]):
        text = plan(s8, *extra)
        assert isinstance(text, str) and text.startswith("Invalid argument: -av1mi_depth") and "8 -> 10 bits is not built" in text, (extra, text)
    text = plan(s10, "-av1mi_depth", "8", "-av1mi_denoise", "4")
    assert isinstance(text, str) and "together with -av1mi_denoise is not built" in text
    assert depth(plan(s8, "-av1mi_depth", "8", "-av1mi_denoise", "4")) == (8, 0, 0)
