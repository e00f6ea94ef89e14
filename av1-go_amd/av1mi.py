"""ctypes binding of libav1mi.so — the same C ABI (include/av1mi.h) a cgo wrapper binds.

Used by tests/, bench.py and __graft_entry__.py.  It is plumbing, not a second implementation:
there is no CPU fallback here.  If the HIP library is missing or no GPU is present, loading /
opening fails loudly (reference behaviour for an unusable encoder: RunTranscode returns
(-1, err), internal/ffmpeg/transcode.go:311).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AV1MI_LIB") or os.path.join(_HERE, "libav1mi.so")   # AV1MI_LIB: diagnostic builds only

TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]


class Av1miError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("av1mi error %d: %s" % (code, text))
        self.code = code


class TxBlock(C.Structure):
    _fields_ = [("coef_off", C.c_uint32), ("x", C.c_uint16), ("y", C.c_uint16), ("tx_type", C.c_uint32),
                ("reserved", C.c_uint32)]


TXB_DTYPE = np.dtype([("coef_off", "<u4"), ("x", "<u2"), ("y", "<u2"), ("tx_type", "<u4"), ("reserved", "<u4")])

INTRA_BLK_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("mode", "u1"), ("angle_delta", "i1"), ("flags", "u1"),
                            ("n_top", "u1"), ("n_topright", "u1"), ("n_left", "u1"), ("n_bottomleft", "u1"),
                            ("reserved", "u1", (5,))])
assert INTRA_BLK_DTYPE.itemsize == 16 and TXB_DTYPE.itemsize == 16

CFL_BLK_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("max_luma_w", "<u2"), ("max_luma_h", "<u2"), ("alpha_q3", "i1"),
                          ("reserved", "u1", (7,))])
assert CFL_BLK_DTYPE.itemsize == 16

MC_BLK_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("mvx", "<i2"), ("mvy", "<i2"), ("filt_x", "u1"), ("filt_y", "u1"),
                         ("reserved", "u1", (6,))])
assert MC_BLK_DTYPE.itemsize == 16


class CdefJob(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("nframes", C.c_int), ("damping", C.c_int),
                ("stride_y", C.c_int), ("stride_uv", C.c_int),
                ("d_src_y", C.c_void_p), ("d_src_u", C.c_void_p), ("d_src_v", C.c_void_p),
                ("d_dst_y", C.c_void_p), ("d_dst_u", C.c_void_p), ("d_dst_v", C.c_void_p),
                ("d_sb_strength", C.c_void_p), ("sb_frame_stride", C.c_size_t),
                ("d_skip8", C.c_void_p), ("skip_frame_stride", C.c_size_t)]


class DeblockCdefJob(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("nframes", C.c_int), ("damping", C.c_int), ("sharpness", C.c_int),
                ("rec_stride_y", C.c_int), ("rec_stride_uv", C.c_int), ("dbl_stride_y", C.c_int), ("dbl_stride_uv", C.c_int),
                ("dst_stride_y", C.c_int), ("dst_stride_uv", C.c_int),
                ("d_rec_y", C.c_void_p), ("d_rec_u", C.c_void_p), ("d_rec_v", C.c_void_p),
                ("d_dbl_y", C.c_void_p), ("d_dbl_u", C.c_void_p), ("d_dbl_v", C.c_void_p),
                ("d_dst_y", C.c_void_p), ("d_dst_u", C.c_void_p), ("d_dst_v", C.c_void_p),
                ("d_mi_y", C.c_void_p), ("d_mi_uv", C.c_void_p), ("mi_stride_y", C.c_int), ("mi_stride_uv", C.c_int),
                ("mi_frame_stride_y", C.c_size_t), ("mi_frame_stride_uv", C.c_size_t),
                ("d_sb_strength", C.c_void_p), ("sb_frame_stride", C.c_size_t),
                ("d_skip8", C.c_void_p), ("skip_frame_stride", C.c_size_t)]


class IntraJob(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("nframes", C.c_int), ("qindex", C.c_int),
                ("block_size", C.c_int), ("stride_y", C.c_int), ("stride_uv", C.c_int),
                ("d_src_y", C.c_void_p), ("d_src_u", C.c_void_p), ("d_src_v", C.c_void_p),
                ("d_rec_y", C.c_void_p), ("d_rec_u", C.c_void_p), ("d_rec_v", C.c_void_p),
                ("d_lev_y", C.c_void_p), ("d_lev_u", C.c_void_p), ("d_lev_v", C.c_void_p),
                ("d_modes_y", C.c_void_p), ("d_modes_uv", C.c_void_p), ("open_loop", C.c_int), ("frame_rows", C.c_int),
                ("modes_frame_stride", C.c_int)]


class InterJob(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("nframes", C.c_int), ("qindex", C.c_int),
                ("search_range", C.c_int), ("stride_y", C.c_int), ("stride_uv", C.c_int),
                ("d_src_y", C.c_void_p), ("d_src_u", C.c_void_p), ("d_src_v", C.c_void_p),
                ("d_ref_y", C.c_void_p), ("d_ref_u", C.c_void_p), ("d_ref_v", C.c_void_p),
                ("d_rec_y", C.c_void_p), ("d_rec_u", C.c_void_p), ("d_rec_v", C.c_void_p),
                ("d_lev_y", C.c_void_p), ("d_lev_u", C.c_void_p), ("d_lev_v", C.c_void_p),
                ("d_mvs", C.c_void_p), ("d_skip", C.c_void_p),
                ("d_ref_alt_y", C.c_void_p), ("d_ref_alt_u", C.c_void_p), ("d_ref_alt_v", C.c_void_p), ("d_ref_sel", C.c_void_p),
                ("coarse_range", C.c_int)]


class LrDecideJob(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("nframes", C.c_int), ("unit_size", C.c_int),
                ("stride_y", C.c_int), ("stride_uv", C.c_int),
                ("d_cdef_y", C.c_void_p), ("d_cdef_u", C.c_void_p), ("d_cdef_v", C.c_void_p),
                ("d_dbl_y", C.c_void_p), ("d_dbl_u", C.c_void_p), ("d_dbl_v", C.c_void_p),
                ("d_out_y", C.c_void_p), ("d_out_u", C.c_void_p), ("d_out_v", C.c_void_p),
                ("d_orig_y", C.c_void_p), ("d_orig_u", C.c_void_p), ("d_orig_v", C.c_void_p),
                ("d_units_y", C.c_void_p), ("d_units_uv", C.c_void_p), ("unit_frame_stride_y", C.c_size_t), ("unit_frame_stride_uv", C.c_size_t),
                ("d_scratch", C.c_void_p), ("d_on", C.c_void_p), ("no_self_guided_units", C.c_int),
                ("d_units_v", C.c_void_p), ("unit_frame_stride_v", C.c_size_t)]


class LrSearchJob(C.Structure):
    """include/av1mi.h av1mi_lr_search_job"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("nframes", C.c_int), ("unit_size", C.c_int), ("qindex", C.c_int),
                ("stride_y", C.c_int), ("stride_uv", C.c_int),
                ("d_cdef_y", C.c_void_p), ("d_cdef_u", C.c_void_p), ("d_cdef_v", C.c_void_p),
                ("d_dbl_y", C.c_void_p), ("d_dbl_u", C.c_void_p), ("d_dbl_v", C.c_void_p),
                ("d_orig_y", C.c_void_p), ("d_orig_u", C.c_void_p), ("d_orig_v", C.c_void_p),
                ("d_scratch", C.c_void_p), ("d_units_y", C.c_void_p), ("d_units_u", C.c_void_p), ("d_units_v", C.c_void_p), ("d_choice", C.c_void_p)]


class CdefSearchJob(C.Structure):
    """include/av1mi.h av1mi_cdef_search_job"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("nframes", C.c_int), ("stride_y", C.c_int), ("stride_uv", C.c_int),
                ("d_src_y", C.c_void_p), ("d_src_u", C.c_void_p), ("d_src_v", C.c_void_p),
                ("d_orig_y", C.c_void_p), ("d_orig_u", C.c_void_p), ("d_orig_v", C.c_void_p),
                ("d_skip8", C.c_void_p), ("skip_frame_stride", C.c_size_t), ("true_width", C.c_int), ("true_height", C.c_int), ("bits", C.c_int),
                ("params", C.c_void_p), ("d_sse", C.c_void_p), ("d_strength", C.c_void_p), ("d_idx", C.c_void_p)]


class LfSearchJob(C.Structure):
    """include/av1mi.h av1mi_lf_search_job"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("nframes", C.c_int), ("stride_y", C.c_int), ("stride_uv", C.c_int),
                ("d_rec_y", C.c_void_p), ("d_rec_u", C.c_void_p), ("d_rec_v", C.c_void_p),
                ("d_orig_y", C.c_void_p), ("d_orig_u", C.c_void_p), ("d_orig_v", C.c_void_p),
                ("true_width", C.c_int), ("true_height", C.c_int),
                ("d_mi_y", C.c_void_p), ("d_mi_uv", C.c_void_p), ("mi_stride_y", C.c_int), ("mi_stride_uv", C.c_int),
                ("mi_frame_stride_y", C.c_size_t), ("mi_frame_stride_uv", C.c_size_t),
                ("params", C.c_void_p), ("d_scratch", C.c_void_p), ("d_sse", C.c_void_p), ("d_choice", C.c_void_p), ("d_levels", C.c_void_p),
                ("d_mi_y_out", C.c_void_p), ("d_mi_uv_out", C.c_void_p)]


class EntropyCdef(C.Structure):
    """include/av1mi.h av1mi_av1_entropy_cdef"""
    _fields_ = [("cdef_bits", C.c_int), ("d_idx", C.c_void_p), ("frame_stride", C.c_size_t)]


class GopConfig(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("base_q_idx", C.c_int), ("gop_length", C.c_int),
                ("segments", C.c_int), ("search_range", C.c_int), ("gpu_entropy", C.c_int), ("visible_width", C.c_int),
                ("visible_height", C.c_int), ("coder_streams", C.c_int), ("key_block_size", C.c_int), ("input_format", C.c_int), ("source_width", C.c_int),
                ("source_height", C.c_int), ("quality_stats", C.c_int), ("coarse_range", C.c_int), ("source_chroma", C.c_int),
                ("source_bit_depth", C.c_int), ("store_frames", C.c_int), ("deinterlace", C.c_int), ("denoise", C.c_int),
                ("crop_x", C.c_int), ("crop_y", C.c_int), ("crop_width", C.c_int), ("crop_height", C.c_int), ("denoise_range", C.c_int),
                ("tone_map", C.c_int), ("tone_map_peak", C.c_int), ("grain_cov", C.c_int), ("lr_search", C.c_int),
                ("cdef_search", C.c_int), ("lf_search", C.c_int), ("coded_bit_depth", C.c_int), ("depth_dither", C.c_int),
                ("deinterlace_fields", C.c_int), ("telecine", C.c_int)]


class FrameParams(C.Structure):
    _fields_ = [("frame_type", C.c_int), ("base_q_idx", C.c_int), ("lf_level", C.c_int * 4), ("lf_sharpness", C.c_int),
                ("cdef_damping", C.c_int), ("cdef_y", C.c_uint8), ("cdef_uv", C.c_uint8), ("lr_unit_size", C.c_int),
                ("lr_unit_y", C.c_int8 * 8), ("lr_unit_uv", C.c_int8 * 8)]


class GopFrame(C.Structure):
    _fields_ = [("params", FrameParams), ("segments", C.c_int), ("blocks_per_frame", C.c_size_t), ("y_mode", C.c_void_p),
                ("uv_mode", C.c_void_p), ("mv", C.c_void_p), ("skip", C.c_void_p), ("lev_y", C.c_void_p), ("lev_u", C.c_void_p),
                ("lev_v", C.c_void_p), ("tiles_per_frame", C.c_int), ("tile_size", C.c_void_p), ("tile_payload", C.c_void_p),
                ("payload_bytes", C.c_uint64), ("lr_on", C.c_void_p), ("key_block_size", C.c_int), ("key_modes_stride", C.c_int),
                ("key_modes_band", C.c_int), ("quality", C.c_void_p), ("grain", C.c_void_p), ("grain_cov", C.c_void_p),
                ("lr_units", C.c_void_p * 3), ("lr_units_per_frame", C.c_int * 3), ("lr_choice", C.c_void_p),
                ("cdef_bits", C.c_int), ("cdef_y", C.c_uint8 * 8), ("cdef_uv", C.c_uint8 * 8), ("cdef_idx", C.c_void_p),
                ("lf_levels", C.c_void_p), ("lf_choice", C.c_void_p), ("bit_depth", C.c_int)]


def policy_frame_params(base_q_idx, bit_depth, frame_type):
    """the session's filter-parameter policy for one frame (include/av1mi.h av1mi_policy_frame_params); no GPU needed"""
    p = FrameParams()
    rc = load().av1mi_policy_frame_params(int(base_q_idx), int(bit_depth), int(frame_type), C.byref(p))
    if rc:
        raise Av1miError(rc, "av1mi_policy_frame_params")
    return p


# av1mi_quality (include/av1mi.h): one record per (frame, plane)
# av1mi_scene_record (include/av1mi.h "scene analysis"): one record per frame
GRAIN_BINS = 16      # AV1MI_GRAIN_BINS; a record (av1mi_grain_record) is that many bins
GRAIN_DTYPE = np.dtype([("sum_sq", "<u8"), ("count", "<u4"), ("reserved", "<u4")])      # av1mi_grain_bin
GRAIN_COV_DTYPE = np.dtype([("sum", "<i8", (4, 13))])      # av1mi_grain_cov_record ("grain covariance"): sum[dy][dx + 6]
DENOISE_VEC_DTYPE = np.dtype([("dx_p", "i1"), ("dy_p", "i1"), ("dx_n", "i1"), ("dy_n", "i1")])      # av1mi_denoise_vec: a block's vectors towards P and N
SCENE_DTYPE = np.dtype([("inter_sad", "<u8"), ("intra_sad", "<u8"), ("blocks", "<u4"), ("reserved", "<u4")])
CROP_DTYPE = np.dtype([("top", "<u4"), ("bottom", "<u4"), ("left", "<u4"), ("right", "<u4")])      # av1mi_crop_record ("bar detection")
# av1mi_noise_record ("noise records"): the histogram of the eligible blocks' mean |difference| in 1/16 code, their number, all whole blocks
NOISE_DTYPE = np.dtype([("hist", "<u4", 256), ("eligible", "<u4"), ("blocks", "<u4")])
# av1mi_peak_record ("peak records"): the histogram of a frame's max(R', G', B') as 10-bit PQ codes, and its pixels (the sum of hist)
PEAK_DTYPE = np.dtype([("hist", "<u4", 1024), ("pixels", "<u4")])
# av1mi_telecine_record ("inverse telecine"): comb of the candidates p, c, n; bdiff
TELECINE_DTYPE = np.dtype([("comb", "<u8", 3), ("bdiff", "<u8")])
assert SCENE_DTYPE.itemsize == 24
QUALITY_DTYPE = np.dtype([("sse", "<u8"), ("ssim_sum", "<f8"), ("samples", "<u4"), ("windows", "<u4")])
assert QUALITY_DTYPE.itemsize == 24


def quality_psnr(rec, bit_depth):
    """10 log10(L^2 samples / sse) of one record, or of several taken together (summed sse over summed samples); inf when sse is 0"""
    sse, n = float(np.sum(rec["sse"], dtype=np.uint64)), float(np.sum(rec["samples"], dtype=np.uint64))
    L = float((1 << bit_depth) - 1)
    return float("inf") if sse == 0 else 10.0 * np.log10(L * L * n / sse)


def quality_ssim(rec):
    """ssim_sum / windows of one record"""
    return float(rec["ssim_sum"]) / float(rec["windows"])


INPUT_PLANAR, INPUT_PACKED10, INPUT_P010, INPUT_NV12 = 0, 1, 2, 3      # enum av1mi_input_format


def input_plane_bytes(fmt, bit_depth, plane, width, rows):
    """bytes of one plane of a stack of `rows` luma rows in an input format (av1mi_input_plane_bytes); 0 = invalid; no GPU needed"""
    lib = load()
    lib.av1mi_input_plane_bytes.restype = C.c_size_t
    lib.av1mi_input_plane_bytes.argtypes = [C.c_int] * 5
    return int(lib.av1mi_input_plane_bytes(int(fmt), int(bit_depth), int(plane), int(width), int(rows)))


CHROMA_420, CHROMA_422, CHROMA_444, CHROMA_400 = 0, 1, 2, 3      # enum av1mi_source_chroma
DEPTH_ROUND, DEPTH_ORDERED = 0, 1      # enum av1mi_depth_mode


def source_plane_bytes(chroma, source_bit_depth, plane, width, rows):
    """bytes of one plane of a source stacked to `rows` luma rows in a chroma layout (av1mi_source_plane_bytes); 0 = invalid, or the
    chroma planes of a grey source; no GPU needed"""
    lib = load()
    lib.av1mi_source_plane_bytes.restype = C.c_size_t
    lib.av1mi_source_plane_bytes.argtypes = [C.c_int] * 5
    return int(lib.av1mi_source_plane_bytes(int(chroma), int(source_bit_depth), int(plane), int(width), int(rows)))


def source_plane_shapes(chroma, width, rows):
    """[rows, width] of the three planes of a source in a chroma layout, buffers of width x rows luma samples; None = no such plane"""
    c = {CHROMA_420: (rows // 2, width // 2), CHROMA_422: (rows, width // 2), CHROMA_444: (rows, width), CHROMA_400: None}[chroma]
    return [(rows, width), c, c]


class SourcePlane(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("frame_bytes", C.c_size_t)]


class SourceLayout(C.Structure):      # av1mi_source_layout
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("true_width", C.c_int), ("true_height", C.c_int), ("bit_depth", C.c_int), ("plane", SourcePlane * 3)]


def gop_source_layout(cfg):
    """what a session opened with `cfg` (GopConfig) is fed (av1mi_gop_source_layout); raises where av1mi_gop_open would refuse cfg; no GPU needed"""
    lib, out = load(), SourceLayout()
    lib.av1mi_gop_source_layout.argtypes = [C.POINTER(GopConfig), C.POINTER(SourceLayout)]
    rc = lib.av1mi_gop_source_layout(C.byref(cfg), C.byref(out))
    if rc:
        raise Av1miError(rc, "av1mi_gop_source_layout")
    return out


def input_pack(fmt, bit_depth, y, u, v, out=None):
    """planar planes (y [rows, width], u / v half size; uint8 or uint16) -> the format's planes as uint8 arrays (av1mi_input_pack, host
    code); out: optional (buffer, byte offset) per plane to pack into instead of fresh arrays"""
    lib = load()
    lib.av1mi_input_pack.argtypes = [C.c_int] * 4 + [C.c_void_p] * 6
    dt = np.uint8 if bit_depth == 8 else np.uint16
    y, u, v = (np.ascontiguousarray(a, dt) for a in (y, u, v))
    rows, width = y.shape
    n = [input_plane_bytes(fmt, bit_depth, p, width, rows) for p in range(3)]
    if out is None:
        out = [(np.zeros(max(k, 1), np.uint8), 0) for k in n]
    ptr = [(b.ctypes.data + off) if k else None for (b, off), k in zip(out, n)]
    rc = lib.av1mi_input_pack(int(fmt), int(bit_depth), width, rows, y.ctypes.data, u.ctypes.data, v.ctypes.data, *ptr)
    if rc:
        raise Av1miError(rc, "av1mi_input_pack(format %d, bit depth %d, %dx%d)" % (fmt, bit_depth, width, rows))
    return [b[off:off + k] for (b, off), k in zip(out, n)]


def scale_filter(src_n, dst_n):
    """the resampler's table for src_n -> dst_n samples (av1mi_scale_filter, host code): (taps, first [dst_n] int32, coef [dst_n, taps]
    int16); no GPU needed"""
    lib = load()
    lib.av1mi_scale_filter.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
    t = C.c_int()
    rc = lib.av1mi_scale_filter(int(src_n), int(dst_n), C.byref(t), None, None)
    if rc:
        raise Av1miError(rc, "av1mi_scale_filter(%d -> %d)" % (src_n, dst_n))
    first, coef = np.empty(dst_n, np.int32), np.empty((dst_n, t.value), np.int16)
    rc = lib.av1mi_scale_filter(int(src_n), int(dst_n), C.byref(t), first.ctypes.data, coef.ctypes.data)
    if rc:
        raise Av1miError(rc, "av1mi_scale_filter(%d -> %d)" % (src_n, dst_n))
    return t.value, first, coef


def _view(ptr, shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_uint8 * n).from_address(ptr), dtype=dtype).reshape(shape)


class GopSession:
    """av1mi_gop_* (include/av1mi.h): closed GOPs in lockstep, policy and PCIe plumbing inside the library."""

    def __init__(self, ctx, width, height, bit_depth, base_q_idx, gop_length, segments=1, search_range=8, gpu_entropy=0, visible=None, coder_streams=0,
                 key_block_size=0, input_format=0, source=None, quality_stats=0, coarse_range=0, source_chroma=0, source_bit_depth=0, store_frames=0, deinterlace=0, denoise=None, crop=None, denoise_range=None, tone_map=0, tone_map_peak=0, grain_cov=None, lr_search=None, cdef_search=None, lf_search=None, coded_bit_depth=None,
                 depth_dither=None, deinterlace_fields=None, telecine=None):
        """visible: the true (width, height) when width x height is it rounded up to 8 (the caller replicates the source edge);
        key_block_size 32: key frames in 32x32 blocks (av1mi_gop_config.key_block_size); input_format: INPUT_* (the layout of the
        source handed to input_planes() / submit_device()); source: the true (width, height) of the frames the session is fed when
        they are to be scaled to the coded frame (av1mi_gop_config.source_width): the input buffers then have that size rounded up to 8;
        quality_stats: 1 = every batch is measured on the GPU, collect()["quality"] holds the records (av1mi_gop_config.quality_stats);
        coarse_range: 0, or a multiple of 4 up to 64: P frames search around a coarse centre per 64x64 tile (av1mi_gop_config.coarse_range);
        source_chroma / source_bit_depth: CHROMA_* and 8 / 10 / 12 of the source the session is fed (av1mi_gop_config.source_chroma): the
        input buffers then have that layout (source_plane_shapes), and no chroma planes for a grey source;
        store_frames: the session owns two frame stores of that many fed frames (av1mi_gop_config.store_frames): store_put(),
        store_analyse() and submit_stored() feed it, submit() is refused;
        deinterlace: 0 none, 1 top field first, 2 bottom field first (av1mi_gop_config.deinterlace; needs store_frames): submit_stored()
        gathers through the deinterlacer;
        denoise: 1 .. 16, the strength of the temporal denoiser (av1mi_gop_config.denoise; needs store_frames, not with deinterlace):
        submit_stored() gathers through it and collect()["grain"] holds the grain records.  None leaves the field unset (0 = none);
        crop: (x, y, width, height), the window of the fed frames that is coded (av1mi_gop_config.crop_*; needs source, the fed frames'
        true size): width x height (or visible) is the target the window is copied or scaled to;
        denoise_range: 4 or 8, the range of the denoiser's block search (av1mi_gop_config.denoise_range; needs denoise): submit_stored()
        gathers through the motion-compensated filter.  None leaves the field unset (0 = none);
        grain_cov: 1 = the covariance of what the denoiser removed is measured behind the gather (av1mi_gop_config.grain_cov; needs
        denoise): collect()["grain_cov"] holds the records.  None leaves the field unset (0 = none);
        coded_bit_depth: 8 in a bit_depth 10 session = the depth reduction at the end of the input chain: everything behind it is an 8-bit
        session (av1mi_gop_config.coded_bit_depth); depth_dither: DEPTH_ROUND or DEPTH_ORDERED.  None leaves a field unset (0);
        deinterlace_fields: 1 = one output frame per field (av1mi_gop_config.deinterlace_fields; needs deinterlace): submit_stored() then
        takes OUTPUT positions, source position * 2 + phase.  None leaves the field unset (0);
        telecine: 1 = inverse telecine (av1mi_gop_config.telecine; needs store_frames): the stores hold store_frames + 2 frames,
        store_telecine() gives the field-match records and submit_woven() weaves a batch from two positions per segment.  None leaves
        the field unset (0)"""
        self.ctx, self.w, self.h, self.bd, self.segments = ctx, width, height, bit_depth, segments
        vw, vh = visible if visible is not None else (0, 0)
        sw, sh = source if source is not None else (0, 0)
        self.cfg = GopConfig(width, height, bit_depth, base_q_idx, gop_length, segments, search_range, gpu_entropy, vw, vh, coder_streams, key_block_size, input_format,
                             sw, sh, int(quality_stats), int(coarse_range), int(source_chroma), int(source_bit_depth), int(store_frames), int(deinterlace))
        if denoise is not None:
            self.cfg.denoise = int(denoise)
        if denoise_range is not None:
            self.cfg.denoise_range = int(denoise_range)
        if grain_cov is not None:
            self.cfg.grain_cov = int(grain_cov)
        if lr_search is not None:       # 1 = a Wiener record or none chosen per restoration unit (av1mi_gop_config.lr_search)
            self.cfg.lr_search = int(lr_search)
        if cdef_search is not None:     # 1 .. 3 = cdef_bits: a CDEF strength set chosen per superblock (av1mi_gop_config.cdef_search)
            self.cfg.cdef_search = int(cdef_search)
        if lf_search is not None:       # 1 = the deblocking levels chosen per frame against the source (av1mi_gop_config.lf_search)
            self.cfg.lf_search = int(lf_search)
        # tone_map: 1 = every batch is tone-mapped (PQ / BT.2020 -> SDR / BT.709) in place behind the input stages; tone_map_peak: cd/m2, 0 = 1000
        self.cfg.tone_map, self.cfg.tone_map_peak = int(tone_map), int(tone_map_peak)
        if coded_bit_depth is not None:
            self.cfg.coded_bit_depth = int(coded_bit_depth)
        if depth_dither is not None:
            self.cfg.depth_dither = int(depth_dither)
        if deinterlace_fields is not None:
            self.cfg.deinterlace_fields = int(deinterlace_fields)
        if telecine is not None:
            self.cfg.telecine = int(telecine)
        if crop is not None:
            self.cfg.crop_x, self.cfg.crop_y, self.cfg.crop_width, self.cfg.crop_height = (int(v) for v in crop)
        self.g = C.c_void_p()
        ctx.lib.av1mi_gop_open.argtypes = [C.c_void_p, C.POINTER(GopConfig), C.POINTER(C.c_void_p)]
        ctx._chk(ctx.lib.av1mi_gop_open(ctx.h, C.byref(self.cfg), C.byref(self.g)))
        self.layout = gop_source_layout(self.cfg)      # the geometry of the input buffers
        for name in ("av1mi_gop_close", "av1mi_gop_acquire_input", "av1mi_gop_submit", "av1mi_gop_collect", "av1mi_gop_pending",
                     "av1mi_gop_download_reference"):
            getattr(ctx.lib, name).argtypes = None
        ctx.lib.av1mi_gop_close.restype = None
        self.coded_bd = self.cfg.coded_bit_depth or bit_depth      # the depth of the reference planes and of the stream
        self.dt = np.uint8 if self.coded_bd == 8 else np.uint16

    def fed_planes(self):
        """(shape, dtype) of the planes of a batch as the session is fed them, from the layout: the planes it has, segments stacked; a
        wire format's planes (input_format not planar) as flat bytes"""
        S, wire = self.segments, self.cfg.input_format != INPUT_PLANAR
        dt = np.uint8 if wire or self.layout.bit_depth == 8 else np.uint16
        return [((S * P.frame_bytes,) if wire else (S * P.height, P.width), dt) for P in self.layout.plane if P.frame_bytes]

    def input_planes(self):
        """numpy views of the pinned host planes of the next batch (fed_planes(): e.g. [segments * height, width] and the half-size chroma)"""
        ptr = (C.c_void_p(), C.c_void_p(), C.c_void_p())
        self.ctx._chk(self.ctx.lib.av1mi_gop_acquire_input(self.g, *[C.byref(p) for p in ptr]))
        return tuple(_view(p.value, shape, dt) for p, (shape, dt) in zip(ptr, self.fed_planes()))

    def submit(self, frame_type=-1):
        self.ctx._chk(self.ctx.lib.av1mi_gop_submit(self.g, int(frame_type)))

    def submit_device(self, d_y, d_u, d_v=None, frame_type=-1):
        """a batch whose source planes (DevBuf, in the session's input format; d_v None for P010 / NV12, d_u and d_v None for a grey source) are already in device
        memory: no upload (av1mi_gop_submit_device)"""
        self.ctx.lib.av1mi_gop_submit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        self.ctx._chk(self.ctx.lib.av1mi_gop_submit_device(self.g, d_y.ptr, d_u.ptr if d_u is not None else None, d_v.ptr if d_v is not None else None, int(frame_type)))

    def store_put(self, store, first, count):
        """the `count` frames written into input_planes() (frame i where segment i would lie) -> positions first .. of store 0 / 1
        (av1mi_gop_store_put); nothing is coded"""
        self.ctx.lib.av1mi_gop_store_put.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        self.ctx._chk(self.ctx.lib.av1mi_gop_store_put(self.g, int(store), int(first), int(count)))

    def store_analyse(self, store, frames):
        """the scene records (SCENE_DTYPE [frames]) of frames 0 .. frames - 1 of a store (av1mi_gop_store_analyse)"""
        out = np.zeros(frames, SCENE_DTYPE)
        self.ctx.lib.av1mi_gop_store_analyse.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        self.ctx._chk(self.ctx.lib.av1mi_gop_store_analyse(self.g, int(store), int(frames), out.ctypes.data))
        return out

    def submit_stored(self, store, index, frame_type):
        """a batch gathered from a store: index[s] = the store position of segment s's frame, -1 = a flat slot (av1mi_gop_submit_stored)"""
        idx = np.ascontiguousarray(index, np.int32)
        assert idx.size == self.segments
        self.ctx.lib.av1mi_gop_submit_stored.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        self.ctx._chk(self.ctx.lib.av1mi_gop_submit_stored(self.g, int(store), idx.ctypes.data, int(frame_type)))

    def store_telecine(self, store, frames):
        """the field-match records (TELECINE_DTYPE [frames]) of the run of frames 0 .. frames - 1 of a store (av1mi_gop_store_telecine)"""
        out = np.zeros(frames, TELECINE_DTYPE)
        self.ctx.lib.av1mi_gop_store_telecine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        self.ctx._chk(self.ctx.lib.av1mi_gop_store_telecine(self.g, int(store), int(frames), out.ctypes.data))
        return out

    def submit_woven(self, store, top, bottom, frame_type):
        """a batch woven from a store: segment s's frame takes its even lines from position top[s] and its odd lines from bottom[s];
        top[s] = -1 = a flat slot (av1mi_gop_submit_woven)"""
        t, b = np.ascontiguousarray(top, np.int32), np.ascontiguousarray(bottom, np.int32)
        assert t.size == self.segments and b.size == self.segments
        self.ctx.lib.av1mi_gop_submit_woven.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        self.ctx._chk(self.ctx.lib.av1mi_gop_submit_woven(self.g, int(store), t.ctypes.data, b.ctypes.data, int(frame_type)))

    def set_q(self, base_q_idx):
        """the quantiser (1..255) of every batch submitted from now on; batches in flight keep theirs (av1mi_gop_set_base_q_idx)"""
        self.ctx.lib.av1mi_gop_set_base_q_idx.argtypes = [C.c_void_p, C.c_int]
        self.ctx._chk(self.ctx.lib.av1mi_gop_set_base_q_idx(self.g, int(base_q_idx)))

    def pending(self):
        return self.ctx.lib.av1mi_gop_pending(self.g)

    def max_in_flight(self):
        return self.ctx.lib.av1mi_gop_max_in_flight()

    def entropy_fallbacks(self):
        self.ctx.lib.av1mi_gop_entropy_fallbacks.restype = C.c_long
        return self.ctx.lib.av1mi_gop_entropy_fallbacks(self.g)

    def collect_raw(self):
        f = GopFrame()
        self.ctx._chk(self.ctx.lib.av1mi_gop_collect(self.g, C.byref(f)))
        return f

    def collect(self):
        """dict of numpy views (valid until the next submit) + params"""
        f = self.collect_raw()
        S, nb = f.segments, f.blocks_per_frame
        out = dict(params=f.params, frame_type=f.params.frame_type, lr_on=_view(f.lr_on, (S, 3), np.uint8), raw=f)      # restoration on / off per segment and plane
        if f.quality:      # quality_stats: records [segment, plane] (QUALITY_DTYPE)
            out["quality"] = _view(f.quality, (S, 3), QUALITY_DTYPE)
        if f.grain:        # denoise: records [segment, plane, bin] (GRAIN_DTYPE)
            out["grain"] = _view(f.grain, (S, 3, GRAIN_BINS), GRAIN_DTYPE)
        if f.lr_choice:    # lr_search: the chosen candidates [segment, unit of Y, U, V end to end] and the planes' records [segment, unit, 8]
            per = list(f.lr_units_per_frame)
            out["lr_choice"] = _view(f.lr_choice, (S, sum(per)), np.uint8)
            out["lr_units"] = [_view(f.lr_units[p], (S, per[p], 8), np.int8) for p in range(3)]
        if f.cdef_bits:    # cdef_search: the frame header's sets and the chosen index per [segment, superblock]
            out["cdef_bits"], out["cdef_y"], out["cdef_uv"] = int(f.cdef_bits), list(f.cdef_y), list(f.cdef_uv)
            out["cdef_idx"] = _view(f.cdef_idx, (S, ((self.w + 63) // 64) * ((self.h + 63) // 64)), np.uint8)
        if f.lf_levels:    # lf_search: the header levels [segment, 4] and the chosen candidates [segment, 2] (luma, chroma)
            out["lf_levels"], out["lf_choice"] = _view(f.lf_levels, (S, 4), np.uint8), _view(f.lf_choice, (S, 2), np.uint8)
        if f.grain_cov:    # grain_cov: records [segment, plane] (GRAIN_COV_DTYPE)
            out["grain_cov"] = _view(f.grain_cov, (S, 3), GRAIN_COV_DTYPE)
        if f.key_block_size == 32:
            out["key_block_size"] = 32
        if f.key_block_size == 32 and f.lev_y:
            # a key frame in 32x32 blocks: per segment the blocks of the complete superblock rows ("32": modes, levels [n, 32, 32] and the
            # 16x16 chroma), then the 8x8 blocks of a last partial row ("8")
            w, h = self.w, self.h
            hA = h // 64 * 64
            nA, nB = (hA // 32) * (w // 32), ((h - hA) // 8) * (w // 8)
            for name, ptr in (("y_mode", f.y_mode), ("uv_mode", f.uv_mode)):
                m = _view(ptr, (S, f.key_modes_stride), np.uint8)
                out[name + "32"], out[name + "8"] = m[:, :nA], m[:, f.key_modes_band:f.key_modes_band + nB]
            for name, ptr, d in (("lev_y", f.lev_y, 1), ("lev_u", f.lev_u, 2), ("lev_v", f.lev_v, 2)):
                pl = _view(ptr, (S, (h // d) * (w // d)), np.int16)
                cut = (hA // d) * (w // d)
                out[name + "32"] = pl[:, :cut].reshape(S, nA, 32 // d, 32 // d)
                out[name + "8"] = pl[:, cut:].reshape(S, nB, 8 // d, 8 // d)
            return out
        if f.lev_y:
            out.update(lev_y=_view(f.lev_y, (S, nb, 8, 8), np.int16), lev_u=_view(f.lev_u, (S, nb, 4, 4), np.int16),
                       lev_v=_view(f.lev_v, (S, nb, 4, 4), np.int16))
        if f.tile_size:
            out.update(tiles_per_frame=f.tiles_per_frame, tile_size=_view(f.tile_size, (S * f.tiles_per_frame,), np.uint32),
                       tile_payload=_view(f.tile_payload, (max(int(f.payload_bytes), 1),), np.uint8)[:int(f.payload_bytes)])
        # (absent when the tiles were coded on the GPU, gpu_entropy = 1: the host then gets the payloads only)
        if f.y_mode:
            out["y_mode"], out["uv_mode"] = _view(f.y_mode, (S, nb), np.uint8), _view(f.uv_mode, (S, nb), np.uint8)
        if f.mv:
            out["mv"], out["skip"] = _view(f.mv, (S, nb, 2), np.int16), _view(f.skip, (S, nb), np.uint8)
        return out

    def download_reference(self):
        S, w, h = self.segments, self.w, self.h
        y, u, v = np.empty((S * h, w), self.dt), np.empty((S * h // 2, w // 2), self.dt), np.empty((S * h // 2, w // 2), self.dt)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self.ctx._chk(self.ctx.lib.av1mi_gop_download_reference(self.g, vp(y), vp(u), vp(v)))
        return y, u, v

    def download_fed(self):
        """the fed buffers of the last submitted batch (av1mi_gop_download_fed): arrays shaped like input_planes()"""
        out = [np.empty(shape, dt) for shape, dt in self.fed_planes()]
        self.ctx.lib.av1mi_gop_download_fed.argtypes = [C.c_void_p] * 4
        self.ctx._chk(self.ctx.lib.av1mi_gop_download_fed(self.g, *([a.ctypes.data for a in out] + [None] * (3 - len(out)))))
        return tuple(out)

    def close(self):
        if self.g:
            self.ctx.lib.av1mi_gop_close(self.g)
            self.g = None


# enum av1mi_kernel_kind.  N_PIPELINE_KINDS counts the kinds of the coding pipeline, AV1MI_K_FWD_TXFM .. AV1MI_K_INPUT; it is NOT
# AV1MI_K_KINDS (19 since AV1MI_K_QUALITY, the measuring stage, follows them).  N_KERNEL_KINDS is its older name: callers take
# N_KERNEL_KINDS - 1 for AV1MI_K_INPUT, so it stays 18.  Whoever wants every kind asks the library (Context.kernel_kinds()).
N_PIPELINE_KINDS = 18
N_KERNEL_KINDS = N_PIPELINE_KINDS
K_QUALITY = 18        # AV1MI_K_QUALITY
K_SCENE = 20          # AV1MI_K_SCENE: the scene analysis and the frame gather
_lib = None


def load():
    """dlopen libav1mi.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.av1mi_version.restype = C.c_char_p
        lib.av1mi_last_error.restype = C.c_char_p
        lib.av1mi_device_name.restype = C.c_char_p
        lib.av1mi_last_error.argtypes = [C.c_void_p]
        lib.av1mi_device_name.argtypes = [C.c_void_p]
        lib.av1mi_close.argtypes = [C.c_void_p]
        lib.av1mi_close.restype = None
        _lib = lib
    return _lib


class ToneTables(C.Structure):      # av1mi_tone_tables ("tone mapping")
    _fields_ = [("lin", C.c_uint32 * 1024), ("gain", C.c_uint32 * 1024), ("oetf_lo", C.c_uint32 * 512), ("oetf_hi", C.c_uint32 * 388),
                ("to_rgb", C.c_int32 * 5), ("gamut", (C.c_int32 * 3) * 3), ("to_yuv", (C.c_int32 * 3) * 3), ("peak", C.c_int32)]


def tone_map_tables(peak, lib=None):
    """av1mi_tone_map_tables(peak): the ToneTables a tone mapping reads; host code, no device"""
    lib = lib or load()
    t = ToneTables()
    lib.av1mi_tone_map_tables.argtypes = [C.c_int, C.c_void_p]
    if lib.av1mi_tone_map_tables(int(peak), C.byref(t)) != 0:
        raise ValueError("av1mi_tone_map_tables: peak %r out of range (100 .. 10000)" % (peak,))
    return t


def cdef_search_sets(params, bits):
    """the candidate strength sets of a frame (av1mi_cdef_search_sets): two lists of 8 bytes, (primary << 2) | secondary, luma and chroma"""
    y, uv = (C.c_uint8 * 8)(), (C.c_uint8 * 8)()
    if load().av1mi_cdef_search_sets(C.byref(params), int(bits), y, uv):
        raise ValueError("CDEF search: bits %d outside 1 .. 3" % bits)
    return list(y), list(uv)


def cdef_search_table_bytes(width, height, nframes):
    lib = load()
    lib.av1mi_cdef_search_table_bytes.restype = C.c_size_t
    return int(lib.av1mi_cdef_search_table_bytes(int(width), int(height), int(nframes)))


LF_SEARCH_CANDIDATES = 8      # AV1MI_LF_SEARCH_CANDIDATES


def lf_search_levels(params, c):
    """the four header levels of candidate c of a frame (av1mi_lf_search_levels): luma vertical, luma horizontal, U, V"""
    out = (C.c_int * 4)()
    if load().av1mi_lf_search_levels(C.byref(params), int(c), out):
        raise ValueError("deblocking search: candidate %d outside 0 .. 7, or policy levels the search refuses" % c)
    return list(out)


def lf_search_scratch_bytes(width, height, nframes):
    lib = load()
    lib.av1mi_lf_search_scratch_bytes.restype = C.c_size_t
    return int(lib.av1mi_lf_search_scratch_bytes(int(width), int(height), int(nframes)))


LR_SEARCH_CANDIDATES = 9      # AV1MI_LR_SEARCH_CANDIDATES


def lr_search_units(width, height, unit_size=64):
    """units of a frame's three planes together (av1mi_lr_search_units)"""
    return int(load().av1mi_lr_search_units(int(width), int(height), int(unit_size)))


def lr_search_scratch_bytes(width, height, nframes, unit_size=64):
    lib = load()
    lib.av1mi_lr_search_scratch_bytes.restype = C.c_size_t
    return int(lib.av1mi_lr_search_scratch_bytes(int(width), int(height), int(unit_size), int(nframes)))


def lr_search_candidate(chroma, c):
    """candidate c's 8-byte unit record for a luma (chroma = 0) or chroma plane, as a list"""
    rec = (C.c_int8 * 8)()
    if load().av1mi_lr_search_candidate(int(chroma), int(c), rec):
        raise ValueError("restoration search candidate %d out of range" % c)
    return list(rec)


def lr_search_bits(chroma, c):
    return int(load().av1mi_lr_search_bits(int(chroma), int(c)))


def lr_search_lambda(qindex, bd):
    lib = load()
    lib.av1mi_lr_search_lambda.restype = C.c_longlong
    return int(lib.av1mi_lr_search_lambda(int(qindex), int(bd)))


def exported_symbols():
    """names declared in include/av1mi.h (parsed from the header)."""
    import re
    hdr = open(os.path.join(_HERE, "..", "include", "av1mi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(av1mi_[a-z0-9_]+)\s*\(", hdr)))


class DevBuf:
    """device allocation owned by a Context."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        ctx._chk(ctx.lib.av1mi_malloc(ctx.h, C.byref(p), C.c_size_t(self.nbytes)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._chk(self.ctx.lib.av1mi_upload(self.ctx.h, C.c_void_p(self.ptr), arr.ctypes.data_as(C.c_void_p),
                                                C.c_size_t(arr.nbytes)))
        return self

    def download(self, shape, dtype):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._chk(self.ctx.lib.av1mi_download(self.ctx.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr),
                                                  C.c_size_t(out.nbytes)))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.av1mi_free(self.ctx.h, C.c_void_p(self.ptr))
            self.ptr = None


class Context:
    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.av1mi_open(int(device), C.byref(h))
        if rc != 0:
            raise Av1miError(rc, "av1mi_open(device=%d) failed: no usable HIP device" % device)
        self.h = h

    def close(self):
        if self.h:
            self.lib.av1mi_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise Av1miError(rc, self.lib.av1mi_last_error(self.h).decode())

    @property
    def device_name(self):
        return self.lib.av1mi_device_name(self.h).decode()

    def alloc(self, nbytes):
        return DevBuf(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DevBuf(self, max(arr.nbytes, 16)).upload(arr)

    def sync(self):
        self._chk(self.lib.av1mi_sync(self.h))

    def memset(self, d_buf, value, nbytes):
        self._chk(self.lib.av1mi_memset(self.h, C.c_void_p(d_buf.ptr), int(value), C.c_size_t(nbytes)))

    def copy(self, d_dst, d_src, nbytes):
        self._chk(self.lib.av1mi_copy(self.h, C.c_void_p(d_dst.ptr), C.c_void_p(d_src.ptr), C.c_size_t(nbytes)))

    def timer_begin(self):
        self._chk(self.lib.av1mi_timer_begin(self.h))

    def timer_end(self):
        ms = C.c_float()
        self._chk(self.lib.av1mi_timer_end(self.h, C.byref(ms)))
        return ms.value

    # ---- K2 / K1 / K8, device-resident
    def inv_txfm_add_grid(self, tx_size, d_coef, d_plane, stride, bd, blocks_per_row, nblocks, d_types=None, uniform_type=0):
        self._chk(self.lib.av1mi_inv_txfm_add_grid(self.h, tx_size, C.c_void_p(d_coef.ptr), C.c_void_p(d_plane.ptr), stride, bd,
                                                   blocks_per_row, nblocks, C.c_void_p(d_types.ptr if d_types else None),
                                                   uniform_type))

    def inv_txfm_add_list(self, tx_size, d_coef, d_plane, stride, bd, d_list, nblocks):
        self._chk(self.lib.av1mi_inv_txfm_add_list(self.h, tx_size, C.c_void_p(d_coef.ptr), C.c_void_p(d_plane.ptr), stride, bd,
                                                   C.c_void_p(d_list.ptr), nblocks))

    def fwd_txfm_grid(self, tx_size, d_resid, stride, d_coef, blocks_per_row, nblocks, d_types=None, uniform_type=0):
        self._chk(self.lib.av1mi_fwd_txfm_grid(self.h, tx_size, C.c_void_p(d_resid.ptr), stride, C.c_void_p(d_coef.ptr),
                                               blocks_per_row, nblocks, C.c_void_p(d_types.ptr if d_types else None),
                                               uniform_type))

    def fwd_txfm_list(self, tx_size, d_resid, stride, d_coef, d_list, nblocks):
        self._chk(self.lib.av1mi_fwd_txfm_list(self.h, tx_size, C.c_void_p(d_resid.ptr), stride, C.c_void_p(d_coef.ptr),
                                               C.c_void_p(d_list.ptr), nblocks))

    def quantize(self, d_coef, d_levels, d_dq, n, coef_per_blk, dc_q, ac_q, log_scale):
        self._chk(self.lib.av1mi_quantize(self.h, C.c_void_p(d_coef.ptr), C.c_void_p(d_levels.ptr),
                                          C.c_void_p(d_dq.ptr if d_dq else None), C.c_size_t(n), coef_per_blk, dc_q, ac_q,
                                          log_scale))

    def dequantize(self, d_levels, d_dq, n, coef_per_blk, dc_q, ac_q, log_scale, bd):
        self._chk(self.lib.av1mi_dequantize(self.h, C.c_void_p(d_levels.ptr), C.c_void_p(d_dq.ptr), C.c_size_t(n), coef_per_blk,
                                            dc_q, ac_q, log_scale, bd))

    # ---- K3
    def intra_pred_list(self, tx_size, d_ref, ref_stride, d_dst, dst_stride, bd, d_list, nblocks):
        self._chk(self.lib.av1mi_intra_pred_list(self.h, tx_size, C.c_void_p(d_ref.ptr), ref_stride, C.c_void_p(d_dst.ptr),
                                                 dst_stride, bd, C.c_void_p(d_list.ptr), nblocks))

    def cfl_pred_list(self, tx_size, d_luma, luma_stride, d_dst, dst_stride, bd, d_list, nblocks):
        self._chk(self.lib.av1mi_cfl_pred_list(self.h, tx_size, C.c_void_p(d_luma.ptr), luma_stride, C.c_void_p(d_dst.ptr), dst_stride,
                                               bd, C.c_void_p(d_list.ptr), nblocks))

    # ---- K4
    def mc_list(self, size_id, d_ref, ref_stride, plane_w, plane_h, d_dst, dst_stride, bd, d_list, nblocks):
        self._chk(self.lib.av1mi_mc_list(self.h, size_id, C.c_void_p(d_ref.ptr), ref_stride, plane_w, plane_h, C.c_void_p(d_dst.ptr),
                                         dst_stride, bd, C.c_void_p(d_list.ptr), nblocks))

    # ---- K5
    def deblock_plane(self, d_src, src_stride, d_dst, dst_stride, w, h, bd, is_chroma, d_mi, mi_stride, sharpness):
        self._chk(self.lib.av1mi_deblock_plane(self.h, C.c_void_p(d_src.ptr), src_stride, C.c_void_p(d_dst.ptr), dst_stride, w, h, bd,
                                               int(is_chroma), C.c_void_p(d_mi.ptr), mi_stride, sharpness))

    def deblock_frames(self, d_src, src_stride, d_dst, dst_stride, w, h, bd, is_chroma, d_mi, mi_stride, mi_frame_stride,
                       sharpness, nframes):
        self._chk(self.lib.av1mi_deblock_frames(self.h, C.c_void_p(d_src.ptr), src_stride, C.c_void_p(d_dst.ptr), dst_stride, w, h,
                                                bd, int(is_chroma), C.c_void_p(d_mi.ptr), mi_stride, C.c_size_t(mi_frame_stride),
                                                sharpness, nframes))

    def input_convert(self, fmt, bit_depth, width, rows, d_in, d_out):
        """d_in: the format's planes (2 or 3 DevBuf), d_out: planar Y, U, V (DevBuf); one launch, asynchronous (av1mi_input_convert)"""
        self.lib.av1mi_input_convert.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 6
        i = [b.ptr for b in d_in] + [None] * (3 - len(d_in))
        self._chk(self.lib.av1mi_input_convert(self.h, int(fmt), int(bit_depth), int(width), int(rows), *i, *[b.ptr for b in d_out]))

    def chroma_convert(self, chroma, source_bit_depth, bit_depth, width, height, frames, d_in, d_out):
        """d_in: the source's planes (3 DevBuf or None) of `frames` stacked frames of TRUE size width x height in a chroma layout, d_out:
        the 4:2:0 planes Y, U, V (DevBuf; Y may be None where the depths are equal); one launch, asynchronous (av1mi_chroma_convert)"""
        self.lib.av1mi_chroma_convert.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 6
        ptr = [b.ptr if b is not None else None for b in list(d_in) + list(d_out)]
        self._chk(self.lib.av1mi_chroma_convert(self.h, int(chroma), int(source_bit_depth), int(bit_depth), int(width), int(height), int(frames), *ptr))

    def tone_map(self, width, height, frames, d_y, d_u, d_v, d_tables):
        """planar 4:2:0 10-bit planes (DevBuf) of `frames` stacked frames of luma size width x height tone-mapped in place with the tables in
        d_tables (a DevBuf holding a ToneTables); one launch, asynchronous (av1mi_tone_map)"""
        self.lib.av1mi_tone_map.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 4
        self._chk(self.lib.av1mi_tone_map(self.h, int(width), int(height), int(frames), d_y.ptr, d_u.ptr, d_v.ptr, d_tables.ptr))

    def depth_reduce(self, mode, width, height, frames, d_in, d_out):
        """d_in: planar 4:2:0 uint16 planes Y, U, V (DevBuf) of `frames` stacked frames of luma buffer size width x height, d_out: the uint8
        planes they are reduced to, mode DEPTH_ROUND / DEPTH_ORDERED; one launch, asynchronous (av1mi_depth_reduce)"""
        self.lib.av1mi_depth_reduce.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2
        src = (C.c_void_p * 3)(*[b.ptr if b is not None else None for b in d_in])
        dst = (C.c_void_p * 3)(*[b.ptr if b is not None else None for b in d_out])
        self._chk(self.lib.av1mi_depth_reduce(self.h, int(mode), int(width), int(height), int(frames), src, dst))

    def scale_planes(self, bit_depth, src_w, src_h, dst_w, dst_h, frames, d_src, d_dst):
        """d_src: planar Y, U, V (DevBuf) of `frames` stacked frames of true size src_w x src_h in buffers of that size rounded up to 8;
        d_dst: the same for dst_w x dst_h; one launch, asynchronous (av1mi_scale_planes)"""
        self.lib.av1mi_scale_planes.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 2
        src, dst = (C.c_void_p * 3)(*[b.ptr for b in d_src]), (C.c_void_p * 3)(*[b.ptr for b in d_dst])
        self._chk(self.lib.av1mi_scale_planes(self.h, int(bit_depth), int(src_w), int(src_h), int(dst_w), int(dst_h), int(frames), src, dst))

    def quality_planes(self, bit_depth, width, height, frames, d_src, d_dec0, d_dec1=None, d_select=None):
        """records [frames, 3] (QUALITY_DTYPE) of `frames` stacked frames of TRUE luma size width x height: d_src against d_dec0, or d_dec1
        where d_select (DevBuf of frames * 3 bytes) holds 0; planar Y, U, V DevBufs at the size rounded up to 8 (av1mi_quality_planes);
        synchronous here: the records are downloaded"""
        self.lib.av1mi_quality_planes.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 5
        arr = lambda bufs: (C.c_void_p * 3)(*[b.ptr for b in bufs]) if bufs is not None else None
        d_out = self.alloc(frames * 3 * QUALITY_DTYPE.itemsize)
        try:
            self._chk(self.lib.av1mi_quality_planes(self.h, int(bit_depth), int(width), int(height), int(frames), arr(d_src), arr(d_dec0), arr(d_dec1),
                                                    d_select.ptr if d_select is not None else None, d_out.ptr))
            return d_out.download((frames, 3), QUALITY_DTYPE)
        finally:
            d_out.free()

    def scene_analyse(self, Y, bit_depth):
        """the scene records (SCENE_DTYPE [frames]) of a run of luma planes Y [frames, h, w], h and w multiples of 8 (av1mi_scene_analyse);
        synchronous here: the records are downloaded"""
        Y = np.ascontiguousarray(Y, np.uint8 if bit_depth == 8 else np.uint16)
        n, h, w = Y.shape
        self.lib.av1mi_scene_analyse.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2
        d_y, d_out = self.to_device(Y), self.alloc(n * SCENE_DTYPE.itemsize)
        try:
            self._chk(self.lib.av1mi_scene_analyse(self.h, int(bit_depth), w, h, n, d_y.ptr, d_out.ptr))
            return d_out.download((n,), SCENE_DTYPE)
        finally:
            d_y.free()
            d_out.free()

    def frames_gather(self, plane_bytes, segments, d_table, d_dst):
        """one launch: per segment and plane plane_bytes[p] bytes from the device pointer d_table (DevBuf of segments * 3 uint64) holds at
        [s * 3 + p], zeros where it holds 0, to d_dst[p] (DevBuf) + s * plane_bytes[p] (av1mi_frames_gather); asynchronous"""
        self.lib.av1mi_frames_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        nb = (C.c_size_t * 3)(*[int(b) for b in plane_bytes])
        dst = (C.c_void_p * 3)(*[b.ptr if b is not None else None for b in d_dst])
        self._chk(self.lib.av1mi_frames_gather(self.h, nb, int(segments), d_table.ptr, dst))

    @staticmethod
    def _gather_planes(plane_sizes, true_sizes, d_dst):
        """the filtering gathers' plane_w, plane_h, true_w, true_h (int[3] each) and d_dst (void *[3], null for an absent plane)"""
        arr = lambda v: (C.c_int * 3)(*[int(x) for x in v])
        sizes = [arr([s[i] for s in v]) for v in (plane_sizes, true_sizes) for i in (0, 1)]
        return sizes, (C.c_void_p * 3)(*[b.ptr if b is not None else None for b in d_dst])

    def deinterlace_gather(self, bit_depth, plane_sizes, true_sizes, parity, segments, d_table, d_dst):
        """one launch: the gather with the deinterlacer in it (av1mi_deinterlace_gather).  plane_sizes / true_sizes: (w, h) in samples per
        plane, (0, 0) = no such plane; d_table: DevBuf of segments * 9 uint64, [(s * 3 + p) * 3 + i] = plane p of segment s's frame P, C, N
        (C 0 = zeros); d_dst[p]: DevBuf (None for an absent plane); asynchronous"""
        self.lib.av1mi_deinterlace_gather.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        sizes, dst = self._gather_planes(plane_sizes, true_sizes, d_dst)
        self._chk(self.lib.av1mi_deinterlace_gather(self.h, int(bit_depth), *sizes, int(parity), int(segments), d_table.ptr, dst))

    def deinterlace_gather_fields(self, bit_depth, plane_sizes, true_sizes, parity, segments, d_table, d_phase, d_dst):
        """the same at field rate (av1mi_deinterlace_gather_fields): d_phase: DevBuf of `segments` bytes, 0 = the first field of the
        segment's frame, 1 = its second (only the low bit is read); the table holds P, C, N of the SOURCE frame"""
        self.lib.av1mi_deinterlace_gather_fields.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        sizes, dst = self._gather_planes(plane_sizes, true_sizes, d_dst)
        self._chk(self.lib.av1mi_deinterlace_gather_fields(self.h, int(bit_depth), *sizes, int(parity), int(segments), d_table.ptr, d_phase.ptr if d_phase is not None else None, dst))

    def telecine_analyse(self, Y, bit_depth, true_size):
        """the field-match records (TELECINE_DTYPE [frames]) of a run of luma planes Y [frames, H8, W8], H8 and W8 multiples of 8, whose
        picture is true_size = (width, height) (av1mi_telecine_analyse)"""
        Y = np.ascontiguousarray(Y, np.uint8 if bit_depth == 8 else np.uint16)
        n, h, w = Y.shape
        self.lib.av1mi_telecine_analyse.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
        d_y, d_out = self.to_device(Y), self.alloc(n * TELECINE_DTYPE.itemsize)
        try:
            self._chk(self.lib.av1mi_telecine_analyse(self.h, int(bit_depth), w, h, int(true_size[0]), int(true_size[1]), n, d_y.ptr, d_out.ptr))
            return d_out.download((n,), TELECINE_DTYPE)
        finally:
            d_y.free()
            d_out.free()

    def telecine_gather(self, bit_depth, plane_sizes, true_sizes, segments, d_table, d_dst):
        """one launch: the weave gather (av1mi_telecine_gather).  plane_sizes / true_sizes / d_dst as deinterlace_gather's; d_table: DevBuf
        of segments * 6 uint64, [(s * 3 + p) * 2 + i] = plane p of segment s's top (i = 0) and bottom (1) source (top 0 = zeros);
        asynchronous"""
        self.lib.av1mi_telecine_gather.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
        sizes, dst = self._gather_planes(plane_sizes, true_sizes, d_dst)
        self._chk(self.lib.av1mi_telecine_gather(self.h, int(bit_depth), *sizes, int(segments), d_table.ptr, dst))

    def crop_analyse(self, Y, bit_depth, true_size, limit=24):
        """the margins (CROP_DTYPE [frames]) of luma planes Y [frames, H8, W8], H8 and W8 multiples of 8, whose picture is true_size =
        (width, height) (av1mi_crop_analyse): the dark rows / columns at every edge, `limit` the mean 8-bit level up to which a line is dark"""
        Y = np.ascontiguousarray(Y, np.uint8 if bit_depth == 8 else np.uint16)
        n, h, w = Y.shape
        self.lib.av1mi_crop_analyse.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p]
        d_y, d_out = self.to_device(Y), self.alloc(n * CROP_DTYPE.itemsize)
        try:
            self._chk(self.lib.av1mi_crop_analyse(self.h, int(bit_depth), w, h, int(true_size[0]), int(true_size[1]), n, d_y.ptr, int(limit), d_out.ptr))
            return d_out.download((n,), CROP_DTYPE)
        finally:
            d_y.free()
            d_out.free()

    def noise_analyse(self, Y, bit_depth, true_size):
        """the noise records (NOISE_DTYPE [pairs]) of luma planes Y [2 * pairs, H8, W8], H8 and W8 multiples of 8, whose picture is true_size =
        (width, height) (av1mi_noise_analyse): pair i is planes 2 i and 2 i + 1, two consecutive frames; av1stream.plan_denoise() turns
        the records into a strength"""
        Y = np.ascontiguousarray(Y, np.uint8 if bit_depth == 8 else np.uint16)
        n, h, w = Y.shape
        assert n % 2 == 0, "pairs of planes"
        self.lib.av1mi_noise_analyse.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
        d_y, d_out = self.to_device(Y), self.alloc(max(n // 2, 1) * NOISE_DTYPE.itemsize)
        try:
            self._chk(self.lib.av1mi_noise_analyse(self.h, int(bit_depth), w, h, int(true_size[0]), int(true_size[1]), n // 2, d_y.ptr, d_out.ptr))
            return d_out.download((n // 2,), NOISE_DTYPE)
        finally:
            d_y.free()
            d_out.free()

    def peak_analyse(self, Y, U, V, true_size):
        """the peak records (PEAK_DTYPE [frames]) of planar 4:2:0 uint16 frames Y [frames, H8, W8], U and V [frames, H8 / 2, W8 / 2], H8 and W8
        multiples of 8, whose picture is true_size = (width, height) (av1mi_peak_analyse); av1stream.plan_peak() turns the records into the
        tone map's source peak"""
        Y, U, V = (np.ascontiguousarray(a, np.uint16) for a in (Y, U, V))
        n, h, w = Y.shape
        assert U.shape == V.shape == (n, h // 2, w // 2), "4:2:0 planes"
        self.lib.av1mi_peak_analyse.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4
        bufs = [self.to_device(a) for a in (Y, U, V)] + [self.alloc(max(n, 1) * PEAK_DTYPE.itemsize)]
        try:
            self._chk(self.lib.av1mi_peak_analyse(self.h, w, h, int(true_size[0]), int(true_size[1]), n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr))
            return bufs[3].download((n,), PEAK_DTYPE)
        finally:
            for b in bufs:
                b.free()

    def denoise_gather(self, bit_depth, plane_sizes, true_sizes, strength, segments, d_table, d_dst, d_records=None):
        """the gather with the denoiser in it (av1mi_denoise_gather): deinterlace_gather's arguments with a strength (1 .. 16) in place of
        the parity; d_records: DevBuf of segments * 3 records (GRAIN_DTYPE [segments, 3, GRAIN_BINS]) or None = nothing is measured;
        asynchronous"""
        self.lib.av1mi_denoise_gather.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        sizes, dst = self._gather_planes(plane_sizes, true_sizes, d_dst)
        self._chk(self.lib.av1mi_denoise_gather(self.h, int(bit_depth), *sizes, int(strength), int(segments), d_table.ptr, dst,
                                                d_records.ptr if d_records is not None else None))

    def denoise_mc_gather(self, bit_depth, plane_sizes, true_sizes, strength, rng, segments, d_table, d_dst, d_records=None, d_vectors=None):
        """the denoising gather behind a block search (av1mi_denoise_mc_gather): denoise_gather's arguments with rng (4 or 8) after the
        strength; d_vectors: DevBuf of segments * blocks records (DENOISE_VEC_DTYPE [segments, blocks], blocks = ceil(w / 16) * ceil(h / 16)
        of the luma plane's true size) or None = the vectors stay in the context; asynchronous"""
        self.lib.av1mi_denoise_mc_gather.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
        sizes, dst = self._gather_planes(plane_sizes, true_sizes, d_dst)
        self._chk(self.lib.av1mi_denoise_mc_gather(self.h, int(bit_depth), *sizes, int(strength), int(rng), int(segments), d_table.ptr, dst,
                                                   d_records.ptr if d_records is not None else None, d_vectors.ptr if d_vectors is not None else None))

    def grain_cov(self, bit_depth, plane_sizes, true_sizes, segments, d_table, d_out, d_cov):
        """the grain covariance behind a denoising gather (av1mi_grain_cov): that gather's sizes, segments and table, d_out the planes it
        wrote; d_cov: DevBuf of segments * 3 records (GRAIN_COV_DTYPE [segments, 3]); asynchronous"""
        self.lib.av1mi_grain_cov.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        sizes, out = self._gather_planes(plane_sizes, true_sizes, d_out)
        self._chk(self.lib.av1mi_grain_cov(self.h, int(bit_depth), *sizes, int(segments), d_table.ptr, out, d_cov.ptr if d_cov is not None else None))

    def prof_enable(self, on):
        self._chk(self.lib.av1mi_prof_enable(self.h, int(on)))

    def prof_reset(self):
        self._chk(self.lib.av1mi_prof_reset(self.h))

    def kernel_kinds(self):
        """the names of the loaded library's kernel kinds, in enum order (av1mi_kernel_kind_name answers "?" from AV1MI_K_KINDS on),
        so a library with fewer kinds than this file knows is asked for no kind it lacks"""
        self.lib.av1mi_kernel_kind_name.restype = C.c_char_p
        names = []
        while len(names) < 256:
            name = self.lib.av1mi_kernel_kind_name(len(names))
            if name == b"?":
                break
            names.append(name.decode())
        return names

    def prof_get(self):
        """{kind name: (launches, total_ms)} for kinds that were launched"""
        out = {}
        for k, name in enumerate(self.kernel_kinds()):
            n, ms = C.c_int(), C.c_double()
            self._chk(self.lib.av1mi_prof_get(self.h, k, C.byref(n), C.byref(ms)))
            if n.value:
                out[name] = (n.value, ms.value)
        return out

    # ---- K6
    def cdef_frames(self, job):
        self._chk(self.lib.av1mi_cdef_frames(self.h, C.byref(job)))

    def cdef_arrays(self, Y, U, V, bd, damping, sb_strength, skip8):
        """tests: Y/U/V [frames,h,w]; sb_strength [frames or 1, nsb, 4]; skip8 [frames or 1, h/8, w/8]"""
        dt = np.uint8 if bd == 8 else np.uint16
        Y, U, V = (np.ascontiguousarray(a, dt) for a in (Y, U, V))
        nf, h, w = Y.shape
        sb_strength = np.ascontiguousarray(sb_strength, np.uint8); skip8 = np.ascontiguousarray(skip8, np.uint8)
        bufs = [self.to_device(a) for a in (Y, U, V)] + [self.alloc(a.nbytes) for a in (Y, U, V)] + [self.to_device(sb_strength), self.to_device(skip8)]
        job = CdefJob(w, h, bd, nf, damping, w, w // 2, *[b.ptr for b in bufs[:6]], bufs[6].ptr,
                      0 if sb_strength.shape[0] == 1 else sb_strength.shape[1], bufs[7].ptr,
                      0 if skip8.shape[0] == 1 else skip8.shape[1] * skip8.shape[2])
        self.cdef_frames(job)
        out = (bufs[3].download(Y.shape, dt), bufs[4].download(U.shape, dt), bufs[5].download(V.shape, dt))
        for b in bufs:
            b.free()
        return out

    # ---- K5 + K6 in one launch
    def deblock_cdef_frames(self, job):
        """deblocking and CDEF of stacked 4:2:0 frames in one kernel (include/av1mi.h av1mi_deblock_cdef_frames; job: DeblockCdefJob)"""
        self._chk(self.lib.av1mi_deblock_cdef_frames(self.h, C.byref(job)))

    # ---- K7
    def lr_frames(self, d_cdef, d_dbl, d_out, stride, w, h, bd, ss, unit_size, d_units, unit_frame_stride, nframes):
        self._chk(self.lib.av1mi_lr_frames(self.h, C.c_void_p(d_cdef.ptr), C.c_void_p(d_dbl.ptr), C.c_void_p(d_out.ptr), stride, w, h, bd,
                                           int(ss), unit_size, C.c_void_p(d_units.ptr), C.c_size_t(unit_frame_stride), nframes))

    def lr_decide_scratch_bytes(self, h, ss, nframes):
        self.lib.av1mi_lr_decide_scratch_bytes.restype = C.c_size_t
        return int(self.lib.av1mi_lr_decide_scratch_bytes(h, int(ss), nframes))

    def lr_frames_decide(self, d_cdef, d_dbl, d_out, stride, w, h, bd, ss, unit_size, d_units, unit_frame_stride, nframes, d_orig, d_scratch, d_on,
                         on_offset=0, on_stride=1):
        """restoration + the per-frame ON / OFF decision against the source d_orig; d_on: uint8 buffer, entry on_offset + f * on_stride"""
        self._chk(self.lib.av1mi_lr_frames_decide(self.h, C.c_void_p(d_cdef.ptr), C.c_void_p(d_dbl.ptr), C.c_void_p(d_out.ptr), stride, w, h, bd,
                                                  int(ss), unit_size, C.c_void_p(d_units.ptr), C.c_size_t(unit_frame_stride), nframes,
                                                  C.c_void_p(d_orig.ptr), C.c_void_p(d_scratch.ptr), C.c_void_p(d_on.ptr + on_offset), int(on_stride)))

    def lr_yuv_decide_scratch_bytes(self, h, nframes):
        self.lib.av1mi_lr_yuv_decide_scratch_bytes.restype = C.c_size_t
        return int(self.lib.av1mi_lr_yuv_decide_scratch_bytes(int(h), int(nframes)))

    def lr_yuv_decide(self, job):
        """the three planes' restoration + ON / OFF decisions in one call (include/av1mi.h av1mi_lr_yuv_decide)"""
        self._chk(self.lib.av1mi_lr_yuv_decide(self.h, C.byref(job)))

    def cdef_search(self, job):
        """a CDEF strength set per superblock against the source (include/av1mi.h av1mi_cdef_search; job: CdefSearchJob)"""
        self._chk(self.lib.av1mi_cdef_search(self.h, C.byref(job)))

    def lf_search(self, job):
        """the deblocking levels per frame against the source, and a map per frame (include/av1mi.h av1mi_lf_search; job: LfSearchJob)"""
        self._chk(self.lib.av1mi_lf_search(self.h, C.byref(job)))

    def lr_search(self, job):
        """a Wiener record or none per restoration unit of the three planes (include/av1mi.h av1mi_lr_search; job: LrSearchJob)"""
        self._chk(self.lib.av1mi_lr_search(self.h, C.byref(job)))

    # ---- fused intra-only segment pipeline
    def extend_frames(self, d_plane, stride, w, h, visible_w, visible_h, bd, nframes):
        self._chk(self.lib.av1mi_extend_frames(self.h, C.c_void_p(d_plane.ptr), stride, w, h, visible_w, visible_h, bd, nframes))

    def intra_encode(self, job):
        self._chk(self.lib.av1mi_intra_encode(self.h, C.byref(job)))

    def intra_encode_arrays(self, Y, U, V, bd, bs, qindex, open_loop=False, stride_y=None, stride_uv=None, frame_rows=None,
                            modes_frame_stride=None):
        """convenience for tests: Y/U/V are [frames, h, w] arrays; returns dict of outputs like the oracle's.  The job's geometry
        (av1mi_intra_job; defaults: compact): stride_y / stride_uv lay the rows of every plane that many samples apart, frame_rows
        makes the job the top band of frames that many luma rows tall (the levels of consecutive frames lie as far apart as those
        frames' samples), modes_frame_stride lays the frames' mode bytes that far apart.  The sources are uploaded into that layout
        and every output buffer is pre-filled with a sentinel (0xA5 bytes, which no mode takes).  rec_*, lev_* and modes_* are the
        compact views; what lies outside them comes back as the kernels left it, each key only where the layout has such bytes:
        rec_pad_* [frames, rows, stride - width] the row padding of the band, rec_gap_* [frames, frame rows - rows, stride] the rows
        between bands, lev_gap_* [frames, n] the levels between the frames' blocks, modes_gap_y / _uv [frames, stride - blocks]."""
        dt = np.uint8 if bd == 8 else np.uint16
        P = [np.ascontiguousarray(a, dt) for a in (Y, U, V)]
        nf, h, w = P[0].shape
        nb, cs = (h // bs) * (w // bs), bs // 2
        strides = [w if stride_y is None else int(stride_y)] + [w // 2 if stride_uv is None else int(stride_uv)] * 2
        job = IntraJob(w, h, bd, nf, qindex, bs, strides[0], strides[1])
        job.open_loop = 1 if open_loop else 0
        job.frame_rows = 0 if frame_rows is None else int(frame_rows)
        job.modes_frame_stride = 0 if modes_frame_stride is None else int(modes_frame_stride)
        # the buffers' own geometry; an impossible value goes to the library as it is, which refuses the job before anything runs
        fr = max(job.frame_rows, h)
        ms = max(job.modes_frame_stride, nb)
        bufs, shape = {}, {}
        try:
            for i, p in enumerate("yuv"):
                rows, width = P[i].shape[1:]
                shape[p] = (nf, fr if i == 0 else fr // 2, max(strides[i], width))
                src = np.zeros(shape[p], dt)
                src[:, :rows, :width] = P[i]
                bufs["src_" + p] = self.to_device(src)
                bufs["rec_" + p] = self.alloc(src.nbytes)
                bufs["lev_" + p] = self.alloc(nf * shape[p][1] * width * 2)
            bufs["modes_y"], bufs["modes_uv"] = self.alloc(nf * ms), self.alloc(nf * ms)
            for name, b in bufs.items():
                if not name.startswith("src_"):
                    self.memset(b, 0xA5, b.nbytes)
                setattr(job, "d_" + name, b.ptr)
            self.intra_encode(job)
            out = {}
            for i, p in enumerate("yuv"):
                rows, width = P[i].shape[1:]
                b = bs if i == 0 else cs
                rec = bufs["rec_" + p].download(shape[p], dt)
                out["rec_" + p] = np.ascontiguousarray(rec[:, :rows, :width])
                if shape[p][2] > width:
                    out["rec_pad_" + p] = np.ascontiguousarray(rec[:, :rows, width:])
                if shape[p][1] > rows:
                    out["rec_gap_" + p] = np.ascontiguousarray(rec[:, rows:])
                lev = bufs["lev_" + p].download((nf, shape[p][1] * width), np.int16)
                out["lev_" + p] = np.ascontiguousarray(lev[:, :rows * width]).reshape(nf, nb, b, b)
                if shape[p][1] > rows:
                    out["lev_gap_" + p] = np.ascontiguousarray(lev[:, rows * width:])
            for k in ("modes_y", "modes_uv"):
                m = bufs[k].download((nf, ms), np.uint8)
                out[k] = np.ascontiguousarray(m[:, :nb])
                if ms > nb:
                    out[k.replace("modes_", "modes_gap_")] = np.ascontiguousarray(m[:, nb:])
            return out
        finally:
            for b in bufs.values():
                b.free()

    # ---- inter (P-frame) pipeline
    def inter_encode(self, job):
        self._chk(self.lib.av1mi_inter_encode(self.h, C.byref(job)))

    def me_search(self, src_y, ref_y, bd, search_range=8, coarse_range=0, ref_alt_y=None, ref_sel=None):
        """the motion search alone (av1mi_me_search): src_y / ref_y [frames, h, w] luma; ref_alt_y + ref_sel ([frames, 3] uint8, 0 = predict
        from ref_alt_y) as in av1mi_inter_job.  Returns dict(mvs [frames, blocks, 2] — the integer vectors in 1/8 samples —, centres
        [frames, tiles, 2], q_src / q_ref [frames, h / 4, w / 4] (None when coarse_range is 0))"""
        dt = np.uint8 if bd == 8 else np.uint16
        S, R = np.ascontiguousarray(src_y, dt), np.ascontiguousarray(ref_y, dt)
        nf, h, w = S.shape
        nb, tiles = (h // 8) * (w // 8), ((h + 63) // 64) * ((w + 63) // 64)
        bufs = dict(src_y=self.to_device(S), ref_y=self.to_device(R), mvs=self.alloc(nf * nb * 4))
        if ref_sel is not None:
            sel = np.zeros((nf * 3 + 3) & ~3, np.uint8)      # read as aligned dwords
            sel[:nf * 3] = np.ascontiguousarray(ref_sel, np.uint8).reshape(-1)
            bufs["ref_alt_y"], bufs["ref_sel"] = self.to_device(np.ascontiguousarray(ref_alt_y, dt)), self.to_device(sel)
        job = InterJob(w, h, bd, nf, 0, search_range, w, w // 2)
        job.coarse_range = coarse_range
        for k, b in bufs.items():
            setattr(job, "d_" + k, b.ptr)
        q = [self.alloc(nf * (h // 4) * (w // 4)) for _ in range(2)]
        cen = self.alloc(nf * tiles * 4)
        self.lib.av1mi_me_search.argtypes = [C.c_void_p, C.POINTER(InterJob), C.c_void_p, C.c_void_p, C.c_void_p]
        try:
            self._chk(self.lib.av1mi_me_search(self.h, C.byref(job), q[0].ptr, q[1].ptr, cen.ptr))
            out = dict(mvs=bufs["mvs"].download((nf, nb, 2), np.int16), centres=cen.download((nf, tiles, 2), np.int16), q_src=None, q_ref=None)
            if coarse_range:
                out["q_src"], out["q_ref"] = (b.download((nf, h // 4, w // 4), np.uint8) for b in q)
            return out
        finally:
            for b in list(bufs.values()) + q + [cen]:
                b.free()

    def inter_encode_arrays(self, src, ref, bd, qindex, search_range=8, coarse_range=0, stride_y=None, stride_uv=None):
        """tests: src / ref = (Y, U, V) with arrays [frames, h, w]; returns dict like the oracle's.  stride_y / stride_uv (samples;
        default: the plane widths) lay the rows of every plane that far apart on the device: source and reference are uploaded into
        padded rows, the reconstruction buffers are pre-filled with a sentinel (0xA5 bytes), rec_* are the w-wide views and
        rec_pad_* the padding columns [frames, rows, stride - width] as the kernels left them (absent for a compact plane)."""
        dt = np.uint8 if bd == 8 else np.uint16
        S = [np.ascontiguousarray(a, dt) for a in src]
        R = [np.ascontiguousarray(a, dt) for a in ref]
        nf, h, w = S[0].shape
        nb = (h // 8) * (w // 8)
        strides = [w if stride_y is None else int(stride_y)] + [w // 2 if stride_uv is None else int(stride_uv)] * 2

        def padded(a, st):       # rows st samples apart; an impossible stride goes to the library as it is, which refuses the job
            if st <= a.shape[2]:
                return a
            out = np.zeros(a.shape[:2] + (st,), dt)
            out[:, :, :a.shape[2]] = a
            return out

        bufs = {}
        try:
            for i, p in enumerate("yuv"):
                st = max(strides[i], S[i].shape[2])
                bufs["src_" + p], bufs["ref_" + p] = self.to_device(padded(S[i], st)), self.to_device(padded(R[i], st))
                bufs["rec_" + p] = self.alloc(nf * S[i].shape[1] * st * dt().itemsize)
                self.memset(bufs["rec_" + p], 0xA5, bufs["rec_" + p].nbytes)
                bufs["lev_" + p] = self.alloc(S[i].size * 2)
            bufs["mvs"], bufs["skip"] = self.alloc(nf * nb * 4), self.alloc(nf * nb)
            job = InterJob(w, h, bd, nf, qindex, search_range, strides[0], strides[1])
            job.coarse_range = coarse_range
            for k, b in bufs.items():
                setattr(job, "d_" + k, b.ptr)
            self.inter_encode(job)
            out = dict(mvs=bufs["mvs"].download((nf, nb, 2), np.int16), skip=bufs["skip"].download((nf, nb), np.uint8))
            for i, p in enumerate("yuv"):
                bs = 8 if i == 0 else 4
                rec = bufs["rec_" + p].download((nf, S[i].shape[1], strides[i]), dt)
                out["rec_" + p] = np.ascontiguousarray(rec[:, :, :S[i].shape[2]])
                if strides[i] > S[i].shape[2]:
                    out["rec_pad_" + p] = np.ascontiguousarray(rec[:, :, S[i].shape[2]:])
                out["lev_" + p] = bufs["lev_" + p].download((nf, nb, bs, bs), np.int16)
            return out
        finally:
            for b in bufs.values():
                b.free()

    # ---- host-pointer single-block forms
    def inv_txfm2d_add(self, coef, pred, tx_size, tx_type, bd):
        coef = np.ascontiguousarray(coef, np.int32)
        dst = np.ascontiguousarray(pred, np.uint8 if bd == 8 else np.uint16).copy()
        self._chk(self.lib.av1mi_inv_txfm2d_add(self.h, coef.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                                                dst.shape[1], tx_size, tx_type, bd))
        return dst

    def fwd_txfm2d(self, resid, tx_size, tx_type):
        resid = np.ascontiguousarray(resid, np.int16)
        coef = np.zeros((min(TX_H[tx_size], 32), min(TX_W[tx_size], 32)), np.int32)
        self._chk(self.lib.av1mi_fwd_txfm2d(self.h, resid.ctypes.data_as(C.c_void_p), resid.shape[1],
                                            coef.ctypes.data_as(C.c_void_p), tx_size, tx_type))
        return coef
