"""ctypes binding of the host AV1 bitstream writer (host/av1_bitstream.hpp, exported by libav1mi_host.so).

Plumbing only: builds the `av1mi_obu_frame` description from numpy arrays (the symbols the GPU pipeline produced) and
returns the Section-5 OBU bytes of one temporal unit.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "libav1mi_host.so")
_lib = None


class FilmGrain(C.Structure):
    """av1mi_film_grain (include/av1mi_host.h): the film_grain_params a frame header carries"""
    _fields_ = [("apply_grain", C.c_int32), ("grain_seed", C.c_int32), ("num_y_points", C.c_int32), ("point_y_value", C.c_uint8 * 14),
                ("point_y_scaling", C.c_uint8 * 14), ("chroma_scaling_from_luma", C.c_int32), ("num_cb_points", C.c_int32), ("num_cr_points", C.c_int32),
                ("point_cb_value", C.c_uint8 * 10), ("point_cb_scaling", C.c_uint8 * 10), ("point_cr_value", C.c_uint8 * 10), ("point_cr_scaling", C.c_uint8 * 10),
                ("grain_scaling_minus_8", C.c_int32), ("ar_coeff_lag", C.c_int32), ("ar_coeffs_y_plus_128", C.c_uint8 * 24),
                ("ar_coeffs_cb_plus_128", C.c_uint8 * 25), ("ar_coeffs_cr_plus_128", C.c_uint8 * 25), ("ar_coeff_shift_minus_6", C.c_int32),
                ("grain_scale_shift", C.c_int32), ("cb_mult", C.c_int32), ("cb_luma_mult", C.c_int32), ("cb_offset", C.c_int32), ("cr_mult", C.c_int32),
                ("cr_luma_mult", C.c_int32), ("cr_offset", C.c_int32), ("overlap_flag", C.c_int32), ("clip_to_restricted_range", C.c_int32)]


def _set_film_grain(f, film_grain, film_grain_present):
    """the two film grain fields of an ObuFrame; film_grain_present None = follows the pointer"""
    f.film_grain_present = int(film_grain is not None if film_grain_present is None else film_grain_present)
    f.film_grain = C.addressof(film_grain) if film_grain is not None else None


class ObuFrame(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32), ("frame_type", C.c_int32),
                ("base_q_idx", C.c_int32), ("lf_level", C.c_int32 * 4), ("lf_sharpness", C.c_int32), ("cdef_damping", C.c_int32),
                ("cdef_bits", C.c_int32), ("cdef_y", C.c_uint8 * 8), ("cdef_uv", C.c_uint8 * 8), ("cdef_idx", C.c_void_p),
                ("lr_type", C.c_int32 * 3), ("lr_unit_shift", C.c_int32), ("lr_uv_shift", C.c_int32), ("lr_units", C.c_void_p * 3),
                ("reduced_tx_set", C.c_int32), ("disable_cdf_update", C.c_int32), ("tile_cols_log2", C.c_int32),
                ("tile_rows_log2", C.c_int32), ("y_mode", C.c_void_p), ("angle_y", C.c_void_p), ("uv_mode", C.c_void_p),
                ("angle_uv", C.c_void_p), ("cfl_alpha", C.c_void_p), ("skip", C.c_void_p), ("tx_type", C.c_void_p),
                ("is_inter", C.c_void_p), ("mv", C.c_void_p), ("lev_y", C.c_void_p), ("lev_u", C.c_void_p), ("lev_v", C.c_void_p),
                ("visible_width", C.c_int32), ("visible_height", C.c_int32), ("film_grain_present", C.c_int32), ("film_grain", C.c_void_p), ("colour", C.c_void_p)]


class Colour(C.Structure):
    """av1mi_colour (include/av1mi_host.h): the colour description and HDR10 static metadata of a stream; Colour() is all-unspecified"""
    _fields_ = [("primaries", C.c_int32), ("transfer", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32), ("have_mdcv", C.c_int32),
                ("primary_x", C.c_uint16 * 3), ("primary_y", C.c_uint16 * 3), ("white_x", C.c_uint16), ("white_y", C.c_uint16),
                ("luminance_max", C.c_uint32), ("luminance_min", C.c_uint32), ("have_cll", C.c_int32), ("max_cll", C.c_uint16), ("max_fall", C.c_uint16)]

    def __init__(self, primaries=2, transfer=2, matrix=2, full_range=0, mdcv=None, cll=None):
        """mdcv: ((rx, ry), (gx, gy), (bx, by), (wx, wy), luminance_max, luminance_min) in the record's fixed point; cll: (max_cll, max_fall)"""
        super().__init__()
        self.primaries, self.transfer, self.matrix, self.full_range = primaries, transfer, matrix, full_range
        if mdcv is not None:
            self.have_mdcv = 1
            for i in range(3):
                self.primary_x[i], self.primary_y[i] = mdcv[i]
            (self.white_x, self.white_y), self.luminance_max, self.luminance_min = mdcv[3], mdcv[4], mdcv[5]
        if cll is not None:
            self.have_cll, self.max_cll, self.max_fall = 1, cll[0], cll[1]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_HOST):
            subprocess.check_call(["make", "-s", "-C", os.path.dirname(_HOST)])
        _lib = C.CDLL(_HOST)
        _lib.av1mi_obu_write_temporal_unit.restype = C.c_longlong
        _lib.av1mi_obu_write_temporal_unit.argtypes = [C.POINTER(ObuFrame), C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_char_p, C.c_int]
        _lib.av1mi_host_opstream_temporal_unit.restype = C.c_longlong
        _lib.av1mi_host_opstream_temporal_unit.argtypes = [C.POINTER(ObuFrame), C.c_int, C.c_void_p, C.c_longlong, C.c_char_p, C.c_int]
    return _lib


_PTR_FIELDS = {"cdef_idx": np.uint8, "y_mode": np.uint8, "angle_y": np.int8, "uv_mode": np.uint8, "angle_uv": np.int8, "cfl_alpha": np.int8,
               "skip": np.uint8, "tx_type": np.uint8, "is_inter": np.uint8, "mv": np.int16, "lev_y": np.int16, "lev_u": np.int16,
               "lev_v": np.int16}


def temporal_unit(width, height, bit_depth, base_q_idx, frame_type=0, with_sequence_header=True, threads=1, lf_level=(0, 0, 0, 0),
                  lf_sharpness=0, cdef_damping=3, cdef_bits=0, cdef_y=(0,), cdef_uv=(0,), lr_type=(0, 0, 0), lr_unit_shift=0, lr_uv_shift=0,
                  lr_units=(None, None, None), reduced_tx_set=0, disable_cdf_update=0, tile_cols_log2=-1, tile_rows_log2=-1, opstream=False,
                  visible=None, key_rows32=0, film_grain=None, film_grain_present=None, colour=None, **arrays):
    """arrays: y_mode, angle_y, uv_mode, angle_uv, cfl_alpha, skip, tx_type, is_inter, mv, lev_y, lev_u, lev_v, cdef_idx (numpy, raster
    order over 8x8 blocks; see av1_bitstream.hpp).  visible: (width, height) a decoder outputs when the coded size is the source's rounded up to 8.
    film_grain: a FilmGrain the frame header carries; film_grain_present: the sequence's flag (None = set iff film_grain is given).
    Returns bytes."""
    f = ObuFrame()
    _set_film_grain(f, film_grain, film_grain_present)
    f.colour = C.addressof(colour) if colour is not None else None      # (a Colour: the stream's description, read where a sequence header is written)
    f.width, f.height, f.bit_depth, f.frame_type, f.base_q_idx = width, height, bit_depth, frame_type, base_q_idx
    if visible is not None:
        f.visible_width, f.visible_height = int(visible[0]), int(visible[1])
    for i in range(4):
        f.lf_level[i] = int(lf_level[i])
    f.lf_sharpness, f.cdef_damping, f.cdef_bits = lf_sharpness, cdef_damping, cdef_bits
    for i, v in enumerate(cdef_y):
        f.cdef_y[i] = int(v)
    for i, v in enumerate(cdef_uv):
        f.cdef_uv[i] = int(v)
    keep = []
    for p in range(3):
        f.lr_type[p] = int(lr_type[p])
        if lr_units[p] is not None:
            a = np.ascontiguousarray(lr_units[p], np.int8)
            keep.append(a)
            f.lr_units[p] = a.ctypes.data
    f.lr_unit_shift, f.lr_uv_shift = lr_unit_shift, lr_uv_shift
    f.reduced_tx_set, f.disable_cdf_update, f.tile_cols_log2, f.tile_rows_log2 = reduced_tx_set, disable_cdf_update, tile_cols_log2, tile_rows_log2
    for k, v in arrays.items():
        if k not in _PTR_FIELDS:
            raise TypeError("unknown field " + k)
        if v is None:
            continue
        a = np.ascontiguousarray(v, _PTR_FIELDS[k])
        keep.append(a)
        setattr(f, k, a.ctypes.data)
    cap = width * height * 4 + (1 << 16)
    out = np.empty(cap, np.uint8)
    err = C.create_string_buffer(256)
    if opstream:    # the op-stream formulation (the GPU tile coder's CPU twin, host/av1_opstream.cpp): must give the same bytes
        # key_rows32: a key frame whose first rows are coded in 32x32 blocks, arrays in the session's layout (host/av1_opstream.cpp)
        h = lib()
        h.av1mi_host_opstream_key32_temporal_unit.restype = C.c_longlong
        h.av1mi_host_opstream_key32_temporal_unit.argtypes = [C.POINTER(ObuFrame), C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_char_p, C.c_int]
        n = h.av1mi_host_opstream_key32_temporal_unit(C.byref(f), int(key_rows32), int(with_sequence_header), out.ctypes.data, cap, err, 256)
    else:
        n = lib().av1mi_obu_write_temporal_unit(C.byref(f), int(with_sequence_header), threads, out.ctypes.data, cap, err, 256)
    if n < 0:
        raise ValueError("av1 bitstream writer: " + err.value.decode())
    if n > cap:
        raise RuntimeError("temporal unit of %d bytes exceeds the buffer" % n)
    return out[:n].tobytes()


BLOCK_DTYPE = np.dtype([("mi_row", "<u2"), ("mi_col", "<u2"), ("bsize", "u1"), ("skip", "u1"), ("is_inter", "u1"), ("y_mode", "u1"), ("uv_mode", "u1"),
                        ("angle_y", "i1"), ("angle_uv", "i1"), ("cfl_alpha_u", "i1"), ("cfl_alpha_v", "i1"), ("tx_depth", "u1"), ("interp_filter", "u1"),
                        ("reserved", "u1"), ("mv_x", "<i2"), ("mv_y", "<i2"), ("tx_type_off", "<u4"), ("lev_off", "<u4", (3,))])
assert BLOCK_DTYPE.itemsize == 36      # struct av1mi_obu_block (include/av1mi_host.h)


class ObuBlocks(C.Structure):
    _fields_ = [("hdr", ObuFrame), ("tx_mode_select", C.c_int32), ("interp_filter", C.c_int32), ("high_precision_mv", C.c_int32), ("partition", C.c_void_p), ("n_partition", C.c_size_t),
                ("blocks", C.c_void_p), ("n_blocks", C.c_size_t), ("tx_type", C.c_void_p), ("levels", C.c_void_p)]


def blocks_temporal_unit(width, height, bit_depth, base_q_idx, partition, blocks, tx_type, levels, frame_type=0, with_sequence_header=True,
                         tx_mode_select=0, interp_filter=0, high_precision_mv=0, reduced_tx_set=0, disable_cdf_update=0, tile_cols_log2=-1,
                         tile_rows_log2=-1, lf_level=(0, 0, 0, 0), lf_sharpness=0, cdef_damping=3, cdef_bits=0, cdef_y=(0,), cdef_uv=(0,), cdef_idx=None,
                         lr_type=(0, 0, 0), lr_units=(None, None, None), lr_unit_shift=0, lr_uv_shift=0, colour=None, visible=None):
    """the general block-structured writer (av1mi_obu_write_blocks_temporal_unit): partition = uint8 partition types in decoding order,
    blocks = array of BLOCK_DTYPE in decoding order, tx_type = uint8 per luma transform block, levels = int16 (see include/av1mi_host.h)"""
    d = ObuBlocks()
    f = d.hdr
    f.width, f.height, f.bit_depth, f.frame_type, f.base_q_idx = width, height, bit_depth, frame_type, base_q_idx
    f.colour = C.addressof(colour) if colour is not None else None
    if visible is not None:
        f.visible_width, f.visible_height = int(visible[0]), int(visible[1])
    for i in range(4):
        f.lf_level[i] = int(lf_level[i])
    f.lf_sharpness, f.cdef_damping, f.cdef_bits = lf_sharpness, cdef_damping, cdef_bits
    for i, v in enumerate(cdef_y):
        f.cdef_y[i] = int(v)
    for i, v in enumerate(cdef_uv):
        f.cdef_uv[i] = int(v)
    f.reduced_tx_set, f.disable_cdf_update, f.tile_cols_log2, f.tile_rows_log2 = reduced_tx_set, disable_cdf_update, tile_cols_log2, tile_rows_log2
    keep = [np.ascontiguousarray(partition, np.uint8), np.ascontiguousarray(blocks, BLOCK_DTYPE), np.ascontiguousarray(tx_type, np.uint8),
            np.ascontiguousarray(levels, np.int16)]
    if cdef_idx is not None:
        keep.append(np.ascontiguousarray(cdef_idx, np.uint8))
        f.cdef_idx = keep[-1].ctypes.data
    for p in range(3):
        f.lr_type[p] = int(lr_type[p])
        if lr_units[p] is not None:
            keep.append(np.ascontiguousarray(lr_units[p], np.int8))
            f.lr_units[p] = keep[-1].ctypes.data
    f.lr_unit_shift, f.lr_uv_shift = lr_unit_shift, lr_uv_shift
    d.tx_mode_select, d.interp_filter, d.high_precision_mv = int(tx_mode_select), int(interp_filter), int(high_precision_mv)
    d.partition, d.n_partition, d.blocks, d.n_blocks = keep[0].ctypes.data, keep[0].size, keep[1].ctypes.data, keep[1].size
    d.tx_type, d.levels = keep[2].ctypes.data, keep[3].ctypes.data
    cap = width * height * 4 + (1 << 16)
    out = np.empty(cap, np.uint8)
    err = C.create_string_buffer(256)
    L = lib()
    L.av1mi_obu_write_blocks_temporal_unit.restype = C.c_longlong
    L.av1mi_obu_write_blocks_temporal_unit.argtypes = [C.POINTER(ObuBlocks), C.c_int, C.c_void_p, C.c_longlong, C.c_char_p, C.c_int]
    n = L.av1mi_obu_write_blocks_temporal_unit(C.byref(d), int(with_sequence_header), out.ctypes.data, cap, err, 256)
    if n < 0:
        raise ValueError("av1 block writer: " + err.value.decode())
    if n > cap:
        raise RuntimeError("temporal unit of %d bytes exceeds the buffer" % n)
    return out[:n].tobytes()


def assemble_temporal_unit(width, height, bit_depth, base_q_idx, payloads, sizes, with_sequence_header=True, **hdr):
    """temporal unit around tile payloads coded on the GPU (av1mi_obu_assemble_temporal_unit); hdr = header_from_params(...)"""
    f = ObuFrame()
    _set_film_grain(f, hdr.get("film_grain"), hdr.get("film_grain_present"))
    f.width, f.height, f.bit_depth, f.base_q_idx = width, height, bit_depth, base_q_idx
    if hdr.get("visible") is not None:
        f.visible_width, f.visible_height = int(hdr["visible"][0]), int(hdr["visible"][1])
    f.frame_type = hdr.get("frame_type", 0)
    for i in range(4):
        f.lf_level[i] = int(hdr.get("lf_level", (0,) * 4)[i])
    f.lf_sharpness, f.cdef_damping, f.cdef_bits = hdr.get("lf_sharpness", 0), hdr.get("cdef_damping", 3), int(hdr.get("cdef_bits", 0))
    for i, v in enumerate(hdr.get("cdef_y", (0,))):      # (the header lists the sets; the tiles carry the indices)
        f.cdef_y[i] = int(v)
    for i, v in enumerate(hdr.get("cdef_uv", (0,))):
        f.cdef_uv[i] = int(v)
    keep = []
    for p in range(3):
        f.lr_type[p] = int(hdr.get("lr_type", (0, 0, 0))[p])
        u = hdr.get("lr_units", (None,) * 3)[p]
        if u is not None:
            a = np.ascontiguousarray(u, np.int8)
            keep.append(a)
            f.lr_units[p] = a.ctypes.data
    f.lr_unit_shift, f.lr_uv_shift = hdr.get("lr_unit_shift", 0), hdr.get("lr_uv_shift", 0)
    f.tile_cols_log2 = f.tile_rows_log2 = -1
    pay = np.ascontiguousarray(payloads, np.uint8)
    sz = np.ascontiguousarray(sizes, np.uint32)
    cap = int(pay.size) + (1 << 16) + 4 * int(sz.size)
    out = np.empty(cap, np.uint8)
    err = C.create_string_buffer(256)
    L = lib()
    L.av1mi_obu_assemble_temporal_unit.restype = C.c_longlong
    L.av1mi_obu_assemble_temporal_unit.argtypes = [C.POINTER(ObuFrame), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_char_p, C.c_int]
    n = L.av1mi_obu_assemble_temporal_unit(C.byref(f), pay.ctypes.data, sz.ctypes.data, int(sz.size), int(with_sequence_header), out.ctypes.data, cap, err, 256)
    if n < 0 or n > cap:
        raise ValueError("assemble: " + err.value.decode())
    return out[:n].tobytes()


def _session_cdef(frame, seg, with_indices):
    """a CDEF-search session's part of the header: cdef_bits and the batch's strength sets, and (host writer) the segment's indices"""
    if not frame.get("cdef_bits"):
        return {}
    n = 1 << frame["cdef_bits"]
    hdr = dict(cdef_bits=frame["cdef_bits"], cdef_y=tuple(frame["cdef_y"][:n]), cdef_uv=tuple(frame["cdef_uv"][:n]))
    if with_indices:
        hdr["cdef_idx"] = frame["cdef_idx"][seg]
    return hdr


def session_frame_unit_gpu(width, height, bit_depth, frame, seg, with_sequence_header=None, visible=None, film_grain=None, film_grain_present=None):
    """the temporal unit of segment `seg` of a collected batch whose tiles were entropy-coded on the GPU (gpu_entropy != 0)"""
    p = frame["params"]
    hdr = header_from_params(p, width, height, frame["lr_on"][seg], visible)
    hdr.update(_session_cdef(frame, seg, False))
    hdr.update(film_grain=film_grain, film_grain_present=film_grain_present)
    nt = frame["tiles_per_frame"]
    sizes = frame["tile_size"][seg * nt:(seg + 1) * nt]
    start = int(frame["tile_size"][:seg * nt].sum(dtype=np.uint64))
    pay = frame["tile_payload"][start:start + int(sizes.sum(dtype=np.uint64))]
    sh = (p.frame_type == 0) if with_sequence_header is None else with_sequence_header
    return assemble_temporal_unit(width, height, bit_depth, p.base_q_idx, pay, sizes, with_sequence_header=sh, **hdr)


def film_grain_from_records(records, bit_depth, frame_index):
    """av1mi_film_grain_from_records: one frame's grain records (av1mi.GRAIN_DTYPE [3, GRAIN_BINS], e.g. collect()["grain"][seg]) -> FilmGrain"""
    h = lib()
    h.av1mi_film_grain_from_records.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(FilmGrain)]
    rec = np.ascontiguousarray(records)
    assert rec.shape == (3, 16) and rec.dtype.itemsize == 16
    g = FilmGrain()
    if h.av1mi_film_grain_from_records(rec.ctypes.data, int(bit_depth), int(frame_index), C.byref(g)):
        raise ValueError("av1mi_film_grain_from_records: bad argument")
    return g


def film_grain_from_records_ar(records, cov, bit_depth, frame_index, lag):
    """av1mi_film_grain_from_records_ar: one frame's grain records and covariance records (int64 [3, 4, 13], or av1mi.GRAIN_COV_DTYPE [3],
    e.g. collect()["grain_cov"][seg]) -> FilmGrain with autoregressive coefficients of up to `lag`"""
    h = lib()
    h.av1mi_film_grain_from_records_ar.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FilmGrain)]
    rec = np.ascontiguousarray(records)
    assert rec.shape == (3, 16) and rec.dtype.itemsize == 16
    cv = np.ascontiguousarray(cov)
    cv = np.ascontiguousarray(cv["sum"] if cv.dtype.names else cv, np.int64)
    assert cv.shape == (3, 4, 13)
    g = FilmGrain()
    if h.av1mi_film_grain_from_records_ar(rec.ctypes.data, cv.ctypes.data, int(bit_depth), int(frame_index), int(lag), C.byref(g)):
        raise ValueError("av1mi_film_grain_from_records_ar: bad argument")
    return g


def film_grain_mid_grey(g):
    h = lib()
    h.av1mi_film_grain_mid_grey.argtypes = [C.POINTER(FilmGrain)]
    return h.av1mi_film_grain_mid_grey(C.byref(g))


def session_temporal_unit(width, height, bit_depth, raw_frame, seg, with_sequence_header=True, threads=1, visible=None, film_grain=None, film_grain_present=None):
    """av1mi_session_temporal_unit (include/av1mi_host.h): the temporal unit of segment `seg` of a collected batch, from the raw
    av1mi_gop_frame (av1mi.GopSession.collect()["raw"]) — whichever coder produced it, whatever the key frames' block size.  With
    film_grain / film_grain_present: av1mi_session_temporal_unit_grain"""
    if film_grain is not None or film_grain_present:
        return _session_temporal_unit_grain(width, height, bit_depth, raw_frame, seg, with_sequence_header, threads, visible, film_grain, film_grain_present)
    h = lib()
    h.av1mi_session_temporal_unit.restype = C.c_longlong
    h.av1mi_session_temporal_unit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_longlong,
                                              C.c_char_p, C.c_int]
    cap = width * height * 4 + (1 << 16)
    out = np.empty(cap, np.uint8)
    err = C.create_string_buffer(256)
    vw, vh = visible if visible is not None else (0, 0)
    n = h.av1mi_session_temporal_unit(C.addressof(raw_frame), int(seg), width, height, bit_depth, int(vw), int(vh), int(with_sequence_header), int(threads),
                                      out.ctypes.data, cap, err, 256)
    if n < 0:
        raise ValueError("av1mi_session_temporal_unit: " + err.value.decode())
    return out[:n].tobytes()


def _session_temporal_unit_grain(width, height, bit_depth, raw_frame, seg, with_sequence_header, threads, visible, film_grain, film_grain_present):
    h = lib()
    h.av1mi_session_temporal_unit_grain.restype = C.c_longlong
    h.av1mi_session_temporal_unit_grain.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.c_void_p, C.c_void_p, C.c_longlong, C.c_char_p, C.c_int]
    cap = width * height * 4 + (1 << 16)
    out = np.empty(cap, np.uint8)
    err = C.create_string_buffer(256)
    vw, vh = visible if visible is not None else (0, 0)
    present = int(film_grain is not None if film_grain_present is None else film_grain_present)
    n = h.av1mi_session_temporal_unit_grain(C.addressof(raw_frame), int(seg), width, height, bit_depth, int(vw), int(vh), int(with_sequence_header), int(threads),
                                            present, C.addressof(film_grain) if film_grain is not None else None, out.ctypes.data, cap, err, 256)
    if n < 0:
        raise ValueError("av1mi_session_temporal_unit_grain: " + err.value.decode())
    return out[:n].tobytes()


SCENECUT_DEFAULT = 15      # host/sceneplan.hpp AV1MI_SCENECUT_DEFAULT


def scene_is_cut(rec, scenecut):
    """the cut rule on one scene record (a numpy record of av1mi.SCENE_DTYPE): av1mi_scene_is_cut"""
    h = lib()
    h.av1mi_scene_is_cut.argtypes = [C.c_void_p, C.c_int]
    a = np.ascontiguousarray(rec).reshape(1).copy()
    return bool(h.av1mi_scene_is_cut(a.ctypes.data, int(scenecut)))


def plan_gops(n, G, S, cut, min_len=0):
    """av1mi_plan_gops (host/sceneplan.hpp): the GOPs of a window of n <= S G frames with cut[f] != 0 marking cuts -> (K, start [S], len [S]);
    ValueError where the planner refuses its arguments"""
    h = lib()
    h.av1mi_plan_gops.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3
    c = np.zeros(max(int(n), 1), np.uint8)
    c[:len(cut)] = np.asarray(cut, np.uint8)[:len(c)]
    start, ln = np.full(max(S, 1), -7, np.int32), np.full(max(S, 1), -7, np.int32)
    K = h.av1mi_plan_gops(int(n), int(G), int(S), int(min_len), c.ctypes.data, start.ctypes.data, ln.ctypes.data)
    if K < 0:
        raise ValueError("av1mi_plan_gops(n %d, G %d, S %d, min_len %d) refused" % (n, G, S, min_len))
    return K, start, ln


DEINTERLACE_MODES = ("off", "auto", "tff", "bff")      # BackendJob::deinterlace, -av1mi_deinterlace


def y4m_interlace(path):
    """the I parameter of a Y4M header as the host's reader keeps it: "p" (Ip, I? or absent), "t", "b" or "m"; ValueError when the file
    does not open"""
    h = lib()
    h.av1mi_host_y4m_interlace.argtypes = [C.c_char_p]
    k = h.av1mi_host_y4m_interlace(str(path).encode())
    if k < 0:
        raise ValueError("not a Y4M source: %s" % path)
    return "ptbm"[k]


def parse_deinterlace_option(argv):
    """what an argument vector asks of the deinterlacer (-av1mi_deinterlace, or a deinterlacing filter in the chain): one of
    DEINTERLACE_MODES; ValueError with the host's text where the vector is refused"""
    h = lib()
    h.av1mi_host_parse_deinterlace_option.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    err = C.create_string_buffer(1024)
    k = h.av1mi_host_parse_deinterlace_option("\n".join(str(x) for x in argv).encode(), err, 1024)
    if k < 0:
        raise ValueError(err.value.decode())
    return DEINTERLACE_MODES[k]


DEINTERLACE_RATES = ("frame", "field")      # BackendJob::deint_rate, -av1mi_deinterlace_rate


def parse_deinterlace_rate(argv):
    """what an argument vector asks of -av1mi_deinterlace_rate: one of DEINTERLACE_RATES; ValueError with the host's text where the vector
    is refused"""
    h = lib()
    h.av1mi_host_parse_deinterlace_rate.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    err = C.create_string_buffer(1024)
    k = h.av1mi_host_parse_deinterlace_rate("\n".join(str(x) for x in argv).encode(), err, 1024)
    if k < 0:
        raise ValueError(err.value.decode())
    return DEINTERLACE_RATES[k]


def job_output(argv, interlace, fps, frames):
    """the output of the job of an argument vector (host/fieldrate.hpp JobOutputOf) on a source with the Y4M I parameter `interlace` ("p",
    "t", "b", "m"), the rate fps = (n, d) and `frames` frames (-1 = a stream): (output frames per source frame, (fps_n, fps_d), frames)"""
    h = lib()
    h.av1mi_host_job_output.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    err, out = C.create_string_buffer(1024), (C.c_longlong * 4)()
    if h.av1mi_host_job_output("\n".join(str(x) for x in argv).encode(), "ptbm".index(interlace), int(fps[0]), int(fps[1]), int(frames), out, err, 1024) < 0:
        raise ValueError(err.value.decode())
    return int(out[0]), (int(out[1]), int(out[2])), int(out[3])


def field_rate_cuts(cut):
    """the cut flags of n source frames as the 2 n output frames of a field-rate job carry them (host/fieldrate.hpp FieldRateCuts)"""
    h = lib()
    h.av1mi_host_field_rate_cuts.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    h.av1mi_host_field_rate_cuts.restype = None
    c = np.ascontiguousarray(cut, np.uint8)
    out = np.full(2 * c.size, 7, np.uint8)
    h.av1mi_host_field_rate_cuts(c.ctypes.data, int(c.size), out.ctypes.data)
    return out


def job_output_ratio(argv, interlace, fps, frames):
    """job_output() with the ratio: (output frames per source frame, (fps_n, fps_d), frames, (num, den)): num output frames per den source
    frames, 4 / 5 for a job with -av1mi_ivtc 1"""
    h = lib()
    h.av1mi_host_job_output_ratio.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    err, out = C.create_string_buffer(1024), (C.c_longlong * 6)()
    if h.av1mi_host_job_output_ratio("\n".join(str(x) for x in argv).encode(), "ptbm".index(interlace), int(fps[0]), int(fps[1]), int(frames), out, err, 1024) < 0:
        raise ValueError(err.value.decode())
    return int(out[0]), (int(out[1]), int(out[2])), int(out[3]), (int(out[4]), int(out[5]))


def parse_ivtc_option(argv):
    """what an argument vector asks of -av1mi_ivtc: 0 or 1; ValueError with the host's text where the vector is refused"""
    h = lib()
    h.av1mi_host_parse_ivtc_option.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    err = C.create_string_buffer(1024)
    k = h.av1mi_host_parse_ivtc_option("\n".join(str(x) for x in argv).encode(), err, 1024)
    if k < 0:
        raise ValueError(err.value.decode())
    return k


def plan_telecine(records, front=0, back=0):
    """av1mi_plan_telecine (host/telecineplan.hpp): the records of a run (av1mi.TELECINE_DTYPE layout: comb [3], bdiff, uint64) whose first
    `front` and last `back` frames are context -> (top, bottom): the run positions every output frame is woven from; ValueError where the
    planner refuses its arguments"""
    h = lib()
    h.av1mi_plan_telecine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    r = np.ascontiguousarray(records)
    assert r.dtype.itemsize == 32
    n = len(r) - int(front) - int(back)
    top, bottom = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.int32)
    k = h.av1mi_plan_telecine(r.ctypes.data, len(r), int(front), int(back), top.ctypes.data, bottom.ctypes.data)
    if k < 0:
        raise ValueError("av1mi_plan_telecine(%d frames, front %d, back %d) refused" % (len(r), front, back))
    return top[:k].copy(), bottom[:k].copy()


def plan_denoise(records):
    """av1mi_plan_denoise (host/noiseplan.hpp): noise records (av1mi.NOISE_DTYPE layout) -> (strength 0 .. 16, the pairs' levels (-1 = not
    valid), the file's sigma in 1/16 of an 8-bit code (-1 = no valid pair))"""
    h = lib()
    h.av1mi_plan_denoise.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    r = np.ascontiguousarray(records)
    assert r.dtype.itemsize == 1032
    q, s16 = np.full(max(len(r), 1), -7, np.int32), np.full(1, -7, np.int32)
    k = h.av1mi_plan_denoise(r.ctypes.data if len(r) else None, len(r), q.ctypes.data, s16.ctypes.data)
    if k < 0:
        raise ValueError("av1mi_plan_denoise(%d pairs) refused" % len(r))
    return k, q[:len(r)].copy(), int(s16[0])


def plan_peak(records):
    """av1mi_plan_peak (host/peakplan.hpp): peak records (av1mi.PEAK_DTYPE layout) -> (the tone map's source peak in cd/m2, 400 .. 10000,
    the frames' codes)"""
    h = lib()
    h.av1mi_plan_peak.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    r = np.ascontiguousarray(records)
    assert r.dtype.itemsize == 4100
    codes = np.full(max(len(r), 1), -7, np.int32)
    peak = h.av1mi_plan_peak(r.ctypes.data if len(r) else None, len(r), codes.ctypes.data)
    if peak < 0:
        raise ValueError("av1mi_plan_peak(%d frames) refused" % len(r))
    return peak, codes[:len(r)].copy()


def peak_sample_slots(frames):
    """the frames -av1mi_tonemap_peak auto samples in a file of `frames` frames (the crop sampler's slots)"""
    h = lib()
    h.av1mi_host_peak_sample_slots.argtypes = [C.c_longlong, C.c_void_p]
    slots = np.full(32, -7, np.int32)
    return slots[:h.av1mi_host_peak_sample_slots(int(frames), slots.ctypes.data)].tolist()


def parse_peak_options(argv):
    """what an argument vector asks of the tone map: dict(tonemap, peak, auto); ValueError with the host's text where the vector is refused"""
    h = lib()
    h.av1mi_host_parse_peak_options.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    err, out = C.create_string_buffer(1024), (C.c_int * 3)()
    if h.av1mi_host_parse_peak_options("\n".join(str(x) for x in argv).encode(), out, err, 1024) < 0:
        raise ValueError(err.value.decode())
    return dict(zip(("tonemap", "peak", "auto"), (int(v) for v in out)))


def noise_pair_slots(frames):
    """the pair slots -av1mi_denoise auto samples in a file of `frames` frames (pair slot s = frames 2 s and 2 s + 1)"""
    h = lib()
    h.av1mi_host_noise_pair_slots.argtypes = [C.c_longlong, C.c_void_p]
    slots = np.full(16, -7, np.int32)
    return slots[:h.av1mi_host_noise_pair_slots(int(frames), slots.ctypes.data)].tolist()


def parse_denoise_options(argv):
    """what an argument vector asks of the denoiser: dict(denoise, auto, range, film_grain, grain_lag); ValueError with the host's text where
    the vector is refused"""
    h = lib()
    h.av1mi_host_parse_denoise_options.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    err, out = C.create_string_buffer(1024), (C.c_int * 5)()
    if h.av1mi_host_parse_denoise_options("\n".join(str(x) for x in argv).encode(), out, err, 1024) < 0:
        raise ValueError(err.value.decode())
    return dict(zip(("denoise", "auto", "range", "film_grain", "grain_lag"), (int(v) for v in out)))


def run_transcode_report(argv):
    """run_transcode() with the job's report: (exit code, error text, the strength -av1mi_denoise auto planned or -1)"""
    h = lib()
    h.av1mi_host_run_transcode_report.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    buf, planned = C.create_string_buffer(2048), C.c_int(-7)
    code = h.av1mi_host_run_transcode_report("\n".join(str(x) for x in argv).encode(), buf, 2048, C.byref(planned))
    return code, buf.value.decode(), int(planned.value)


def run_transcode(argv):
    """av1mi_run_transcode (include/av1mi_host.h) on an argument vector: (exit code, error text)"""
    h = lib()
    h.av1mi_run_transcode.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t]
    a = [str(x).encode() for x in argv]
    buf = C.create_string_buffer(2048)
    code = h.av1mi_run_transcode(len(a), (C.c_char_p * len(a))(*a), buf, 2048)
    return code, buf.value.decode()


def header_from_params(p, width, height, lr_on=None, visible=None):
    """keyword arguments of temporal_unit() for a frame whose filter parameters are an av1mi_frame_params (GOP session policy);
    lr_on: the encoder's restoration ON / OFF decision per plane (the session's frame["lr_on"][segment]; None = the policy's types);
    visible: the true (width, height) when the coded size is rounded up to 8 (the restoration units tile the TRUE frame)"""
    ur = lambda n: max(1, (n + p.lr_unit_size // 2) // p.lr_unit_size)
    vw, vh = visible if visible is not None else (width, height)
    uy = np.tile(np.array(list(p.lr_unit_y), np.int8), (ur(vh), ur(vw), 1))
    uc = np.tile(np.array(list(p.lr_unit_uv), np.int8), (ur((vh + 1) // 2), ur((vw + 1) // 2), 1))
    shift = {64: 0, 128: 1, 256: 2}[p.lr_unit_size]
    types = [int(p.lr_unit_y[0]), int(p.lr_unit_uv[0]), int(p.lr_unit_uv[0])]
    if lr_on is not None:
        types = [t if int(k) else 0 for t, k in zip(types, lr_on)]
    return dict(frame_type=p.frame_type, lf_level=tuple(p.lf_level), lf_sharpness=p.lf_sharpness, cdef_damping=p.cdef_damping,
                cdef_y=(p.cdef_y,), cdef_uv=(p.cdef_uv,), lr_type=tuple(types), lr_unit_shift=shift, lr_uv_shift=0, lr_units=(uy, uc, uc),
                **({} if visible is None else {"visible": (int(vw), int(vh))}))


def session_frame_unit(width, height, bit_depth, frame, seg, with_sequence_header=None, threads=1, visible=None, film_grain=None, film_grain_present=None):
    """the temporal unit of segment `seg` of a collected GOP-session batch (av1mi.GopSession.collect())"""
    p = frame["params"]
    hdr = header_from_params(p, width, height, frame["lr_on"][seg], visible)
    hdr.update(film_grain=film_grain, film_grain_present=film_grain_present)
    hdr.update(_session_cdef(frame, seg, True))
    if p.frame_type == 0:
        sym = dict(y_mode=frame["y_mode"][seg], uv_mode=frame["uv_mode"][seg])
    else:
        sym = dict(mv=frame["mv"][seg], skip=frame["skip"][seg])
    sh = (p.frame_type == 0) if with_sequence_header is None else with_sequence_header
    return temporal_unit(width, height, bit_depth, p.base_q_idx, with_sequence_header=sh, threads=threads, lev_y=frame["lev_y"][seg],
                         lev_u=frame["lev_u"][seg], lev_v=frame["lev_v"][seg], **sym, **hdr)
