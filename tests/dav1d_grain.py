"""dav1d with film grain synthesis selectable (Dav1dSettings.apply_grain): tests/dav1d_ref.py's decoder loop with that one setting
exposed.  TEST INFRASTRUCTURE ONLY, like dav1d_ref (which always decodes with the grain off and stays as it is)."""
import ctypes

import dav1d_ref as D

available, version = D.available, D.version


def decode(obu_bytes, apply_grain):
    """decode a Section-5 OBU stream; apply_grain False = the decoded pictures, True = with the synthesised grain added on output.
    Returns a list of frames [(Y, U, V)] as numpy arrays."""
    lib = D.load()
    settings = ctypes.create_string_buffer(512)
    lib.dav1d_default_settings(settings)
    ints = ctypes.cast(settings, ctypes.POINTER(ctypes.c_int))
    assert ints[2] == 1 and ints[18] == D.INLOOP_ALL, "unexpected Dav1dSettings layout"
    ints[0], ints[1], ints[2], ints[16] = 1, 1, 1 if apply_grain else 0, 1      # n_threads, max_frame_delay, apply_grain, strict_std_compliance
    ctx = ctypes.c_void_p()
    rc = lib.dav1d_open(ctypes.byref(ctx), settings)
    if rc:
        raise RuntimeError("dav1d_open: %d" % rc)
    frames = []

    def drain():
        while True:
            pic = D._Picture()
            rc = lib.dav1d_get_picture(ctx, ctypes.byref(pic))
            if rc == D._EAGAIN:
                return
            if rc:
                raise RuntimeError("dav1d_get_picture: error %d" % rc)
            frames.append(D._planes(pic))
            lib.dav1d_picture_unref(ctypes.byref(pic))

    try:
        data = ctypes.create_string_buffer(128)     # Dav1dData
        ptr = lib.dav1d_data_create(data, len(obu_bytes))
        if not ptr:
            raise RuntimeError("dav1d_data_create failed")
        ctypes.memmove(ptr, obu_bytes, len(obu_bytes))
        szp = ctypes.cast(ctypes.addressof(data) + 8, ctypes.POINTER(ctypes.c_size_t))
        while szp[0] > 0:
            rc = lib.dav1d_send_data(ctx, data)
            if rc and rc != D._EAGAIN:
                raise RuntimeError("dav1d_send_data: error %d (stream rejected)" % rc)
            drain()
        for _ in range(4):
            drain()
    finally:
        lib.dav1d_close(ctypes.byref(ctx))
    return frames
