"""The coder's tail is ONE launch (csrc/av1_entropy_kernels.hip): k_av1_code leaves a sum per group of 64 tiles, every workgroup of
k_av1_gather finds its tile's offset from those sums and the sizes of its own group, the last tile's workgroup writes total and status,
and in a GOP session the same launch stores sizes, total, status and the restoration flags into the slot's pinned mirrors.

Tile counts on either side of the group size — 60 (one partial group), 72 (a full group and a partial one), 64 (exactly one group) —
a key batch and a P batch of each: the session with gpu_entropy = 1 against the host writer on the symbols of a host-mode session, byte
for byte, and through dav1d where present; the same symbols through av1mi_av1_entropy_encode with device pointers only (sizes and total
equal the session's); and a job whose out_cap is one byte short of the total (status 4, nothing written at or past out_cap, every tile
that fits written)."""
import ctypes as C

import numpy as np
import pytest

import dav1d_ref as D
from test_gpu_chains_order import EntropyJob

pytestmark = pytest.mark.gpu

GUARD = 0xEE


def _device_job(ctx, w, h, S, fr, short=0, expect=None):
    """the batch `fr` (symbols on the host, collected from a host-mode session) through av1mi_av1_entropy_encode, device pointers only.
    short: out_cap = total - short (expect = the sizes and payload of the whole job).  Returns (sizes, total, status, the output buffer)"""
    p = fr["params"]
    key = p.frame_type == 0
    names = ("lev_y", "lev_u", "lev_v") + (("y_mode", "uv_mode") if key else ("mv", "skip"))
    dev = {k: ctx.to_device(np.ascontiguousarray(fr[k]).reshape(-1)) for k in names}
    tiles = ((w + 63) // 64) * ((h + 63) // 64)
    room = S * tiles * (1 << 14)
    cap = room if expect is None else int(expect[1]) - short
    d_out = ctx.to_device(np.full(room + 64, GUARD, np.uint8))
    d_size, d_total = ctx.alloc(S * tiles * 4), ctx.alloc(16)
    d_on = ctx.to_device(np.concatenate([np.ascontiguousarray(fr["lr_on"], np.uint8).reshape(-1), np.zeros(4, np.uint8)]))
    j = EntropyJob()
    j.width, j.height, j.nframes, j.key, j.base_q_idx = w, h, S, int(key), p.base_q_idx
    j.d_lev_y, j.d_lev_u, j.d_lev_v = dev["lev_y"].ptr, dev["lev_u"].ptr, dev["lev_v"].ptr
    if key:
        j.d_modes_y, j.d_modes_uv = dev["y_mode"].ptr, dev["uv_mode"].ptr
    else:
        j.d_mvs, j.d_skip = dev["mv"].ptr, dev["skip"].ptr
    j.lr_on[0], j.lr_on[1], j.lr_on[2] = int(p.lr_unit_y[0] == 1), int(p.lr_unit_uv[0] == 1), int(p.lr_unit_uv[0] == 1)
    for i in range(8):
        j.lr_unit_y[i], j.lr_unit_uv[i] = p.lr_unit_y[i], p.lr_unit_uv[i]
    j.d_out, j.out_cap, j.d_tile_size, j.d_total, j.d_lr_on = d_out.ptr, cap, d_size.ptr, d_total.ptr, d_on.ptr
    try:
        ctx.lib.av1mi_av1_entropy_encode_on.argtypes = [C.c_void_p, C.POINTER(EntropyJob), C.c_void_p]
        ctx._chk(ctx.lib.av1mi_av1_entropy_encode_on(ctx.h, C.byref(j), None))
        ctx.sync()
        total, status = (int(v) for v in d_total.download((2,), np.uint64))
        return d_size.download((S * tiles,), np.uint32), total, status, d_out.download((room + 64,), np.uint8)
    finally:
        for b in list(dev.values()) + [d_out, d_size, d_total, d_on]:
            b.free()


@pytest.mark.parametrize("w,h,S,bd", [(256, 192, 5, 8), (256, 192, 6, 10), (512, 256, 2, 10)])
def test_one_launch_tail_equals_the_host_writer(ctx, av1mi, w, h, S, bd):
    import av1stream
    import synth
    q, gop = 128, 2
    tiles = ((w + 63) // 64) * ((h + 63) // 64)
    assert S * tiles == {5: 60, 6: 72, 2: 64}[S]
    Y, U, V = synth.frames(w, h, S * gop, bd, 21)
    a = av1mi.GopSession(ctx, w, h, bd, q, gop, S, gpu_entropy=1)
    b = av1mi.GopSession(ctx, w, h, bd, q, gop, S, gpu_entropy=0)
    try:
        streams, refs = [b""] * S, []
        for t in range(gop):      # a key batch, then a P batch
            for s in (a, b):
                planes = s.input_planes()
                for sg in range(S):
                    f = sg * gop + t
                    planes[0][sg * h:(sg + 1) * h] = Y[f]
                    planes[1][sg * h // 2:(sg + 1) * h // 2] = U[f]
                    planes[2][sg * h // 2:(sg + 1) * h // 2] = V[f]
                s.submit()
            fa, fb = a.collect(), b.collect()
            refs.append(a.download_reference())
            assert a.entropy_fallbacks() == 0 and "tile_size" in fa and "lev_y" not in fa
            assert fa["frame_type"] == (0 if t == 0 else 1) and fa["tiles_per_frame"] == tiles
            # the mirrors the gather stored: the flags the host-mode session downloaded, sizes that add up to the total
            assert fa["lr_on"].tolist() == fb["lr_on"].tolist()
            sizes, pay = fa["tile_size"].copy(), fa["tile_payload"].copy()
            assert (sizes > 0).all() and int(sizes.sum(dtype=np.uint64)) == pay.size
            for sg in range(S):
                gpu = av1stream.session_frame_unit_gpu(w, h, bd, fa, sg)
                assert gpu == av1stream.session_frame_unit(w, h, bd, fb, sg, threads=4), "batch %d segment %d: GPU coder and host writer disagree" % (t, sg)
                streams[sg] += gpu
            # device pointers only: what a caller without mirrors gets
            dsz, dtotal, dstatus, dout = _device_job(ctx, w, h, S, fb)
            assert dstatus == 0 and dtotal == pay.size and (dsz == sizes).all()
            assert (dout[:dtotal] == pay).all() and (dout[dtotal:] == GUARD).all()
            # out_cap one byte short: the last tile does not fit and is not written, every other tile is, the status says so
            csz, ctotal, cstatus, cout = _device_job(ctx, w, h, S, fb, short=1, expect=(sizes, pay.size))
            fits = pay.size - int(sizes[-1])
            assert cstatus == 4 and ctotal == pay.size and (csz == sizes).all()
            assert (cout[:fits] == pay[:fits]).all() and (cout[fits:] == GUARD).all()
        if D.available():
            for sg in range(S):
                got = D.decode(streams[sg])
                assert len(got) == gop
                for t in range(gop):
                    for i, hh in ((0, h), (1, h // 2), (2, h // 2)):
                        assert (got[t][i] == refs[t][i][sg * hh:(sg + 1) * hh]).all()
    finally:
        a.close()
        b.close()
