#!/usr/bin/env python3
"""What the one-pass rate controller (include/av1mi_rc.h, host/ratecontrol.cpp; av1mi_gop_set_base_q_idx) achieves on the bench's
configurations -> profiles/ratecontrol.json (PROF_OUT overrides the directory).

Per configuration (the bench's 4K 10-bit GOP workload and 1080p 8-bit: GOP 30, 12 / 24 segments in lockstep, key frames in 32x32
blocks, the tiles coded on the GPU, sources resident in device memory, three batches in flight) and per target in bits per pixel:
the achieved bits per pixel and its deviation from the target, the q trajectory per batch, mean PSNR-Y and frames/s — and the same
source at the FIXED quantiser nearest to the trajectory's mean, with its bytes, PSNR-Y and frames/s.  The controller is the library's
(libav1mi_host.so av1mi_rc_*) with av1mi_rc_defaults' tuning unless --tune overrides a value; bytes are tile payload bytes.

Usage: python tools/bench_ratecontrol.py [--configs 4k10,1080p8] [--targets 0.15,0.12,0.30,0.06] [--gops 6] [--start-q 128]
                                         [--tune max_step=8,window_gops=4] [--segments N]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))
import av1mi  # noqa: E402
import av1stream  # noqa: E402
import synth  # noqa: E402

CONFIGS = {"4k10": (3840, 2160, 10, 12), "1080p8": (1920, 1080, 8, 24)}
GOP = 30


class Params(C.Structure):      # av1mi_rc_params
    _fields_ = [("target_num", C.c_int64), ("target_den", C.c_int64), ("gop_length", C.c_int32), ("start_q", C.c_int32), ("qmin", C.c_int32),
                ("qmax", C.c_int32), ("bit_depth", C.c_int32), ("weight_num", C.c_int32), ("weight_den", C.c_int32), ("window_gops", C.c_int32),
                ("band_low_pct", C.c_int32), ("band_high_pct", C.c_int32), ("max_step", C.c_int32)]


def controller(host, bpp, w, h, bd, start_q, tune):
    p = Params()
    host.av1mi_rc_defaults(C.byref(p))
    p.target_num, p.target_den = int(round(bpp * 1e6)) * w * h, 8000000
    p.gop_length, p.start_q, p.bit_depth = GOP, start_q, bd
    for k, v in tune.items():
        setattr(p, k, v)
    rc, err = C.c_void_p(), C.create_string_buffer(256)
    if host.av1mi_rc_open(C.byref(p), C.byref(rc), err, 256):
        sys.exit("av1mi_rc_open: " + err.value.decode())
    return rc, {k: getattr(p, k) for k, _ in Params._fields_[5:]}


def run(ctx, host, d_src, w, h, bd, segs, gops, q, rc=None):
    """`gops` GOPs of the resident source; rc: the controller that sets every batch's quantiser, else fixed q"""
    sess = av1mi.GopSession(ctx, w, h, bd, q, GOP, segs, gpu_entropy=1, key_block_size=32, quality_stats=1)
    lag = sess.max_in_flight() - 1
    out = dict(bytes=0, frames=0, q=[], fallbacks=0)
    sse = samples = 0

    def take():
        nonlocal sse, samples
        fr = sess.collect()
        b = int(fr["raw"].payload_bytes)
        out["bytes"] += b
        out["frames"] += segs
        sse += int(fr["quality"]["sse"][:, 0].sum())
        samples += int(fr["quality"]["samples"][:, 0].sum())
        if rc is not None:
            host.av1mi_rc_collected(rc, b)
    try:
        ctx.sync()
        t0 = time.perf_counter()
        for g in range(gops):
            for t in range(GOP):
                if rc is not None:
                    qt = host.av1mi_rc_next_q(rc, 0 if t == 0 else 1, segs)
                    sess.set_q(qt)
                    out["q"].append(qt)
                sess.submit_device(d_src[t][0], d_src[t][1], d_src[t][2], 0 if t == 0 else 1)
                if sess.pending() > lag:
                    take()
        while sess.pending():
            take()
        ctx.sync()
        out["seconds"] = time.perf_counter() - t0
        out["fallbacks"] = sess.entropy_fallbacks()
    finally:
        sess.close()
    peak = float((1 << bd) - 1)
    out["psnr_y"] = float(10 * np.log10(peak * peak * samples / sse)) if sse else float("inf")
    out["frames_per_s"] = out["frames"] / out["seconds"]
    out["bpp"] = 8.0 * out["bytes"] / (out["frames"] * w * h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4k10,1080p8")
    ap.add_argument("--targets", default="0.15,0.12,0.30,0.06")
    ap.add_argument("--gops", type=int, default=6)
    ap.add_argument("--start-q", type=int, default=128)
    ap.add_argument("--segments", type=int, default=0)
    ap.add_argument("--tune", default="")
    args = ap.parse_args()
    tune = {k: int(v) for k, v in (kv.split("=") for kv in args.tune.split(",") if kv)}
    host = av1stream.lib()
    host.av1mi_rc_defaults.restype = None
    host.av1mi_rc_open.argtypes = [C.POINTER(Params), C.POINTER(C.c_void_p), C.c_char_p, C.c_int]
    host.av1mi_rc_next_q.argtypes = [C.c_void_p, C.c_int, C.c_int]
    host.av1mi_rc_collected.argtypes = [C.c_void_p, C.c_int64]
    host.av1mi_rc_close.argtypes = [C.c_void_p]
    host.av1mi_rc_close.restype = None
    result = dict(tool="tools/bench_ratecontrol.py", gop=GOP, gops=args.gops, start_q=args.start_q, configs={})
    with av1mi.Context(0) as ctx:
        result["device"] = ctx.device_name
        for name in args.configs.split(","):
            w, h, bd, segs = CONFIGS[name]
            segs = args.segments or segs
            Y, U, V = synth.frames(w, h, segs * GOP, bd, 0)
            src = [a.reshape(segs, GOP, *a.shape[1:]) for a in (Y, U, V)]
            d_src = [[ctx.to_device(np.ascontiguousarray(src[p][:, t])) for p in range(3)] for t in range(GOP)]
            del Y, U, V, src
            run(ctx, host, d_src, w, h, bd, segs, 1, args.start_q)      # warm-up
            rows = []
            for bpp in (float(x) for x in args.targets.split(",")):
                rc, tuning = controller(host, bpp, w, h, bd, args.start_q, tune)
                r = run(ctx, host, d_src, w, h, bd, segs, args.gops, args.start_q, rc)
                host.av1mi_rc_close(rc)
                mean_q = int(round(sum(r["q"]) / len(r["q"])))
                f = run(ctx, host, d_src, w, h, bd, segs, args.gops, mean_q)
                tail = r["q"][len(r["q"]) // 2:]
                rows.append(dict(target_bpp=bpp, achieved_bpp=r["bpp"], deviation=r["bpp"] / bpp - 1.0, q_per_batch=r["q"], q_second_half=[min(tail), max(tail)],
                                 psnr_y=r["psnr_y"], frames_per_s=r["frames_per_s"], bytes=r["bytes"], frames=r["frames"], entropy_fallbacks=r["fallbacks"],
                                 fixed=dict(q=mean_q, bpp=f["bpp"], bytes=f["bytes"], psnr_y=f["psnr_y"], frames_per_s=f["frames_per_s"], entropy_fallbacks=f["fallbacks"])))
                print(name, {k: v for k, v in rows[-1].items() if k != "q_per_batch"}, flush=True)
            result["configs"][name] = dict(size="%dx%d" % (w, h), bit_depth=bd, segments=segs, tuning=tuning, targets=rows)
            for t in d_src:
                for b in t:
                    b.free()
    out = os.path.join(os.environ.get("PROF_OUT", os.path.join(ROOT, "profiles")), "ratecontrol.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
