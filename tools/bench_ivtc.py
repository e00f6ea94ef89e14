#!/usr/bin/env python3
"""What inverse telecine (include/av1mi.h "inverse telecine", av1mi_gop_config.telecine, -av1mi_ivtc) costs on the GPU, each number beside
what it is measured against, in the same process, legs alternated, `--reps` repetitions with min / median / max:

1. The field-match records (av1mi_telecine_analyse: k_telecine_rows + k_telecine_sum) of a run of `--run` frames, 1080p 8-bit and 4K
   10-bit, HIP events around `--launches` calls: ms per run and per frame, and the rate against the algorithmic bytes (every luma sample
   of the run once).
2. The weave (av1mi_telecine_gather) against k_frames_gather — the copy it stands in for, whose code this change does not touch — on the
   same batch of 12 segments, every segment with its own two source frames in a store past the Infinity Cache: ms per batch, the ratio,
   and both rates against one read plus one write of the batch.
3. av1mi_run_transcode on a telecined 1080p clip (tests/telecine_ref.py's film, 3:2 pulldown, top field first): -av1mi_ivtc 1 against
   -av1mi_deinterlace auto and against the source coded as it is; wall clock, OUTPUT frames per second, source frames per second, bytes.

    python tools/bench_ivtc.py --out profiles/ivtc.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import av1mi          # noqa: E402
import av1stream      # noqa: E402
import telecine_ref   # noqa: E402


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def gbs(nbytes, ms):
    return nbytes / (ms * 1e-3) / 1e9


def filled(ctx, nbytes, frames, seed):
    """`frames` copies of one frame of noise in device memory: the kernels' work does not depend on the values"""
    d = ctx.alloc(nbytes * frames)
    one = av1mi.DevBuf(ctx, nbytes).upload(np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8))
    for f in range(frames):
        ctx._chk(ctx.lib.av1mi_copy(ctx.h, C.c_void_p(d.ptr + f * nbytes), C.c_void_p(one.ptr), C.c_size_t(nbytes)))
    ctx.sync()
    one.free()
    return d


def analyse_leg(ctx, W, H, bd, run, reps, launches):
    bps = 1 if bd == 8 else 2
    H8 = (H + 7) & ~7      # (1080 and 2160 are multiples of 8)
    nbytes = W * H8 * bps
    d_y, d_rec = filled(ctx, nbytes, run, W), ctx.alloc(run * av1mi.TELECINE_DTYPE.itemsize)
    ctx.lib.av1mi_telecine_analyse.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    t = []
    for rep in range(reps + 1):      # the first repetition warms up
        ctx.timer_begin()
        for _ in range(launches):
            ctx._chk(ctx.lib.av1mi_telecine_analyse(ctx.h, bd, W, H8, W, H, run, d_y.ptr, d_rec.ptr))
        ms = ctx.timer_end() / launches
        if rep:
            t.append(ms)
    d_y.free()
    d_rec.free()
    m = statistics.median(t)
    return {"width": W, "height": H, "bit_depth": bd, "run_frames": run, "run_luma_bytes": W * H * bps * run, "analyse_ms_per_run": spread(t),
            "analyse_ms_per_frame": m / run, "gb_per_s_of_the_luma_read_once": gbs(W * H * bps * run, m)}


def weave_leg(ctx, W, H, bd, segs, reps, launches):
    bps = 1 if bd == 8 else 2
    H8 = (H + 7) & ~7      # (1080 and 2160 are multiples of 8)
    sizes = [(W, H8), (W // 2, H8 // 2), (W // 2, H8 // 2)]
    true = [(W, H), (W // 2, H // 2), (W // 2, H // 2)]
    nbytes = [w * h * bps for w, h in sizes]
    frames = 2 * segs      # segment s weaves frames 2 s and 2 s + 1: no two segments share a source
    d_store = [filled(ctx, nbytes[p], frames, W + p) for p in range(3)]
    plain = np.array([[d_store[p].ptr + 2 * s * nbytes[p] for p in range(3)] for s in range(segs)], np.uint64)
    pairs = np.array([[[d_store[p].ptr + (2 * s + i) * nbytes[p] for i in range(2)] for p in range(3)] for s in range(segs)], np.uint64)
    same = np.array([[[d_store[p].ptr + 2 * s * nbytes[p]] * 2 for p in range(3)] for s in range(segs)], np.uint64)      # top == bottom: the copy's reads exactly
    d_plain, d_pairs, d_same = ctx.to_device(plain), ctx.to_device(pairs), ctx.to_device(same)
    d_dst = [ctx.alloc(segs * b) for b in nbytes]
    t_weave, t_same, t_plain = [], [], []
    for rep in range(reps + 1):
        ctx.timer_begin()
        for _ in range(launches):
            ctx.telecine_gather(bd, sizes, true, segs, d_pairs, d_dst)
        a = ctx.timer_end() / launches
        ctx.timer_begin()
        for _ in range(launches):
            ctx.telecine_gather(bd, sizes, true, segs, d_same, d_dst)
        b = ctx.timer_end() / launches
        ctx.timer_begin()
        for _ in range(launches):
            ctx.frames_gather(nbytes, segs, d_plain, d_dst)
        c = ctx.timer_end() / launches
        if rep:
            t_weave.append(a)
            t_same.append(b)
            t_plain.append(c)
    for b in d_store + d_dst + [d_plain, d_pairs, d_same]:
        b.free()
    batch = sum(nbytes) * segs
    mw, mp = statistics.median(t_weave), statistics.median(t_plain)
    return {"width": W, "height": H, "bit_depth": bd, "segments": segs, "batch_bytes": batch, "weave_ms": spread(t_weave), "weave_equal_sources_ms": spread(t_same),
            "frames_gather_ms": spread(t_plain), "weave_over_frames_gather": mw / mp, "weave_gb_per_s_one_read_one_write": gbs(2 * batch, mw),
            "frames_gather_gb_per_s": gbs(2 * batch, mp)}


def write_clip(path, frames, W, H):
    film = {}

    def get(k):
        if k not in film:
            film[k] = telecine_ref.film_frame(k, W, H)
        return film[k]
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F30000:1001 It A1:1 C420jpeg\n" % (W, H)).encode())
        for v in range(frames):
            t, b = telecine_ref.video_sources(v, "tff")
            f.write(b"FRAME\n")
            for p in range(3):
                f.write(telecine_ref.interleave(get(t)[p], get(b)[p]).tobytes())
            for k in [k for k in film if k < min(t, b)]:
                del film[k]


def transcode_leg(reps, frames):
    W, H = 1920, 1080
    out = {"width": W, "height": H, "source_frames": frames}
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "tc.y4m")
        write_clip(src, frames, W, H)
        # -g counts output frames under ivtc: -g 24 there is the 30 source frames of the other legs' GOP
        legs = {"ivtc": ["-g", 24, "-av1mi_ivtc", 1], "deinterlace_auto": ["-g", 30, "-av1mi_deinterlace", "auto"], "as_it_is": ["-g", 30]}
        t = {mode: [] for mode in legs}
        for rep in range(reps + 1):
            for mode, extra in legs.items():
                t0 = time.perf_counter()
                code, err = av1stream.run_transcode(["-i", src, "-av1mi_segments", 2] + extra + [os.path.join(d, mode + ".ivf")])
                dt = time.perf_counter() - t0
                if code:
                    raise RuntimeError(err)
                if rep:
                    t[mode].append(dt)
        for mode in t:
            n_out = frames - frames // 5 if mode == "ivtc" else frames
            out[mode + "_seconds"] = spread(t[mode])
            out[mode + "_output_frames"] = n_out
            out[mode + "_output_frames_per_s"] = n_out / statistics.median(t[mode])
            out[mode + "_source_frames_per_s"] = frames / statistics.median(t[mode])
            out[mode + "_bytes"] = os.path.getsize(os.path.join(d, mode + ".ivf"))
    out["ivtc_bytes_over_deinterlace_auto"] = out["ivtc_bytes"] / out["deinterlace_auto_bytes"]
    out["ivtc_bytes_over_as_it_is"] = out["ivtc_bytes"] / out["as_it_is_bytes"]
    out["ivtc_seconds_over_as_it_is"] = out["ivtc_seconds"]["median"] / out["as_it_is_seconds"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivtc.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--run", type=int, default=32, help="frames of the analysed run")
    ap.add_argument("--transcode-frames", type=int, default=90)
    ap.add_argument("--skip-transcode", action="store_true")
    a = ap.parse_args()
    res = {}
    with av1mi.Context(0) as ctx:
        res["device"] = ctx.device_name
        res["analyse"] = {"1080p8": analyse_leg(ctx, 1920, 1080, 8, a.run, a.reps, a.launches), "4k10": analyse_leg(ctx, 3840, 2160, 10, a.run, a.reps, a.launches)}
        res["weave"] = {"1080p8x12": weave_leg(ctx, 1920, 1080, 8, 12, a.reps, a.launches), "4k10x12": weave_leg(ctx, 3840, 2160, 10, 12, a.reps, a.launches)}
    if not a.skip_transcode:
        res["transcode_1080p8"] = transcode_leg(min(a.reps, 3), a.transcode_frames)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
