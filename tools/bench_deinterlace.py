#!/usr/bin/env python3
"""What deinterlacing (include/av1mi.h "deinterlacing", av1mi_gop_config.deinterlace) costs on the GPU, each number beside what it is
measured against, in the same process, legs alternated, `--reps` repetitions with min / median / max:

1. k_deint_gather against k_frames_gather (the gather it stands in for, the floor) on the same batch: 4K 10-bit x 12 segments and
   1080p 8-bit x 12, every segment with its own P, C and N frames in a store past the Infinity Cache; HIP events around `--launches`
   launches.  Rates against the algorithmic bytes (one read of C plus one write) and against three reads plus one write.
2. av1mi_run_transcode on an interlaced 1080p clip, -av1mi_deinterlace auto against off, wall clock, frames per second.
3. Field rate (include/av1mi.h "FIELD-RATE OUTPUT"): the field-rate launch (av1mi_deinterlace_gather_fields; phases alternating over the
   segments, and all second fields) beside the same-rate launch in leg 1's loop, on the same batch; and the transcode with
   -av1mi_deinterlace_rate field beside frame, in OUTPUT frames per second (field rate makes two of every source frame).

    python tools/bench_deinterlace.py --out profiles/deinterlace.json
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

import av1mi        # noqa: E402
import av1stream    # noqa: E402
import deint_clips  # noqa: E402


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def kernel_leg(ctx, W, H, bd, segs, reps, launches):
    bps = 1 if bd == 8 else 2
    sizes = [(W, H), (W // 2, H // 2), (W // 2, H // 2)]
    nbytes = [w * h * bps for w, h in sizes]
    rng = np.random.default_rng(W + bd)
    frames = 3 * segs      # position 3 s + 1 is segment s's frame: no two segments share a neighbour
    d_store = []
    for p in range(3):
        d = ctx.alloc(nbytes[p] * frames)
        one = av1mi.DevBuf(ctx, nbytes[p]).upload(rng.integers(0, 256, nbytes[p], dtype=np.uint8))
        for f in range(frames):      # the same noise in every frame: the kernel's work does not depend on the values
            ctx._chk(ctx.lib.av1mi_copy(ctx.h, C.c_void_p(d.ptr + f * nbytes[p]), C.c_void_p(one.ptr), C.c_size_t(nbytes[p])))
        ctx.sync()
        one.free()
        d_store.append(d)
    plain = np.array([[d_store[p].ptr + (3 * s + 1) * nbytes[p] for p in range(3)] for s in range(segs)], np.uint64)
    three = np.array([[[d_store[p].ptr + (3 * s + i) * nbytes[p] for i in range(3)] for p in range(3)] for s in range(segs)], np.uint64)
    d_plain, d_three = ctx.to_device(plain), ctx.to_device(three)
    d_mixed, d_second = ctx.to_device(np.arange(segs, dtype=np.uint8) & 1), ctx.to_device(np.ones(segs, np.uint8))      # the phases
    d_dst = [ctx.alloc(segs * b) for b in nbytes]
    t_deint, t_plain, t_mixed, t_second = [], [], [], []
    for rep in range(reps + 1):      # the first repetition warms up
        ctx.timer_begin()
        for _ in range(launches):
            ctx.deinterlace_gather(bd, sizes, sizes, 0, segs, d_three, d_dst)
        a = ctx.timer_end() / launches
        ctx.timer_begin()
        for _ in range(launches):
            ctx.frames_gather(nbytes, segs, d_plain, d_dst)
        b = ctx.timer_end() / launches
        fields = []
        for d_phase in (d_mixed, d_second):
            ctx.timer_begin()
            for _ in range(launches):
                ctx.deinterlace_gather_fields(bd, sizes, sizes, 0, segs, d_three, d_phase, d_dst)
            fields.append(ctx.timer_end() / launches)
        if rep:
            t_deint.append(a)
            t_plain.append(b)
            t_mixed.append(fields[0])
            t_second.append(fields[1])
    for b in d_store + d_dst + [d_plain, d_three, d_mixed, d_second]:
        b.free()
    frame = sum(nbytes) * segs
    md, mp = statistics.median(t_deint), statistics.median(t_plain)
    gbs = lambda n, ms: n / (ms * 1e-3) / 1e9
    return {"width": W, "height": H, "bit_depth": bd, "segments": segs, "batch_bytes": frame,
            "deint_gather_ms": spread(t_deint), "frames_gather_ms": spread(t_plain), "ratio_to_the_plain_gather": md / mp,
            "fields_gather_mixed_phases_ms": spread(t_mixed), "fields_gather_second_fields_ms": spread(t_second),
            "fields_mixed_over_same_rate": statistics.median(t_mixed) / md, "fields_second_over_same_rate": statistics.median(t_second) / md,
            "deint_gb_per_s_one_read_one_write": gbs(2 * frame, md), "deint_gb_per_s_three_reads_one_write": gbs(4 * frame, md),
            "frames_gather_gb_per_s": gbs(2 * frame, mp)}


def transcode_leg(reps, frames):
    W, H = 1920, 1080
    out = {"width": W, "height": H, "frames": frames}
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "it.y4m")
        deint_clips.write_y4m(src, deint_clips.pan_clip(W, H, frames, 8, 0), 8, interlace="t")
        # field: -g counts output frames, so -g 60 keeps a GOP the 30 source frames long that the other two legs code
        legs = {"auto": ["-g", 30, "-av1mi_deinterlace", "auto"], "off": ["-g", 30, "-av1mi_deinterlace", "off"],
                "field": ["-g", 60, "-av1mi_deinterlace", "auto", "-av1mi_deinterlace_rate", "field"]}
        t = {mode: [] for mode in legs}
        for rep in range(reps + 1):
            for mode, extra in legs.items():
                t0 = time.perf_counter()
                code, err = av1stream.run_transcode(["-i", src, "-av1mi_segments", 4] + extra + [os.path.join(d, mode + ".ivf")])
                dt = time.perf_counter() - t0
                if code:
                    raise RuntimeError(err)
                if rep:
                    t[mode].append((2 if mode == "field" else 1) * frames / dt)      # OUTPUT frames per second
        for mode in t:
            out[mode + "_frames_per_s"] = spread(t[mode])
            out[mode + "_bytes"] = os.path.getsize(os.path.join(d, mode + ".ivf"))
    out["auto_over_off"] = out["auto_frames_per_s"]["median"] / out["off_frames_per_s"]["median"]
    out["field_over_auto_in_output_frames"] = out["field_frames_per_s"]["median"] / out["auto_frames_per_s"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deinterlace.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--transcode-frames", type=int, default=120)
    ap.add_argument("--skip-transcode", action="store_true")
    a = ap.parse_args()
    res = {}
    with av1mi.Context(0) as ctx:
        res["device"] = ctx.device_name
        res["kernel"] = {"4k10x12": kernel_leg(ctx, 3840, 2160, 10, 12, a.reps, a.launches), "1080p8x12": kernel_leg(ctx, 1920, 1080, 8, 12, a.reps, a.launches)}
    if not a.skip_transcode:
        res["transcode_1080p8"] = transcode_leg(min(a.reps, 3), a.transcode_frames)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
