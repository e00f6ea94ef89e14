#!/usr/bin/env python3
"""What cropping costs and gains (include/av1mi.h "bar detection", av1mi_gop_config.crop_*; av1-go_amd/csrc/crop_kernels.hip), each number
beside what it is measured against, `--reps` repetitions with min / median / max:

(a) av1mi_crop_analyse on 32 frames — 1920x1080 8 bit and 3840x2160 10 bit — HIP events around `--launches` calls: time, the bytes it
    reads (every luma sample once) per second as a fraction of the 8 TB/s HBM roofline bench.py reports against, and beside it the
    device-to-device copy rate of this box measured in the same loop (av1mi_copy over the same bytes).
(b) The window stage of a 12-segment batch, 1920x1080 8-bit frames with a 1920x800 window: k_crop_copy (the window is the target) and the
    windowed k_scale (the window scaled to 1280x534), from the session's own profile (AV1MI_K_INPUT, one launch per batch), against
    k_frames_gather moving the bytes of the window: the project's plain-copy yardstick.
(c) The point of it: av1mi_run_transcode of a 1920x1080 source whose picture is 1920x800 (synth content inside black bars), q 24, 12
    segments, `-av1mi_crop off` against `auto`, alternated: frames per second end to end (file to file), bytes per frame, and PSNR-Y over
    the PICTURE area (off: the stats file's whole-frame squared error divided by the picture's samples, i.e. every error counted as the
    picture's; auto: the stats file's figure, measured on the cropped frame).
(d) With --parent-lib: `bench.py --gpus 1 --steps 10 --warmup 2` for this tree's library and for that build of the parent commit's
    (AV1MI_LIB), alternated: the default path must sit within the run-to-run spread.

    python tools/bench_crop.py --out profiles/crop.json [--parent-lib /path/to/parent/libav1mi.so]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))

import av1mi      # noqa: E402

HBM_PEAK_GBPS = 8000.0      # bench.py's roofline: the HBM3E specification


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "n": len(v)}


def analyse(ctx, reps, launches):
    out = {}
    lib = ctx.lib
    lib.av1mi_crop_analyse.argtypes = [av1mi.C.c_void_p] + [av1mi.C.c_int] * 6 + [av1mi.C.c_void_p, av1mi.C.c_int, av1mi.C.c_void_p]
    for name, bd, w, h in (("1080p_8bit", 8, 1920, 1080), ("4k_10bit", 10, 3840, 2160)):
        frames, h8 = 32, (h + 7) & ~7
        rng = np.random.default_rng(3)
        one = rng.integers(0, 1 << bd, (h8, w)).astype(np.uint8 if bd == 8 else np.uint16)
        one[:140 * h // 1080] = 16 << (bd - 8)
        Y = np.broadcast_to(one, (frames, h8, w))
        nbytes = frames * h * w * one.itemsize
        d_y, d_rec, d_copy = ctx.to_device(np.ascontiguousarray(Y)), ctx.alloc(frames * 16), ctx.alloc(nbytes)
        call = lambda: ctx._chk(lib.av1mi_crop_analyse(ctx.h, bd, w, h8, w, h, frames, d_y.ptr, 24, d_rec.ptr))
        ms, copy_ms = [], []
        call()
        ctx.sync()
        for _ in range(reps):
            ctx.timer_begin()
            for _ in range(launches):
                call()
            ms.append(ctx.timer_end() / launches)
            ctx.timer_begin()
            for _ in range(launches):
                ctx.copy(d_copy, d_y, nbytes)
            copy_ms.append(ctx.timer_end() / launches)
        for b in (d_y, d_rec, d_copy):
            b.free()
        gbps = [nbytes / (m * 1e-3) / 1e9 for m in ms]
        out[name] = {"frames": frames, "bytes_read": nbytes, "ms_per_32_frames": spread(ms), "read_GBps": spread(gbps),
                     "fraction_of_hbm_roofline": statistics.median(gbps) / HBM_PEAK_GBPS,
                     "copy_of_the_same_bytes_ms": spread(copy_ms), "copy_GBps_moved": 2 * nbytes / (statistics.median(copy_ms) * 1e-3) / 1e9,
                     "analyse_time_over_copy_time": statistics.median(ms) / statistics.median(copy_ms)}
        print(json.dumps({name: out[name]}), flush=True)
    return out


def window_stage(ctx, reps):
    bd, sw, sh, segs, win = 8, 1920, 1080, 12, (0, 140, 1920, 800)
    sh8 = (sh + 7) & ~7
    rng = np.random.default_rng(4)
    planes = [rng.integers(0, 256, (segs * sh8 // d, sw // d)).astype(np.uint8) for d in (1, 2, 2)]
    bufs = [ctx.to_device(a) for a in planes]
    out = {"config": "1920x1080 8 bit, 12 segments per batch, window 1920x800+0+140, submit_device, one launch per batch"}
    for name, tw, th in (("k_crop_copy", 1920, 800), ("k_scale_windowed_to_1280x534", 1280, 534)):
        w, h = (tw + 7) & ~7, (th + 7) & ~7
        s = av1mi.GopSession(ctx, w, h, bd, 128, 30, segs, gpu_entropy=1, visible=(tw, th) if (w, h) != (tw, th) else None, source=(sw, sh), crop=win)
        ms = []
        try:
            ctx.prof_enable(1)
            for r in range(reps + 1):
                ctx.prof_reset()
                for t in range(3):
                    s.submit_device(bufs[0], bufs[1], bufs[2], frame_type=0 if t == 0 else 1)
                    s.collect()
                n, total = ctx.prof_get()["input_convert"]
                if r:
                    ms.append(total / n)
        finally:
            ctx.prof_enable(0)
            s.close()
        out[name] = {"ms_per_batch": spread(ms)}
    # the yardstick: k_frames_gather over the window's bytes
    nb = [1920 * 800, 960 * 400, 960 * 400]
    src = [ctx.alloc(n * segs) for n in nb]
    dst = [ctx.alloc(n * segs) for n in nb]
    table = np.array([[src[p].ptr + sg * nb[p] for p in range(3)] for sg in range(segs)], np.uint64)
    d_table = ctx.to_device(table)
    ms = []
    for r in range(reps + 1):
        ctx.timer_begin()
        for _ in range(10):
            ctx.frames_gather(nb, segs, d_table, dst)
        t = ctx.timer_end() / 10
        if r:
            ms.append(t)
    out["k_frames_gather_same_bytes"] = {"bytes_moved_one_way": sum(nb) * segs, "ms_per_batch": spread(ms)}
    out["k_crop_copy_over_gather"] = out["k_crop_copy"]["ms_per_batch"]["median"] / statistics.median(ms)
    for b in bufs + src + dst + [d_table]:
        b.free()
    print(json.dumps({"window_stage": out}), flush=True)
    return out


def letterboxed(path, frames):
    import synth
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W1920 H1080 F24:1 Ip A1:1 C420jpeg\n")
        Y, U, V = synth.frames(1920, 800, frames, 8, 0)
        by, bc = np.full((140, 1920), 16, np.uint8).tobytes(), np.full((70, 960), 128, np.uint8).tobytes()
        for t in range(frames):
            f.write(b"FRAME\n" + by + Y[t].tobytes() + by + bc + U[t].tobytes() + bc + bc + V[t].tobytes() + bc)


def transcodes(reps, frames, timeout):
    import av1stream
    out = {"config": "1920x1080 8 bit, picture 1920x800 between black bars (synth content), %d frames, -global_quality 24, -g 30, 12 segments, .obu output" % frames}
    runs = {"off": [], "auto": []}
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "bars.y4m")
        letterboxed(src, frames)
        for r in range(reps):
            for mode in ("off", "auto"):
                dst, stats = os.path.join(d, mode + ".obu"), os.path.join(d, mode + ".stats")
                t0 = time.perf_counter()
                code, err = av1stream.run_transcode(["-i", src, "-global_quality:v:0", 24, "-g", 30, "-av1mi_segments", 12, "-av1mi_crop", mode, "-av1mi_stats", stats, dst])
                wall = time.perf_counter() - t0
                if code:
                    raise RuntimeError("transcode (%s) failed with %d: %s" % (mode, code, err))
                summary = dict(kv.split(":") for kv in open(stats).read().splitlines()[-1].split()[1:])
                psnr = float(summary["psnr_y"])
                if mode == "off":      # whole-frame error over the picture's samples
                    psnr -= 10 * math.log10(1080 / 800)
                runs[mode].append({"frames_per_s": frames / wall, "bytes_per_frame": os.path.getsize(dst) / frames, "psnr_y_picture_dB": psnr,
                                   "first_line": open(stats).readline().strip()})
                print(json.dumps({mode: runs[mode][-1]}), flush=True)
    for mode in runs:
        out[mode] = {"frames_per_s": spread([x["frames_per_s"] for x in runs[mode]]), "bytes_per_frame": runs[mode][0]["bytes_per_frame"],
                     "psnr_y_picture_dB": runs[mode][0]["psnr_y_picture_dB"], "first_stats_line": runs[mode][0]["first_line"]}
    out["auto_over_off_frames_per_s"] = out["auto"]["frames_per_s"]["median"] / out["off"]["frames_per_s"]["median"]
    out["auto_over_off_bytes"] = out["auto"]["bytes_per_frame"] / out["off"]["bytes_per_frame"]
    return out


def bench_ab(parent_lib, reps, timeout):
    runs = {"this": [], "parent": []}
    for _ in range(reps):
        for name in ("parent", "this"):
            env = dict(os.environ)
            if name == "parent":
                env["AV1MI_LIB"] = os.path.abspath(parent_lib)
            else:
                env.pop("AV1MI_LIB", None)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2"], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=timeout)
            if p.returncode != 0:
                raise RuntimeError("bench.py (%s) failed with %d: %s" % (name, p.returncode, p.stderr[-2000:]))
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            runs[name].append(res["value"])
            print(json.dumps({"bench": name, "value": res["value"], "unit": res.get("unit")}), flush=True)
    return {"command": "bench.py --gpus 1 --steps 10 --warmup 2", "this_commit_value": spread(runs["this"]), "parent_commit_value": spread(runs["parent"]),
            "this_commit_runs": runs["this"], "parent_commit_runs": runs["parent"],
            "this_median_within_parent_spread": min(runs["parent"]) <= statistics.median(runs["this"]) <= max(runs["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--transcode-reps", type=int, default=2)
    ap.add_argument("--transcode-frames", type=int, default=360)
    ap.add_argument("--skip-transcode", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libav1mi.so built from the parent commit: adds the bench.py A/B")
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--bench-timeout", type=int, default=400, help="seconds for one bench.py process")
    args = ap.parse_args()
    out = {}
    with av1mi.Context(0) as ctx:
        out["device"] = ctx.device_name
        out["crop_analyse"] = analyse(ctx, args.reps, args.launches)
        out["window_stage"] = window_stage(ctx, args.reps)
    if not args.skip_transcode:
        out["transcode"] = transcodes(args.transcode_reps, args.transcode_frames, 600)
    if args.parent_lib:
        out["bench_default_path"] = bench_ab(args.parent_lib, args.bench_reps, args.bench_timeout)
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
