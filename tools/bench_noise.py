#!/usr/bin/env python3
"""What -av1mi_denoise auto costs and where its plan lands (include/av1mi.h "noise records"; av1-go_amd/csrc/noise_kernels.hip;
av1-go_amd/host/noiseplan.hpp).

(a) av1mi_noise_analyse on 16 pairs — 1920x1080 8 bit and 3840x2160 10 bit — HIP events around `--launches` calls after a warm-up: ms, the
    bytes it reads (every luma sample of both planes once) and bytes/s; beside it k_frames_gather (the project's plain-copy yardstick)
    over the same planes in the same loop, its bytes/s counted on the bytes it READS.  The ratio is reported, not fixed.
(b) The two clips of tools/bench_grain.py — tests/synth.py content, and the clip that translates as a whole by 3 / -2 samples per frame
    (tests/denoise_mc_clips.py), on both of which a temporal estimate finds nothing that stands still — and that clip with its right half
    standing still, under Gaussian noise of sigma 2, 4 and 8:
    the strength auto plans, and the coded bytes and the stats file's psnr_y (measured against the source as the session codes it, i.e. the DENOISED frames
    where the job denoises) of auto, of no denoiser and of every fixed strength 1 .. 16 at q 23: where the plan lands on the saving curve.
(c) The wall time of the sampling step in a 1080p job: -av1mi_denoise auto against -av1mi_denoise N with the N it plans (the same job but
    for the step), alternated.

    python tools/bench_noise.py --out profiles/noise.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "av1-go_amd"), os.path.join(ROOT, "tests"), ROOT]
import av1mi  # noqa: E402
import av1stream  # noqa: E402
import deint_clips  # noqa: E402
import denoise_mc_clips  # noqa: E402
import synth  # noqa: E402

C = av1mi.C


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def analyse(ctx, reps, launches):
    out = {}
    lib = ctx.lib
    lib.av1mi_noise_analyse.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    for name, bd, w, h in (("1080p_8bit", 8, 1920, 1080), ("4k_10bit", 10, 3840, 2160)):
        pairs, h8 = 16, (h + 7) & ~7
        rng = np.random.default_rng(3)
        dt = np.uint8 if bd == 8 else np.uint16
        base = rng.integers(40, 200, (1, h8, w))
        Y = np.clip((base << (bd - 8)) + np.rint(rng.normal(0, 2 << (bd - 8), (2 * pairs, h8, w))), 0, (1 << bd) - 1).astype(dt)      # still, sigma 2: the bins spread
        plane = h8 * w * Y.itemsize
        nbytes = 2 * pairs * plane
        d_y, d_rec, d_copy = ctx.to_device(Y), ctx.alloc(pairs * av1mi.NOISE_DTYPE.itemsize), ctx.alloc(nbytes)
        table = np.zeros((2 * pairs, 3), np.uint64)
        table[:, 0] = [d_y.ptr + i * plane for i in range(2 * pairs)]
        d_table = ctx.to_device(table)
        call = lambda: ctx._chk(lib.av1mi_noise_analyse(ctx.h, bd, w, h8, w, h, pairs, d_y.ptr, d_rec.ptr))
        gather = lambda: ctx.frames_gather([plane, 0, 0], 2 * pairs, d_table, [d_copy, None, None])
        call()
        gather()
        ctx.sync()
        ms, gather_ms = [], []
        for _ in range(reps):
            ctx.timer_begin()
            for _ in range(launches):
                call()
            ms.append(ctx.timer_end() / launches)
            ctx.timer_begin()
            for _ in range(launches):
                gather()
            gather_ms.append(ctx.timer_end() / launches)
        rec = d_rec.download((pairs,), av1mi.NOISE_DTYPE)
        k, q, s16 = av1stream.plan_denoise(rec)
        for b in (d_y, d_rec, d_copy, d_table):
            b.free()
        gbps, ggbps = [nbytes / (m * 1e-3) / 1e9 for m in ms], [nbytes / (m * 1e-3) / 1e9 for m in gather_ms]
        out[name] = {"pairs": pairs, "bytes_read": nbytes, "ms": spread(ms), "read_GBps": spread(gbps), "k_frames_gather_same_planes_ms": spread(gather_ms),
                     "k_frames_gather_read_GBps": spread(ggbps), "analyse_read_rate_over_gather_read_rate": statistics.median(gbps) / statistics.median(ggbps),
                     "planned_on_this_content": {"strength": k, "sigma": s16 / 16, "true_sigma": 2}}
        print(json.dumps({name: out[name]}), flush=True)
    return out


def stats_of(path):
    lines = open(path).read().splitlines()
    return dict(kv.split(":") for kv in lines[-1].split()[1:]), lines[0]


def curve(w, h, frames):
    out = []
    sizes = [(w, h), (w // 2, h // 2), (w // 2, h // 2)]
    clean = dict(synth=synth.frames(w, h, frames, 8, 5), pan=[np.stack(a) for a in denoise_mc_clips.translating(sizes, frames, 8, 5, 0)])
    clean["half_pan"] = [a.copy() for a in clean["pan"]]      # the right half of the picture stands still: frame 0's, in every frame
    for a in clean["half_pan"]:
        a[:, :, a.shape[2] // 2:] = a[0, :, a.shape[2] // 2:]
    with tempfile.TemporaryDirectory() as d:
        for content, sigma in ((c, s) for c in clean for s in (2, 4, 8)):
            rng = np.random.default_rng(sigma)
            clip = [np.clip(np.stack(a) + np.rint(rng.normal(0, sigma, np.stack(a).shape)), 0, 255).astype(np.uint8) for a in clean[content]]
            src = os.path.join(d, "%s%d.y4m" % (content, sigma))
            deint_clips.write_y4m(src, clip, 8, interlace="p")
            row = {"size": "%dx%d" % (w, h), "frames": frames, "content": content, "sigma": sigma, "q": 23, "runs": {}}
            for name, extra in [("auto", ["-av1mi_denoise", "auto"]), ("off", [])] + [(str(n), ["-av1mi_denoise", n]) for n in range(1, 17)]:
                dst, st = os.path.join(d, "o.obu"), os.path.join(d, "o.stats")
                code, err, planned = av1stream.run_transcode_report(["-i", src, "-global_quality:v:0", 23, "-g", 30, "-av1mi_segments", 4, "-av1mi_stats", st] + extra + [dst])
                assert code == 0, err
                summary, first = stats_of(st)
                row["runs"][name] = {"bytes": os.path.getsize(dst), "psnr_y": float(summary["psnr_y"])}
                if name == "auto":
                    row["planned"] = planned
                    row["first_stats_line"] = first
            off = row["runs"]["off"]["bytes"]
            row["auto_bytes_over_off"] = row["runs"]["auto"]["bytes"] / off
            row["best_fixed"] = min(range(1, 17), key=lambda n: row["runs"][str(n)]["bytes"])
            row["auto_equals_fixed_bytes"] = row["planned"] > 0 and row["runs"]["auto"]["bytes"] == row["runs"][str(row["planned"])]["bytes"]
            out.append(row)
            print(json.dumps(row), flush=True)
        # (c) the sampling step: the same source, auto against the strength it plans
        planned = [r for r in out if r["content"] == "half_pan" and r["sigma"] == 4][0]["planned"]
        src = os.path.join(d, "half_pan4.y4m")
        wall = {"auto": [], "fixed": []}
        for _ in range(3):
            for name, extra in (("auto", ["-av1mi_denoise", "auto"]), ("fixed", ["-av1mi_denoise", planned] if planned else [])):
                t0 = time.perf_counter()
                code, err = av1stream.run_transcode(["-i", src, "-global_quality:v:0", 23, "-g", 30, "-av1mi_segments", 4] + extra + [os.path.join(d, "t.obu")])
                wall[name].append(time.perf_counter() - t0)
                assert code == 0, err
        step = {"job": "%dx%d 8 bit, %d frames, sigma 4, q 23; the file is in the page cache" % (w, h, frames), "auto_wall_s": spread(wall["auto"]), "fixed_wall_s": spread(wall["fixed"]),
                "sampling_step_s": statistics.median(wall["auto"]) - statistics.median(wall["fixed"]), "pairs_sampled": min(16, frames // 2)}
        print(json.dumps(step), flush=True)
    return out, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise.json"))
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    res = {"tool": "tools/bench_noise.py"}
    with av1mi.Context(0) as ctx:
        res["device"] = ctx.device_name
        res["noise_analyse"] = analyse(ctx, a.reps, a.launches)
    res["plan_on_the_saving_curve"], res["sampling_step"] = curve(1920, 1080, a.frames)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
