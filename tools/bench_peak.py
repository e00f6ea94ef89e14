#!/usr/bin/env python3
"""What the measurement behind -av1mi_tonemap_peak auto costs (include/av1mi.h "peak records"; av1-go_amd/csrc/peak_kernels.hip).

av1mi_peak_analyse (k_peak_rows + k_peak_sum) on `--frames` frames of 3840x2160 10-bit 4:2:0 — enough of them that the planes do not fit
the 256 MiB last-level cache — HIP events around `--launches` calls after a warm-up: ms per frame, the bytes the two launches must read
(3 bytes per pixel: every luma sample and every chroma sample once) and bytes/s; beside it k_frames_gather (the project's plain-copy
yardstick) over the same three planes in the same loop, its bytes/s counted on the bytes it READS.  Two contents, alternated in one
process: TEXTURED (a noisy ramp: neighbouring pixels rarely share a code) and FLAT (one code everywhere: every lane of every wave on one
LDS counter, the case that merging equal neighbours in a lane is there for).  The ratios are reported, not fixed in advance.

    python tools/bench_peak.py --out profiles/peak.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "av1-go_amd"), os.path.join(ROOT, "tests"), ROOT]
import av1mi  # noqa: E402
import av1stream  # noqa: E402

C = av1mi.C
W, H = 3840, 2160


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def content(name, frames):
    if name == "flat":
        return np.full((frames, H, W), 300, np.uint16), np.full((frames, H // 2, W // 2), 512, np.uint16), np.full((frames, H // 2, W // 2), 700, np.uint16)
    rng = np.random.default_rng(3)
    ramp = (np.arange(W) * 876 // W + 64).astype(np.int16)[None, None, :]
    Y = (ramp + rng.integers(-40, 41, (frames, H, W), dtype=np.int16)).clip(0, 1023).astype(np.uint16)
    U, V = (rng.integers(400, 625, (frames, H // 2, W // 2), dtype=np.uint16) for _ in range(2))
    return Y, U, V


def measure(ctx, frames, reps, launches):
    lib = ctx.lib
    lib.av1mi_peak_analyse.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4
    sizes = [W * H * 2, W * H // 2, W * H // 2]      # bytes of a frame's planes
    nbytes = frames * sum(sizes)
    dev, calls, gathers = {}, {}, {}
    for name in ("textured", "flat"):
        planes = content(name, frames)
        d = [ctx.to_device(a) for a in planes]
        d_rec, d_copy = ctx.alloc(frames * av1mi.PEAK_DTYPE.itemsize), [ctx.alloc(frames * s) for s in sizes]
        table = np.zeros((frames, 3), np.uint64)
        for p in range(3):
            table[:, p] = [d[p].ptr + i * sizes[p] for i in range(frames)]
        d_table = ctx.to_device(table)
        dev[name] = d + [d_rec, d_table] + d_copy
        calls[name] = lambda d=d, d_rec=d_rec: ctx._chk(lib.av1mi_peak_analyse(ctx.h, W, H, W, H, frames, d[0].ptr, d[1].ptr, d[2].ptr, d_rec.ptr))
        gathers[name] = lambda d_table=d_table, d_copy=d_copy: ctx.frames_gather(sizes, frames, d_table, d_copy)
        calls[name]()
        gathers[name]()
        rec = d_rec.download((frames,), av1mi.PEAK_DTYPE)
        assert (rec["hist"].sum(axis=1) == W * H).all() and (rec["pixels"] == W * H).all()
        if name == "flat":
            assert (rec["hist"][:, 592] == W * H).all()
        dev[name + "_plan"] = av1stream.plan_peak(rec)[0]
    ctx.sync()
    ms = {k: [] for k in ("textured", "flat", "textured_gather", "flat_gather")}
    for _ in range(reps):      # the variants alternate inside one process
        for name in ("textured", "flat"):
            for key, fn in ((name, calls[name]), (name + "_gather", gathers[name])):
                ctx.timer_begin()
                for _ in range(launches):
                    fn()
                ms[key].append(ctx.timer_end() / launches)
    out = {"size": "%dx%d 10 bit 4:2:0" % (W, H), "frames": frames, "bytes_read": nbytes, "bytes_read_per_pixel": 3}
    for name in ("textured", "flat"):
        rate = [nbytes / (m * 1e-3) / 1e9 for m in ms[name]]
        copy = [nbytes / (m * 1e-3) / 1e9 for m in ms[name + "_gather"]]
        out[name] = {"ms_per_frame": spread([m / frames for m in ms[name]]), "read_GBps": spread(rate), "k_frames_gather_same_planes_ms_per_frame": spread([m / frames for m in ms[name + "_gather"]]),
                     "k_frames_gather_read_GBps": spread(copy), "analyse_read_rate_over_gather_read_rate": statistics.median(rate) / statistics.median(copy),
                     "planned_peak": dev[name + "_plan"]}
        print(json.dumps({name: out[name]}), flush=True)
    out["flat_ms_over_textured_ms"] = statistics.median(ms["flat"]) / statistics.median(ms["textured"])
    for name in ("textured", "flat"):
        for b in dev[name]:
            b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peak.json"))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    a = ap.parse_args()
    res = {"tool": "tools/bench_peak.py"}
    with av1mi.Context(0) as ctx:
        res["device"] = ctx.device_name
        res["peak_analyse"] = measure(ctx, a.frames, a.reps, a.launches)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
