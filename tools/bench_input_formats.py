#!/usr/bin/env python3
"""What the session's input formats (include/av1mi.h enum av1mi_input_format) cost and gain on the GPU, each number beside what
it is measured against, in the same process, legs alternated, `--reps` repetitions with min / median / max:

1. k_input_convert alone, per format, on a 12-segment 4K batch (past the Infinity Cache), HIP events around `--launches` launches,
   beside av1mi_copy (device to device) of the same total bytes (read + written): the copy roofline bench.py uses.
2. End to end at 4K 10-bit, 12 segments, GOP 30, GPU entropy coding, the loop of bench.py's e2e_leg (restated here): the planar
   session (today's path), PACKED10 with the source packed beforehand (what the transport alone gains) and PACKED10 packed by the
   host threads inside the timed loop (what the product's -av1mi_pack10 1 gets), at q 128 and q 23.

    python tools/bench_input_formats.py --out profiles/input_formats.json
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))
sys.path.insert(0, ROOT)

import av1mi      # noqa: E402
import av1stream  # noqa: E402
import synth      # noqa: E402
from bench import frame_unit  # noqa: E402

NAMES = {av1mi.INPUT_PLANAR: "planar", av1mi.INPUT_PACKED10: "packed10", av1mi.INPUT_P010: "p010", av1mi.INPUT_NV12: "nv12"}


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def kernel_leg(ctx, W, H, segs, reps, launches):
    """device time of one conversion launch against one device-to-device copy of the same bytes, alternated"""
    out = {}
    rows = H * segs
    for fmt in (av1mi.INPUT_PACKED10, av1mi.INPUT_P010, av1mi.INPUT_NV12):
        bd = 8 if fmt == av1mi.INPUT_NV12 else 10
        n_in = [av1mi.input_plane_bytes(fmt, bd, p, W, rows) for p in range(3)]
        n_out = [av1mi.input_plane_bytes(av1mi.INPUT_PLANAR, bd, p, W, rows) for p in range(3)]
        total = sum(n_in) + sum(n_out)
        rng = np.random.default_rng(fmt)
        d_in = [ctx.to_device(rng.integers(0, 256, k, dtype=np.uint8)) for k in n_in if k]
        d_out = [ctx.alloc(k) for k in n_out]
        d_a, d_b = ctx.alloc(total // 2), ctx.alloc(total // 2)      # a copy that reads and writes `total` bytes together
        conv, copy = [], []
        for rep in range(reps + 1):      # the first repetition warms up
            ctx.timer_begin()
            for _ in range(launches):
                ctx.input_convert(fmt, bd, W, rows, d_in, d_out)
            t_conv = ctx.timer_end() / launches
            ctx.timer_begin()
            for _ in range(launches):
                ctx.copy(d_b, d_a, total // 2)
            t_copy = ctx.timer_end() / launches
            if rep:
                conv.append(t_conv)
                copy.append(t_copy)
        for b in d_in + d_out + [d_a, d_b]:
            b.free()
        gbs = lambda ms: total / (ms * 1e-3) / 1e9
        out[NAMES[fmt]] = {"bit_depth": bd, "bytes_read": sum(n_in), "bytes_written": sum(n_out), "samples": W * rows * 3 // 2,
                           "convert_ms": spread(conv), "convert_gb_per_s": gbs(statistics.median(conv)),
                           "copy_same_bytes_ms": spread(copy), "copy_gb_per_s": gbs(statistics.median(copy)),
                           "convert_rate_over_copy_rate": statistics.median(copy) / statistics.median(conv)}
    return out


class E2eLeg:
    """bench.py's e2e_leg loop with the session's input format and the way its pinned buffers are filled as parameters"""

    def __init__(self, ctx, name, src, packed, W, H, q, gop, threads, kbs):
        self.name, self.src, self.packed, self.W, self.H, self.gop, self.threads = name, src, packed, W, H, gop, threads
        self.segs = src[0].shape[0]
        self.fmt = av1mi.INPUT_PLANAR if name == "planar" else av1mi.INPUT_PACKED10
        self.sess = av1mi.GopSession(ctx, W, H, 10, q, gop, self.segs, gpu_entropy=1, key_block_size=kbs, input_format=self.fmt)
        self.pool = ThreadPoolExecutor(max(1, min(threads, 3 * self.segs)))
        self.ctx = ctx
        self.up = sum(av1mi.input_plane_bytes(self.fmt, 10, p, W, H) for p in range(3))
        self.runs = []
        self.c = {"bytes": 0, "frames": 0, "t_fill": 0.0, "t_code": 0.0, "t_wait": 0.0}

    def fill(self, t):
        t0 = time.perf_counter()
        planes = self.sess.input_planes()
        jobs = []
        if self.name == "packed10_pack_in_loop":      # one job per segment, like the product's reader threads
            n = [av1mi.input_plane_bytes(self.fmt, 10, p, self.W, self.H) for p in range(3)]
            for sg in range(self.segs):
                jobs.append(self.pool.submit(av1mi.input_pack, self.fmt, 10, self.src[0][sg, t], self.src[1][sg, t], self.src[2][sg, t],
                                             [(planes[p], n[p] * sg) for p in range(3)]))
        else:
            for p in range(3):
                for sg in range(self.segs):
                    if self.name == "planar":
                        hh = self.H if p == 0 else self.H // 2
                        jobs.append(self.pool.submit(np.copyto, planes[p][sg * hh:(sg + 1) * hh], self.src[p][sg, t]))
                    else:
                        a = self.packed[p][sg][t]
                        jobs.append(self.pool.submit(np.copyto, planes[p][sg * a.size:(sg + 1) * a.size], a))
        for j in jobs:
            j.result()
        self.c["t_fill"] += time.perf_counter() - t0

    def code(self):
        t0 = time.perf_counter()
        fr = self.sess.collect()
        t1 = time.perf_counter()
        for sg in range(self.segs):
            self.c["bytes"] += len(frame_unit(av1stream, self.W, self.H, 10, fr, sg, 1, self.threads))
            self.c["frames"] += 1
        self.c["t_wait"] += t1 - t0
        self.c["t_code"] += time.perf_counter() - t1

    def run_gop(self, nframes):
        lag = self.sess.max_in_flight() - 1
        for t in range(nframes):
            self.fill(t)
            self.sess.submit(0 if t == 0 else 1)
            if t >= lag:
                self.code()
        while self.sess.pending():
            self.code()

    def timed(self, steps, record=True):
        self.c = {"bytes": 0, "frames": 0, "t_fill": 0.0, "t_code": 0.0, "t_wait": 0.0}
        self.ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.run_gop(self.gop)
        self.ctx.sync()
        dt = time.perf_counter() - t0
        if record:
            self.runs.append(dict(self.c, seconds=dt, frames_per_s=self.c["frames"] / dt))

    def result(self):
        fb = int(self.sess.entropy_fallbacks())
        self.sess.close()
        self.pool.shutdown()
        r = self.runs
        return {"frames_per_s": spread([x["frames_per_s"] for x in r]), "frames_per_run": r[0]["frames"], "coded_bytes_per_frame": r[0]["bytes"] / r[0]["frames"],
                "pcie_bytes_per_frame_up": self.up, "entropy_fallbacks": fb,
                "host_seconds_per_run": {"fill_or_pack_pinned_input": spread([x["t_fill"] for x in r]), "wait_for_gpu": spread([x["t_wait"] for x in r]),
                                         "assemble_obu": spread([x["t_code"] for x in r])}}


def e2e(ctx, src, W, H, gop, qs, reps, steps, threads):
    segs = src[0].shape[0]
    t0 = time.perf_counter()
    pool = ThreadPoolExecutor(threads)
    packed = [[None] * segs for _ in range(3)]

    def pack_segment(sg):
        per = [av1mi.input_pack(av1mi.INPUT_PACKED10, 10, src[0][sg, t], src[1][sg, t], src[2][sg, t]) for t in range(gop)]
        for p in range(3):
            packed[p][sg] = [x[p] for x in per]
    list(pool.map(pack_segment, range(segs)))
    pool.shutdown()
    out = {"prepacking_seconds": time.perf_counter() - t0, "bytes_per_coded_frame_are_equal": True}
    kbs = 32 if W % 32 == 0 else 0
    for q in qs:
        legs = [E2eLeg(ctx, name, src, packed, W, H, q, gop, threads, kbs) for name in ("planar", "packed10_prepacked", "packed10_pack_in_loop")]
        for leg in legs:
            leg.run_gop(min(3, gop))      # warm up
        for rep in range(reps):
            for leg in legs:
                leg.timed(steps)
        res = {leg.name: leg.result() for leg in legs}
        if len({round(r["coded_bytes_per_frame"], 6) for r in res.values()}) != 1:
            out["bytes_per_coded_frame_are_equal"] = False
        out["q%d" % q] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_formats.json"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--segments", type=int, default=12)
    ap.add_argument("--gop", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2, help="GOPs per timed end-to-end window")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--qindex", type=int, nargs="+", default=[128, 23])
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    W, H, segs, gop = args.width, args.height, args.segments, args.gop
    out = {"what": __doc__.strip().split("\n\n")[0], "date": time.strftime("%Y-%m-%d"), "width": W, "height": H, "segments": segs, "gop": gop,
           "repetitions": args.reps, "host_threads": args.threads}
    with av1mi.Context(0) as ctx:
        out["device"] = ctx.device_name
        out["kernel"] = kernel_leg(ctx, W, H, segs, args.reps, args.launches)
        print(json.dumps({"kernel": out["kernel"]}), flush=True)
        if not args.no_e2e:
            Y, U, V = synth.frames(W, H, segs * gop, 10, 0)
            src = [a.reshape(segs, gop, *a.shape[1:]) for a in (Y, U, V)]
            out["end_to_end"] = e2e(ctx, src, W, H, gop, args.qindex, args.reps, args.steps, args.threads)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
