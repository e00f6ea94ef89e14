#!/usr/bin/env python3
"""What sources that are not 4:2:0 (include/av1mi.h "chroma formats") cost on the GPU, each number beside what it is measured against,
in the same process, legs alternated, `--reps` repetitions with min / median / max:

1. k_chroma_convert alone on a 12-frame 4K batch (past the Infinity Cache) for 4:2:2 10-bit, 4:4:4 10-bit and 4:4:4 12-bit, HIP events
   around `--launches` launches: the time and the achieved GB/s over the bytes read + written, beside k_input_convert P010 at the same
   size, the project's existing pure-bandwidth input kernel.
2. End to end at 4K, GPU entropy coding, the loop of bench.py's e2e_leg (restated here): a 4:4:4 10-bit session fed the clip against a
   planar session fed the same clip converted beforehand — what the wider upload (50 MB a frame instead of 25) and the stage cost.

    python tools/bench_chroma_formats.py --out profiles/chroma_formats.json
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

CASES = (("422_10bit", av1mi.CHROMA_422, 10), ("444_10bit", av1mi.CHROMA_444, 10), ("444_12bit", av1mi.CHROMA_444, 12))


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def kernel_leg(ctx, W, H, frames, reps, launches):
    """device time of one chroma launch and of one P010 conversion launch at the same size, alternated"""
    out = {}
    rows = H * frames
    p010_in = [av1mi.input_plane_bytes(av1mi.INPUT_P010, 10, p, W, rows) for p in range(3)]
    planar = [av1mi.input_plane_bytes(av1mi.INPUT_PLANAR, 10, p, W, rows) for p in range(3)]
    d_p_in = [ctx.to_device(np.random.default_rng(1).integers(0, 256, k, dtype=np.uint8)) for k in p010_in if k]
    d_out = [ctx.alloc(k) for k in planar]
    p010_total = sum(p010_in) + sum(planar)
    for name, chroma, src_bd in CASES:
        n_in = [av1mi.source_plane_bytes(chroma, src_bd, p, W, rows) for p in range(3)]
        luma = src_bd != 10
        total = sum(n_in[1:]) + sum(planar[1:]) + (n_in[0] + planar[0] if luma else 0)      # the luma plane is touched only where the depths differ
        rng = np.random.default_rng(chroma + src_bd)
        d_in = [ctx.to_device(rng.integers(0, 1 << src_bd, k // 2, dtype=np.uint16)) for k in n_in]
        conv, p010 = [], []
        for rep in range(reps + 1):      # the first repetition warms up
            ctx.timer_begin()
            for _ in range(launches):
                ctx.chroma_convert(chroma, src_bd, 10, W, H, frames, d_in, d_out)
            t_conv = ctx.timer_end() / launches
            ctx.timer_begin()
            for _ in range(launches):
                ctx.input_convert(av1mi.INPUT_P010, 10, W, rows, d_p_in, d_out)
            t_p010 = ctx.timer_end() / launches
            if rep:
                conv.append(t_conv)
                p010.append(t_p010)
        for b in d_in:
            b.free()
        gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9
        c, y = statistics.median(conv), statistics.median(p010)
        out[name] = {"source_bit_depth": src_bd, "luma_converted": luma, "bytes_read_and_written": total, "chroma_convert_ms": spread(conv),
                     "chroma_convert_gb_per_s": gbs(total, c), "p010_convert_bytes": p010_total, "p010_convert_ms": spread(p010),
                     "p010_convert_gb_per_s": gbs(p010_total, y), "rate_over_p010_rate": gbs(total, c) / gbs(p010_total, y)}
    for b in d_p_in + d_out:
        b.free()
    return out


class E2eLeg:
    """bench.py's e2e_leg loop; src: per plane [segments, frames, rows, columns] in the layout the session is fed"""

    def __init__(self, ctx, name, src, W, H, q, gop, threads, kbs, **kw):
        self.name, self.src, self.W, self.H, self.gop, self.threads, self.ctx = name, src, W, H, gop, threads, ctx
        self.segs = src[0].shape[0]
        self.sess = av1mi.GopSession(ctx, W, H, 10, q, gop, self.segs, gpu_entropy=1, key_block_size=kbs, **kw)
        self.pool = ThreadPoolExecutor(max(1, min(threads, 3 * self.segs)))
        self.up = sum(a[0, 0].nbytes for a in src)
        self.runs = []

    def fill(self, t):
        planes = self.sess.input_planes()
        jobs = []
        for p, a in enumerate(self.src):
            rows = a.shape[2]
            for sg in range(self.segs):
                jobs.append(self.pool.submit(np.copyto, planes[p][sg * rows:(sg + 1) * rows], a[sg, t]))
        for j in jobs:
            j.result()

    def code(self):
        fr = self.sess.collect()
        for sg in range(self.segs):
            self.c["bytes"] += len(frame_unit(av1stream, self.W, self.H, 10, fr, sg, 1, self.threads))
            self.c["frames"] += 1

    def run_gop(self):
        lag = self.sess.max_in_flight() - 1
        for t in range(self.gop):
            self.fill(t)
            self.sess.submit(0 if t == 0 else 1)
            if t >= lag:
                self.code()
        while self.sess.pending():
            self.code()

    def timed(self, steps, record=True):
        self.c = {"bytes": 0, "frames": 0}
        self.ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.run_gop()
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
                "pcie_bytes_per_frame_up": self.up, "entropy_fallbacks": fb}


def e2e(ctx, W, H, segs, gop, q, reps, steps, threads):
    """the clip: synth's 4:2:0 frames; its 4:4:4 chroma is their chroma enlarged 2 x 2 by repetition plus a one-sample pattern (so that the
    filter has something to remove: full-size synthetic chroma would cost minutes of host time at 4K).  The 4:2:0 form of the same clip
    comes from av1mi_chroma_convert, which the tests pin to the definition"""
    Y, U, V = synth.frames(W, H, segs * gop, 10, 0)
    pat = (np.indices((H, W)).sum(0) & 1).astype(np.uint16) * 8
    wide = [np.minimum(a.repeat(2, 1).repeat(2, 2) + pat, 1023).astype(np.uint16) for a in (U, V)]
    src444 = [a.reshape(segs, gop, *a.shape[1:]) for a in [Y] + wide]
    conv = [np.empty_like(a) for a in (U, V)]
    d_out = [ctx.alloc(U[0].nbytes) for _ in range(2)]
    for i in range(segs * gop):
        d_in = [ctx.to_device(a[i]) for a in wide]
        ctx.chroma_convert(av1mi.CHROMA_444, 10, 10, W, H, 1, [None] + d_in, [None] + d_out)
        ctx.sync()
        for p in range(2):
            conv[p][i] = d_out[p].download(U[0].shape, np.uint16)
            d_in[p].free()
    for b in d_out:
        b.free()
    src420 = [a.reshape(segs, gop, *a.shape[1:]) for a in [Y] + conv]
    kbs = 32 if W % 32 == 0 else 0
    legs = [E2eLeg(ctx, "420_converted_beforehand", src420, W, H, q, gop, threads, kbs),
            E2eLeg(ctx, "444_10bit", src444, W, H, q, gop, threads, kbs, source_chroma=av1mi.CHROMA_444)]
    for leg in legs:
        leg.timed(1, record=False)      # warm up
    for rep in range(reps):
        for leg in legs:
            leg.timed(steps)
    res = {leg.name: leg.result() for leg in legs}
    res["bytes_per_coded_frame_are_equal"] = len({round(r["coded_bytes_per_frame"], 6) for r in res.values()}) == 1
    res["frames_per_s_444_over_420"] = res["444_10bit"]["frames_per_s"]["median"] / res["420_converted_beforehand"]["frames_per_s"]["median"]
    res["qindex"] = q
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chroma_formats.json"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=12, help="stacked frames of the kernel leg = segments of the end-to-end leg")
    ap.add_argument("--gop", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2, help="GOPs per timed end-to-end window")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--qindex", type=int, default=128)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    W, H = args.width, args.height
    out = {"what": __doc__.strip().split("\n\n")[0], "date": time.strftime("%Y-%m-%d"), "width": W, "height": H, "frames": args.frames, "gop": args.gop,
           "repetitions": args.reps, "host_threads": args.threads}
    with av1mi.Context(0) as ctx:
        out["device"] = ctx.device_name
        out["kernel"] = kernel_leg(ctx, W, H, args.frames, args.reps, args.launches)
        print(json.dumps({"kernel": out["kernel"]}), flush=True)
        if not args.no_e2e:
            out["end_to_end"] = e2e(ctx, W, H, args.frames, args.gop, args.qindex, args.reps, args.steps, args.threads)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
