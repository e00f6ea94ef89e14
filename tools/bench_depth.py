#!/usr/bin/env python3
"""What the depth reduction (include/av1mi.h "depth reduction", av1mi_gop_config.coded_bit_depth) costs and gains on the GPU, each number
beside what it is measured against, in the same process, legs alternated, `--reps` repetitions with min / median / max:

1. k_depth_reduce alone on a 12-frame 4K batch (past the Infinity Cache), HIP events around `--launches` launches, beside k_input_convert
   P010 at the same size: the yardstick DESIGN 5.00 set for pointwise input stages.  Bytes per second are read + written.
2. Session frames per second at 4K, q 23, the source resident in HBM (av1mi_gop_submit_device, GPU entropy coding): a 10-bit session as
   ever, the 10-bit session coded at 8 bits through the stage, and an 8-bit session fed the 8-bit planes the stage makes.  The first is the
   baseline, the third the ceiling; the stage's cost is the gap between the second and the third.
3. Ordered against round: bytes per frame (key and P frames apart) and PSNR-Y of the decoder's picture shifted left by 2 against the 10-bit
   source, on a smooth gradient that pans one sample per frame and on tests/synth.py's texture.

    python tools/bench_depth.py --out profiles/depth.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import av1mi      # noqa: E402
import synth      # noqa: E402


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def kernel_leg(ctx, W, H, frames, reps, launches):
    rows = H * frames
    ny, nc = W * rows, W * rows // 4
    rng = np.random.default_rng(1)
    d_in = [ctx.to_device(rng.integers(0, 1024, n, dtype=np.uint16)) for n in (ny, nc, nc)]
    d_out = [ctx.alloc(n) for n in (ny, nc, nc)]
    n_p = [av1mi.input_plane_bytes(av1mi.INPUT_P010, 10, p, W, rows) for p in range(3)]
    d_p = [ctx.to_device(rng.integers(0, 256, k, dtype=np.uint8)) for k in n_p if k]
    d_planar = [ctx.alloc(2 * n) for n in (ny, nc, nc)]
    red, conv = [], []
    for rep in range(reps + 1):      # the first repetition warms up
        ctx.timer_begin()
        for _ in range(launches):
            ctx.depth_reduce(av1mi.DEPTH_ORDERED, W, H, frames, d_in, d_out)
        t_red = ctx.timer_end() / launches
        ctx.timer_begin()
        for _ in range(launches):
            ctx.input_convert(av1mi.INPUT_P010, 10, W, rows, d_p, d_planar)
        t_conv = ctx.timer_end() / launches
        if rep:
            red.append(t_red)
            conv.append(t_conv)
    for b in d_in + d_out + d_p + d_planar:
        b.free()
    b_red, b_conv = (ny + 2 * nc) * 3, sum(n_p) + (ny + 2 * nc) * 2
    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9
    r, c = statistics.median(red), statistics.median(conv)
    return {"frames": frames, "depth_reduce_ms": spread(red), "depth_reduce_bytes": b_red, "depth_reduce_gb_per_s": gbs(b_red, r),
            "input_convert_p010_ms": spread(conv), "input_convert_p010_bytes": b_conv, "input_convert_p010_gb_per_s": gbs(b_conv, c),
            "rate_ratio_reduce_over_convert": gbs(b_red, r) / gbs(b_conv, c)}


class Leg:
    def __init__(self, ctx, name, W, H, bd, q, segs, planes, **kw):
        self.ctx, self.name, self.segs, self.planes = ctx, name, segs, planes
        self.sess = av1mi.GopSession(ctx, W, H, bd, q, len(planes), segs, gpu_entropy=1, key_block_size=32 if W % 32 == 0 else 0, **kw)
        self.runs, self.bytes = [], 0

    def gop(self):
        lag = self.sess.max_in_flight() - 1
        for t, p in enumerate(self.planes):
            self.sess.submit_device(p[0], p[1], p[2], 0 if t == 0 else 1)
            if t >= lag:
                self.bytes += int(self.sess.collect_raw().payload_bytes)
        while self.sess.pending():
            self.bytes += int(self.sess.collect_raw().payload_bytes)

    def timed(self, steps):
        self.bytes = 0
        self.ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.gop()
        self.ctx.sync()
        dt = time.perf_counter() - t0
        self.runs.append((self.segs * len(self.planes) * steps / dt, self.bytes / (self.segs * len(self.planes) * steps)))

    def result(self):
        fb = int(self.sess.entropy_fallbacks())
        self.sess.close()
        return {"frames_per_s": spread([r[0] for r in self.runs]), "coded_bytes_per_frame": self.runs[0][1], "entropy_fallbacks": fb}


def reduced_on_device(ctx, W, H, segs, p10, mode):
    out = [ctx.alloc(n) for n in (W * H * segs, W * H * segs // 4, W * H * segs // 4)]
    ctx.depth_reduce(mode, W, H, segs, p10, out)
    ctx.sync()
    return out


def session_leg(ctx, W, H, segs, T, q, reps, steps):
    Y, U, V = synth.frames(W, H, segs * T, 10, 0)
    src = [a.reshape(segs, T, *a.shape[1:]) for a in (Y, U, V)]
    p10 = [[ctx.to_device(np.ascontiguousarray(a[:, t]).reshape(-1, a.shape[-1])) for a in src] for t in range(T)]
    p8 = [reduced_on_device(ctx, W, H, segs, p, av1mi.DEPTH_ORDERED) for p in p10]
    legs = [Leg(ctx, "ten_bit", W, H, 10, q, segs, p10), Leg(ctx, "ten_to_eight", W, H, 10, q, segs, p10, coded_bit_depth=8, depth_dither=1),
            Leg(ctx, "eight_bit", W, H, 8, q, segs, p8)]
    for leg in legs:
        leg.gop()      # warm up
    for _ in range(reps):
        for leg in legs:
            leg.timed(steps)
    res = {leg.name: leg.result() for leg in legs}
    for b in [x for p in p10 + p8 for x in p]:
        b.free()
    a, b = res["ten_to_eight"]["frames_per_s"]["median"], res["eight_bit"]["frames_per_s"]["median"]
    res["stage_cost_ms_per_frame"] = 1e3 / a - 1e3 / b
    res["same_bytes_as_the_8_bit_session"] = res["ten_to_eight"]["coded_bytes_per_frame"] == res["eight_bit"]["coded_bytes_per_frame"]
    return res


def dither_leg(ctx, W, H, T, q):
    yy, xx = np.mgrid[0:H, 0:W]
    grad = []
    for t in range(T):      # 64 .. 940 over four widths' worth of samples: a quarter code per sample, panning one sample per frame
        Y = (256 + ((xx + t) * 220) // W + (yy * 60) // H).astype(np.uint16)
        grad.append((Y, np.full((H // 2, W // 2), 512, np.uint16) + (xx[::2, ::2] * 40 // W).astype(np.uint16), np.full((H // 2, W // 2), 480, np.uint16)))
    Ys, Us, Vs = synth.frames(W, H, T, 10, 0)
    clips = {"gradient": grad, "texture": [(Ys[t], Us[t], Vs[t]) for t in range(T)]}
    out = {}
    for cname, clip in clips.items():
        out[cname] = {}
        for mname, mode in (("round", av1mi.DEPTH_ROUND), ("ordered", av1mi.DEPTH_ORDERED)):
            s = av1mi.GopSession(ctx, W, H, 10, q, T, 1, gpu_entropy=1, key_block_size=32 if W % 32 == 0 else 0, coded_bit_depth=8, depth_dither=mode)
            size, sse = [], []
            for t, planes in enumerate(clip):
                for dst, a in zip(s.input_planes(), planes):
                    dst[:] = a
                s.submit(0 if t == 0 else 1)
                size.append(int(s.collect_raw().payload_bytes))
                ref = s.download_reference()[0].astype(np.int64) << 2
                sse.append(float(np.mean((ref - planes[0].astype(np.int64)) ** 2)))
            s.close()
            out[cname][mname] = {"key_frame_bytes": size[0], "p_frame_bytes_mean": statistics.mean(size[1:]), "p_frame_bytes": size[1:],
                                 "psnr_y_vs_10_bit_source_db": 10 * np.log10(1023.0 ** 2 / statistics.mean(sse))}
        o, r = out[cname]["ordered"], out[cname]["round"]
        out[cname]["ordered_over_round_p_bytes"] = o["p_frame_bytes_mean"] / max(r["p_frame_bytes_mean"], 1e-9)
        out[cname]["ordered_minus_round_psnr_db"] = o["psnr_y_vs_10_bit_source_db"] - r["psnr_y_vs_10_bit_source_db"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth.json"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--segments", type=int, default=12)
    ap.add_argument("--gop", type=int, default=4, help="frames per GOP of the session legs (a key frame and P frames)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2, help="GOPs per timed window")
    ap.add_argument("--qindex", type=int, default=23)
    ap.add_argument("--dither-size", type=int, nargs=2, default=[1280, 720])
    ap.add_argument("--dither-frames", type=int, default=8)
    args = ap.parse_args()
    W, H = args.width, args.height
    out = {"what": __doc__.strip().split("\n\n")[0], "date": time.strftime("%Y-%m-%d"), "width": W, "height": H, "segments": args.segments, "repetitions": args.reps}
    with av1mi.Context(0) as ctx:
        out["device"] = ctx.device_name
        out["kernel"] = kernel_leg(ctx, W, H, args.segments, args.reps, args.launches)
        print(json.dumps({"kernel": out["kernel"]}), flush=True)
        out["session"] = dict(session_leg(ctx, W, H, args.segments, args.gop, args.qindex, args.reps, args.steps), qindex=args.qindex, gop=args.gop)
        print(json.dumps({"session": out["session"]}), flush=True)
        out["dither"] = dict(dither_leg(ctx, args.dither_size[0], args.dither_size[1], args.dither_frames, args.qindex), qindex=args.qindex,
                             size=args.dither_size, frames=args.dither_frames)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
