#!/usr/bin/env python3
"""What scaling on the GPU (include/av1mi.h "scaling", av1-go_amd/csrc/scale_kernels.hip) costs, each number beside what it is
measured against, in the same process, legs alternated, `--reps` repetitions with min / median / max:

1. The scale launch alone on a 12-segment batch — 3840x2160 -> 1920x1080 (10 bit), 1440x1080 -> 1920x1080 (8 bit) and
   3840x2160 -> 3840x2160 (the identity, 10 bit) — HIP events around `--launches` launches, beside av1mi_copy (device to device)
   moving the same number of bytes (read + written): the yardstick is the copy.
2. With --parent-lib: `bench.py --gpus 1 --steps 10 --warmup 2` for this tree's library and for that build of the parent commit's
   (AV1MI_LIB), alternated: the unscaled path must not shift.

    python tools/bench_scale.py --out profiles/scale.json [--parent-lib /path/to/parent/libav1mi.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))

import av1mi      # noqa: E402

CASES = [("4k_to_1080p_10bit", 10, (3840, 2160), (1920, 1080)), ("1440x1080_to_1080p_8bit", 8, (1440, 1080), (1920, 1080)),
         ("4k_identity_10bit", 10, (3840, 2160), (3840, 2160))]


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def r8(n):
    return (n + 7) & ~7


def kernel_leg(ctx, segs, reps, launches):
    out = {}
    for name, bd, (sw, sh), (dw, dh) in CASES:
        bps = 1 if bd == 8 else 2
        n_in = [r8(sw) * r8(sh) * segs * bps // (1 if p == 0 else 4) for p in range(3)]
        n_out = [r8(dw) * r8(dh) * segs * bps // (1 if p == 0 else 4) for p in range(3)]
        # the bytes the kernel must move: the true source samples once, the coded destination once
        read = ((sw * sh) + 2 * ((sw + 1) // 2) * ((sh + 1) // 2)) * segs * bps
        total = read + sum(n_out)
        rng = np.random.default_rng(bd)
        d_in = []
        for k in n_in:
            a = rng.integers(0, 1 << bd, k // bps, dtype=np.uint16)
            d_in.append(ctx.to_device(a.astype(np.uint8) if bd == 8 else a))
        d_out = [ctx.alloc(k) for k in n_out]
        d_a, d_b = ctx.alloc(total // 2), ctx.alloc(total // 2)      # a copy that reads and writes `total` bytes together
        scale, copy = [], []
        for rep in range(reps + 1):      # the first repetition warms up
            ctx.timer_begin()
            for _ in range(launches):
                ctx.scale_planes(bd, sw, sh, dw, dh, segs, d_in, d_out)
            t_scale = ctx.timer_end() / launches
            ctx.timer_begin()
            for _ in range(launches):
                ctx.copy(d_b, d_a, total // 2)
            t_copy = ctx.timer_end() / launches
            if rep:
                scale.append(t_scale)
                copy.append(t_copy)
        for b in d_in + d_out + [d_a, d_b]:
            b.free()
        gbs = lambda ms: total / (ms * 1e-3) / 1e9
        taps = [av1mi.scale_filter(sw, dw)[0], av1mi.scale_filter(sh, dh)[0]]
        out[name] = {"bit_depth": bd, "source": [sw, sh], "target": [dw, dh], "frames": segs, "taps_h_v": taps, "bytes_read": read, "bytes_written": sum(n_out),
                     "scale_ms": spread(scale), "scale_gb_per_s": gbs(statistics.median(scale)),
                     "copy_same_bytes_ms": spread(copy), "copy_gb_per_s": gbs(statistics.median(copy)),
                     "scale_rate_over_copy_rate": statistics.median(copy) / statistics.median(scale)}
    return out


def bench_leg(parent_lib, reps, timeout):
    """bench.py's headline for this tree's library and the parent's, alternated, one fresh process each"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale.json"))
    ap.add_argument("--segments", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libav1mi.so built from the parent commit: adds the bench.py A/B")
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--bench-timeout", type=int, default=400, help="seconds for one bench.py process")
    args = ap.parse_args()
    out = {"what": __doc__.strip().split("\n\n")[0], "date": time.strftime("%Y-%m-%d"), "segments": args.segments, "repetitions": args.reps,
           "launches_per_repetition": args.launches}
    with av1mi.Context(0) as ctx:
        out["device"] = ctx.device_name
        out["kernel"] = kernel_leg(ctx, args.segments, args.reps, args.launches)
    print(json.dumps({"kernel": out["kernel"]}), flush=True)
    if args.parent_lib:
        out["bench_py"] = bench_leg(args.parent_lib, args.bench_reps, args.bench_timeout)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
