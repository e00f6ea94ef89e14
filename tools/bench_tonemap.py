#!/usr/bin/env python3
"""What tone mapping (include/av1mi.h "tone mapping", av1-go_amd/csrc/tonemap_kernels.hip) costs, `--reps` repetitions with min / median / max:

(a) k_tone_map alone on a batch of 12 frames, 3840x2160 and 1920x1080 at 10 bits, HIP events around one launch on the restored source per repetition: time per batch,
    the rate over the algorithmic bytes 3 S 2 (S luma samples; 1.5 samples per luma sample, 2 bytes each, read and written once), that
    rate as a fraction of the HBM peak (8 TB/s) and beside av1mi_copy moving the same number of bytes in the same loop.
(b) `bench.py --gpus 1 --steps 10 --warmup 2` (tone_map off: the headline workload) for this tree's library and, with --parent-lib, for
    that build of the parent commit's (AV1MI_LIB), alternated.

    python tools/bench_tonemap.py --out profiles/tonemap.json [--parent-lib /path/to/parent/libav1mi.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))

import av1mi      # noqa: E402

CASES = [("4k_10bit_x12", 3840, 2160, 12), ("1080p_10bit_x12", 1920, 1080, 12)]
HBM_PEAK = 8.0e12      # bytes per second, MI355X


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def kernel_leg(ctx, reps, launches):
    out = {}
    t = av1mi.tone_map_tables(1000)
    d_tab = ctx.to_device(np.frombuffer(bytes(t), np.uint8))
    rng = np.random.default_rng(1)
    for name, w, h, frames in CASES:
        n = w * h * frames
        # HDR-looking content: the whole legal range of codes (the lookups spread over the tables as a film's would)
        planes = [rng.integers(64, 941, n, dtype=np.uint16), rng.integers(384, 641, n // 4, dtype=np.uint16), rng.integers(384, 641, n // 4, dtype=np.uint16)]
        src = [ctx.to_device(p) for p in planes]
        work = [ctx.alloc(p.nbytes) for p in planes]
        total = 6 * n
        d_a, d_b = ctx.alloc(total // 2), ctx.alloc(total // 2)
        k_ms, c_ms = [], []
        try:
            ctx.tone_map(w, h, frames, work[0], work[1], work[2], d_tab)      # (warm: code object and tables)
            for _ in range(reps):
                for d, s, p in zip(work, src, planes):      # the map runs in place: every timed launch starts from the HDR source
                    ctx.copy(d, s, p.nbytes)
                ctx.sync()
                ctx.timer_begin()
                ctx.tone_map(w, h, frames, work[0], work[1], work[2], d_tab)
                k_ms.append(ctx.timer_end())
                ctx.timer_begin()
                for _ in range(launches):
                    ctx.copy(d_b, d_a, total // 2)
                c_ms.append(ctx.timer_end() / launches)
        finally:
            for b in src + work + [d_a, d_b]:
                b.free()
        rate = lambda ms: total / (ms * 1e-3)
        out[name] = {"width": w, "height": h, "frames": frames, "algorithmic_bytes": total, "tone_map_ms_per_batch": spread(k_ms),
                     "tone_map_bytes_per_s": rate(statistics.median(k_ms)), "fraction_of_hbm_peak": rate(statistics.median(k_ms)) / HBM_PEAK,
                     "copy_same_bytes_ms": spread(c_ms), "tone_map_rate_over_copy_rate": statistics.median(c_ms) / statistics.median(k_ms),
                     "note": "one launch per repetition, each on the restored HDR source; the copy is timed over --launches calls"}
    d_tab.free()
    return out


def bench_value(lib):
    env = dict(os.environ)
    if lib:
        env["AV1MI_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2"], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("bench.py failed: " + p.stderr[-800:])
    return json.loads(p.stdout.strip().splitlines()[-1])["value"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tonemap.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--bench-reps", type=int, default=2)
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    with av1mi.Context(0) as ctx:
        res = {"device": ctx.device_name, "hbm_peak_bytes_per_s": HBM_PEAK, "kernel": kernel_leg(ctx, a.reps, a.launches)}
    vals = {"this": [], "parent": []}
    for _ in range(a.bench_reps):      # alternated, a fresh process each
        vals["this"].append(bench_value(""))
        if a.parent_lib:
            vals["parent"].append(bench_value(a.parent_lib))
    res["bench_value_frames_per_s"] = {k: spread(v) for k, v in vals.items() if v}
    res["bench_command"] = "bench.py --gpus 1 --steps 10 --warmup 2"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
