#!/usr/bin/env python3
"""Measures the scene-cut option (-av1mi_scenecut) -> profiles/scenecut.json.  Not part of bench.py.

    python tools/bench_scenecut.py [--out profiles/scenecut.json] [--steps kernels,e2e,effect]

Every step that uses the GPU runs as a child process of its own under `timeout`; the steps are chained and nothing is started after a
step that failed, faulted or ran out of time.
  kernels  device time of the analysis (three launches) and of the gather at 4K 10-bit x 12 segments x 30 frames and at 1080p 8-bit,
           from the library's per-kernel profile (kind "scene"), median and range over the repetitions
  e2e      frames/s of av1mi_transcode on a clip WITHOUT cuts, option on and off alternating, >= 5 runs each, median and range
  effect   bytes, PSNR-Y, SSIM (from -av1mi_stats) and the key frames' positions on a 1080p clip with cuts, on against off, at q 128
           and q 24
The default sensitivity and the clips it was chosen on are recorded under "default" (computed on the CPU by tests/scene_ref.py)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "av1-go_amd"), os.path.join(ROOT, "tests")]
TRANSCODE = os.path.join(ROOT, "av1-go_amd", "host", "av1mi_transcode")


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def step_default():
    import av1stream
    import scene_clips as K
    import scene_ref as R
    c = K.DEFAULT_CLIPS
    out = dict(clips=c, scenecut_default=av1stream.SCENECUT_DEFAULT, ranges={})
    for bd in (8, 10):
        cut = R.records(K.cut_clip(c["w"], c["h"], c["cut"]["n"], bd, c["cut"]["cuts"])[0], bd)
        calm = dict(c["calm"])
        calm_r = R.records(K.calm_clip(c["w"], c["h"], calm.pop("n"), bd, **calm)[0], bd)
        a, b = R.cut_range(cut, c["cut"]["cuts"]), R.cut_range(calm_r, [])
        pct = lambda r: [round(100.0 * int(x["inter_sad"]) / max(1, int(x["intra_sad"])), 1) for x in r]
        out["ranges"]["%d bit" % bd] = dict(cut_clip=a, calm_clip=b, both=(max(a[0], b[0]), min(a[1], b[1])) if a and b else None,
                                            cut_clip_inter_over_intra_percent=pct(cut), calm_clip_inter_over_intra_percent=pct(calm_r))
    return out


def step_kernels():
    import ctypes as C
    import numpy as np
    import av1mi
    out = {}
    with av1mi.Context(0) as ctx:
        lib = ctx.lib
        lib.av1mi_scene_analyse.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2
        for name, w, h, bd, S, G in (("4k10_12x30", 3840, 2160, 10, 12, 30), ("1080p8_12x30", 1920, 1088, 8, 12, 30)):
            bps, n = (1 if bd == 8 else 2), S * G
            fb = [w * h * bps, w * h * bps // 4, w * h * bps // 4]
            store = [ctx.alloc(b * n) for b in fb]
            rng = np.random.default_rng(1)
            frame = rng.integers(0, 1 << bd, (h, w)).astype(np.uint8 if bd == 8 else np.uint16)
            for i in range(n):      # luma: noise shifted from frame to frame, so that the search has something to find
                ctx._chk(lib.av1mi_upload(ctx.h, C.c_void_p(store[0].ptr + i * fb[0]), np.roll(frame, i, axis=1).ctypes.data_as(C.c_void_p), C.c_size_t(fb[0])))
            for p in (1, 2):
                ctx.memset(store[p], 128, fb[p] * n)
            d_rec = ctx.alloc(n * 24)
            dst = [ctx.alloc(b * S) for b in fb]
            table = np.array([[store[p].ptr + ((s * G) % n) * fb[p] for p in range(3)] for s in range(S)], np.uint64)
            d_table = ctx.to_device(table)
            res = {}
            for what, call in (("analyse", lambda: ctx._chk(lib.av1mi_scene_analyse(ctx.h, bd, w, h, n, store[0].ptr, d_rec.ptr))),
                               ("gather", lambda: ctx.frames_gather(fb, S, d_table, dst))):
                call()
                ctx.sync()
                times = []
                for _ in range(7):
                    ctx.prof_reset()
                    ctx.prof_enable(1)
                    call()
                    times.append(ctx.prof_get()["scene"][1])
                    ctx.prof_enable(0)
                res[what + "_ms"] = med(times)
            res["analyse_frames"], res["gather_bytes"] = n, sum(fb) * S
            res["store_bytes_each"] = sum(fb) * n
            out[name] = res
            for b in store + dst + [d_rec, d_table]:
                b.free()
    return out


def run_job(y4m, out, extra, q, G, S, stats=None):
    argv = [TRANSCODE, "-i", y4m, "-global_quality:v:0", str(q), "-g", str(G), "-av1mi_segments", str(S)] + ([("-av1mi_stats"), stats] if stats else []) + extra + [out]
    t0 = time.perf_counter()
    subprocess.check_call(argv, timeout=600)
    return time.perf_counter() - t0


def step_e2e():
    import scene_clips as K
    w, h, n, G, S = 1920, 1088, 240, 30, 4
    out = dict(clip="calm_clip %dx%d, %d frames, 8 bit" % (w, h, n), gop=G, segments=S, on=[], off=[])
    with tempfile.TemporaryDirectory() as d:
        y4m = os.path.join(d, "calm.y4m")
        K.write_y4m(y4m, K.calm_clip(w, h, n, 8), 8)
        run_job(y4m, os.path.join(d, "w.ivf"), [], 110, G, S)      # warm-up (file cache, first use of the device)
        for i in range(5):
            for name, extra in (("off", []), ("on", ["-av1mi_scenecut", "15"])):
                out[name].append(n / run_job(y4m, os.path.join(d, name + ".ivf"), extra, 110, G, S))
    return dict(clip=out["clip"], gop=G, segments=S, frames_per_s_off=med(out["off"]), frames_per_s_on=med(out["on"]))


def step_effect():
    import scene_clips as K
    w, h, n, G, S, cuts = 1920, 1088, 120, 30, 4, (17, 49, 71, 100)
    out = dict(clip="cut_clip %dx%d, %d frames, 8 bit, cuts at %s" % (w, h, n, list(cuts)), gop=G, segments=S)
    with tempfile.TemporaryDirectory() as d:
        y4m = os.path.join(d, "cuts.y4m")
        K.write_y4m(y4m, K.cut_clip(w, h, n, 8, cuts), 8)
        for q in (128, 24):
            for name, extra in (("off", []), ("on", ["-av1mi_scenecut", "15"])):
                stats = os.path.join(d, "s.txt")
                env = dict(os.environ, AV1MI_DEBUG="1")
                p = subprocess.run([TRANSCODE, "-i", y4m, "-global_quality:v:0", str(q), "-g", str(G), "-av1mi_segments", str(S), "-av1mi_stats", stats] + extra +
                                   [os.path.join(d, "o.ivf")], env=env, stderr=subprocess.PIPE, timeout=600, check=True)
                lines = open(stats).read().splitlines()
                per = [dict(kv.split(":") for kv in ln.split()) for ln in lines[:-1]]
                summary = dict(kv.split(":") for kv in lines[-1].split()[1:])
                out["q%d_%s" % (q, name)] = dict(bytes=int(summary["bytes"]), psnr_y=float(summary["psnr_y"]), ssim_y=float(summary.get("ssim_y", "nan")),
                                                 keys=[int(x["n"]) for x in per if x["type"] == "K"], flagged=[int(x["n"]) for x in per if x.get("cut") == "1"],
                                                 entropy_fallbacks=p.stderr.decode().count("falls back to the host coder"))
    return out


STEPS = dict(default=(step_default, 300), kernels=(step_kernels, 600), e2e=(step_e2e, 900), effect=(step_effect, 900))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scenecut.json"))
    ap.add_argument("--steps", default="default,kernels,e2e,effect")
    ap.add_argument("--step", help="(internal) run one step and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(STEPS[a.step][0]()))
        sys.exit(0)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for name in a.steps.split(","):
        p = subprocess.run(["timeout", "-k", "10", str(STEPS[name][1]), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
        if p.returncode != 0:
            print("step %s ended with status %d: nothing more is started" % (name, p.returncode))
            res[name] = dict(failed=p.returncode)
            break
        res[name] = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(name, json.dumps(res[name])[:400])
    json.dump(res, open(a.out, "w"), indent=1)
