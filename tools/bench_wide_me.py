#!/usr/bin/env python3
"""What the wide-range motion search (av1mi_gop_config.coarse_range; av1-go_amd/csrc/me_coarse_kernels.hip) buys and costs, each number
beside what it is measured on -> profiles/wide_me.json (PROF_OUT overrides the directory).

  effect    the figures tests/test_gpu_session_wide_me.py asserts: P-frame bytes and PSNR-Y of its fast pan with the option off and
            on, and of the same texture at (1.25, 0.75) samples per frame with the option off
  speeds    P-frame bytes, PSNR-Y and entropy_fallbacks for the texture at 1.25 .. 40 samples per frame, option off and on (64)
  kernels   HIP-event time of the coarse search's two launches and of k_me_int per batch of stacked frames (av1mi_prof_*), median of
            `--reps` batches; every kernel runs alone on the stream
  session   frames/s of a session fed from device memory (gpu_entropy 1) with coarse_range 0, 32 and 64 on the slow clip and on the
            fast pan, the settings alternating within one process; median and spread of `--reps` rounds
  hashes    SHA-256 of the option-off streams of the test's clips (run with AV1MI_LIB pointing at another build to compare builds)

Usage: python tools/bench_wide_me.py [--parts effect,speeds,kernels,session,hashes] [--reps 5] [--size 1920x1080] [--bd 10]"""
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
import av1mi  # noqa: E402
import me_ref as M  # noqa: E402
import test_gpu_session_wide_me as T  # noqa: E402


def effect(ctx):
    w, h, bd, q = T.CASES["pan8"]
    fast, slow = T.clip_of("pan", w, h, bd), T.clip_of("pan", w, h, bd, 1)
    off = T.run_session(ctx, av1mi, fast, bd, q, 0, mode=0, keep_refs=False)
    on = T.run_session(ctx, av1mi, fast, bd, q, 64, mode=0, keep_refs=False)
    sl = T.run_session(ctx, av1mi, slow, bd, q, 0, mode=0, keep_refs=False)
    return dict(size="%dx%d" % (w, h), bit_depth=bd, q=q, p_frames=(T.GOP - 1) * T.SEGS,
                off=dict(p_bytes=off["p_bytes"], psnr_y=off["p_psnr_y"]), on=dict(p_bytes=on["p_bytes"], psnr_y=on["p_psnr_y"]),
                slow_off=dict(p_bytes=sl["p_bytes"], psnr_y=sl["p_psnr_y"]),
                saving=1.0 - on["p_bytes"] / off["p_bytes"], ratio_on_to_slow=on["p_bytes"] / sl["p_bytes"])


def speeds(ctx, w, h, bd, qs):
    rows = []
    for scale in (1, 4, 8, 16, 32):
        clip = T.clip_of("pan", w, h, bd, scale)
        for q in qs:
            for cr in (0, 64):
                r = T.run_session(ctx, av1mi, clip, bd, q, cr, mode=2, compare_coders=False, keep_refs=False)
                rows.append(dict(size="%dx%d" % (w, h), bit_depth=bd, q=q, samples_per_frame=1.25 * scale, coarse_range=cr, p_frames=(T.GOP - 1) * T.SEGS,
                                 p_bytes=r["p_bytes"], psnr_y=r["p_psnr_y"], entropy_fallbacks=r["fallbacks"]))
                print(rows[-1], flush=True)
    return rows


def kernels(ctx, w, h, bd, frames, reps):
    Y, _, _ = M.pan_clip(w, h, 2, bd, 20)
    src, ref = np.repeat(Y[1:], frames, 0), np.repeat(Y[:1], frames, 0)
    out = {}
    ctx.prof_enable(1)
    try:
        for cr in (0, 32, 64):
            t = {"me_coarse": [], "me_integer": []}
            for _ in range(reps + 1):
                ctx.prof_reset()
                ctx.me_search(src, ref, bd, 8, cr)
                p = ctx.prof_get()
                for k in t:
                    t[k].append(p[k][1] if k in p else 0.0)
            out["coarse_range_%d" % cr] = {k + "_ms": statistics.median(v[1:]) for k, v in t.items()}      # the first batch warms up
    finally:
        ctx.prof_enable(0)
        ctx.prof_reset()
    return dict(size="%dx%d" % (w, h), bit_depth=bd, stacked_frames=frames, reps=reps, note="me_coarse = k_me_down + k_me_coarse", **out)


def session(ctx, w, h, bd, q, segs, gop, reps):
    clips = {"slow": M.pan_clip(w, h, segs * gop, bd, 1), "fast": M.pan_clip(w, h, segs * gop, bd, 20)}
    dev = {k: [[ctx.to_device(np.concatenate([a[sg * gop + t] for sg in range(segs)])) for a in c] for t in range(gop)] for k, c in clips.items()}
    fps = {}
    for rep in range(reps + 1):
        for name in clips:
            for cr in (0, 32, 64):
                s = av1mi.GopSession(ctx, w, h, bd, q, gop, segs, gpu_entropy=1, coarse_range=cr)
                ctx.sync()
                t0 = time.perf_counter()
                for rnd in range(3):
                    for t in range(gop):
                        s.submit_device(*dev[name][t])
                        if s.pending() > 2:
                            s.collect_raw()
                while s.pending():
                    s.collect_raw()
                dt = time.perf_counter() - t0
                fb = s.entropy_fallbacks()
                s.close()
                if rep:
                    fps.setdefault("%s_coarse_%d" % (name, cr), []).append(3 * gop * segs / dt)
                    fps.setdefault("%s_coarse_%d_fallbacks" % (name, cr), []).append(fb)
    for bufs in dev.values():
        for planes in bufs:
            for b in planes:
                b.free()
    out = {}
    for k, v in fps.items():
        out[k] = max(v) if k.endswith("fallbacks") else dict(median_fps=statistics.median(v), min_fps=min(v), max_fps=max(v))
    return dict(size="%dx%d" % (w, h), bit_depth=bd, q=q, segments=segs, gop=gop, reps=reps, **out)


def hashes(ctx):
    out = {}
    for case, (w, h, bd, q) in T.CASES.items():
        out[case] = T.sha(T.run_session(ctx, av1mi, T.clip_of("pan", w, h, bd), bd, q, 0, mode=0, keep_refs=False))
    return dict(library=av1mi.LIB_PATH, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="effect,speeds,kernels,session,hashes")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--bd", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.split("x"))
    parts = a.parts.split(",")
    res = {}
    with av1mi.Context(0) as ctx:
        res["device"] = ctx.device_name
        if "hashes" in parts:
            res["hashes"] = hashes(ctx)
        if "effect" in parts:
            res["effect"] = effect(ctx)
        if "kernels" in parts:
            res["kernels"] = kernels(ctx, 3840, 2160, 10, 12, a.reps)
        if "speeds" in parts:
            res["speeds"] = speeds(ctx, w, h, a.bd, (128, 23 if h >= 1440 else 24))
        if "session" in parts:
            res["session"] = session(ctx, w, h, a.bd, 128, 12, 4, a.reps)
    path = a.out or os.path.join(os.environ.get("PROF_OUT", os.path.join(ROOT, "profiles")), "wide_me.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
