#!/usr/bin/env python3
"""What denoising (include/av1mi.h "denoising", av1mi_gop_config.denoise, -av1mi_denoise) costs and saves on the GPU.

1. k_denoise_gather + k_grain_sum beside k_frames_gather (the floor) and k_deint_gather on the same batch: 4K 10-bit x 12 segments and
   1080p 8-bit x 12, every leg alternated in one process, HIP events; bytes/s against 3.5 x bytes (the deinterlacer's row) and against the
   denoiser's own 4 x bytes (three reads, one write).
   k_denoise_search + k_denoise_mc_gather + k_grain_sum (av1mi_denoise_mc_gather, range 4 and 8) are further legs of the same alternation,
   and so is k_grain_cov + k_grain_cov_sum (av1mi_grain_cov, "grain covariance") on the same planes: what -av1mi_grain_lag adds to a batch,
   beside the gather it follows.
2. av1mi_run_transcode at q 23 and 24 on tests/synth.py content and on a translating clip (tests/denoise_mc_clips.py, 3 / -2 samples per
   frame), with Gaussian grain of sigma 2, 4, 8 added per frame; without -av1mi_denoise, with it, and with -av1mi_denoise_range 4 and 8:
   coded bytes and frames per second, wall clock.

    python tools/bench_grain.py --out profiles/grain.json
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


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def kernels(ctx, w, h, bd, segs, reps=7, launches=10):
    dt = np.uint8 if bd == 8 else np.uint16
    sizes = [(w, h), (w // 2, h // 2), (w // 2, h // 2)]
    rng = np.random.default_rng(1)
    nbytes = [sw * sh * dt().itemsize for sw, sh in sizes]
    # every segment has its own P, C, N: 3 x segs frames per plane, still content + noise (the weights are high: the measured path is the full one)
    base = [rng.integers(60, 200, (1, sh, sw)) for sw, sh in sizes]
    d_store = [ctx.to_device(np.clip((b << (bd - 8)) + rng.standard_normal((3 * segs, sh, sw), dtype=np.float32) * (2 << (bd - 8)), 0, (1 << bd) - 1).astype(dt)) for b, (sw, sh) in zip(base, sizes)]
    three = np.array([[[d_store[p].ptr + (3 * s + i) * nbytes[p] for i in range(3)] for p in range(3)] for s in range(segs)], np.uint64)
    one = np.ascontiguousarray(three[:, :, 1])
    d_three, d_one = ctx.to_device(three), ctx.to_device(one)
    d_dst = [ctx.alloc(segs * b) for b in nbytes]
    d_rec = ctx.alloc(segs * 3 * 16 * 16)
    d_cov = ctx.alloc(segs * 3 * av1mi.GRAIN_COV_DTYPE.itemsize)
    legs = dict(denoise=lambda: ctx.denoise_gather(bd, sizes, sizes, 4, segs, d_three, d_dst, d_rec),
                denoise_mc_range4=lambda: ctx.denoise_mc_gather(bd, sizes, sizes, 4, 4, segs, d_three, d_dst, d_rec),
                denoise_mc_range8=lambda: ctx.denoise_mc_gather(bd, sizes, sizes, 4, 8, segs, d_three, d_dst, d_rec),
                grain_cov=lambda: ctx.grain_cov(bd, sizes, sizes, segs, d_three, d_dst, d_cov),      # (no branch of it depends on the content)
                denoise_no_records=lambda: ctx.denoise_gather(bd, sizes, sizes, 4, segs, d_three, d_dst, None),
                deint=lambda: ctx.deinterlace_gather(bd, sizes, sizes, 0, segs, d_three, d_dst),
                frames=lambda: ctx.frames_gather(nbytes, segs, d_one, d_dst))
    times = {k: [] for k in legs}
    for f in legs.values():
        f()
    ctx.sync()
    for _ in range(reps):
        for name, f in legs.items():
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(launches):
                f()
            ctx.sync()
            times[name].append((time.perf_counter() - t0) * 1e3 / launches)
    frame = sum(nbytes) * segs
    md = statistics.median(times["denoise"])
    out = {"batch": "%dx%d %d-bit x %d segments" % (w, h, bd, segs), "batch_bytes": frame, "timing": "host clock around %d back-to-back launches, synchronised, %d repetitions alternated" % (launches, reps)}
    for k, v in times.items():
        out[k + "_ms"] = spread(v)
    out["denoise_gb_per_s_at_3.5_x_bytes"] = 3.5 * frame / md / 1e6
    out["denoise_gb_per_s_at_4_x_bytes"] = 4 * frame / md / 1e6
    out["deint_gb_per_s_at_3.5_x_bytes"] = 3.5 * frame / statistics.median(times["deint"]) / 1e6
    out["frames_gb_per_s_at_2_x_bytes"] = 2 * frame / statistics.median(times["frames"]) / 1e6
    for b in d_store + d_dst + [d_three, d_one, d_rec, d_cov]:
        b.free()
    return out


def transcodes(w, h, frames, runs=2):
    out = []
    clean = dict(synth=synth.frames(w, h, frames, 8, 5), pan=denoise_mc_clips.translating([(w, h), (w // 2, h // 2), (w // 2, h // 2)], frames, 8, 5, 0))
    with tempfile.TemporaryDirectory() as d:
        for content, sigma in ((c, s) for c in clean for s in (2, 4, 8)):
            rng = np.random.default_rng(sigma)
            clip = [np.clip(a + np.rint(rng.normal(0, sigma, a.shape)), 0, 255).astype(np.uint8) for a in clean[content]]
            src = os.path.join(d, "%s%d.y4m" % (content, sigma))
            deint_clips.write_y4m(src, clip, 8, interlace="p")
            den = ["-av1mi_denoise", max(sigma, 2) * 2]
            for q in (23, 24):
                for name, extra in (("plain", []), ("denoise", den), ("denoise_no_film_grain", den + ["-av1mi_film_grain", 0]),
                                    ("denoise_range4", den + ["-av1mi_denoise_range", 4]), ("denoise_range8", den + ["-av1mi_denoise_range", 8])):
                    fps = []
                    for _ in range(runs):
                        dst = os.path.join(d, "o.mkv")
                        t0 = time.perf_counter()
                        code, err = av1stream.run_transcode(["-i", src, "-global_quality:v:0", q, "-g", 30, "-av1mi_segments", 4] + extra + [dst])
                        fps.append(frames / (time.perf_counter() - t0))
                        assert code == 0, err
                    out.append(dict(size="%dx%d" % (w, h), frames=frames, content=content, sigma=sigma, q=q, run=name, args=[str(x) for x in extra], bytes=os.path.getsize(dst), frames_per_s=spread(fps)))
                    print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grain.json"))
    ap.add_argument("--frames", type=int, default=120)
    a = ap.parse_args()
    res = {"tool": "tools/bench_grain.py"}
    with av1mi.Context(0) as ctx:
        res["device"] = ctx.device_name
        res["kernels"] = [kernels(ctx, 3840, 2160, 10, 12), kernels(ctx, 1920, 1080, 8, 12)]
        for k in res["kernels"]:
            print(json.dumps(k), flush=True)
    res["transcode"] = transcodes(1920, 1080, a.frames)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
