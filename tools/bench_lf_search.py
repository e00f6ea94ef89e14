#!/usr/bin/env python3
"""The deblocking search, measured.  Writes profiles/lf_search.json (PROF_OUT overrides the directory).

  stage     av1mi_lf_search (k_lf_search + k_lf_pick + k_mi_levels_frames) on one batch of 12 frames of 3840 x 2160, 10 bit, beside
            av1mi_deblock_frames of the three planes with the written maps, from the library's own event profile ("deblock").
  session   GOP sessions of 12 segments at the same size, lf_search 1 against 0, at q 23 and q 128, two alternating runs per leg:
            frames per second of submit + collect (the source is written into the session's pinned planes before the clock starts, so
            the figure includes the upload, unlike bench.py's `value`), luma PSNR from the session's quality records, coded bytes per
            frame, the histogram of the chosen candidates.  The legs run in ONE process on the same frames; the search is off in the
            parent commit, so the "off" leg is the parent's path.

Content: bench_lr_search.py's (flat left half, textured right half, noise), so that the two searches' figures stand side by side.

    python tools/bench_lf_search.py [--frames 12] [--width 3840] [--height 2160] [--bd 10] [--reps 10] [--batches 6]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_lr_search import content      # noqa: E402


def stage(ctx, av1mi, a, res):
    import lf_search_ref as R
    w, h, bd, nf = a.width, a.height, a.bd, a.frames
    src = content(w, h, bd, nf)
    rng = np.random.default_rng(2)
    # a reconstruction with an offset per 8x8 (4x4 chroma) block on top of the source: blocking for the filters to work on
    rec = []
    for p, s in enumerate(src):
        b = 8 >> (p > 0)
        off = rng.integers(-4 << (bd - 8), (4 << (bd - 8)) + 1, (nf, s.shape[1] // b, s.shape[2] // b))
        rec.append(np.clip(s.astype(np.int32) + np.repeat(np.repeat(off, b, axis=1), b, axis=2), 0, (1 << bd) - 1).astype(s.dtype))
    d = [ctx.to_device(x) for x in rec + src]
    dbl = [ctx.alloc(x.nbytes) for x in rec]
    mi = [ctx.to_device(m) for m in R.base_maps(w, h)]
    ny, nc = (h // 4) * (w // 4), (h // 8) * (w // 8)
    scr, sse, choice, lv = ctx.alloc(av1mi.lf_search_scratch_bytes(w, h, nf)), ctx.alloc(nf * 128), ctx.alloc(nf * 2), ctx.alloc(nf * 4)
    out = [ctx.alloc(nf * ny * 4), ctx.alloc(nf * nc * 4)]
    p = av1mi.policy_frame_params(a.stage_q, bd, 1)
    job = av1mi.LfSearchJob(w, h, bd, nf, w, w // 2, *[b.ptr for b in d], 0, 0, mi[0].ptr, mi[1].ptr, w // 4, w // 8, 0, 0, C.addressof(p),
                            scr.ptr, sse.ptr, choice.ptr, lv.ptr, out[0].ptr, out[1].ptr)

    def deblock():
        for i in range(3):
            ss = int(i > 0)
            ctx.deblock_frames(d[i], w >> ss, dbl[i], w >> ss, w >> ss, h >> ss, bd, ss, out[ss], (w >> ss) // 4, (ny, nc)[ss], 0, nf)
    for name, run in (("lf_search", lambda: ctx.lf_search(job)), ("deblock_frames_with_the_maps", deblock)):
        for _ in range(3):
            run()
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(1)
        for _ in range(a.reps):
            run()
        ctx.sync()
        launches, ms = ctx.prof_get()["deblock"]
        ctx.prof_enable(0)
        res[name] = dict(launches_per_call=launches / a.reps, ms_per_batch=ms / a.reps)
    res["stage_qindex"] = a.stage_q
    res["stage_policy_levels"] = list(p.lf_level)
    res["stage_choice"] = choice.download((nf, 2), np.uint8).tolist()
    for b in d + dbl + mi + out + [scr, sse, choice, lv]:
        b.free()


def session_leg(ctx, av1mi, a, planes, q, lf_search):
    """one session: a key batch and a.batches - 1 P batches of a.frames segments; the clock runs over submit + collect"""
    w, h, bd, S = a.width, a.height, a.bd, a.frames
    sess = av1mi.GopSession(ctx, w, h, bd, q, a.batches, S, gpu_entropy=1, key_block_size=32 if w % 32 == 0 else 8, quality_stats=1, lf_search=lf_search)
    sse = samples = nbytes = 0
    hist = np.zeros((2, 8), np.int64)
    elapsed = 0.0
    for t in range(a.batches):
        for dst, src in zip(sess.input_planes(), planes):
            dst[:] = np.concatenate([src[(t + s) % len(src)] for s in range(S)])
        t0 = time.perf_counter()
        sess.submit()
        fr = sess.collect()
        elapsed += time.perf_counter() - t0
        q_rec = fr["quality"]
        sse += int(q_rec["sse"][:, 0].sum())
        samples += int(q_rec["samples"][:, 0].sum())
        nbytes += int(fr["raw"].payload_bytes)
        if "lf_choice" in fr:
            for g in range(2):
                hist[g] += np.bincount(fr["lf_choice"][:, g], minlength=8)
    fallbacks = sess.entropy_fallbacks()
    sess.close()
    frames = a.batches * S
    mse = sse / max(samples, 1)
    psnr = 10 * np.log10(((1 << bd) - 1) ** 2 / mse) if mse > 0 else float("inf")
    return dict(frames_per_s=frames / elapsed, luma_psnr_db=float(psnr), bytes_per_frame=nbytes / frames, choice_histogram_luma=hist[0].tolist(),
                choice_histogram_chroma=hist[1].tolist(), entropy_fallbacks=int(fallbacks))


def sessions(ctx, av1mi, a, res):
    planes = content(a.width, a.height, a.bd, 4, seed=3)
    res["session"] = {}
    for q in (23, 128):
        session_leg(ctx, av1mi, a, planes, q, 0)          # warm-up: the first session pays for the pinned allocations
        legs = {}
        for run in range(2):
            for name, flag in (("off", 0), ("on", 1)):
                legs.setdefault(name, []).append(session_leg(ctx, av1mi, a, planes, q, flag))
        res["session"]["q%d" % q] = legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bd", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--stage-q", dest="stage_q", type=int, default=60)
    a = ap.parse_args()
    import av1mi
    res = {}
    with av1mi.Context(0) as ctx:
        stage(ctx, av1mi, a, res)
        sessions(ctx, av1mi, a, res)
        rec = dict(tool="tools/bench_lf_search.py", device=ctx.device_name, width=a.width, height=a.height, bit_depth=a.bd, frames=a.frames, reps=a.reps,
                   batches=a.batches, **res)
    outdir = os.environ.get("PROF_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "lf_search.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
