#!/usr/bin/env python3
"""The restoration search, measured.  Writes profiles/lr_search.json (PROF_OUT overrides the directory).

  stage     av1mi_lr_search (zeroing launch + k_lr_search + k_lr_pick) on one batch of 12 frames of 3840 x 2160, 10 bit, beside
            av1mi_lr_yuv_decide with the policy's record and with the chosen units, from the library's own event profile.
  session   GOP sessions of 12 segments at the same size, lr_search 1 against 0, at q 23 and q 128, two runs per leg: frames per
            second of submit + collect (the source is written into the session's pinned planes before the clock starts, so the
            figure includes the upload, unlike bench.py's `value`), luma PSNR from the session's quality records, coded bytes per
            frame, units filtered.  The legs run in ONE process on the same frames; the search is off in the parent commit, so the
            "off" leg is the parent's path.
  --cpu-filters   no GPU: the oracle experiment on the low-pass filter L: the summed cost J of the best
            candidate per unit at q 23 / 128 / 200 on the oracle chain's CDEF output of the synthetic frames, for several L.

Content: the left half of every frame is flat, the right half the synthetic texture, under noise: the choice varies over the units.

    python tools/bench_lr_search.py [--frames 12] [--width 3840] [--height 2160] [--bd 10] [--reps 10] [--batches 6]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def content(w, h, bd, n, seed=1):
    """n frames (Y, U, V): flat left half, textured right half that moves two samples a frame, +-2 (8-bit scale) noise everywhere"""
    import synth
    rng = np.random.default_rng(seed)
    tw, th = min(w, 512), min(h, 512)
    tex = [a[0] for a in synth.frames(tw, th, 1, bd, 3)]
    dt = np.uint8 if bd == 8 else np.uint16
    out = []
    for p, t in enumerate(tex):
        hh, ww = (h >> (p > 0)), (w >> (p > 0))
        base = np.tile(t, (hh // t.shape[0] + 1, ww // t.shape[1] + 1))[:hh, :ww].astype(np.int32)
        frames = np.empty((n, hh, ww), dt)
        for f in range(n):
            a = np.roll(base, 2 * f >> (p > 0), axis=1)
            a[:, :ww // 2] = 1 << (bd - 1)
            a = a + rng.integers(-2 << (bd - 8), (2 << (bd - 8)) + 1, a.shape)
            frames[f] = np.clip(a, 0, (1 << bd) - 1)
        out.append(frames)
    return out


def stage(ctx, av1mi, a, res):
    w, h, bd, nf = a.width, a.height, a.bd, a.frames
    dims = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    src = content(w, h, bd, nf)
    rng = np.random.default_rng(2)
    cdef = [np.clip(s.astype(np.int32) + rng.integers(-3 << (bd - 8), (3 << (bd - 8)) + 1, s.shape), 0, (1 << bd) - 1).astype(s.dtype) for s in src]
    d_c, d_s = [ctx.to_device(x) for x in cdef], [ctx.to_device(x) for x in src]
    out = [ctx.alloc(x.nbytes) for x in cdef]
    n = av1mi.lr_search_units(w, h)
    per = [max(1, (hh + 32) // 64) * max(1, (ww + 32) // 64) for hh, ww in dims]
    scr = ctx.alloc(av1mi.lr_search_scratch_bytes(w, h, nf))
    d_u = [ctx.alloc(nf * k * 8) for k in per]
    d_choice = ctx.alloc(nf * n)
    search = av1mi.LrSearchJob(w, h, bd, nf, 64, a.stage_q, w, w // 2, *[b.ptr for b in d_c + d_c + d_s], scr.ptr, *[b.ptr for b in d_u], d_choice.ptr)
    p = av1mi.policy_frame_params(a.stage_q, bd, 1)
    pol = [ctx.to_device(np.array(list(p.lr_unit_y), np.int8)), ctx.to_device(np.array(list(p.lr_unit_uv), np.int8))]
    dscr = ctx.alloc(ctx.lr_yuv_decide_scratch_bytes(h, nf))
    on = ctx.alloc(3 * nf + 4)
    policy = av1mi.LrDecideJob(w, h, bd, nf, 64, w, w // 2, *[b.ptr for b in d_c + d_c + out + d_s], pol[0].ptr, pol[1].ptr, 0, 0, dscr.ptr, on.ptr, 1)
    chosen = av1mi.LrDecideJob(w, h, bd, nf, 64, w, w // 2, *[b.ptr for b in d_c + d_c + out + d_s], d_u[0].ptr, d_u[1].ptr, per[0], per[1], dscr.ptr,
                               on.ptr, 1, d_u[2].ptr, per[2])
    for name, run in (("lr_search", lambda: ctx.lr_search(search)), ("lr_yuv_decide_policy", lambda: ctx.lr_yuv_decide(policy)),
                      ("lr_yuv_decide_chosen_units", lambda: ctx.lr_yuv_decide(chosen))):
        for _ in range(3):
            run()
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(1)
        for _ in range(a.reps):
            run()
        ctx.sync()
        launches, ms = ctx.prof_get()["loop_restoration"]
        ctx.prof_enable(0)
        res[name] = dict(launches_per_call=launches / a.reps, ms_per_batch=ms / a.reps)
    choice = d_choice.download((nf * n,), np.uint8)
    res["stage_qindex"] = a.stage_q
    res["units_filtered_share"] = float((choice != 0).mean())
    res["candidate_histogram"] = np.bincount(choice, minlength=9).tolist()
    for b in d_c + d_s + out + d_u + pol + [scr, d_choice, dscr, on]:
        b.free()


def session_leg(ctx, av1mi, a, planes, q, lr_search):
    """one session: a key batch and a.batches - 1 P batches of a.frames segments; the clock runs over submit + collect"""
    w, h, bd, S = a.width, a.height, a.bd, a.frames
    sess = av1mi.GopSession(ctx, w, h, bd, q, a.batches, S, gpu_entropy=1, key_block_size=32 if w % 32 == 0 else 8, quality_stats=1, lr_search=lr_search)
    sse = samples = nbytes = filtered = units = 0
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
        if "lr_choice" in fr:
            per = list(fr["raw"].lr_units_per_frame)
            first = np.concatenate([[0], np.cumsum(per)])
            for p in range(3):
                c = fr["lr_choice"][:, first[p]:first[p + 1]]
                filtered += int(((c != 0) & (fr["lr_on"][:, p:p + 1] != 0)).sum())
            units += fr["lr_choice"].size
    fallbacks = sess.entropy_fallbacks()
    sess.close()
    frames = a.batches * S
    mse = sse / max(samples, 1)
    psnr = 10 * np.log10(((1 << bd) - 1) ** 2 / mse) if mse > 0 else float("inf")
    return dict(frames_per_s=frames / elapsed, luma_psnr_db=float(psnr), bytes_per_frame=nbytes / frames, units_filtered=filtered, units=units, entropy_fallbacks=int(fallbacks))


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


def cpu_filters(a):
    """the oracle experiment on L: per candidate table the sum over units, planes, frames and q of min_c J_c"""
    import lr_search_ref as R
    import pipeline
    import synth
    from oracle import oracle as O
    O.build()
    w, h, bd = 192, 136, 8
    Y, U, V = synth.frames(w, h, 2, bd, 5)
    shapes = {"L=(0,2,14)": (0, 2, 14), "(0,0,12)": (0, 0, 12), "(0,4,16)": (0, 4, 16), "(2,4,14)": (2, 4, 14), "(0,-2,18)": (0, -2, 18), "(-2,0,20)": (-2, 0, 20)}
    out = {}
    for q in (23, 128, 200):
        ref, chain = None, []
        for t in range(2):
            pa = pipeline.policy_arrays(q, bd, t, w, h)
            src = (Y[t], U[t], V[t])
            if t == 0:
                r = O.intra_encode_frame(*src, bd, 8, q)
                skip8 = np.zeros((h // 8, w // 8), np.uint8)
            else:
                r = O.inter_encode_frame(src, ref, bd, q, 8)
                skip8 = r["skip"].reshape(h // 8, w // 8)
            dbl = [O.deblock_plane(r["rec_y"], bd, 0, pa["mi_y"]), O.deblock_plane(r["rec_u"], bd, 1, pa["mi_c"]), O.deblock_plane(r["rec_v"], bd, 1, pa["mi_c"])]
            cdef = O.cdef_frame(dbl[0], dbl[1], dbl[2], bd, pa["cdef_damping"], pa["cdef_sb"], skip8)
            lr = [O.lr_plane(cdef[p], dbl[p], bd, int(p > 0), pa["lr_unit"], pa["lr_units_c"] if p else pa["lr_units_y"]) for p in range(3)]
            ref, _ = O.lr_select(src, cdef, lr, bd)
            chain.append((src, cdef, dbl))
        for name, taps in shapes.items():
            saved = R.FILTERS
            R.FILTERS = ((saved[0][0], saved[0][1], taps), (saved[1][0], saved[1][1], (0,) + tuple(taps[1:])))
            total = 0
            for src, cdef, dbl in chain:
                for p in range(3):
                    _, j = R.pick(R.sse_table(O, cdef[p], dbl[p], src[p], bd, int(p > 0)), int(p > 0), R.lam(O, q, bd))
                    total += int(j.min(axis=1).sum())
            R.FILTERS = saved
            out.setdefault(name, {})["q%d" % q] = total
    for name in out:
        out[name]["sum"] = sum(out[name].values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bd", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--stage-q", dest="stage_q", type=int, default=60)
    ap.add_argument("--cpu-filters", action="store_true")
    a = ap.parse_args()
    if a.cpu_filters:
        print(json.dumps(cpu_filters(a), indent=1))
        return
    import av1mi
    res = {}
    with av1mi.Context(0) as ctx:
        stage(ctx, av1mi, a, res)
        sessions(ctx, av1mi, a, res)
        rec = dict(tool="tools/bench_lr_search.py", device=ctx.device_name, width=a.width, height=a.height, bit_depth=a.bd, frames=a.frames, reps=a.reps,
                   batches=a.batches, **res)
    outdir = os.environ.get("PROF_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "lr_search.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
