#!/usr/bin/env python3
"""What the quality records (include/av1mi.h "quality", av1-go_amd/csrc/quality_kernels.hip) cost, each number beside what it is measured
against, legs alternated, `--reps` repetitions with min / median / max:

(a) The two launches alone on a 12-frame batch — 3840x2160 10 bit and 1920x1080 8 bit — HIP events around `--launches` calls: time
    and the share of the device-to-device copy rate (av1mi_copy moving the same number of bytes, measured in the same loop) against the
    algorithmic bytes 2 b S (source + decoded picture, each sample once).
(b) The bench's session (4K 10 bit, GOP 30, 12 segments, GPU coder, device-resident source) with quality_stats 0 and 1: one fresh process
    per run, the two arms alternated, frames per second end to end.
(c) With --parent-lib: `bench.py --gpus 1 --steps 10 --warmup 2` for this tree's library and for that build of the parent commit's
    (AV1MI_LIB), alternated: with the option off the headline must lie within the parent's own spread.

    python tools/bench_quality.py --out profiles/quality.json [--parent-lib /path/to/parent/libav1mi.so]
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

CASES = [("4k_10bit", 10, 3840, 2160), ("1080p_8bit", 8, 1920, 1080)]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags of av1-go_amd/Makefile, device side only
RESOURCE_CMD = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only",
                "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join("csrc", "quality_kernels.hip")]
RESOURCE_KEYS = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "LDS Size [bytes/block]": "lds_bytes",
                 "Occupancy [waves/SIMD]": "waves_per_simd", "VGPRs Spill": "vgpr_spills", "SGPRs Spill": "sgpr_spills"}


def resources():
    """the compiler's resource report of the kernels, taken from a compilation of the source as it stands (not transcribed)"""
    import re
    try:
        p = subprocess.run(RESOURCE_CMD, cwd=os.path.join(ROOT, "av1-go_amd"), capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.TimeoutExpired) as e:
        return {"derived": False, "why": "could not run %s: %s" % (HIPCC, e)}
    if p.returncode != 0:
        return {"derived": False, "why": "%s failed with %d: %s" % (HIPCC, p.returncode, p.stderr[-500:])}
    out, cur = {"derived": True, "how": "hipcc -Rpass-analysis=kernel-resource-usage, the Makefile's flags, at the time of the run"}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = "k_quality_sum" if "k_quality_sum" in val else "k_quality_tiles_8bit" if "k_quality_tilesIh" in val else \
                  "k_quality_tiles_10bit" if "k_quality_tilesIt" in val else val
            out[cur] = {}
        elif cur and key in RESOURCE_KEYS:
            out[cur][RESOURCE_KEYS[key]] = int(val)
    if not all(k in out for k in ("k_quality_tiles_8bit", "k_quality_tiles_10bit", "k_quality_sum")):
        return {"derived": False, "why": "the compiler's report names none of the kernels", "report": p.stderr[-1000:]}
    return out


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs), "n": len(xs)}


def r8(n):
    return (n + 7) & ~7


def kernel_leg(ctx, frames, reps, launches):
    out = {}
    for name, bd, w, h in CASES:
        bps = 1 if bd == 8 else 2
        sizes = [r8(w) * r8(h) * frames * bps // (1 if p == 0 else 4) for p in range(3)]
        total = 2 * (w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)) * frames * bps      # 2 b S
        rng = np.random.default_rng(bd)
        src, dec = [], []
        for k in sizes:
            a = rng.integers(0, 1 << bd, k // bps, dtype=np.uint16)
            b = np.clip(a.astype(np.int32) + rng.integers(-3, 4, k // bps), 0, (1 << bd) - 1).astype(np.uint16)
            src.append(ctx.to_device(a.astype(np.uint8) if bd == 8 else a))
            dec.append(ctx.to_device(b.astype(np.uint8) if bd == 8 else b))
        d_out = ctx.alloc(frames * 3 * av1mi.QUALITY_DTYPE.itemsize)
        d_a, d_b = ctx.alloc(total // 2), ctx.alloc(total // 2)      # a copy that reads and writes `total` bytes together
        ctx.lib.av1mi_quality_planes.argtypes = [av1mi.C.c_void_p] + [av1mi.C.c_int] * 4 + [av1mi.C.c_void_p] * 5
        arr = lambda bufs: (av1mi.C.c_void_p * 3)(*[b.ptr for b in bufs])
        ps, pd = arr(src), arr(dec)
        q_ms, c_ms = [], []
        for rep in range(reps + 1):      # the first repetition warms up
            ctx.timer_begin()
            for _ in range(launches):
                ctx._chk(ctx.lib.av1mi_quality_planes(ctx.h, bd, w, h, frames, ps, pd, None, None, d_out.ptr))
            t_q = ctx.timer_end() / launches
            ctx.timer_begin()
            for _ in range(launches):
                ctx.copy(d_b, d_a, total // 2)
            t_c = ctx.timer_end() / launches
            if rep:
                q_ms.append(t_q)
                c_ms.append(t_c)
        for b in src + dec + [d_out, d_a, d_b]:
            b.free()
        gbs = lambda ms: total / (ms * 1e-3) / 1e9
        out[name] = {"bit_depth": bd, "size": [w, h], "frames": frames, "algorithmic_bytes": total, "quality_ms": spread(q_ms),
                     "quality_gb_per_s": gbs(statistics.median(q_ms)), "copy_same_bytes_ms": spread(c_ms), "copy_gb_per_s": gbs(statistics.median(c_ms)),
                     "quality_rate_over_copy_rate": statistics.median(c_ms) / statistics.median(q_ms)}
    return out


def session_once(quality, batches, warm):
    """the bench's session configuration, device-resident source: frames per second over `batches` batches after `warm`"""
    sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))
    import synth
    w, h, bd, gop, segs, q = 3840, 2160, 10, 30, 12, 128
    with av1mi.Context(0) as ctx:
        Y, U, V = synth.frames(w, h, 3, bd, 7)
        held = [[ctx.to_device(np.concatenate([a[t]] * segs)) for a in (Y, U, V)] for t in range(3)]
        s = av1mi.GopSession(ctx, w, h, bd, q, gop, segs, gpu_entropy=1, key_block_size=32, quality_stats=quality)
        n, t0, psnr = 0, None, None
        for t in range(warm + batches):
            if t == warm:
                while s.pending():
                    s.collect_raw()
                ctx.sync()
                t0 = time.perf_counter()
            s.submit_device(*held[t % 3])
            if s.pending() > 2:
                fr = s.collect()
                if quality:
                    psnr = av1mi.quality_psnr(fr["quality"][:, 0], bd)
        while s.pending():
            s.collect_raw()
        dt = time.perf_counter() - t0
        n = batches * segs
        s.close()
        return {"frames_per_s": n / dt, "last_psnr_y": psnr}


def session_leg(reps, batches, warm, timeout):
    runs = {0: [], 1: []}
    for _ in range(reps):
        for quality in (0, 1):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--session-once", str(quality), "--batches", str(batches), "--warm", str(warm)],
                               cwd=ROOT, capture_output=True, text=True, timeout=timeout)
            if p.returncode != 0:
                raise RuntimeError("session run (quality_stats %d) failed with %d: %s" % (quality, p.returncode, p.stderr[-2000:]))
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            runs[quality].append(res["frames_per_s"])
            print(json.dumps({"session_quality_stats": quality, **res}), flush=True)
    m0, m1 = statistics.median(runs[0]), statistics.median(runs[1])
    return {"config": "3840x2160 10 bit, GOP 30, 12 segments, q 128, gpu_entropy 1, key_block_size 32, submit_device, three batches in flight",
            "batches_timed": batches, "batches_warmup": warm, "off_frames_per_s": spread(runs[0]), "on_frames_per_s": spread(runs[1]),
            "off_runs": runs[0], "on_runs": runs[1], "on_over_off_median": m1 / m0}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality.json"))
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--session-reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--session-timeout", type=int, default=240, help="seconds for one session process")
    ap.add_argument("--skip-session", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libav1mi.so built from the parent commit: adds the bench.py A/B")
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--bench-timeout", type=int, default=400, help="seconds for one bench.py process")
    ap.add_argument("--session-once", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--resources-only", action="store_true", help="print the compiler's resource report of the kernels and stop (needs no GPU)")
    args = ap.parse_args()
    if args.session_once is not None:
        print(json.dumps(session_once(args.session_once, args.batches, args.warm)))
        return
    if args.resources_only:
        print(json.dumps(resources(), indent=1))
        return
    out = {"what": __doc__.strip().split("\n\n")[0], "date": time.strftime("%Y-%m-%d"), "frames": args.frames, "repetitions": args.reps,
           "launches_per_repetition": args.launches, "resources": resources()}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    with av1mi.Context(0) as ctx:
        out["device"] = ctx.device_name
        out["kernel"] = kernel_leg(ctx, args.frames, args.reps, args.launches)
    print(json.dumps({"kernel": out["kernel"]}), flush=True)
    save()
    if not args.skip_session:
        out["session"] = session_leg(args.session_reps, args.batches, args.warm, args.session_timeout)
        save()
    if args.parent_lib:
        out["bench_py"] = bench_leg(args.parent_lib, args.bench_reps, args.bench_timeout)
        save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
