#!/usr/bin/env python3
"""Do two builds of the host library write the same files?  45 transcode jobs without colour options or tone mapping — three synthetic clips
(192x128 at 8 and 10 bits, 130x70 at 10 bits; 7 frames, GOP 3, 2 segments, q 120: the shapes of tests/test_host.py's transcode tests) x five
option sets (none, the reference's filter chain, host entropy coding, -av1mi_pack10 1, key frames in 8x8 blocks) x .obu / .ivf / .mkv — run
through this tree's libav1mi_host.so and through another build's (a checkout of the parent commit, built), one child process per library;
the SHA-256 of every output is printed and compared.  Exit code 0 = all 45 equal.  Needs a GPU.

    python tools/compare_job_bytes.py /path/to/other/av1-go_amd/host/libav1mi_host.so
"""
import ctypes as C, hashlib, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "av1-go_amd", "host", "libav1mi_host.so")
sys.path.insert(0, os.path.join(ROOT, "av1-go_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
CHAIN = "scale_vaapi=w=ceil(iw/2)*2:h=ceil(ih/2)*2,hwdownload,format=nv12,setsar=1,format=nv12,hwupload"
def child(lib, d):
    h = C.CDLL(lib)
    buf = C.create_string_buffer(2048)
    for clip, bd in (("c8", 8), ("c10", 10), ("odd10", 10)):
        for name, extra in (("plain", []), ("chain", ["-vf:v:0", CHAIN]), ("host", ["-av1mi_gpu_entropy", "0"]), ("pack", ["-av1mi_pack10", "1"]), ("k8", ["-av1mi_key_block_size", "8"])):
            for ext in ("obu", "ivf", "mkv"):
                out = os.path.join(d, "%s_%s.%s" % (clip, name, ext))
                a = ["-hide_banner", "-i", os.path.join(d, clip + ".y4m"), "-global_quality:v:0", "120", "-g", "3", "-av1mi_segments", "2"] + extra + [out]
                rc = h.av1mi_host_run_transcode("\n".join(a).encode(), buf, 2048)
                print("%s %s %s rc=%d %s %s" % (clip, name, ext, rc, hashlib.sha256(open(out, "rb").read()).hexdigest() if rc == 0 else "-", buf.value.decode()[:80]), flush=True)
if len(sys.argv) > 2:
    child(sys.argv[1], sys.argv[2]); sys.exit(0)
if len(sys.argv) != 2:
    sys.exit(__doc__)
OTHER = os.path.abspath(sys.argv[1])
import numpy as np, synth, deint_clips as K
d = tempfile.mkdtemp()
for clip, w, h, bd in (("c8", 192, 128, 8), ("c10", 192, 128, 10), ("odd10", 130, 70, 10)):
    Y, U, V = synth.frames((w + 7) & ~7, (h + 7) & ~7, 7, bd, 3)
    K.write_y4m(os.path.join(d, clip + ".y4m"), [np.stack(Y)[:, :h, :w], np.stack(U)[:, :(h + 1) // 2, :(w + 1) // 2], np.stack(V)[:, :(h + 1) // 2, :(w + 1) // 2]], bd, interlace=None)
outs = []
for lib, sub in ((OTHER, "other"), (HERE, "this")):
    dd = os.path.join(d, sub); os.makedirs(dd)
    for f in os.listdir(d):
        if f.endswith(".y4m"): os.link(os.path.join(d, f), os.path.join(dd, f))
    r = subprocess.run([sys.executable, __file__, lib, dd], capture_output=True, text=True, timeout=240)
    if r.returncode: print(r.stderr[-2000:]); sys.exit(r.returncode)
    outs.append(r.stdout.splitlines())
bad = [(a, b) for a, b in zip(*outs) if a != b or "rc=0" not in a]
print("\n".join(outs[1])); print("jobs compared: %d, differing or failed: %d" % (len(outs[1]), len(bad)))
for a, b in bad: print("OTHER", a, "\nTHIS ", b)
sys.exit(1 if bad or not outs[1] else 0)
