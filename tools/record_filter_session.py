#!/usr/bin/env python3
"""Records what two small GOP sessions produce — the tile payloads and the reference planes of every batch, as SHA-256 digests — into
tests/golden/deblock_cdef_session.json, and is the driver tests/test_gpu_deblock_cdef.py runs to compare a build against that record.

The record pins the in-loop filter chain of the session (deblocking, CDEF, loop restoration) bit for bit across a change of its
kernels: run it on the commit whose results are to be kept,

    python tools/record_filter_session.py --commit <that commit's hash>

and commit the file.  Cases: a session whose size is a multiple of 8 (the fused deblocking + CDEF kernel) and one fed at a true size
that is not (the two kernels on their own, then the edge replication)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deblock_cdef_session.json")

CASES = {
    "192x136": dict(width=192, height=136, visible=None, key_block_size=32),
    "200x136_true_197x131": dict(width=200, height=136, visible=(197, 131), key_block_size=8),      # (32 needs a width that is a multiple of 32)
}
BIT_DEPTH, QINDEX, GOP, SEGMENTS, FRAMES = 10, 110, 4, 2, 4


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(av1mi, ctx, case):
    """one GOP (a key frame + three P frames) of two segments; per batch a dict of digests"""
    import synth
    w, h, vis = case["width"], case["height"], case["visible"]
    planes = []
    for s in range(SEGMENTS):      # segments: the same texture further along its motion
        Y, U, V = synth.frames(w, h, FRAMES, BIT_DEPTH, first=5 * s)
        if vis:                    # the caller replicates the true picture's last column / row into the padding
            vw, vh = vis
            for a, cw, ch in ((Y, vw, vh), (U, (vw + 1) // 2, (vh + 1) // 2), (V, (vw + 1) // 2, (vh + 1) // 2)):
                a[:, :, cw:] = a[:, :, cw - 1:cw]
                a[:, ch:, :] = a[:, ch - 1:ch, :]
        planes.append((Y, U, V))
    sess = av1mi.GopSession(ctx, w, h, BIT_DEPTH, QINDEX, GOP, SEGMENTS, gpu_entropy=1, visible=vis, key_block_size=case["key_block_size"])
    out = []
    try:
        for t in range(FRAMES):
            dst = sess.input_planes()
            for p in range(3):
                dst[p][:] = np.concatenate([planes[s][p][t] for s in range(SEGMENTS)])
            sess.submit()
            fr = sess.collect()
            rec = dict(frame_type=int(fr["frame_type"]), lr_on=np.asarray(fr["lr_on"]).reshape(-1).tolist(),
                       tile_size=np.asarray(fr["tile_size"]).tolist(), tile_payload=_sha(fr["tile_payload"]))
            rec["reference"] = [_sha(a) for a in sess.download_reference()]
            out.append(rec)
    finally:
        sess.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="the commit this build is of (written into the record)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "av1-go_amd"))
    import av1mi
    with av1mi.Context(0) as ctx:
        rec = dict(recorded_from_commit=a.commit, bit_depth=BIT_DEPTH, qindex=QINDEX, gop=GOP, segments=SEGMENTS,
                   cases={name: run_case(av1mi, ctx, c) for name, c in CASES.items()})
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
