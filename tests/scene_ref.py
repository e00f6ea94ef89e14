"""The scene analysis of include/av1mi.h ("scene analysis") restated in numpy: quarter planes, per-block inter / intra SADs, the
per-frame records and the cut rule.  Test infrastructure: the GPU kernels (av1-go_amd/csrc/scene_kernels.hip) must give these numbers
bit for bit."""
import numpy as np

RECORD_DTYPE = np.dtype([("inter_sad", "<u8"), ("intra_sad", "<u8"), ("blocks", "<u4"), ("reserved", "<u4")])      # av1mi_scene_record
assert RECORD_DTYPE.itemsize == 24


def quarter(P, bd):
    """Q of one luma plane [h, w] (multiples of 8): the 8-bit view, 4x4 box sums, + 8, >> 4"""
    v = (np.asarray(P).astype(np.uint32) >> (bd - 8)) & 0xFF
    h, w = v.shape
    return ((v.reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3)) + 8) >> 4).astype(np.int32)


def block_sads(Q, Qp):
    """(inter [nby, nbx], intra [nby, nbx]) of quarter plane Q against its predecessor Qp (None: inter = 0)"""
    qh, qw = Q.shape
    nby, nbx = (qh + 7) // 8, (qw + 7) // 8
    ys, xs = np.arange(8 * nby), np.arange(8 * nbx)
    cy, cx = np.minimum(ys, qh - 1), np.minimum(xs, qw - 1)
    cur = Q[cy][:, cx]
    per_block = lambda a: a.reshape(nby, 8, nbx, 8).sum(axis=(1, 3))
    m = (per_block(cur) + 32) >> 6
    intra = per_block(np.abs(cur - np.repeat(np.repeat(m, 8, axis=0), 8, axis=1)))
    if Qp is None:
        return np.zeros_like(intra), intra
    inter = None
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            prev = Qp[np.clip(ys + dy, 0, qh - 1)][:, np.clip(xs + dx, 0, qw - 1)]
            sad = per_block(np.abs(cur - prev))
            inter = sad if inter is None else np.minimum(inter, sad)
    return inter, intra


def records(Y, bd):
    """the records of a run of frames: Y [n, h, w] luma planes (h, w multiples of 8) -> RECORD_DTYPE [n]"""
    out = np.zeros(len(Y), RECORD_DTYPE)
    Qp = None
    for f in range(len(Y)):
        Q = quarter(Y[f], bd)
        inter, intra = block_sads(Q, Qp)
        out[f] = (int(inter.sum()), int(intra.sum()), inter.size, 0)
        Qp = Q
    return out


def is_cut(rec, scenecut):
    """the cut rule: 100 inter >= (100 - scenecut) intra and intra > 0"""
    return bool(100 * int(rec["inter_sad"]) >= (100 - int(scenecut)) * int(rec["intra_sad"]) and int(rec["intra_sad"]) > 0)


def cuts(recs, scenecut):
    return [f for f in range(len(recs)) if is_cut(recs[f], scenecut)]


def cut_range(recs, want):
    """the scenecut values 1..99 that flag exactly the frames `want` in recs: (lowest, highest) or None"""
    ok = [v for v in range(1, 100) if cuts(recs, v) == sorted(want)]
    return (ok[0], ok[-1]) if ok else None
