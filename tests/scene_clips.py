"""Clips for the scene-cut tests and measurements, built from the generators of av1-go_amd/synth.py: shots of different textures joined
at hard cuts, and a clip WITHOUT cuts (a fast pan, then a slow drift, then the drift under a slow fade towards grey).  Deterministic;
nothing is read from disk."""
import numpy as np

import synth

# the two clips the product's default sensitivity was chosen on (profiles/scenecut.json)
DEFAULT_CLIPS = dict(w=192, h=128, cut=dict(n=24, cuts=(6, 17)), calm=dict(n=30, pan=4.0, drift=0.4, fade_to=0.5))


def _textures(w, h, shot, reach):
    seed = synth.SEED + 16 * shot
    return [(synth.texture(w >> d, h >> d, seed + p, reach), seed + p) for p, d in ((0, 0), (1, 1), (2, 1))]


def _frame(tex, w, h, t, pos, bd):
    """the three planes of frame number t (its noise) at texture position `pos` (in units of synth's (1.25, 0.75) step)"""
    scale = pos / t if t else 1.0
    return [synth.plane(tx, w >> d, h >> d, t, seed, bd, scale * (0.5 if d else 1.0)) for (tx, seed), d in zip(tex, (0, 1, 1))]


def _stack(frames, bd):
    dt = np.uint8 if bd == 8 else np.uint16
    return tuple(np.stack([f[p] for f in frames]).astype(dt) for p in range(3))


def cut_clip(w, h, n, bd, cuts):
    """(Y, U, V) of n frames: a new shot (another texture, moving on at synth's pace) starts at every frame of `cuts`"""
    bounds = [0] + sorted(cuts) + [n]
    frames = []
    for shot in range(len(bounds) - 1):
        tex = _textures(w, h, shot, n + 2)
        frames += [_frame(tex, w, h, t, float(t), bd) for t in range(bounds[shot], bounds[shot + 1])]
    return _stack(frames, bd)


def calm_clip(w, h, n, bd, pan=4.0, drift=0.4, fade_to=0.5):
    """(Y, U, V) of n frames of ONE shot: a third panning at `pan` times synth's pace ((5, 3) samples a frame at 4), a third drifting at
    `drift` times it, and a third drifting while the picture fades linearly towards grey, down to the contrast fade_to.  No cuts."""
    a, b = n // 3, 2 * n // 3
    tex = _textures(w, h, 0, int(n * pan) + 2)
    mid = 1 << (bd - 1)
    frames, pos = [], 0.0
    for t in range(n):
        if t:
            pos += pan if t < a else drift
        f = _frame(tex, w, h, t, pos, bd)
        if t >= b:
            g = 1.0 - (1.0 - fade_to) * (t - b + 1) / (n - b)
            f = [np.rint(mid + (p.astype(np.float64) - mid) * g) for p in f]
        frames.append(f)
    return _stack(frames, bd)


def write_y4m(path, clip, bd, fps=30):
    Y, U, V = clip
    h, w = Y.shape[1:]
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F%d:1 Ip A1:1 C%s\n" % (w, h, fps, "420jpeg" if bd == 8 else "420p10")).encode())
        for t in range(Y.shape[0]):
            f.write(b"FRAME\n")
            for p in (Y[t], U[t], V[t]):
                f.write(np.ascontiguousarray(p).astype("<u2" if bd == 10 else np.uint8).tobytes())
