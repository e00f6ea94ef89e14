"""The motion search of include/av1mi.h ("motion search") restated in numpy from the header's text: the quarter planes, the coarse
search's centre per 64x64 tile and the integer search around those centres.  Test infrastructure only; the GPU kernels
(av1-go_amd/csrc/me_coarse_kernels.hip, k_me_int) must agree with it bit for bit.  Also the clips the wide-range tests run on: the
synthetic texture of synth.py panning at any speed, and a scene whose halves pan in opposite directions."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "av1-go_amd"))
import synth  # noqa: E402


def m8(P, bd):
    """the 8-bit view the searches compare"""
    return (np.asarray(P).astype(np.int32) >> (bd - 8))


def quarter_plane(P, bd):
    """Q[y][x] = (sum of the 4x4 samples' 8-bit views + 8) >> 4; [h / 4, w / 4] uint8"""
    h, w = P.shape
    v = m8(P, bd).reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3))
    return ((v + 8) >> 4).astype(np.uint8)


def _ranks(R):
    """rank of displacement (dy, dx), [2R+1, 2R+1]: 0 for (0, 0), else 1 + raster index"""
    n = 2 * R + 1
    rk = 1 + np.arange(n * n, dtype=np.int64).reshape(n, n)
    rk[R, R] = 0
    return rk


def coarse_centres(q_src, q_ref, coarse_range):
    """centres [tiles_y, tiles_x, 2] (x, y) in luma samples: per tile the minimum of (SAD << 16) | rank over [-Rc, Rc]^2 of the 16x16
    block of q_src against q_ref, all coordinates clamped into the quarter plane"""
    Rc = coarse_range // 4
    qh, qw = q_src.shape
    ty, tx = (qh + 15) // 16, (qw + 15) // 16
    S = np.pad(q_src.astype(np.int32), ((0, 16 * ty - qh), (0, 16 * tx - qw)), mode="edge")
    Rf = np.pad(q_ref.astype(np.int32), ((Rc, 16 * ty - qh + Rc), (Rc, 16 * tx - qw + Rc)), mode="edge")
    rk = _ranks(Rc)
    best = np.full((ty, tx), np.iinfo(np.int64).max, np.int64)
    for dy in range(-Rc, Rc + 1):
        for dx in range(-Rc, Rc + 1):
            d = np.abs(S - Rf[Rc + dy:Rc + dy + 16 * ty, Rc + dx:Rc + dx + 16 * tx])
            sad = d.reshape(ty, 16, tx, 16).sum(axis=(1, 3)).astype(np.int64)
            best = np.minimum(best, (sad << 16) | rk[dy + Rc, dx + Rc])
    rank = best & 0xFFFF
    n = 2 * Rc + 1
    dy = np.where(rank > 0, (rank - 1) // n - Rc, 0)
    dx = np.where(rank > 0, (rank - 1) % n - Rc, 0)
    return np.stack([4 * dx, 4 * dy], axis=-1).astype(np.int16)


def integer_vectors(src, ref, bd, centres, search_range):
    """the integer search around the tiles' centres: vectors [h / 8, w / 8, 2] (x, y) in 1/8 luma samples = (centre + d) * 8, d the
    minimum of (SAD over the block's even rows << 16) | rank over [-R, R]^2, reference coordinates clamped into the plane"""
    R = search_range
    h, w = src.shape
    S8, R8 = m8(src, bd), m8(ref, bd)
    n = 2 * R + 1
    rk = _ranks(R)
    out = np.zeros((h // 8, w // 8, 2), np.int16)
    for sby in range((h + 63) // 64):
        for sbx in range((w + 63) // 64):
            cx, cy = int(centres[sby, sbx, 0]), int(centres[sby, sbx, 1])
            ys = np.clip(sby * 64 + cy - R + np.arange(64 + 2 * R), 0, h - 1)
            xs = np.clip(sbx * 64 + cx - R + np.arange(64 + 2 * R), 0, w - 1)
            win = R8[np.ix_(ys, xs)]
            tile = S8[np.ix_(np.minimum(sby * 64 + np.arange(64), h - 1), np.minimum(sbx * 64 + np.arange(64), w - 1))]
            cand = np.lib.stride_tricks.sliding_window_view(win, (64, 64))[:, :, ::2, :]      # [dy, dx, 32 even rows, 64]
            sad = np.abs(cand - tile[::2]).reshape(n, n, 8, 4, 8, 8).sum(axis=(3, 5)).astype(np.int64)
            key = ((sad << 16) | rk[:, :, None, None]).reshape(n * n, 8, 8).min(axis=0)
            rank = key & 0xFFFF
            dy = np.where(rank > 0, (rank - 1) // n - R, 0)
            dx = np.where(rank > 0, (rank - 1) % n - R, 0)
            by, bx = min(8, h // 8 - sby * 8), min(8, w // 8 - sbx * 8)
            out[sby * 8:sby * 8 + by, sbx * 8:sbx * 8 + bx, 0] = ((cx + dx) * 8)[:by, :bx]
            out[sby * 8:sby * 8 + by, sbx * 8:sbx * 8 + bx, 1] = ((cy + dy) * 8)[:by, :bx]
    return out


def search(src, ref, bd, search_range, coarse_range):
    """one frame through the whole search: dict(q_src, q_ref, centres [tiles, 2], mvs [blocks, 2]) in the layouts of av1mi_me_search"""
    h, w = src.shape
    ty, tx = (h + 63) // 64, (w + 63) // 64
    if coarse_range:
        qs, qr = quarter_plane(src, bd), quarter_plane(ref, bd)
        cen = coarse_centres(qs, qr, coarse_range)
    else:
        qs = qr = None
        cen = np.zeros((ty, tx, 2), np.int16)
    mv = integer_vectors(src, ref, bd, cen, search_range)
    return dict(q_src=qs, q_ref=qr, centres=cen.reshape(ty * tx, 2), mvs=mv.reshape(-1, 2))


# ---- clips -----------------------------------------------------------------------------------------------------------------------
def pan_clip(w, h, n, bd, scale, first=0):
    """synth.frames with the texture moving `scale` times as fast: (1.25, 0.75) * scale luma samples per frame (scale 20 = (25, 15));
    returns (Y [n, h, w], U, V [n, h / 2, w / 2])"""
    T = int(np.ceil((first + n) * abs(scale))) + 1
    tex = [synth.texture(w, h, synth.SEED, T), synth.texture(w // 2, h // 2, synth.SEED + 1, T), synth.texture(w // 2, h // 2, synth.SEED + 2, T)]
    Y = np.stack([synth.plane(tex[0], w, h, first + t, synth.SEED, bd, scale) for t in range(n)])
    U = np.stack([synth.plane(tex[1], w // 2, h // 2, first + t, synth.SEED + 1, bd, 0.5 * scale) for t in range(n)])
    V = np.stack([synth.plane(tex[2], w // 2, h // 2, first + t, synth.SEED + 2, bd, 0.5 * scale) for t in range(n)])
    return Y, U, V


def split_clip(w, h, n, bd, scale):
    """the left half of every frame pans by (1.25, 0.75) * scale per frame, the right half by the opposite (the same clip played
    backwards); the seam is at w / 2"""
    A = pan_clip(w, h, n, bd, scale)
    out = []
    for a in A:
        o = a.copy()
        half = a.shape[2] // 2
        o[:, :, half:] = a[::-1, :, half:]
        out.append(o)
    return tuple(out)
