"""Depth reduction in numpy: include/av1mi.h "depth reduction" restated line by line.  uint16 planes in, uint8 planes of the same shape out.
A plane may be a batch (frames stacked vertically): the heights are even, so a row's parity in the batch is its parity in its frame."""
import numpy as np

ROUND, ORDERED = 0, 1      # enum av1mi_depth_mode
T = np.array([[0, 2], [3, 1]], np.uint32)


def thresholds(shape, p, mode):
    """t_p(x, y) over a plane of `shape` = (rows, width): plane p = 0, 1, 2 for Y, U, V"""
    h, w = shape
    if mode == ROUND:
        return np.full((h, w), 2, np.uint32)
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    return T[y & 1, (x + p) & 1]


def reduce_plane(v, p, mode):
    """out = min((v + t_p(x, y)) >> 2, 255)"""
    v = np.asarray(v)
    assert v.dtype == np.uint16 and v.ndim == 2 and mode in (ROUND, ORDERED) and p in (0, 1, 2)
    return np.minimum((v.astype(np.uint32) + thresholds(v.shape, p, mode)) >> 2, 255).astype(np.uint8)


def reduce(Y, U, V, mode):
    """the three planes of a frame or of a batch"""
    return reduce_plane(Y, 0, mode), reduce_plane(U, 1, mode), reduce_plane(V, 2, mode)
