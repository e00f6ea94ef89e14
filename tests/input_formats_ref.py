"""numpy restatement of the input formats of include/av1mi.h (enum av1mi_input_format), shared by test_input_formats.py and
test_gpu_input_formats.py.  Nothing here calls the library: these are the definitions the library is checked against."""
import numpy as np

PLANAR, PACKED10, P010, NV12 = 0, 1, 2, 3


def plane_bytes(fmt, bd, plane, width, rows):
    """bytes of one plane of a stack of `rows` luma rows; 0 = invalid combination / no such plane"""
    ok = {PLANAR: bd in (8, 10), PACKED10: bd == 10, P010: bd == 10, NV12: bd == 8}.get(fmt, False)
    if not ok or plane not in (0, 1, 2):
        return 0
    n = width * rows if plane == 0 else (width // 2) * (rows // 2)
    if fmt == PLANAR:
        return n * (1 if bd == 8 else 2)
    if fmt == PACKED10:
        return n * 10 // 8
    bps = 2 if fmt == P010 else 1
    return (n * bps, 2 * n * bps, 0)[plane]


def pack10_bits(s):
    """the normative definition: one little-endian bit string, sample i occupies bits [10 i, 10 i + 10)"""
    s = np.asarray(s).ravel().astype(np.uint16)
    bits = ((s[:, None] >> np.arange(10, dtype=np.uint16)) & 1).astype(np.uint8).ravel()
    return np.packbits(bits, bitorder="little")


def pack10_bytes(s):
    """the equivalent byte formula of the header: bytes 5k .. 5k + 4 from samples 4k .. 4k + 3 (integer arithmetic only; cheap
    enough for a whole 4K batch)"""
    s = np.asarray(s).ravel().astype(np.uint16).reshape(-1, 4)
    s0, s1, s2, s3 = (s[:, i] for i in range(4))
    out = np.empty((s.shape[0], 5), np.uint8)
    out[:, 0] = s0 & 0xFF
    out[:, 1] = (s0 >> 8) | ((s1 & 0x3F) << 2)
    out[:, 2] = (s1 >> 6) | ((s2 & 0x0F) << 4)
    out[:, 3] = (s2 >> 4) | ((s3 & 0x03) << 6)
    out[:, 4] = s3 >> 2
    return out.ravel()


def pack(fmt, bd, y, u, v, low_bits=None, pack10=pack10_bytes):
    """planar planes -> the format's planes as flat uint8 arrays (two for the semi-planar formats).  low_bits (P010): a generator
    whose random bits fill the six ignored low bits of every sample"""
    if fmt == PACKED10:
        return [pack10(p) for p in (y, u, v)]
    dt = np.uint16 if fmt == P010 else np.uint8
    sh = 6 if fmt == P010 else 0
    luma = (np.asarray(y).astype(dt) << sh).ravel()
    pairs = np.empty((u.size, 2), dt)
    pairs[:, 0] = np.asarray(u).astype(dt).ravel() << sh
    pairs[:, 1] = np.asarray(v).astype(dt).ravel() << sh
    pairs = pairs.ravel()
    if low_bits is not None and fmt == P010:
        luma = luma | low_bits.integers(0, 64, luma.size, dtype=np.uint16)
        pairs = pairs | low_bits.integers(0, 64, pairs.size, dtype=np.uint16)
    return [luma.view(np.uint8), pairs.view(np.uint8)]


def content(kind, bd, width, rows, seed=0):
    """test planes: "random", "zeros", "max" or "ramp" (i mod 2^bd over every plane: every bit position of every byte pattern)"""
    dt = np.uint8 if bd == 8 else np.uint16
    shapes = ((rows, width), (rows // 2, width // 2), (rows // 2, width // 2))
    rng = np.random.default_rng(seed)
    out = []
    for sh in shapes:
        n = sh[0] * sh[1]
        if kind == "random":
            a = rng.integers(0, 1 << bd, n, dtype=np.uint16)
        elif kind == "zeros":
            a = np.zeros(n, np.uint16)
        elif kind == "max":
            a = np.full(n, (1 << bd) - 1, np.uint16)
        else:
            a = (np.arange(n, dtype=np.uint64) % (1 << bd)).astype(np.uint16)
        out.append(a.astype(dt).reshape(sh))
    return out
