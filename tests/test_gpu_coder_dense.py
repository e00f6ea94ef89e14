"""The tile coder's scratch on the GPU (av1-go_amd/csrc/av1_entropy_kernels.hip): a tile's list words and grouped entries lie in whole
cache lines a tile's wave reserves from two pools, in the order the tiles arrive there, and the chains and the range coder find them
through per-tile offsets.  Whatever the placement, the coded bytes are the host writer's (the CPU twin behind av1stream), byte for byte:
at one tile, at a partial last group of 64 tiles, across a group boundary, at more groups than there are XCDs, under a key frame's 32x32
band, on the second and third batch of a session, twice in a row, and around a batch that has a tile over the list capacity."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _feed(s, frames, f0, segs, h):
    planes = s.input_planes()
    for sgi in range(segs):
        for p, d in zip(range(3), (1, 2, 2)):
            planes[p][sgi * h // d:(sgi + 1) * h // d] = frames[p][f0 + sgi]


def _run(av1mi, ctx, w, h, bd, q, segs, mode, batches, kbs=None):
    """one session; batches = [(frames, first frame, frame type)].  Per batch: the segments' temporal units, and the GPU coder's tile sizes
    and payloads (None when the batch came back as symbols for the host writer); + the session's fallbacks"""
    import av1stream
    kw = {} if kbs is None else dict(key_block_size=kbs)
    s = av1mi.GopSession(ctx, w, h, bd, q, max(len(batches), 1), segs, gpu_entropy=mode, **kw)
    try:
        out = []
        for i, (frames, f0, ftype) in enumerate(batches):
            _feed(s, frames, f0, segs, h)
            s.submit(ftype)
            fr = s.collect()
            tus = [av1stream.session_temporal_unit(w, h, bd, fr["raw"], sgi, with_sequence_header=(ftype == 0)) for sgi in range(segs)]
            coded = (fr["tile_size"].copy(), fr["tile_payload"].copy()) if "tile_size" in fr else None
            out.append((tus, coded))
        return out, s.entropy_fallbacks()
    finally:
        s.close()


def _key_then_p(frames, segs):
    """segment s codes frames s (key) and segs + s (P)"""
    return [(frames, 0, 0), (frames, segs, 1)]


def _check_against_host(av1mi, ctx, w, h, bd, q, segs, batches, kbs=None):
    gpu, fallbacks = _run(av1mi, ctx, w, h, bd, q, segs, 1, batches, kbs)
    assert fallbacks == 0 and all(coded is not None for _, coded in gpu), "the GPU coder gave a batch back"
    host, _ = _run(av1mi, ctx, w, h, bd, q, segs, 0, batches, kbs)
    for i, ((g, _), (c, _)) in enumerate(zip(gpu, host)):
        assert g == c, "batch %d: the GPU coder's bytes differ from the host writer's" % i
    return gpu


@pytest.mark.parametrize("segs", [1, 9])
@pytest.mark.parametrize("w,h", [(64, 64), (520, 72), (1352, 136)], ids=["64x64_one_tile", "520x72_9x2_tiles", "1352x136_66_tiles"])
def test_8bit_key_and_p_frames_equal_the_host_writer(ctx, av1mi, w, h, segs):
    """one tile in one lane of one group; 9 x 2 tiles, a partial last group and a tile row that is no whole superblock; 22 x 3 = 66 tiles, one
    group boundary; with nine segments 9, 162 and 594 tiles: 10 groups of 64, more than the eight XCDs the groups are dealt to"""
    import synth
    frames = synth.frames(w, h, 2 * segs, 8, 3)
    _check_against_host(av1mi, ctx, w, h, 8, 60, segs, _key_then_p(frames, segs))


def test_10bit_equals_the_host_writer(ctx, av1mi):
    import synth
    w, h, segs = 520, 72, 2
    _check_against_host(av1mi, ctx, w, h, 10, 60, segs, _key_then_p(synth.frames(w, h, 2 * segs, 10, 3), segs))


def test_key_frame_with_both_bands_equals_the_host_writer(ctx, av1mi):
    """key_block_size 32, 544 x 72: a 32x32 band of one superblock row whose last tile is half a superblock wide, 8x8 tiles in the eight
    rows below; nine segments make 162 tiles in three groups, each walked by both chains launches, each launch taking its own band's"""
    import synth
    w, h, segs = 544, 72, 9
    _check_against_host(av1mi, ctx, w, h, 8, 60, segs, _key_then_p(synth.frames(w, h, 2 * segs, 8, 3), segs), kbs=32)


def test_later_batches_of_a_session_equal_a_fresh_sessions(ctx, av1mi):
    """three batches on one session: the cursors start at zero again for every batch, the lists' offsets alternate between two sets with
    the lists while the entries' offsets are one.  Batches two and three must be what a fresh session makes of the same frames."""
    import synth
    w, h, segs = 520, 72, 2
    frames = synth.frames(w, h, 3 * segs, 8, 5)
    tail = [(frames, segs, 0), (frames, 2 * segs, 1)]
    long_run = _check_against_host(av1mi, ctx, w, h, 8, 60, segs, [(frames, 0, 0)] + tail)
    fresh, _ = _run(av1mi, ctx, w, h, 8, 60, segs, 1, tail)
    for (a, ca), (b, cb) in zip(long_run[1:], fresh):
        assert a == b
        assert (ca[0] == cb[0]).all() and (ca[1] == cb[1]).all()


def test_the_same_batch_twice_gives_the_same_payloads_and_tile_sizes(ctx, av1mi):
    """where a tile's areas lie depends on the order in which the tiles' waves reach the cursors; nothing the coder hands out may"""
    import synth
    w, h, segs = 1352, 136, 9
    batches = _key_then_p(synth.frames(w, h, 2 * segs, 8, 3), segs)
    a, _ = _run(av1mi, ctx, w, h, 8, 60, segs, 1, batches)
    b, _ = _run(av1mi, ctx, w, h, 8, 60, segs, 1, batches)
    for (ta, ca), (tb, cb) in zip(a, b):
        assert ca is not None and cb is not None
        assert (ca[0] == cb[0]).all() and ca[1].shape == cb[1].shape and (ca[1] == cb[1]).all()
        assert ta == tb


def test_a_tile_over_the_list_capacity_sends_its_batch_to_the_host_and_the_next_is_coded_on_the_gpu(ctx, av1mi):
    """white noise at base_q_idx 2 (tests/test_gpu_tokens8.py) in ONE 64x64 tile beside an ordinary one: the tile needs more list words
    than a tile may have, reserves nothing and raises status bit 0; the session sees the bit, counts a fallback and hands the batch to
    the host writer as symbols.  The next batch of the same session, ordinary content, is coded on the GPU again."""
    import synth
    w, h, bd, q = 128, 64, 8, 2
    Y, U, V = (a.copy() for a in synth.frames(w, h, 2, bd, 3))
    rng = np.random.default_rng(0)
    Y[0, :, :64] = rng.integers(0, 256, (64, 64))
    U[0, :, :32] = rng.integers(0, 256, (32, 32))
    V[0, :, :32] = rng.integers(0, 256, (32, 32))
    batches = [((Y, U, V), 0, 0), ((Y, U, V), 1, 0)]
    gpu, fallbacks = _run(av1mi, ctx, w, h, bd, q, 1, 1, batches)
    assert fallbacks == 1
    assert gpu[0][1] is None and gpu[1][1] is not None
    host, _ = _run(av1mi, ctx, w, h, bd, q, 1, 0, batches)
    assert [g for g, _ in gpu] == [c for c, _ in host]
