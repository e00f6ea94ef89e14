"""The tile tokenizer of 8x8 blocks on the GPU (k_av1_tokens, av1-go_amd/csrc/av1_ops8.hpp tok_tile8): the session's GPU-coded tile
bytes equal the host writer's at the smallest shapes at which a tile is partial in either direction, holds one block row, or sits under
a key frame's 32x32 band; a batch whose lists overflow falls back and its bytes equal the host's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _streams(av1mi, ctx, w, h, bd, q, gop, segs, mode, frames, kbs):
    """per segment the temporal units of a session with gpu_entropy = mode; + how many batches the GPU coder coded, + the fallbacks"""
    import av1stream
    Y, U, V = frames
    kw = {} if kbs is None else dict(key_block_size=kbs)
    s = av1mi.GopSession(ctx, w, h, bd, q, gop, segs, gpu_entropy=mode, **kw)
    try:
        out, coded = [b""] * segs, 0
        for t in range(gop):
            planes = s.input_planes()
            for sgi in range(segs):
                f = sgi * gop + t
                planes[0][sgi * h:(sgi + 1) * h] = Y[f]
                planes[1][sgi * h // 2:(sgi + 1) * h // 2] = U[f]
                planes[2][sgi * h // 2:(sgi + 1) * h // 2] = V[f]
            s.submit()
            fr = s.collect()
            coded += "tile_size" in fr
            for sgi in range(segs):
                out[sgi] += av1stream.session_temporal_unit(w, h, bd, fr["raw"], sgi, with_sequence_header=(t == 0))
        return out, coded, s.entropy_fallbacks()
    finally:
        s.close()


@pytest.mark.parametrize("w,h,bd,q,gop,segs,kbs", [(64, 64, 8, 1, 2, 1, None), (136, 72, 10, 255, 3, 3, None), (200, 120, 10, 23, 3, 2, None), (128, 72, 10, 60, 2, 2, 32),
                                                    (72, 136, 8, 128, 3, 2, None)],
                         ids=["64x64_q1_densest", "136x72_q255_sparsest", "200x120_q23", "128x72_one_block_row_under_the_32x32_band", "72x136_q128"])
def test_gpu_coded_tiles_equal_the_host_writer(ctx, av1mi, w, h, bd, q, gop, segs, kbs):
    import synth
    frames = synth.frames(w, h, segs * gop, bd, 4)
    gpu, coded, fallbacks = _streams(av1mi, ctx, w, h, bd, q, gop, segs, 1, frames, kbs)
    assert coded == gop and fallbacks == 0, "the GPU coder gave %d of %d batches back" % (gop - coded, gop)
    host, _, _ = _streams(av1mi, ctx, w, h, bd, q, gop, segs, 0, frames, kbs)
    assert gpu == host


def test_a_batch_whose_lists_overflow_falls_back_to_the_host_bytes(ctx, av1mi):
    """white noise at base_q_idx 2: a tile needs more words than its list holds; the batch comes back as symbols and is coded on the host"""
    w, h, bd, q, gop = 128, 128, 8, 2, 2
    rng = np.random.default_rng(0)
    frames = tuple(rng.integers(0, 256, (gop, h // d, w // d)).astype(np.uint8) for d in (1, 2, 2))
    gpu, coded, fallbacks = _streams(av1mi, ctx, w, h, bd, q, gop, 1, 1, frames, None)
    assert fallbacks >= 1 and coded < gop
    host, _, _ = _streams(av1mi, ctx, w, h, bd, q, gop, 1, 0, frames, None)
    assert gpu == host
