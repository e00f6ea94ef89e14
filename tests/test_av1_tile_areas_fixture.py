"""The host tile entries (av1mi_host_opstream_tile8 / _tile32) hand the tile tokenizers the caller's pointers as the tile's areas
(av1-go_amd/csrc/av1_ops32.hpp CallerAreas).  What they return and write — list words, grouped entries, totals and bases of every slot,
the untouched rest of the caller's areas, what a refused tile leaves — is recorded in tests/golden/host_tile_areas.npz, made before
the tokenizers asked anybody for their areas, and must stay exactly that.  CPU only.

    python3 tests/test_av1_tile_areas_fixture.py      writes the fixture from the library as built"""
import os
import sys

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_tile_areas.npz")
CASES = ["tile8_key", "tile8_inter", "tile8_two_passes", "tile8_refused", "tile32", "tile32_half", "tile32_refused"]


def _run(case):
    import test_av1_tokens32_ranges as T32
    import test_av1_tokens8_tile as T8
    rng = np.random.default_rng(CASES.index(case) + 40)
    if case.startswith("tile8"):
        key = case != "tile8_inter"
        if case == "tile8_two_passes":
            w, h = 64, 64
            sym = T8._symbols(rng, "eob_full_everywhere", w, h, key)
            sym.update(T8._frame(rng, w, h, [64, 33, 9, 2, 50], [16, 7, 3, 1, 12], density=0.6, big_y=(0, 5), big_c=(1,), hi=12))
            return T8._tile8((w, h, 10, 60), sym, key, 0, 0, 1 << 16)[:5]
        w, h = 136, 72
        sym = T8._symbols(rng, "golomb_at_the_first_and_last_position", w, h, key)
        return T8._tile8((w, h, 10, 60), sym, key, 0, 1, 100 if case == "tile8_refused" else 1 << 14)[:5]
    w, h = (160, 64) if case == "tile32_half" else (128, 64)
    sym = T32._frame(rng, w, h, [1024, 700], [256, 100], density=0.6, big_y=(0, 1023), big_c=(1,))
    return T32._tile32((w, h, 10, 60), sym, 0, 2 if case == "tile32_half" else 1, 100 if case == "tile32_refused" else 1 << 14)[:5]


@pytest.mark.parametrize("case", CASES)
def test_host_tile_entries_return_what_they_returned(case):
    want = np.load(FIXTURE)
    n, lst, grp, tot, base = _run(case)
    assert n == int(want[case + ".words"])
    assert (n < 0) == case.endswith("refused")
    for name, got in (("list", lst), ("grouped", grp), ("total", tot), ("base", base)):
        assert got.shape == want[case + "." + name].shape and (got == want[case + "." + name]).all(), name


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(os.path.dirname(FIXTURE), "..", "..", "av1-go_amd")]
    out = {}
    for c in CASES:
        r = _run(c)
        out[c + ".words"] = np.int32(r[0])
        out.update({c + "." + k: v for k, v in zip(("list", "grouped", "total", "base"), r[1:])})
    np.savez_compressed(FIXTURE, **out)
    print(FIXTURE, os.path.getsize(FIXTURE), {c: int(out[c + ".words"]) for c in CASES})
