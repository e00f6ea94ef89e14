"""k_av1_chains takes its work from ticket counters (csrc/av1_entropy_kernels.hip): a fixed grid of 8 x 32 x W
workgroups, each drawing (group, slot) items of its XCD from a word of the batch's cursor line until the XCD's groups are used up.
Every item must be walked exactly once whatever the grid, the group count and the order in which workgroups arrive, so through
av1mi_av1_entropy_encode the tile payloads and sizes stay byte-identical to the host twin (host/av1_opstream.cpp):

  64x64 x 1 frame       one tile, one group: seven XCDs find no work
  640x384 x 10 frames   600 tiles, 10 groups: the group index wraps the 8 XCDs, the last group is partial (24 tiles)
  640x384 x 11 frames   key frames with a 32x32 band: both chains launches, each with its own row of tickets
  200x136 x 3 frames    partial tiles at the right and bottom edges

each as a key batch and as a P batch, on a context made with AV1MI_CHAINS_CAP=tickets.  Then: the parent's limiter (unused dynamic
LDS, one workgroup per item) gives the same bytes; a grid of 6 144 workgroups for one tile's 198 items; and two jobs one after the
other on one context (a ticket row that was not zeroed would make the second job walk nothing)."""
import contextlib

import numpy as np
import pytest

from test_gpu_chains_order import _gpu_units, _inter_symbols, _key_symbols, _twin_unit

pytestmark = pytest.mark.gpu

Q = 128
#        name        w    h  frames  key_rows32 (of the key batch)
SHAPES = {"one_tile": (64, 64, 1, 0), "ten_groups": (640, 384, 10, 0), "band32": (640, 384, 11, 192), "edges": (200, 136, 3, 0)}
CASES = [(s, key) for s in SHAPES for key in (True, False)]


@contextlib.contextmanager
def _context(av1mi, monkeypatch, cap, waves=None):
    """a context of its own: the limiter is read once, when a context's coder state is made"""
    monkeypatch.setenv("AV1MI_CHAINS_CAP", cap)
    if waves is None:
        monkeypatch.delenv("AV1MI_CHAINS_WAVES", raising=False)
    else:
        monkeypatch.setenv("AV1MI_CHAINS_WAVES", str(waves))
    c = av1mi.Context(0)
    try:
        yield c
    finally:
        c.close()


_cache = {}


def _case(O, shape, key):
    """(job arguments, the frames' symbols, the host twin's temporal units), computed once per case and shared"""
    if (shape, key) not in _cache:
        import synth
        w, h, n, rows32 = SHAPES[shape]
        bd = 10
        if key:
            Y, U, V = synth.frames(w, h, n, bd, 31)
            frames = [_key_symbols(O, Y[f], U[f], V[f], w, h, bd, Q, rows32) for f in range(n)]
            kw = dict(key_rows32=rows32, lr_on=(1, 0, 1))
        else:
            rng = np.random.default_rng(w + h + n)
            frames = [_inter_symbols(rng, w, h, bd) for _ in range(n)]
            kw = {}
        twin = [_twin_unit(w, h, bd, Q, key, sym, **kw) for sym in frames]
        _cache[(shape, key)] = ((w, h, bd, Q, key), frames, kw, twin)
    return _cache[(shape, key)]


def _run(ctx, case):
    args, frames, kw, _ = case
    return _gpu_units(ctx, *args, frames, **kw)


def _check(got, case, what):
    for f, unit in enumerate(case[3]):
        assert got[f] == unit, "%s, frame %d: GPU payloads or tile sizes differ from the host twin" % (what, f)


@pytest.mark.parametrize("shape,key", CASES, ids=["%s-%s" % (s, "key" if k else "inter") for s, k in CASES])
def test_tickets_equal_the_host_writer(av1mi, monkeypatch, O, shape, key):
    case = _case(O, shape, key)
    with _context(av1mi, monkeypatch, "tickets") as c:
        _check(_run(c, case), case, "tickets")


@pytest.mark.parametrize("key", [True, False], ids=["key", "inter"])
def test_both_limiters_give_the_same_payloads(av1mi, monkeypatch, O, key):
    case = _case(O, "ten_groups", key)
    got = {}
    for cap in ("lds", "tickets"):
        with _context(av1mi, monkeypatch, cap, 12) as c:
            got[cap] = _run(c, case)
    assert got["lds"] == got["tickets"]
    _check(got["lds"], case, "lds")


@pytest.mark.parametrize("key", [True, False], ids=["key", "inter"])
def test_a_grid_far_larger_than_the_work(av1mi, monkeypatch, O, key):
    """W = 24: 6 144 workgroups, 768 per XCD, for the one group of XCD 0 — all but some two hundred draw a ticket past the end and leave,
    and the seven other XCDs' workgroups all do"""
    case = _case(O, "one_tile", key)
    with _context(av1mi, monkeypatch, "tickets", 24) as c:
        _check(_run(c, case), case, "tickets, W = 24")


@pytest.mark.parametrize("shape,key", [("ten_groups", False), ("band32", True)], ids=["inter", "key-band32"])
def test_tickets_are_zeroed_for_every_job(av1mi, monkeypatch, O, shape, key):
    """three jobs on one context (the list sets alternate, the cursor line is one): each must find its ticket rows at zero"""
    case = _case(O, shape, key)
    with _context(av1mi, monkeypatch, "tickets") as c:
        for job in range(3):
            _check(_run(c, case), case, "tickets, job %d on the context" % job)
