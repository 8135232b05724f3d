"""GPU tests of the tile kernels' prologue: ask, ticket, decide (csrc/wah_device.hpp).

A workgroup of compress_pair_kernel / decode_tile_kernel asks for the control block's words in front of its arrival ticket and
issues its tile's first loads right behind the ticket, before the launch epoch is decided.  What that order could get wrong: a
workspace whose words are another launch's (grids that differ from launch to launch, a used workspace against a fresh one, the
epoch wrap, the decoder's counter pair of deferred tiles), and a workspace that is not ours at all, where the loads are in flight
(or, with a ticket outside the grid, must not have been issued) when the kernel finds out.  Bit-exact against the oracle
(tests/_oracle), as test_gpu_parity.py, at the smallest shapes that reach these places.
"""
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_FORCED_NO_WAIT = os.environ.get("WAH_FORCE_FALLBACK") == "1"
_SCAN_ROUTE_ONLY = pytest.mark.skipif(_FORCED_NO_WAIT,
                                      reason="tests the scan route's workspace protocol (epochs, tickets); WAH_FORCE_FALLBACK=1 "
                                             "sends every launch down the no-wait route, which reads nothing of the workspace")
WAH_OK, WAH_ERR_WORKSPACE = 0, -2
SEG = 992                         # words of a segment
TILE_WORDS = 48 * SEG             # a compressor tile of three pairs per wave: 48 segments
BATCH = 2 * 8192                  # compressed words of a decoder workgroup: two tiles
DT_MAX_GROUPS = 60 * 1024         # groups a decoder tile may expand to before it goes onto the list of deferred tiles
CTL_START, CTL_EPOCH, CTL_MAGIC, CTL_WRAPS = 0, 64, 65, 66  # words of the control block (the workspace's first KiB)
MAGIC, EPOCH_WRAP = 0x57414832, 65535
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _route_is(got, want):
    return got == "no wait" if _FORCED_NO_WAIT else got == want


def _ctrl(ws):
    import torch

    return ws[:1024].view(torch.int32)


class _Shapes:
    """The inputs every test here draws from, and the oracle's answers, made once."""

    def __init__(self, oracle):
        # ---- compressor: one bitmap of 513 tiles; its prefixes are the smaller launches
        self.comp_sizes = [2 * SEG, TILE_WORDS, TILE_WORDS + 1, 513 * TILE_WORDS]
        self.bitmap = oracle.gen_uniform(self.comp_sizes[-1], 77, 0.02)
        self.comp_want = {n: oracle.compress(self.bitmap[:n]) for n in self.comp_sizes}
        # ---- decoder: one stream of a little more than 800 batches (literals and short fills: no tile is deferred); its
        #      prefixes are streams too
        self.dec_sizes = [1, BATCH, BATCH + 1, 800 * BATCH]
        self.stream = self.comp_want[self.comp_sizes[-1]]
        assert len(self.stream) >= self.dec_sizes[-1]
        self.dec_want = {c: oracle.decompress(self.stream[:c]) for c in self.dec_sizes}
        # ---- a stream whose tiles go onto the list of deferred tiles (long fills), and an incompressible one of two batches
        self.deferring = oracle.compress(oracle.gen_clustered(3_000_000, 78))
        self.dense = oracle.compress(oracle.gen_uniform(2 * BATCH * 31 // 32, 79, 0.5))
        self.deferring_want = oracle.decompress(self.deferring)
        self.dense_want = oracle.decompress(self.dense)


@pytest.fixture(scope="module")
def shapes(oracle):
    return _Shapes(oracle)


def _tile_groups(stream):
    """Groups each 8192-word decoder tile of a stream expands to."""
    w = stream.astype(np.uint64)
    groups = np.where(w & 0x80000000, w & 0x3FFFFFFF, 1)
    pad = (-len(groups)) % 8192
    return np.concatenate([groups, np.zeros(pad, np.uint64)]).reshape(-1, 8192).sum(axis=1)


def test_the_shapes_are_what_the_tests_mean(shapes):
    assert len(shapes.dense) == 2 * BATCH and not np.any(shapes.dense & 0x80000000)           # two batches of literals
    assert _tile_groups(shapes.deferring).max() > DT_MAX_GROUPS and len(shapes.deferring) > 8192  # tiles that are deferred
    assert _tile_groups(shapes.stream[: shapes.dec_sizes[-1]]).max() <= DT_MAX_GROUPS          # none here


def test_one_compress_workspace_grids_that_differ(wah, shapes):
    """1 pair, exactly one tile of 48 segments, one tile + 1 word, 513 tiles, and back: one DeviceCompressor throughout, so
    every launch finds the ticket counter, the epoch and the scan area as a launch with ANOTHER grid left them."""
    sizes = shapes.comp_sizes
    comp = wah.DeviceCompressor(sizes[-1])
    d = _dev(shapes.bitmap)
    for n in sizes + sizes[-2::-1]:
        comp.run(d, n_words=n)
        assert np.array_equal(_host(comp.result()), shapes.comp_want[n]), n


def test_one_decode_workspace_grids_that_differ(wah, oracle, shapes):
    """Streams of 1 word, one batch (16 384 words), one batch + 1 word and 800 batches -- more workgroups than the chip holds at
    once -- and back, through one DeviceDecompressor (the one-pass decoder)."""
    sizes = shapes.dec_sizes
    dec = wah.DeviceDecompressor(sizes[-1], len(shapes.dec_want[sizes[-1]]) + 1, one_pass=True)
    d = _dev(shapes.stream[: sizes[-1]])
    for c in sizes + sizes[-2::-1]:
        dec.run(d, c_words=c)
        assert _route_is(dec.route, "one pass")
        assert np.array_equal(_host(dec.result()), shapes.dec_want[c]), c


def test_fresh_and_used_workspace_give_the_same_stream(wah, oracle, shapes):
    n = shapes.comp_sizes[-1] // 8  # 64 tiles and a bit
    d = _dev(shapes.bitmap[:n])
    used = wah.DeviceCompressor(n)
    got = []
    for k in range(3):
        used.run(d)
        got.append(_host(used.result()).copy())
    fresh = wah.DeviceCompressor(n)
    fresh.run(d)
    got.append(_host(fresh.result()).copy())
    assert all(np.array_equal(g, got[0]) for g in got[1:]) and np.array_equal(got[0], oracle.compress(shapes.bitmap[:n]))
    c = 5 * BATCH + 77
    want = oracle.decompress(shapes.stream[:c])
    s = _dev(shapes.stream[:c])
    used = wah.DeviceDecompressor(c, len(want) + 1, one_pass=True)
    back = []
    for k in range(3):
        used.run(s)
        back.append(_host(used.result()).copy())
    fresh = wah.DeviceDecompressor(c, len(want) + 1, one_pass=True)
    fresh.run(s)
    back.append(_host(fresh.result()).copy())
    assert all(np.array_equal(b, back[0]) for b in back[1:]) and np.array_equal(back[0], want)


@_SCAN_ROUTE_ONLY
def test_epoch_wrap_with_the_loads_in_flight(wah, oracle, shapes):
    """A workspace whose stored epoch is one launch short of the wrap value, with a valid magic word: the first launch uses the
    last epoch, the second one wraps -- tile 0 clears the scan area while the other tiles wait, now with their loads in flight.
    Launches of more than one tile; bit-exact, WAH_OK."""
    L = wah.lib()
    n = 3 * TILE_WORDS + 5
    comp = wah.DeviceCompressor(n)
    c = 3 * BATCH + 5
    dec = wah.DeviceDecompressor(c, 4 * c, one_pass=True)
    for ws in (comp.workspace, dec.workspace):
        _ctrl(ws)[CTL_EPOCH] = EPOCH_WRAP - 1
        _ctrl(ws)[CTL_MAGIC] = MAGIC
    want, back_want = oracle.compress(shapes.bitmap[:n]), oracle.decompress(shapes.stream[:c])
    assert len(back_want) < 4 * c
    d, s = _dev(shapes.bitmap[:n]), _dev(shapes.stream[:c])
    for launch in range(2):
        comp.run(d)
        assert L.wah_compress_status(comp.workspace.data_ptr(), None) == WAH_OK
        assert np.array_equal(_host(comp.result()), want), launch
        dec.run(s)
        assert _route_is(dec.route, "one pass")
        assert L.wah_decompress_status(dec.workspace.data_ptr(), None) == WAH_OK
        assert np.array_equal(_host(dec.result()), back_want), launch
    assert int(_ctrl(comp.workspace)[CTL_WRAPS].item()) == 1 and int(_ctrl(comp.workspace)[CTL_EPOCH].item()) == 2  # wrapped once, counting again
    assert int(_ctrl(dec.workspace)[CTL_WRAPS].item()) == 1


# what is wrong with the workspace: a foreign magic word (tickets inside the grid: the tile's loads are in flight when the kernel
# finds out), a ticket counter that hands out tile numbers outside the grid (no load may be issued), both
_FOREIGN = {"magic": {CTL_MAGIC: 0x0BADF00D}, "tickets": {CTL_START: 0x7FFF0000}, "both": {CTL_MAGIC: 0x0BADF00D, CTL_START: 0x7FFF0000}}


@_SCAN_ROUTE_ONLY
@pytest.mark.parametrize("what", sorted(_FOREIGN))
def test_a_workspace_that_is_not_ours(wah, oracle, shapes, what):
    """WAH_ERR_WORKSPACE, an output buffer nobody wrote to, and after wah_workspace_init_device the oracle's words -- for inputs of
    one tile and of two, the compressor's two layouts and the one-pass decoder."""
    L = wah.lib()
    for n in (16 * SEG, 16 * SEG + 1, TILE_WORDS, 2 * TILE_WORDS):  # (one and two tiles of one pair per wave, and of the issue's 48 segments)
        data = shapes.bitmap[:n]
        want = oracle.compress(data)
        for unsegmented in (False, True):
            comp = wah.DeviceCompressor(n, unsegmented=unsegmented)
            for word, value in _FOREIGN[what].items():
                _ctrl(comp.workspace)[word] = value
            comp.out.fill_(SENTINEL)
            comp.run(_dev(data))
            assert L.wah_compress_status(comp.workspace.data_ptr(), None) == WAH_ERR_WORKSPACE, (n, unsegmented)
            assert np.all(_host(comp.out) == SENTINEL), (n, unsegmented)
            assert L.wah_workspace_init_device(comp.workspace.data_ptr(), comp.ws_bytes, None) == 0
            comp.run(_dev(data))
            got = _host(comp.result())
            if not unsegmented:
                assert np.array_equal(got, want), n
            else:
                assert np.array_equal(oracle.decompress(got)[:n], data), n
    for c in (BATCH, BATCH + 1):
        stream = shapes.stream[:c]
        want = shapes.dec_want[c]
        dec = wah.DeviceDecompressor(c, len(want) + 1, one_pass=True)
        for word, value in _FOREIGN[what].items():
            _ctrl(dec.workspace)[word] = value
        dec.out.fill_(SENTINEL)
        dec.run(_dev(stream))
        assert _route_is(dec.route, "one pass")
        assert L.wah_decompress_status(dec.workspace.data_ptr(), None) == WAH_ERR_WORKSPACE, c
        assert np.all(_host(dec.out) == SENTINEL), c
        assert L.wah_workspace_init_device(dec.workspace.data_ptr(), dec.ws_bytes, None) == 0
        dec.run(_dev(stream))
        assert np.array_equal(_host(dec.result()), want), c


@pytest.mark.parametrize("order", ["deferring first", "dense first"])
def test_the_counter_pair_read_early_is_the_launch_s_own(wah, shapes, order):
    """Two decodes in a row on one workspace, one that defers tiles to the list's launch and one of two batches that defers none,
    in both orders, twice over: the pair of counters a launch appends to is the one it read in front of its ticket."""
    both = [(shapes.deferring, shapes.deferring_want), (shapes.dense, shapes.dense_want)]
    if order == "dense first":
        both.reverse()
    c_max = max(len(s) for s, _ in both)
    cap = max(len(w) for _, w in both) + 1
    dec = wah.DeviceDecompressor(c_max, cap, one_pass=True)
    devs = [_dev(s) for s, _ in both]
    for rnd in range(2):
        for (s, want), d in zip(both, devs):
            dec.run(d, c_words=len(s))
            assert _route_is(dec.route, "one pass")
            assert np.array_equal(_host(dec.result()), want), (order, rnd, len(s))
