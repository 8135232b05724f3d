"""GPU tests of the tile kernels' critical path: issue priority for the waves every later tile waits for.

decode_tile_kernel and compress_pair_kernel run a workgroup's front (ticket, loads, counts, publication) and wave 0's row scan
at raised issue priority, and the decoder does a batch's bookkeeping (tile_base[], tile_flags[], the list of deferred tiles, the
last batch's info[] and launch epoch) behind the barrier that hands the batch's base to the other waves, not in front of it.
Priorities change no result; what could go wrong is what was moved: the bookkeeping of ordinary, plain and deferred tiles, the
list, the capacity report, the epoch and the counter pair from launch to launch, and the compressor's offsets and index at the
tile shapes.  Bit-exact against the oracle (tests/_oracle), at the smallest shapes that reach these places; no bitmap is larger
than 1 MiB (longer streams are whole-segment streams of several bitmaps, back to back).
"""
import importlib
import os

import numpy as np
import pytest

from tests import _foreign as fg

pytestmark = pytest.mark.gpu

_FORCED_NO_WAIT = os.environ.get("WAH_FORCE_FALLBACK") == "1"
WAH_OK, WAH_ERR_CAPACITY = 0, -4
SEG = 992                         # words of a segment
MIB_SEGS = 264                    # whole segments of a bitmap just below 1 MiB
TILE = 8192                       # compressed words of a decoder tile
BATCH = 2 * TILE                  # ... of a decoder workgroup
DT_MAX_GROUPS = 60 * 1024         # groups a decoder tile may expand to before it goes onto the list of deferred tiles
BODY_SEGS = 48                    # segments of a compressor body tile
DEC_SIZES = [1, BATCH, BATCH + 1, 3 * BATCH + 5000]
COMP_SIZES = [SEG * BODY_SEGS, SEG * BODY_SEGS + 1, SEG * (BODY_SEGS * 3 + 5) + 17]
KINDS = ["sparse", "dense", "clustered"]


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


def _tile_groups(stream):
    """Groups each 8192-word decoder tile of a stream expands to."""
    w = stream.astype(np.uint64)
    groups = np.where(w & 0x80000000, w & 0x3FFFFFFF, 1)
    pad = (-len(groups)) % TILE
    return np.concatenate([groups, np.zeros(pad, np.uint64)]).reshape(-1, TILE).sum(axis=1)


def _bitmap(oracle, kind, n, seed):
    if kind == "clustered":
        return oracle.gen_clustered(n, seed, 4096)
    return oracle.gen_uniform(n, seed, 0.01 if kind == "sparse" else 0.5)


def _stream_of(oracle, kind, c_min, seed):
    """A stream of at least c_min words of one kind: bitmaps of whole segments (none above 1 MiB), compressed, back to back."""
    parts, have = [], 0
    while have < c_min:
        parts.append(oracle.compress(_bitmap(oracle, kind, SEG * MIB_SEGS, seed + len(parts))))
        have += len(parts[-1])
    return np.concatenate(parts)


class _Shapes:
    """The inputs every test here draws from, and the oracle's answers, made once."""

    def __init__(self, oracle):
        # ---- decoder: per kind one stream of four batches' worth; its prefixes are the shorter streams
        self.stream = {k: _stream_of(oracle, k, DEC_SIZES[-1], 900 + 37 * i)[: DEC_SIZES[-1]] for i, k in enumerate(KINDS)}
        self.dec_want = {(k, c): oracle.decompress(self.stream[k][:c]) for k in KINDS for c in DEC_SIZES}
        # ---- whole segments dense || clustered || sparse: two plain batches, deferred ones, ordinary ones
        self.mixed = np.concatenate([oracle.compress(_bitmap(oracle, "dense", SEG * 32, 31)),
                                     _stream_of(oracle, "clustered", BATCH + TILE, 41),
                                     oracle.compress(_bitmap(oracle, "sparse", SEG * 64, 51))])
        self.mixed_want = oracle.decompress(self.mixed)
        # ---- compressor: per kind one bitmap with a word in front (the 4-byte shifted address); its prefixes are the smaller inputs
        self.bitmap = {k: _bitmap(oracle, k, COMP_SIZES[-1] + 1, 700 + i) for i, k in enumerate(KINDS)}


@pytest.fixture(scope="module")
def shapes(oracle):
    return _Shapes(oracle)


def test_the_shapes_are_what_the_tests_mean(shapes):
    full = DEC_SIZES[-1] // TILE  # whole tiles of the longest stream
    assert np.all(_tile_groups(shapes.stream["clustered"])[:full] > DT_MAX_GROUPS)   # every tile deferred
    assert _tile_groups(shapes.stream["sparse"]).max() <= DT_MAX_GROUPS              # none
    assert np.any(shapes.stream["sparse"] & 0x80000000)                              # ordinary tiles: fills among the literals
    assert not np.any(shapes.stream["dense"] & 0x80000000)                           # plain tiles: literals only
    m = shapes.mixed
    assert not np.any(m[: 2 * BATCH] & 0x80000000) and np.any(m[2 * BATCH: 2 * BATCH + 8] & 0x80000000)  # two plain batches, no more
    g = _tile_groups(m)
    assert np.all(g[4:7] > DT_MAX_GROUPS) and g[-3:].max() <= DT_MAX_GROUPS and len(m) > 4 * BATCH + TILE


# ---- decoder ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", DEC_SIZES)
def test_decode_streams_of_one_to_four_batches(wah, shapes, kind, c):
    """1 word, exactly one batch, one batch + 1 word, and four workgroups that wait for each other -- ordinary tiles, plain tiles,
    and tiles that all go onto the list: the output, info[0] / info[1] and the status."""
    want = shapes.dec_want[kind, c]
    dec = wah.DeviceDecompressor(c, len(want) + 1, one_pass=True)
    dec.out.fill_(0x5A5A5A5A)
    dec.run(_dev(shapes.stream[kind][:c]))
    assert _route_is(dec.route, "one pass")
    assert wah.lib().wah_decompress_status(dec.workspace.data_ptr(), None) == WAH_OK
    st = shapes.stream[kind][:c].astype(np.uint64)
    groups = int(np.where(st & 0x80000000, st & 0x3FFFFFFF, 1).sum())
    assert int(dec.info[0].item()) == len(want) and int(dec.info[1].item()) == groups
    assert np.array_equal(_host(dec.result()), want)


def test_decode_plain_deferred_and_ordinary_batches_side_by_side(wah, shapes):
    dec = wah.DeviceDecompressor(len(shapes.mixed), len(shapes.mixed_want) + 1, one_pass=True)
    dec.run(_dev(shapes.mixed))
    assert _route_is(dec.route, "one pass")
    st = shapes.mixed.astype(np.uint64)
    assert int(dec.info[1].item()) == int(np.where(st & 0x80000000, st & 0x3FFFFFFF, 1).sum())
    assert int(dec.info[0].item()) == len(shapes.mixed_want)
    assert np.array_equal(_host(dec.result()), shapes.mixed_want)


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_a_capacity_one_word_short(wah, shapes, kind):
    """WAH_ERR_CAPACITY from the last batch's bookkeeping, and the part that fits is right (the one-pass decoder writes as the
    tiles come by)."""
    c = DEC_SIZES[-1]
    want = shapes.dec_want[kind, c]
    dec = wah.DeviceDecompressor(c, len(want) - 1, one_pass=True)
    dec.run(_dev(shapes.stream[kind]))
    assert wah.lib().wah_decompress_status(dec.workspace.data_ptr(), None) == WAH_ERR_CAPACITY
    if not _FORCED_NO_WAIT:  # (the two-launch routes write nothing when the output is too small: include/wah.h)
        assert np.array_equal(_host(dec.out)[: len(want) - 1], want[:-1])


def test_three_runs_back_to_back_on_one_workspace(wah, shapes):
    """Clustered, sparse, clustered without a synchronisation between them, then the other way round: every launch finds the epoch
    and the pair of deferred-tile counters as the launch in front of it flipped them in its last batch's bookkeeping."""
    c = DEC_SIZES[-1]
    both = {k: (_dev(shapes.stream[k]), shapes.dec_want[k, c]) for k in ("clustered", "sparse")}
    cap = max(len(w) for _, w in both.values()) + 1
    dec = wah.DeviceDecompressor(c, cap, one_pass=True)
    outs = [wah.DeviceDecompressor(c, cap, one_pass=True) for _ in range(3)]
    for order in (("clustered", "sparse", "clustered"), ("sparse", "clustered", "sparse")):
        for k, o in zip(order, outs):  # one workspace, an output buffer per run: nothing is read back in between
            rc = wah.lib().wah_decompress_device_ex(both[k][0].data_ptr(), c, o.out.data_ptr(), cap, o.info.data_ptr(), 8,
                                                    dec.workspace.data_ptr(), dec.ws_bytes, None)
            assert rc == WAH_OK
        dec.status()
        for k, o in zip(order, outs):
            want = both[k][1]
            assert int(o.info[0].item()) == len(want), (order, k)
            assert np.array_equal(_host(o.out)[: len(want)], want), (order, k)


@pytest.mark.parametrize("at", [TILE, BATCH], ids=["behind the batch's first tile", "behind the batch"])
def test_an_empty_fill_behind_a_tile_s_last_segment(wah, oracle, at):
    """A foreign stream (every fill of two groups or more written as two fill words) with a fill word of count 0 as the first word behind a tile: the
    tile's last segment needs words from there and cannot flag that one, so the segment's expand tile goes onto the list from
    inside the segment loop."""
    n = 75000
    stream = fg.reencode(oracle.gen_uniform(n, 77, 0.01), n, "split 8")
    assert len(stream) > 2 * BATCH and _tile_groups(stream).max() <= DT_MAX_GROUPS
    assert int(_tile_groups(stream[:at]).sum()) % 1024 != 0  # the tile's last segment runs on behind the tile
    stream = np.concatenate([stream[:at], np.array([0x80000000], np.uint32), stream[at:]])
    want = oracle.decompress(stream)
    assert np.array_equal(want[:n], oracle.gen_uniform(n, 77, 0.01))
    dec = wah.DeviceDecompressor(len(stream), len(want) + 1, one_pass=True)
    dec.run(_dev(stream))
    assert _route_is(dec.route, "one pass")
    assert np.array_equal(_host(dec.result()), want)


# ---- compressor ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shift", [0, 1], ids=["16-byte aligned", "4-byte shifted"])
@pytest.mark.parametrize("n", COMP_SIZES)
def test_compress_body_tiles_tail_tile_and_ragged_segment(wah, oracle, shapes, kind, shift, n):
    """One body tile of 48 segments, one body tile + 1 word, and three body tiles, a tail-shape tile and a ragged last segment:
    the whole stream, and with indexed=True the segment offsets (the oracle's running counts)."""
    data = shapes.bitmap[kind][shift: shift + n]
    want = oracle.compress(data)
    d = _dev(shapes.bitmap[kind])[shift: shift + n]
    assert d.data_ptr() % 16 == 4 * shift
    comp = wah.DeviceCompressor(n)
    comp.run(d)
    assert np.array_equal(_host(comp.result()), want)
    icomp = wah.DeviceCompressor(n, indexed=True)
    icomp.run(d)
    assert np.array_equal(_host(icomp.result()), want)
    n_seg = (n + SEG - 1) // SEG
    counts = [len(oracle.compress(data[s * SEG: (s + 1) * SEG])) for s in range(n_seg)]
    assert np.array_equal(icomp.seg_offsets[: n_seg + 1].cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
