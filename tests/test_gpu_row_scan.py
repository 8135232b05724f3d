"""GPU tests: the one-hop row scan (gpu-wah_amd/csrc/wah_rowscan.hpp) at its row edge and in row 2, for the scans that no other
test takes there.

A tile of row r, index i adds up part a (its row's granules below it), part b (the previous row) and the slots of the rows
before that.  Part b is first used by tile 256, the first slot behind the superrow's prefix by the tiles of row 2 (512 ..), and
tile 255 is the first that publishes a row's slot.  So every case here gives its kernel 2 x 256 + 2 tiles under the kernel's own
tile shape -- the smallest launch that has a tile in row 2 behind a whole row -- with totals that differ from tile to tile, and
compares the WHOLE output, its word count and (where the call has one) the segment index with the CPU oracle, exactly.

Who covers what (tile 1 / tiles 255, 256, 257 / row 2 / the superrow edge at tile 16 384):
  compress by pairs      test_gpu_parity: test_tile_shapes_of_a_launch (up to 1025 tiles), the 1 GiB configurations (5649 tiles),
                         _check_column_launch (90 200 tiles: five superrow edges)
  unsegmented compress   test_gpu_parity: test_unsegmented_encoder_mode (851 tiles of clustered data and of zeros with islands;
                         12 606 tiles of zeros: no superrow edge)
  tile body, bitmaps     here: test_bitop_pair_mode_reaches_row_two (no other test gives it a whole row of 256 tiles)
  tile body, indexed     here: test_indexed_bitop_reaches_row_two (the same)
  decoder's sums pass    here: test_sums_pass_reaches_row_two (the same: the long streams of the other tests take the one pass)
  one-pass decoder       test_gpu_parity: the 1 GiB configurations (sparse: 7850 tiles; dense: 16 913 tiles, one superrow edge, every
                         tile the same total); here with the route asserted: test_one_pass_decoder_reaches_row_two
"""
import os
import re

import numpy as np
import pytest

from tests import _switch as sw
from tests.test_gpu_parity import _dev, _host, _route_is, wah  # noqa: F401 (wah: the fixture)

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-wah_amd", "csrc")


def _source_constants():
    text = "\n".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)))
    out = {}
    for name in ("kRowTiles", "kSumTilesPerGroup", "kScanTileWords", "kIndexedSegsPerWave", "kCompressMaxWaveSegs"):
        m = re.search(rf"constexpr \w+ {name} = (\d+);", text)
        assert m, f"{name}: definition not found in gpu-wah_amd/csrc"
        out[name] = int(m.group(1))
    return out


K = _source_constants()
TILES = 2 * K["kRowTiles"] + 2                                      # rows 0 and 1, and two tiles of row 2
SUMS_TILE_WORDS = K["kSumTilesPerGroup"] * K["kScanTileWords"]      # decode_sums_kernel<1>: one expand tile per wave
ONE_PASS_TILE_WORDS = sw.DT_BATCH * sw.DT_TILE_WORDS                # decode_tile_kernel: a batch of tiles per workgroup
THREADS = min(os.cpu_count() or 1, 16)


def _segment_index(oracle, bitmap):
    """The segment index of compress(bitmap), from the oracle alone: where every segment's words start, and the total."""
    lengths = [oracle.compress(bitmap[lo: lo + sw.SEG_WORDS]).size for lo in range(0, bitmap.size, sw.SEG_WORDS)]
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def test_bitop_pair_mode_reaches_row_two(wah, oracle):
    """wah_bitop_device: compress_tile_pair_kernel at five segments per wave, 514 tiles of 40 segments (the last one segment),
    clustered operands: compress(A xor B), every word and the count."""
    n_segments = (TILES - 1) * sw.TILE_WAVES * K["kCompressMaxWaveSegs"] + 1
    assert sw.wave_segs(n_segments) == K["kCompressMaxWaveSegs"]
    n = n_segments * sw.SEG_WORDS - 300
    a, b = _host(wah.gen_clustered_device(n, 41)), _host(wah.gen_clustered_device(n, 42, 700))  # (the oracle's generators, faster)
    want = oracle.compress_mt(a ^ b, THREADS)
    got = _host(wah.bitop_device("xor", _dev(oracle.compress_mt(a, THREADS)), _dev(oracle.compress_mt(b, THREADS)), n))
    assert got.size == want.size and np.array_equal(got, want)


def test_indexed_bitop_reaches_row_two(wah, oracle):
    """wah_bitop_indexed_device by the decode-based route: bitop_tile_kernel<kTileScan>, 514 tiles of 16 segments (the last one
    segment, cut short): compress(A and B), every word, the count and the result's segment index."""
    import torch

    n_segments = (TILES - 1) * sw.TILE_WAVES * K["kIndexedSegsPerWave"] + 1
    n = n_segments * sw.SEG_WORDS - 300
    a, b = _host(wah.gen_uniform_device(n, 43, 0.05)), _host(wah.gen_clustered_device(n, 44, 700))
    ca, cb, want = oracle.compress_mt(a, THREADS), oracle.compress_mt(b, THREADS), oracle.compress_mt(a & b, THREADS)
    assert ca.size + cb.size > sw.RUNS_MAX_WORDS_PER_SEG * n_segments  # (not the run merge's case)
    index = _segment_index(oracle, a & b)
    assert index[-1] == want.size
    got, offs = wah.bitop_indexed_device("and", _dev(ca), torch.from_numpy(_segment_index(oracle, a)).cuda(), _dev(cb),
                                         torch.from_numpy(_segment_index(oracle, b)).cuda(), n)
    assert wah.lib().wah_last_bitop_route() == 2
    assert got.numel() == want.size and np.array_equal(_host(got), want)
    assert np.array_equal(offs.cpu().numpy()[: index.size], index)


@pytest.fixture(scope="module")
def long_stream(oracle):
    """(stream, decoded words, groups): a foreign stream of 514 workgroup tiles of the sums pass less a few words -- literals and
    fills of 1 to 8 groups, the share of fills drawn anew for every 4096 words (0 to 30 %), so that no two tiles expand alike."""
    rng = np.random.default_rng(514)
    n = TILES * SUMS_TILE_WORDS - 37
    st = rng.integers(1, sw.M31, n, dtype=np.uint64).astype(np.uint32)
    share = np.repeat(rng.random((n + 4095) // 4096) * 0.3, 4096)[:n]
    fills = np.flatnonzero(rng.random(n) < share)
    st[fills] = (np.where(rng.integers(0, 2, fills.size), sw.FILL1, sw.FILL0) | rng.integers(1, 9, fills.size)).astype(np.uint32)
    want = oracle.decompress(st)
    groups = oracle.decoded_groups(st)
    per_tile = np.add.reduceat(np.where(st & sw.FILL0, st & 0xF, 1).astype(np.int64), np.arange(0, n, SUMS_TILE_WORDS))
    assert per_tile.size == TILES and np.unique(per_tile).size > TILES * 9 // 10
    return st, want, groups


def _decode(wah, long_stream, route, **kw):
    st, want, groups = long_stream
    dec = wah.DeviceDecompressor(st.size, want.size, **kw)
    dec.run(_dev(st))
    assert _route_is(dec.route, route), dec.route
    got = _host(dec.result())
    assert dec.info.tolist() == [want.size, groups]
    assert got.size == want.size and np.array_equal(got, want)


def test_sums_pass_reaches_row_two(wah, long_stream):
    """The two launches: decode_sums_kernel<1> over 514 workgroup tiles of 32 768 words, then the expansion from its bases."""
    assert long_stream[0].size < 16384 * K["kScanTileWords"]  # (one expand tile per wave: the short-stream shape)
    _decode(wah, long_stream, "two launches", two_launches=True)


def test_one_pass_decoder_reaches_row_two(wah, long_stream):
    """decode_tile_kernel over the same stream: 1028 batches of 16 384 words (the default for this capacity)."""
    st, want, _ = long_stream
    assert st.size > (TILES - 1) * ONE_PASS_TILE_WORDS and sw.default_route(st.size, want.size) == 1
    _decode(wah, long_stream, "one pass")
