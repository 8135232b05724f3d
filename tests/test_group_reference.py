"""CPU test of tests/_group.py: the bitmap-level, the stream-level and the value-level reference of the grouped sum agree with
each other and with the CPU oracle's compress / decompress, the pad rule holds in the group's own row count as in the counts,
the fold is exact beyond 64 bits, and the hand builders and the restated item and chunk rule are what they say."""
import numpy as np
import pytest

from tests import _group as grp
from tests import _masked as msk
from tests import _select as sel


@pytest.mark.parametrize("n", [5, 992, 992 * 3 + 5])
def test_bitmap_and_stream_references_equal_the_oracle(oracle, n):
    """Filters, group rows and slices taken from tests/_select.py's bitmaps: the conjunction ANDed by hand from the oracle's
    decoded words, both references against it."""
    maps = sel.bitmaps(oracle, n)
    streams = {name: oracle.compress(words) for name, words in maps.items()}
    decoded = {name: oracle.decompress(st)[:n] for name, st in streams.items()}
    for name in maps:
        assert np.array_equal(decoded[name], maps[name]), name
    names = list(maps)
    filters = ["uniform 0.9", "ones"]
    groups = [["uniform 0.3", "clustered"], ["ones", "edges"], ["zeros", "uniform 0.9"], ["last bit", "ones"]]
    slices = names[2:9]
    attr_bits = [3, 1, 3]
    for f in (0, 1, 2):
        want_rows, want_counts = [], []
        for own in groups:
            both = np.full(n, 0xFFFFFFFF, np.uint32)
            for name in filters[:f] + own:
                both &= decoded[name]
            want_rows.append(sel.ref_count(both, n))
            want_counts.append([msk.ref_counts(both, decoded[s], n) for s in slices])
        want = (want_rows, want_counts, [grp.fold(c, attr_bits) for c in want_counts])
        assert grp.ref_group([maps[x] for x in filters[:f]], [[maps[x] for x in own] for own in groups], [maps[x] for x in slices], attr_bits, n) == want
        assert grp.stream_group([streams[x] for x in filters[:f]], [[streams[x] for x in own] for own in groups], [streams[x] for x in slices], attr_bits, n) == want
    assert want_rows[2] == 0 and want_rows[3] <= 1 and len(set(want_rows)) >= 3


def test_value_model_equals_the_bitmap_reference():
    """Keys, values and a filter as a table has them; their equality-encoded and bit-sliced bitmaps give the same aggregates."""
    rng = np.random.default_rng(5)
    rows, n = 3000, 992
    a, b = rng.integers(0, 3, rows), rng.integers(0, 2, rows)
    x, y = rng.integers(0, 1 << 12, rows), rng.integers(0, 1 << 20, rows)
    y_exists = rng.random(rows) < 0.8
    chosen = (x >= 100) & (x <= 3000)
    want_rows, want_sums, want_counts = grp.value_model([a, b], [3, 2], [(x, None), (y, y_exists)], chosen)
    assert sum(sum(r) for r in want_rows) == int(chosen.sum()) and want_counts[0] == want_rows and want_counts[1] != want_rows
    ka, kb = grp.key_bitmaps(a, 3, n), grp.key_bitmaps(b, 2, n)
    slices = grp.slices_of(x, 12, n) + grp.slices_of(y, 20, n, y_exists)
    assert len(slices) == 12 + 21
    filt = sel.bitmap_of(np.flatnonzero(chosen), n)
    got_rows, _, got_sums = grp.ref_group([filt], [[ka[i], kb[j]] for i in range(3) for j in range(2)], slices, [12, 20, 1], n)
    assert got_rows == [r for row in want_rows for r in row]
    assert [s[0] for s in got_sums] == [s for row in want_sums[0] for s in row]
    assert [s[1] for s in got_sums] == [s for row in want_sums[1] for s in row]
    assert [s[2] for s in got_sums] == [c for row in want_counts[1] for c in row]
    assert [s[0] for s in got_sums] == [int(x[chosen & (a == i) & (b == j)].sum()) for i in range(3) for j in range(2)]


def test_pad_rule_in_rows_and_counts():
    """Hand-built streams that set pad bits as filter, group row and operand at once: neither the rows nor a count sees them."""
    for _, n, st, bits in sel.pad_streams():
        rows, counts, sums = grp.stream_group([st], [[st]], [st], [1], n)
        assert rows == [bits] and counts == [[bits]] and sums == [[bits]], n
        assert rows[0] == sel.stream_count(st, n) == grp.ref_group([], [[grp.bitmap_of_stream(st, n)]], [], [], n)[0][0]
    # without the rule the one-fill over both groups of one word would count 62
    assert int(np.unpackbits(msk.groups_of_stream(np.array([0xC0000002], np.uint32)).view(np.uint8)).sum()) == 62


def test_fold_beyond_64_bits():
    ones = 31744  # a one-fill over 992 words
    assert grp.fold([ones] * 64, [64]) == [ones * ((1 << 64) - 1)]
    low, high = grp.split128(ones * ((1 << 64) - 1))
    assert high == ones - 1 and low == (1 << 64) - ones and high != 0
    assert grp.fold([5], [1]) == [5] and grp.fold(list(range(64)), [1] * 64) == list(range(64))
    assert grp.fold([1, 2, 3, 4], [3, 1]) == [4 + 4 + 3, 4]
    # a count is below 2^45 and an attribute has at most 64 slices: below 2^109
    assert grp.fold([(1 << 45) - 1] * 64, [64])[0] < 1 << 109


@pytest.mark.parametrize("n", [5, 992, 992 * 3 + 5])
def test_kind_streams_are_indexed_streams_of_every_kind(n):
    rng = np.random.default_rng(n)
    names, streams, indexes = grp.kind_streams(rng, n)
    assert len(names) == 14 and names[:4] == ["zero fill", "one fill", "literals", "mixed"]
    for st, index in zip(streams, indexes):
        assert msk.groups_of_stream(st).size == sel.groups_of(n) and not np.any((st & sel.FILL != 0) & (st & sel.MASK == 0))
        assert np.array_equal(index, sel.index_of(st)) and index.size == sel.segments_of(n) + 1
        words = grp.bitmap_of_stream(st, n)
        assert words.size == n and sel.ref_count(words, n) == sel.stream_count(st, n)
    # the stream level equals the bitmap level over the streams' bitmaps, pad bits or not
    maps = [grp.bitmap_of_stream(st, n) for st in streams]
    pick = [[streams[k], streams[(k + 3) % 14]] for k in range(14)]
    pick_maps = [[maps[k], maps[(k + 3) % 14]] for k in range(14)]
    assert grp.stream_group([streams[2]], pick, streams, [7, 7], n) == grp.ref_group([maps[2]], pick_maps, maps, [7, 7], n)


def test_hand_built_segments():
    rng = np.random.default_rng(3)
    kinds = grp.segment_kinds(rng)
    assert len(kinds) == 14
    for name, st in kinds.items():
        g = msk.groups_of_stream(st)
        assert g.size == sel.SEG_GROUPS and np.array_equal(sel.index_of(st), [0, st.size]), name
    assert kinds["zero fill"].size == kinds["one fill"].size == 1 and kinds["literals"].size == sel.SEG_GROUPS
    assert np.array_equal(np.flatnonzero(msk.groups_of_stream(kinds["ones up to group 64"])), np.arange(64))
    assert np.array_equal(np.flatnonzero(msk.groups_of_stream(kinds["ones from group 1023"])), [1023])
    assert np.array_equal(np.flatnonzero(msk.groups_of_stream(kinds["ones in the last group"])), [1023])
    mixed = kinds["mixed"]
    assert np.any(mixed >> 30 == 3) and np.any(mixed >> 30 == 2) and np.any(mixed >> 31 == 0)
    for groups in (3, 6, 1023):
        for name, st in grp.partial_kinds(rng, groups).items():
            assert msk.groups_of_stream(st).size == groups, (groups, name)


def test_items_chunks_and_runs():
    """The rule of launch_group_sum restated: the masked count's with the groups in the masks' place."""
    assert grp.chunk_of(3, 130, 37) == msk.chunk_of(3, 130, 37) == 1
    assert [grp.chunk_of(*shape) for shape in ((16, 4097, 1), (1, 70, 8200), (2, 70, 33000))] == [2, 16, 64]
    assert grp.chunk_of(4097, 2, 1) == 1 and grp.chunk_of(14, 14, 4) == 1
    items = grp.items_of(2, 3, 2)
    assert items == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 2, 0), (0, 2, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 2, 0), (1, 2, 1)]
    # more items than a full grid has wavefronts: a wavefront's run holds several, and changes (g, c) inside
    per, waves = grp.runs_of(3, 130, 37)
    assert 3 * 130 * 37 > msk.GRID_WAVES and per == 4 and waves <= msk.GRID_WAVES and per < 37
    per, waves = grp.runs_of(4097, 2, 1)
    assert per == 3 and waves <= msk.GRID_WAVES  # three (g, c) per wavefront, twelve per workgroup
    assert grp.runs_of(14, 14, 1) == (1, 196)
    assert (grp.MAX_FILTERS, grp.MAX_ROWS, grp.MAX_ATTRS) == (64, 8, 64)
