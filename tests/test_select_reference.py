"""CPU test of tests/_select.py: the stream-level references (a walk over the words, with the pad rule) equal the bitmap-level
ones (popcount and flatnonzero of the decoded words) on compress() outputs at ragged lengths; the pad rule holds on hand-built
streams that set pad bits; and every builder sits where it says it does, on both sides of the kernels' constants."""
import numpy as np
import pytest

from tests import _select as sel


@pytest.mark.parametrize("n", [1, 7, 30, 31, 32, 991, 992, 993, 992 * 3 + 5, 992 * 9 + 991])
def test_stream_references_equal_the_bitmap_references(oracle, n):
    maps = sel.bitmaps(oracle, n)
    counts = []
    for name, words in maps.items():
        stream = oracle.compress(words)
        decoded = oracle.decompress(stream)
        assert np.array_equal(decoded[:n], words), name
        want = sel.ref_positions(decoded, n)
        assert np.array_equal(want, sel.ref_positions(words, n))
        got = sel.stream_positions(stream, n)
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, name)
        assert sel.stream_count(stream, n) == sel.ref_count(decoded, n) == want.size, (n, name)
        counts.append(want.size)
    assert counts[0] == 0 and counts[1] == 32 * n and len(set(counts)) > 3
    assert maps["first bit"][0] == 1 and maps["last bit"][-1] == 0x80000000


def test_pad_rule_on_hand_built_streams():
    for what, n, stream, bits in sel.pad_streams():
        groups = int(np.where(stream & sel.FILL, stream & sel.MASK, 1).sum())
        assert groups == sel.groups_of(n), what
        pos = sel.stream_positions(stream, n)
        assert pos.size == bits == sel.stream_count(stream, n), what
        assert pos.size == 0 or pos[-1] < 32 * n, what
    # the pad bits ARE set in these streams: a walk without the rule counts more
    what, n, stream, bits = sel.pad_streams()[0]
    assert n == 1 and stream.tolist() == [0xC0000002] and bits == 32
    assert sel.stream_positions(stream, 2).size == 62
    with_pad = [sel.stream_positions(st, n + 1).size > bits for _, n, st, bits in sel.pad_streams() if sel.pad_bits(n)]
    assert len(with_pad) >= 6 and all(with_pad)
    assert [sel.pad_bits(n) for n in (1, 30, 31, 992, 993)] == [30, 1, 0, 0, 30]


def test_builders_sit_on_the_constants(oracle):
    assert (sel.STEP_GROUPS, sel.SEG_GROUPS, sel.BATCH_WORDS, sel.STAGE_SLOTS, sel.SEG_BITS) == (64, 1024, 128, 1984, 31744)
    rng = np.random.default_rng(1)
    assert {sel.BATCH_WORDS - 1, sel.BATCH_WORDS, sel.BATCH_WORDS + 1} <= set(sel.SEGMENT_WORD_EDGES)
    for words in sel.SEGMENT_WORD_EDGES:
        for bit in (0, 1):
            seg = sel.segment_of_words(words, rng, bit)
            assert seg.size == sel.SEG_WORDS and oracle.compress(seg).size == words, (words, bit)
    assert {sel.STAGE_SLOTS - 1, sel.STAGE_SLOTS, sel.STAGE_SLOTS + 1} <= set(sel.SEGMENT_BIT_EDGES)
    for k in sel.SEGMENT_BIT_EDGES:
        seg = sel.segment_of_bits(k)
        pos = sel.ref_positions(seg, sel.SEG_WORDS)
        assert seg.size == sel.SEG_WORDS and pos.size == k == sel.ref_count(seg, sel.SEG_WORDS)
        # the step the last bit lies in: STAGE_SLOTS bits end the first step exactly, one more begins the second
        assert k == 0 or pos[-1] // (31 * sel.STEP_GROUPS) == (k - 1) // sel.STAGE_SLOTS
    assert sel.ref_positions(sel.segment_of_bits(sel.STAGE_SLOTS), 992)[-1] // 31 == sel.STEP_GROUPS - 1
    assert sel.ref_positions(sel.segment_of_bits(sel.STAGE_SLOTS + 1), 992)[-1] // 31 == sel.STEP_GROUPS
    # a bit on each side of every segment and step edge
    n = 992 * 3 + 5
    pos = set(sel.ref_positions(sel.edge_bits(n), n).tolist())
    for s in (1, 2, 3):
        assert {sel.SEG_BITS * s - 1, sel.SEG_BITS * s} <= pos
    for s in range(1, 16):
        assert {1984 * s - 1, 1984 * s} <= pos
    assert sel.ref_positions(sel.edge_bits(992), 992)[-1] == sel.SEG_BITS - 1  # (the far side of the last edge is not in the bitmap)
    # the index of a stream
    stream = oracle.compress(sel.edge_bits(n))
    offs = sel.index_of(stream)
    assert offs.size == sel.segments_of(n) + 1 and offs[0] == 0 and offs[-1] == stream.size and np.all(np.diff(offs) > 0)


def test_long_stream_is_what_it_says():
    """The stream of more segments than a rank-scan chunk holds: proven on a short one with the walk, then by arithmetic."""
    n, stream, index, positions = sel.long_stream(9, {0: 0, 3: 30, 8: 7})
    assert n == 9 * 992 and np.array_equal(sel.index_of(stream), index)
    assert np.array_equal(sel.stream_positions(stream, n), positions) and sel.stream_count(stream, n) == 3
    assert positions.tolist() == [0, 3 * 31744 + 30, 8 * 31744 + 7]
    big = sel.RANK_CHUNK * 2 + 5
    n, stream, index, positions = sel.long_stream(big, {0: 1, sel.RANK_CHUNK - 1: 2, sel.RANK_CHUNK: 3, big - 1: 30})
    assert index.size == big + 1 > sel.RANK_CHUNK and stream.size == big + 4 == index[-1]
    assert np.array_equal(sel.index_of(stream), index) and sel.stream_count(stream, n) == 4
    assert np.array_equal(sel.stream_positions(stream, n), positions)
