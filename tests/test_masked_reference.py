"""CPU test of tests/_masked.py: the bitmap-level and the stream-level reference of the masked count equal the popcount of the
AND of the oracle's decoded words for every pair of tests/_select.py's bitmaps at ragged lengths, the pad rule holds for every
pair of its hand-built streams that set pad bits, and the hand builders are what they say."""
import numpy as np
import pytest

from tests import _masked as msk
from tests import _select as sel


@pytest.mark.parametrize("n", [1, 30, 31, 32, 991, 992, 993, 2 * 992 + 5])
def test_references_equal_the_oracle(oracle, n):
    maps = sel.bitmaps(oracle, n)
    streams = {name: oracle.compress(words) for name, words in maps.items()}
    decoded = {name: oracle.decompress(st) for name, st in streams.items()}
    seen = set()
    for a in maps:
        assert np.array_equal(decoded[a][:n], maps[a]), a
        for b in maps:
            both = decoded[a][:n] & decoded[b][:n]
            want = int(np.unpackbits(both.view(np.uint8)).sum(dtype=np.int64))
            assert msk.ref_counts(maps[a], maps[b], n) == want, (n, a, b)
            assert msk.stream_counts(streams[a], streams[b], n) == want, (n, a, b)
            seen.add(want)
        assert msk.ref_counts(maps[a], maps[a], n) == sel.ref_count(maps[a], n) == msk.ref_counts(maps["ones"], maps[a], n)
        assert msk.ref_counts(maps["zeros"], maps[a], n) == 0
    assert len(seen) > 4 and 32 * n in seen and 0 in seen


def test_pad_rule_for_pairs_of_hand_built_streams():
    pads = sel.pad_streams()
    pairs = 0
    for what_a, n, a, bits_a in pads:
        assert msk.stream_counts(a, a, n) == bits_a == sel.stream_count(a, n), what_a
        for what_b, m, b, bits_b in pads:
            if m != n:
                continue
            want = np.intersect1d(sel.stream_positions(a, n), sel.stream_positions(b, n)).size
            assert msk.stream_counts(a, b, n) == want == msk.stream_counts(b, a, n), (what_a, what_b)
            assert want <= min(bits_a, bits_b)
            pairs += 1
    assert pairs >= 8 + 2 * 5  # every stream with itself, and the lengths 1, 30 and 993 with more than one stream
    # the pad bits ARE set in both: without the rule the first two streams share 62 bits, not 32
    (_, n, a, _), (_, _, b, _) = pads[0], pads[1]
    assert n == 1 and msk.stream_counts(a, b, 1) == 32
    assert int(np.unpackbits((msk.groups_of_stream(a) & msk.groups_of_stream(b)).view(np.uint8)).sum()) == 62


def test_hand_builders():
    rng = np.random.default_rng(2)
    for a in msk.RUN_EDGES:
        for ab in msk.RUN_EDGES:
            if ab < a:
                continue
            st = msk.run_operand(a, ab - a)
            g = msk.groups_of_stream(st)
            assert g.size == sel.SEG_GROUPS and not np.any(st & sel.MASK == 0), (a, ab)
            assert np.array_equal(np.flatnonzero(g), np.arange(a, ab)), (a, ab)
            assert np.array_equal(sel.index_of(st), [0, st.size])
    mask = msk.alternating_mask(rng)
    g = msk.groups_of_stream(mask)
    assert mask.size == g.size == sel.SEG_GROUPS and np.all(g[0::2] == sel.M31) and np.all(mask[1::2] >> 31 == 0)
    assert msk.stream_counts(mask, msk.run_operand(63, 2), 992) == int(bin(int(g[63])).count("1")) + 31
    assert msk.GRID_WAVES == 4096 and 3 * 130 * 37 > msk.GRID_WAVES
    # the chunks the GPU tests reach: one operand per image in the small tables, 2, 16 and 64 in those made for it
    assert [msk.chunk_of(*shape) for shape in ((10, 10, 37), (3, 130, 37), (3, 4097, 1))] == [1, 1, 1]
    assert [msk.chunk_of(*shape) for shape in ((16, 4097, 1), (1, 70, 8200), (2, 70, 33000))] == [2, 16, 64]
