"""CPU test of tests/_foreign.py: every (bitmap, way) is the same bitmap to the oracle's decoder, has a segment index by the
word-by-word restatement of wah_build_index_device, is NOT the canonical stream (so a kernel that is only right on streams of
compress() can fail on it) with the checker's counter that names the way moved, and sits where its name says: the split parts
at the word indices that put them in one lane's pair, in neighbouring lanes and across a batch edge; whole batches of zero
literals; as many words as groups in a ragged last segment.
"""
import numpy as np
import pytest

from tests import _foreign as fg
from tests import _switch as sw
from tests import _walk as wk
from tests.test_walk_reference import _py_index

# n_words: whole segments of every kind; the same with a short last segment of 2 groups (30 pad bits) and of 31 (1 pad bit)
SIZES = (6 * 992, 6 * 992 + 1, 6 * 992 + 30)


def _cases():
    for n in SIZES:
        for way in fg.ways_for(n):
            yield n, way


def _bitmap(n, way, seed=0):
    rng = np.random.default_rng(100 + n + seed)
    return fg.bitmap(n, rng, fg.kinds_for(way, n // 992), fg.tail_for(way, seed)), rng


def test_unpack_is_the_inverse_of_pack():
    rng = np.random.default_rng(1)
    for n in (1, 30, 31, 32, 992, 993, 2 * 992 + 30):
        words = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        g = fg.unpack(words)
        assert g.size == fg.n_groups(n) and not np.any(g >> 31)
        assert np.array_equal(sw.pack(g)[:n], words) and not sw.pack(g)[n:].any()
        assert int(g[-1]) >> (31 - fg.pad_bits(n)) == 0
    assert [fg.pad_bits(n) for n in (992, 993, 2 * 992 + 30, 31)] == [0, 30, 1, 0]


@pytest.mark.parametrize("n,way", list(_cases()))
def test_every_way_is_the_bitmap_has_an_index_and_is_not_canonical(oracle, n, way):
    for seed in range(3):
        data, rng = _bitmap(n, way, seed)
        st = fg.reencode(data, n, way, rng)
        what = (n, way, seed)
        # the same bitmap
        back = oracle.decompress(st)
        assert np.array_equal(back[:n], data), what
        assert oracle.decoded_groups(st) == fg.n_groups(n), what
        if way in fg.PAD_WAYS:   # every pad bit is set in the stream: they decode into the one word behind the bitmap
            pad = fg.pad_bits(n)
            assert pad and back.size == n + 1 and int(back[n]) == (1 << pad) - 1, what
        elif back.size > n:
            assert back[n] == 0, what
        # an index, by both restatements, with the preconditions of the index builder
        offsets, groups = fg.segment_ranges(st)
        assert offsets == _py_index(st) == wk.index(st).tolist() and groups == fg.n_groups(n), what
        per_segment = [int(np.where(st[a:b] & sw.FILL0, st[a:b] & sw.COUNT_MASK, 1).sum()) for a, b in zip(offsets[:-1], offsets[1:])]
        assert per_segment == [1024] * (groups // 1024) + ([groups % 1024] if groups % 1024 else []), what
        # canonical, or provably not
        canon = oracle.compress(data)
        report = wk.report(st)
        assert report[0] == groups and report[2] == 0 and report[4] == 0, what
        if way == "canonical":
            assert np.array_equal(st, canon) and report[6], what
            continue
        assert not np.array_equal(st, canon), what
        if way in fg.EXPECTED_COUNTER:
            assert report[fg.EXPECTED_COUNTER[way]] > 0 and not report[6], (what, report)
        elif way == "mixed":
            assert not report[6] and report[fg.UNMERGED] > 0 and report[fg.FILLABLE] > 0, (what, report)
        else:
            # "pad: literal" and "pad: one-fill" are the canonical streams of ANOTHER bitmap, one that has the pad bits: the
            # checker, which is not told n_words, cannot tell -- the difference from compress(bitmap) above is the proof
            assert way in ("pad: literal", "pad: one-fill"), way


def test_split_parts_lie_where_the_names_say():
    """In the placement segment the parts of the three placed fills lie at words 4 | 5 (one lane's pair), 9 | 10 (neighbouring
    lanes) and 127 | 128 (two batches), under every split way; k = 8 and 9 put a part on either side of kListShortFill."""
    assert fg.SPLITS[1] == sw.LIST_SHORT_FILL and fg.SPLITS[2] == sw.LIST_SHORT_FILL + 1
    rng = np.random.default_rng(5)
    data = fg.bitmap(6 * 992, rng)
    at = 5  # the segment of kind "placement"
    assert fg.KINDS[at] == "placement"
    for way in fg.SPLIT_WAYS:
        st = fg.reencode(data, 6 * 992, way, rng)
        seg = st[fg.segment_ranges(st)[0][at]:]
        k = way[len("split "):]
        k = fg.SPLIT_FILL_GROUPS - 1 if k == "n-1" else int(k)
        for (i, where), kind in zip(fg.PLACED_SPLITS, (sw.FILL1, sw.FILL0, sw.FILL1)):
            assert int(seg[i]) == kind | k and int(seg[i + 1]) == kind | (fg.SPLIT_FILL_GROUPS - k), (way, where)
            assert not seg[i - 1] & sw.FILL0 and not seg[i + 2] & sw.FILL0, (way, where)
        (a, _), (b, _), (c, _) = fg.PLACED_SPLITS
        assert a % 2 == 0 and a // 2 == (a + 1) // 2                      # words 2 l and 2 l + 1: one lane
        assert b % 2 == 1 and b // 2 + 1 == (b + 1) // 2 and b + 1 < sw.LIST_BATCH   # lane l's second word, lane l + 1's first
        assert c // sw.LIST_BATCH + 1 == (c + 1) // sw.LIST_BATCH           # the last word of a batch, the first of the next


def test_zero_literal_batches_and_as_many_words_as_groups():
    rng = np.random.default_rng(6)
    for n in SIZES:
        data = fg.bitmap(n, rng, tail="zeros")
        zeros_at = fg.KINDS.index("zeros")
        st = fg.reencode(data, n, "fillable literals", rng)
        offsets, _ = fg.segment_ranges(st)
        seg = st[offsets[zeros_at]: offsets[zeros_at + 1]]
        assert seg.size == 1024 and not seg.any()                            # batches of 128 zero literals: words 0 .. 127, 128 .. 255, ...
        assert not seg[: sw.LIST_BATCH].any() and not seg[sw.LIST_BATCH: 2 * sw.LIST_BATCH].any()
        ones = st[offsets[fg.KINDS.index("ones")]: offsets[fg.KINDS.index("ones") + 1]]
        assert ones.size == 1024 and bool((ones == sw.M31).all())
        st = fg.reencode(data, n, "fills of one", rng)
        offsets, groups = fg.segment_ranges(st)
        seg = st[offsets[zeros_at]: offsets[zeros_at + 1]]
        assert seg.size == 1024 and bool((seg == (sw.FILL0 | 1)).all())      # w1 - w0 == nvalid == 1024
        if groups % 1024:                                                    # ... and == nvalid in the ragged last segment
            last = st[offsets[-2]:]
            assert last.size == groups % 1024 and bool((last == (sw.FILL0 | 1)).all())
            lits = fg.reencode(data, n, "fillable literals", rng)
            assert lits.size - fg.segment_ranges(lits)[0][-2] == groups % 1024
        for way in fg.TWO_FILL_WAYS:
            st = fg.reencode(data, n, way, rng)
            offsets, _ = fg.segment_ranges(st)
            k = 1 if way == "two fills 1" else 512
            assert st[offsets[zeros_at]: offsets[zeros_at + 1]].tolist() == [sw.FILL0 | k, sw.FILL0 | (1024 - k)]


def test_rows_foreign_rotates_the_ways():
    rng = np.random.default_rng(7)
    n = 2 * 992 + 30
    rows = np.stack([fg.bitmap(n, rng, tail=fg.TAILS[j % 3]) for j in range(16)])
    got = fg.rows_foreign(rows, n, rng)
    assert {way for way, _ in got} >= set(fg.WAYS[1:]) | {"pad: literal"}
    for (way, st), row in zip(got, rows):
        assert way != "canonical" and wk.groups(st) == fg.n_groups(n)


@pytest.mark.parametrize("n", (2 * 992, 2 * 992 + 30))
def test_off_by_one_moves_one_segment_by_one_group(n):
    """The refused streams: by the hand-made index exactly one segment holds one group too many or too few, the changed word lies
    in the stream's non-canonical part, and every other word is the intact stream's."""
    for way in fg.ways_for(n):
        rng = np.random.default_rng(n)
        data = fg.bitmap(n, rng, fg.kinds_for(way, 2), fg.tail_for(way))
        st = fg.reencode(data, n, way, rng)
        total = fg.n_groups(n)
        for delta in (1, -1):
            bad, index, t = fg.off_by_one(st, way, delta)
            assert index.dtype == np.int64 and index[0] == 0 and index[-1] == bad.size and index.size == -(-total // 1024) + 1, (way, delta)
            groups = [int(np.where(bad[a:b] & sw.FILL0, bad[a:b] & sw.COUNT_MASK, 1).sum()) for a, b in zip(index[:-1], index[1:])]
            want = [min(1024, total - 1024 * s) for s in range(len(groups))]
            off = [s for s in range(len(groups)) if groups[s] != want[s]]
            assert len(off) == 1 and groups[off[0]] == want[off[0]] + delta and index[off[0]] <= t < index[off[0] + 1] + (delta < 0), (way, delta)
            assert wk.groups(bad) == total + delta and not np.any((bad & sw.FILL0 != 0) & (bad & sw.COUNT_MASK == 0)), (way, delta)
            if way in fg.PAD_WAYS:
                assert t == st.size - 1
            elif way != "canonical":
                assert t in fg.noncanonical_words(st), (way, delta)
