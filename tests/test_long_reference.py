"""CPU proof of tests/_long.py, the segment-sparse model the GPU tests of long bitmaps (tests/test_gpu_long_bitmaps.py) assert
against.  On bitmaps of 40 segments, whole and ragged, every reference of the model equals the dense numpy models of the other
helper modules applied to the decoded bitmap; the named rows and segments of the two long sizes are where they are said to be;
every count, sum and rank the GPU tests assert passes 2^32 where its name says so; and the stream of every operand decodes, on its
live segments, to the model."""
import numpy as np
import pytest

from tests import _arith, _bsi, _cmp, _fetch, _group, _kth, _long as lg, _mul, _select as sel, _splice

SEG_WORDS, SEG_BITS = lg.SEG_WORDS, lg.SEG_BITS
SHORT = 40
RUNS = (([0], [0]), ([0], [1]), ([0, 9, 20, 33], [0, 1, 0, 1]), ([0, 1, 39], [1, 0, 1]), ([0, 10, 25], [1, 0, 1]))
LIVE = ((0, 8, 9, 10, 19, 39), (3, 9, 20, 38), (0, 1, 32, 33), (5, ), (0, 39), ())


def short(j, ragged=False):
    """Short bitmap j: runs of defaults and live segments that differ from one j to the next; ragged: a last segment of 7 words."""
    rng = np.random.default_rng(j)
    live = {s: lg.random_segment(rng, (0.5, 0.03, 0.98)[(j + s) % 3]) for s in LIVE[j % len(LIVE)]}
    if ragged:
        live[SHORT - 1] = np.concatenate([lg.random_segment(rng)[:7], np.zeros(SEG_WORDS - 7, np.uint32)])
    return lg.LongBitmap(SHORT, RUNS[j % len(RUNS)], live, 7 if ragged else SEG_WORDS)


def short_column(n_bits, seed, ragged=False):
    return [short(seed + i, ragged) for i in range(n_bits)]


def values_of(slices):
    return _bsi.values_of_slices(np.stack([s.decoded() for s in slices]), len(slices))[0]


def bools(bitmap):
    return _bsi.unpack_bits(bitmap.decoded())


# ---- 1: the model against the dense models ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", (False, True))
def test_stream_count_positions_and_bits(oracle, ragged):
    for j in range(8):
        b = short(j, ragged)
        words, n = b.decoded(), b.n_words
        assert n == (SHORT * SEG_WORDS if not ragged else (SHORT - 1) * SEG_WORDS + 7)
        stream, index = b.stream_index(oracle)
        assert np.array_equal(stream, oracle.compress(words)) and np.array_equal(index, sel.index_of(stream))
        got = b.expected_stream_index(oracle)
        assert np.array_equal(got[0], stream) and np.array_equal(got[1], index)
        assert b.count() == sel.ref_count(words, n) == sel.stream_count(stream, n)
        pos = sel.ref_positions(words, n)
        for first, limit in ((0, None), (0, 5), (31_000, 2000), (max(pos.size - 3, 0), 10), (pos.size, 4), (100_000, 70_000)):
            assert np.array_equal(b.positions(first, limit), pos[first: None if limit is None else first + limit]), (j, first, limit)
        rows = np.sort(np.random.default_rng(j).integers(0, b.n_bits, 500))
        assert np.array_equal(b.bits_at(rows), _fetch.bits_at(stream, rows))
        assert [b.bit(r) for r in (0, b.n_bits - 1)] == _fetch.bits_at(stream, [0, b.n_bits - 1]).tolist()
        if not ragged:   # a split stream is the same bitmap in other words
            for split in (2, 128):
                st, ix = b.stream_index(oracle, split)
                assert np.array_equal(oracle.decompress(st)[:n], words) and np.array_equal(ix, sel.index_of(st))
                assert st.size == stream.size + (split - 1) * (SHORT - len(b.live))


def test_of_words_and_from_rows_and_below(oracle):
    words = oracle.gen_uniform(3 * SEG_WORDS + 5, 3, 0.2)
    assert np.array_equal(lg.LongBitmap.of_words(words).decoded(), words)
    rows = np.unique(np.random.default_rng(1).integers(0, SHORT * SEG_BITS, 300))
    assert np.array_equal(lg.from_rows(SHORT, rows).decoded(), sel.bitmap_of(rows, SHORT * SEG_WORDS))
    for row in (0, 1, SEG_BITS, 5 * SEG_BITS + 77, SHORT * SEG_BITS - 1):
        assert np.array_equal(lg.below(SHORT, row).decoded(), sel.bitmap_of(np.arange(row), SHORT * SEG_WORDS)), row


@pytest.mark.parametrize("ragged", (False, True))
def test_bit_operations_and_clauses(ragged):
    ops = [short(j, ragged) for j in range(9)]
    dense = [o.decoded() for o in ops]
    keep = np.full(ops[0].n_words, 0xFFFFFFFF, np.uint32)
    fold = {"and": np.bitwise_and, "or": np.bitwise_or, "xor": np.bitwise_xor, "andnot": lambda a, b: a & ~b}
    for k in (2, 3, 9):
        for name, fn in fold.items():
            want = dense[0]
            for d in dense[1:k]:
                want = fn(want, d)
            assert np.array_equal(lg.bitop(name, ops[:k]).decoded(), want), (k, name)
    assert np.array_equal(lg.invert(ops[2]).decoded(), ~dense[2] & keep)
    clause_list = [(ops[0:3], False), (ops[3:4], True), (ops[4:9], False)]
    want = (dense[0] | dense[1] | dense[2]) & ~dense[3] & np.bitwise_or.reduce(np.stack(dense[4:9]))
    assert np.array_equal(lg.clauses(clause_list).decoded(), want)
    assert lg.bitop("or", ops[:3]).count() == sel.ref_count(dense[0] | dense[1] | dense[2], ops[0].n_words)


@pytest.mark.parametrize("ragged", (False, True))
def test_range_compare_and_value_at(ragged):
    a, b = short_column(5, 10, ragged), short_column(3, 20, ragged)
    xa, xb = short(30, ragged), short(31, ragged)
    va, vb = values_of(a), values_of(b)
    for lo, hi in ((0, 31), (3, 17), (17, 3), (31, 31), (0, 0), (5, 1 << 70), (40, 50)):
        assert np.array_equal(lg.range_predicate(a, lo, hi).decoded(), _bsi.expected_range(va, lo, hi)), (lo, hi)
        assert np.array_equal(lg.range_predicate(a, lo, hi, xa).decoded(), _bsi.expected_range(va, lo, hi, bools(xa))), (lo, hi)
    for op in _cmp.OPS:
        assert np.array_equal(lg.compare(a, b, op).decoded(), _cmp.expected_compare(va, vb, op)), op
        assert np.array_equal(lg.compare(a, b, op, xa, xb).decoded(), _cmp.expected_compare(va, vb, op, bools(xa), bools(xb))), op
        assert np.array_equal(lg.compare(a, b, op, None, xb).decoded(), _cmp.expected_compare(va, vb, op, None, bools(xb))), op
    rows = np.random.default_rng(2).integers(0, a[0].n_bits, 200).tolist() + [0, a[0].n_bits - 1]
    have = bools(xa)
    for r in rows:
        assert lg.value_at(a, None, r) == int(va[r])
        assert lg.value_at(a, xa, r) == (int(va[r]) if have[r] else None)


@pytest.mark.parametrize("ragged", (False, True))
def test_add_subtract_and_multiply(ragged):
    a, b = short_column(5, 40, ragged), short_column(3, 50, ragged)
    xa, xb = short(60, ragged), short(61, ragged)
    va, vb = values_of(a), values_of(b)
    for n_out in (2, 6, 9):
        for pa, pb in ((None, None), (xa, None), (None, xb), (xa, xb)):
            ba, bb = (None if pa is None else bools(pa)), (None if pb is None else bools(pb))
            for op in _arith.OPS:
                got = np.stack([s.decoded() for s in lg.arith(a, b, op, n_out, pa, pb)])
                assert np.array_equal(got, _arith.expected_matrix(va, vb, op, n_out, ba, bb)), (op, n_out)
            got = np.stack([s.decoded() for s in lg.arith(a, b, "*", n_out, pa, pb)])
            assert np.array_equal(got, _mul.expected_matrix(va, vb, n_out, ba, bb)), ("*", n_out)


@pytest.mark.parametrize("ragged", (False, True))
def test_sums_counts_and_ranks(ragged):
    a = short_column(6, 70, ragged)
    mask, exists = short(80, ragged), short(81, ragged)
    va, n = values_of(a), a[0].n_words
    for m in (None, mask):
        chosen = np.ones(va.size, bool) if m is None else bools(m)
        counts = lg.value_counts(a, m)
        uniq, c = np.unique(va[chosen], return_counts=True)
        assert counts == dict(zip(uniq.tolist(), c.tolist()))
        ranks, model = lg.Ranks(a, m), _kth.Model(va, chosen)
        for q in [c[1:] for c in _kth.query_cases(model.total, spread=True)]:
            assert ranks(*q) == model(*q) == _kth.model(va, chosen, *q), q
    f = [] if mask is None else [mask.decoded()]
    rows, per_slice, sums = _group.ref_group(f, [[np.full(n, 0xFFFFFFFF, np.uint32)]], [s.decoded() for s in a], [6], n)
    assert lg.sum_count(a, mask) == (sums[0][0], rows[0], rows[0])
    assert [lg.bitop("and", [mask, s]).count() for s in a] == per_slice[0]
    have = bools(mask) & bools(exists)
    stored = [lg.bitop("and", [s, exists]) for s in a]   # an index stores 0 where the row does not exist
    assert lg.sum_count(stored, mask, exists) == (int(va[have].astype(object).sum()), int(have.sum()), int(bools(mask).sum()))


def test_splice():
    srcs = [short(j) for j in range(4)] + [short(5, ragged=True)]
    cases = [[(0, 0, SHORT * SEG_BITS)],
             [(1, 5, 3 * SEG_BITS + 11), (2, 9 * SEG_BITS - 3, 12 * SEG_BITS), (3, 0, 1), (0, 20 * SEG_BITS, 0), (4, SEG_BITS - 1, 38 * SEG_BITS + 200)],
             [(2, 31, 10 * SEG_BITS), (2, 31, 10 * SEG_BITS), (1, 33 * SEG_BITS + 4096, 6 * SEG_BITS)],
             [(3, 7 * SEG_BITS, SEG_BITS), (0, 8 * SEG_BITS + 1, 2 * SEG_BITS - 1)]]
    for pieces in cases:
        total = sum(n for _, _, n in pieces)
        for n_words_out in {-(-total // 32), -(-total // 32) + 1, (-(-total // SEG_BITS) + 2) * SEG_WORDS}:
            n_seg, last = -(-n_words_out // SEG_WORDS), n_words_out - (-(-n_words_out // SEG_WORDS) - 1) * SEG_WORDS
            got = lg.splice([(srcs[j], first, n) for j, first, n in pieces], n_seg, last)
            want = _splice.model([(srcs[j].decoded(), first, n) for j, first, n in pieces], n_words_out)
            assert got.n_words == n_words_out and np.array_equal(got.decoded(), want), (pieces, n_words_out)


def test_expected_streams_is_the_layout_of_the_calls_that_return_several_bitmaps(oracle):
    class Case:   # what _splice.reference reads
        n_words_out, n_columns = SHORT * SEG_WORDS, 3

        def column(self, c):
            return [(short(c).decoded(), 0, SHORT * SEG_BITS)]

    want = _splice.reference(oracle, Case())
    got = lg.expected_streams(oracle, [short(c) for c in range(3)])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 2: the two long sizes -----------------------------------------------------------------------------------------------------------
def test_named_rows_and_segments_of_size_a():
    assert divmod(2**31, SEG_BITS) == (67_650, 2048) and divmod(2**32, SEG_BITS) == (135_300, 4096)
    a = lg.operand(lg.A_SEGMENTS, 0)
    assert a.n_bits == 135_400 * SEG_BITS > 2**32 and (135_400 - 1) * SEG_BITS > 2**32 > 135_300 * SEG_BITS
    assert set(lg.A_NAMED) <= set(a.live) and len(a.live) == len(lg.A_NAMED) + 2
    assert all(a.bit(r) for r in (0, 2**31 - 1, 2**31, 2**32 - 1, 2**32, a.n_bits - 1))
    assert lg.edge_rows(lg.A_SEGMENTS) == lg.A_ROWS


def test_named_rows_and_segments_of_size_b():
    n = lg.B_SEGMENTS
    assert n * SEG_WORDS > 2**32 and n * lg.SEG_GROUPS > 2**32 and n * SEG_BITS > 2**36
    assert 4_194_304 * lg.SEG_GROUPS == 2**32 and 4_329_604 * SEG_WORDS <= 2**32 < 4_329_605 * SEG_WORDS
    b = lg.operand(n, 0)
    live = set(b.live)
    assert {0, n - 1, 4_194_303, 4_194_304, 4_329_603, 4_329_604} <= live and set(lg.B_NAMED) <= live
    rows = lg.edge_rows(n)
    assert rows[1] // 31 == 2**32 - 1 and rows[2] // 31 == 2**32 and rows[3] // 32 == 2**32 - 1 and rows[4] // 32 == 2**32
    assert [r // SEG_BITS for r in rows] == [0, 4_194_303, 4_194_304, 4_329_604, 4_329_604, n - 1] and all(b.bit(r) for r in rows)


def _stream_is_model(oracle, b, split=1):
    """The words of the constant segments by their defaults, the live segments by the oracle's decode of their own words."""
    n_segments = b.n_segments
    stream, index = b.stream_index(oracle, split)
    assert index.dtype == np.int64 and index.size == n_segments + 1 and index[0] == 0 and index[-1] == stream.size
    words_in = np.diff(index)
    constant = np.ones(n_segments, bool)
    constant[b.live_segments()] = False
    assert np.all(words_in[constant] == split) and stream.size == split * int(constant.sum()) + int(words_in[~constant].sum())
    fills = np.repeat(np.uint32(lg.FILL | (lg.SEG_GROUPS // split)) | (b.defaults()[constant].astype(np.uint32) * np.uint32(lg.ONE)), split)
    at = np.ones(stream.size, bool)
    for s in b.live:
        at[index[s]: index[s + 1]] = False
    assert np.array_equal(stream[at], fills)
    for s, w in lg.decode_live(oracle, stream, index, sorted(b.live), n_segments).items():
        assert np.array_equal(w, b.live[s]), s


@pytest.mark.parametrize("n_segments,split", ((lg.A_SEGMENTS, 1), (lg.A_SEGMENTS, 128), (lg.B_SEGMENTS, 1)))
def test_streams_of_the_long_operands_decode_to_the_model(oracle, n_segments, split):
    for j in range(10 if n_segments == lg.A_SEGMENTS and split == 1 else 2):
        _stream_is_model(oracle, lg.operand(n_segments, j), split)
        assert len({tuple(sorted(lg.operand(n_segments, i).live)) for i in range(j + 1)}) == j + 1   # differing live segments


def test_streams_of_the_columns_groups_and_splice_sources_decode_to_the_model(oracle):
    a, b, xa, xb = lg.columns_12()
    bitmaps = lg.column_40() + list(lg.groups_at_2_32()) + a + b + [xa, xb] + lg.kth_case()[0] + lg.top_case()[0]
    bitmaps += [src for _, pieces in lg.splice_cases().values() for srcs, _, _ in pieces for src in srcs]
    assert len(bitmaps) > 100
    for bitmap in bitmaps:
        _stream_is_model(oracle, bitmap)


# ---- 3: what the GPU tests' names claim --------------------------------------------------------------------------------------------
def test_counts_and_sums_pass_2_32_where_the_gpu_tests_say_so():
    mask = lg.operand(lg.A_SEGMENTS, 1)
    assert mask.count() > 2**32 and not any(mask.bits == 0)   # ones throughout, holes only in live segments
    g0, g1 = lg.groups_at_2_32()
    assert g0.count() == 2**32 and g1.count() == g0.n_bits - 2**32 and g0.bit(2**32 - 1) == 1 and g0.bit(2**32) == 0 and g1.bit(2**32) == 1
    column = lg.column_40()
    total, have, rows = lg.sum_count(column, mask)
    assert rows == have == mask.count() and total > 2**64 > (2**64 >> 10) and total > lg.COLUMN_40 * 2**32
    assert all(lg.bitop("and", [mask, s]).count() > 2**31 for s, bit in zip(column, f"{lg.COLUMN_40:040b}") if bit == "1")
    per_group = [lg.sum_count(column, lg.bitop("and", [mask, g])) for g in (g0, g1)]
    assert sum(p[0] for p in per_group) == total and sum(p[2] for p in per_group) == rows and 2**31 < per_group[0][2] < 2**32
    assert lg.range_predicate(column, lg.COLUMN_40 - 5, lg.COLUMN_40 + 5).count() > 2**32
    assert 0 < lg.range_predicate(column, lg.COLUMN_40 + 1, (1 << 40) - 1).count() < 2**20   # the sparse result
    a, b, xa, xb = lg.columns_12()
    assert lg.compare(a, b, "==", xa, xb).count() > 2**30 and lg.compare(a, b, "<", xa, xb).count() > 2**31
    assert lg.compare(a, b, "<=", xa, xb).count() > 2**32 and 0 < lg.compare(a, b, ">", xa, xb).count() < 2**20


def test_ranks_around_2_32_have_different_answers():
    slices, mask = lg.kth_case()
    ranks = lg.Ranks(slices, mask)
    assert ranks.total == mask.count() > 2**32 + 1
    low, high = ranks(lg.ASCENDING, 2**32 - 1), ranks(lg.ASCENDING, 2**32)
    assert low[:2] == (1, lg.KTH_LOW) and low[3] + low[4] == 2**32 and high[0] == 1 and high[1] > lg.KTH_LOW and high[3] == 2**32
    assert ranks(lg.ASCENDING, 2**32 + 1)[0] == 1 and ranks(lg.ASCENDING, ranks.total - 1)[:2] == (1, 4095)
    assert ranks(lg.ASCENDING, ranks.total) == (0, 0, ranks.total, 0, 0)
    assert ranks(lg.QUANTILE, 1, 2)[1] == lg.KTH_LOW and ranks(lg.DESCENDING, 0)[1] == 4095 and ranks(lg.ASCENDING, 0)[1] < lg.KTH_LOW
    column, mask = lg.top_case()
    rows = lg.top_rows(column, mask, 5)
    assert rows.size == 5 and rows.min() > 2**32
    values = [lg.value_at(column, None, r) for r in rows.tolist()]
    assert min(values) == values[-1] == lg.Ranks(column, mask)(lg.DESCENDING, 4)[1] > 5 and all(mask.bit(r) for r in rows.tolist())


def test_top_rows_on_a_short_column():
    column, mask = short_column(4, 90), short(92)
    va, chosen = values_of(column), bools(mask)
    for k in (1, 5, 40_000):
        got = lg.top_rows(column, mask, k)
        t = np.sort(va[chosen])[::-1][k - 1]
        better, ties = np.flatnonzero(chosen & (va > t)), np.flatnonzero(chosen & (va == t))
        assert np.array_equal(got, np.concatenate([better, ties[: k - better.size]])), k


def test_long_splices_cross_what_their_names_say_and_map_row_by_row():
    cases = lg.splice_cases()
    lands = cases["a piece lands at 2^32 - 7"][1]
    assert lands[0][2] + lands[1][2] == 2**32 - 7 and lands[1][1] < 2**32 < lands[1][1] + lands[1][2] and lands[2][1] < 2**31 < lands[2][1] + lands[2][2]
    wide = cases["a piece of more than 2^32 rows"][1]
    assert wide[0][2] > 2**32 and not wide[0][0][0].live and wide[1][1] < 2**32 < wide[1][1] + wide[1][2]
    high = cases["source rows above 2^36"][1]
    assert high[1][1] > 2**36 and high[0][2] > 2**36 and any(high[1][1] <= s * SEG_BITS < high[1][1] + high[1][2] for s in high[1][0][0].live)
    rng = np.random.default_rng(3)
    for name, (n_segments, pieces) in cases.items():
        total = sum(n for _, _, n in pieces)
        assert total <= n_segments * SEG_BITS
        for c in range(len(pieces[0][0])):
            out = lg.splice([(srcs[c], first, n) for srcs, first, n in pieces], n_segments)
            start = 0
            for srcs, first, n in pieces:   # the ends of every piece, the images of its source's live segments, random rows
                at = [0, 1, n - 2, n - 1] + rng.integers(0, n, 40).tolist()
                for s in srcs[c].live:
                    at += [r - first for r in (s * SEG_BITS - 1, s * SEG_BITS, s * SEG_BITS + 777, (s + 1) * SEG_BITS - 1, (s + 1) * SEG_BITS)
                           if first <= r < first + n]
                at = np.array(at, dtype=np.int64)
                assert np.array_equal(out.bits_at(start + at), srcs[c].bits_at(first + at)), (name, c, start)
                start += n
            behind = np.arange(total, min(total + 100, out.n_bits))
            assert not out.bits_at(behind).any() and out.count() == sum(
                lg.bitop("and", [srcs[c], lg.bitop("andnot", [lg.below(srcs[c].n_segments, first + n), lg.below(srcs[c].n_segments, first)])]).count()
                for srcs, first, n in pieces), (name, c)


def test_fetch_rows_and_row_lists_lie_where_they_should():
    for n_segments, per_edge in ((lg.A_SEGMENTS, 20), (lg.B_SEGMENTS, 5)):
        rows, n_bits = lg.fetch_rows(n_segments, per_edge), n_segments * SEG_BITS
        assert np.all(np.diff(rows) >= 0) and np.any(np.diff(rows) == 0) and rows[0] == 0 and rows[-1] == rows[-2] == n_bits - 1
        for e in lg.edge_rows(n_segments)[1:5]:
            assert {e - 2, e - 1, e, e + 1} <= set(rows.tolist())
        assert (250 <= rows.size <= 350) if n_segments == lg.A_SEGMENTS else (80 <= rows.size <= 130)
        for rows in lg.row_lists(n_segments, 4)[:3]:
            assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n_bits and rows[-1] >= n_bits - SEG_BITS
        assert lg.row_lists(n_segments, 4)[3].size == 0
