"""GPU tests of wah_fetch_indexed_device: the values of listed rows, fetched from the index without decoding it (include/wah.h),
and its front ends in api.py and columns.py.  Every case compares all outputs with tests/_fetch.py's ref_fetch -- a walk over the
same streams on the CPU, proven by tests/test_fetch_reference.py -- or with the values / keys the index was built from;
everything is exact.  The streams are the CPU oracle's, their indices tests/_select.py's index_of.

The shapes are the smallest at which the kernels can go wrong: the bits on both sides of a group, a word and a segment edge, lists
around the 64 rows of an item, tables around the 64 rows of a chunk and the 64 bits of a value, segments around the 128 words of
a batch, and one list of one item more than the items pass has wavefronts."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _fetch, _oracle, _select, _switch as sw

pytestmark = pytest.mark.gpu

WAH_OK, WAH_ERR_STREAM = 0, -6
SEG = _fetch.SEG_WORDS
SEG_BITS = _fetch.SEG_BITS
BITS, FIRST = _fetch.BITS, _fetch.FIRST


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


def _rows_dev(rows):
    import torch

    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).cuda()


def _operand(stream):
    """(stream, index) on the device of one whole compressed bitmap."""
    import torch

    return _dev(stream), torch.from_numpy(_select.index_of(stream)).cuda()


class Table:
    """Streams of the oracle for a list of decoded bitmaps of n words, uploaded once; a table row may name any of them."""

    def __init__(self, wah, bitmaps, n):
        oracle = _oracle.load()
        self.wah, self.n = wah, n
        self.streams = [oracle.compress(np.ascontiguousarray(b, dtype=np.uint32)) for b in bitmaps]
        self.dev = [_operand(st) for st in self.streams]

    def check(self, rows, mode, what, order=None):
        order = list(range(len(self.streams))) if order is None else order
        rows = np.asarray(rows, dtype=np.int64)
        got = self.wah.fetch_device([self.dev[j] for j in order], _rows_dev(rows), self.n, mode)
        want = _fetch.ref_fetch([self.streams[j] for j in order], rows, mode)
        assert _fetch.as_u64(got) == want, what
        return want


def _random_bitmaps(seed, k, n, p=0.5):
    oracle = _oracle.load()
    return [oracle.gen_uniform(n, seed + j, p) for j in range(k)]


# ---- 1: bit addressing ----------------------------------------------------------------------------------------------------------
def test_bits_on_both_sides_of_group_word_and_segment_edges(wah):
    one = Table(wah, _random_bitmaps(1, 5, SEG), SEG)
    two = Table(wah, _random_bitmaps(2, 5, 2 * SEG), 2 * SEG)
    for mode in (BITS, FIRST):
        want = one.check([0, 30, 31, 32, 61, 62, 31743], mode, "one segment")
        assert len(set(want)) > 2  # (not all the same answer)
        two.check([31743, 31744], mode, "the last group of segment 0, the first of segment 1")
        two.check([0, 30, 31, 32, 61, 62, 31743, 31744, 31745, 2 * SEG_BITS - 1], mode, "two segments")


@pytest.mark.parametrize("n", [1, 31, 993, 992 + 31])
def test_last_position_of_a_ragged_bitmap(wah, n):
    last = 32 * n - 1
    bitmaps = _random_bitmaps(n, 3, n) + [_select.bitmap_of([last], n), np.full(n, 0xFFFFFFFF, np.uint32)]
    t = Table(wah, bitmaps, n)
    for mode in (BITS, FIRST):
        t.check([last], mode, "the last position alone")
        t.check(sorted({0, 30 % (32 * n), 31, last - 1, last}), mode, "with its neighbours")
    assert t.check([last], BITS, "bits")[0] & 3 == 3  # the two bitmaps that certainly have it


# ---- 2: item edges --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_segments(wah):
    return Table(wah, _random_bitmaps(20, 3, 3 * SEG), 3 * SEG)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 128, 129])
def test_rows_of_one_segment(wah, three_segments, count):
    rng = np.random.default_rng(count)
    for segment in (0, 2):
        rows = np.sort(rng.integers(segment * SEG_BITS, (segment + 1) * SEG_BITS, count))
        assert len(_fetch.items_of(rows, 3 * SEG)) == -(-count // 64)
        for mode in (BITS, FIRST):
            three_segments.check(rows, mode, (count, segment))


@pytest.mark.parametrize("at", [63, 64, 65])
def test_segment_change_at_a_list_index(wah, three_segments, at):
    rng = np.random.default_rng(at)
    rows = np.concatenate([np.sort(rng.integers(0, SEG_BITS, at)), np.sort(rng.integers(SEG_BITS, 2 * SEG_BITS, 70))])
    assert [h for h, _ in _fetch.items_of(rows, 3 * SEG)] == sorted({0, 64, at, 128})
    for mode in (BITS, FIRST):
        three_segments.check(rows, mode, at)


def test_duplicates_one_row_and_every_row_of_a_segment(wah, three_segments):
    rng = np.random.default_rng(9)
    rows = np.sort(rng.integers(SEG_BITS - 500, SEG_BITS + 500, 100))
    rows[64] = rows[63]  # a duplicate on both sides of an item's edge
    rows[10:14] = rows[10]
    assert np.all(rows[1:] >= rows[:-1])
    for mode in (BITS, FIRST):
        three_segments.check(rows, mode, "duplicates")
        three_segments.check([SEG_BITS + 12345], mode, "one row")
    want = three_segments.check(np.arange(SEG_BITS, 2 * SEG_BITS), BITS, "every row of segment 1")
    words = np.stack(_random_bitmaps(20, 3, 3 * SEG))
    bits = np.stack([_bsi.unpack_bits(w)[SEG_BITS: 2 * SEG_BITS] for w in words]).astype(np.int64)
    assert want == (4 * bits[0] + 2 * bits[1] + bits[2]).tolist()  # ... and the reference against plain indexing once more


def test_a_segment_change_at_every_row(wah):
    n = 200 * SEG
    t = Table(wah, _random_bitmaps(40, 2, n), n)
    rng = np.random.default_rng(40)
    rows = np.arange(200) * SEG_BITS + rng.integers(0, SEG_BITS, 200)
    assert len(_fetch.items_of(rows, n)) == 200
    for mode in (BITS, FIRST):
        t.check(rows, mode, "200 rows in 200 segments")


def test_no_row_at_all(wah):
    import torch

    t = Table(wah, _random_bitmaps(3, 2, SEG), SEG)
    got = wah.fetch_device(t.dev, torch.empty(0, dtype=torch.int64, device="cuda"), SEG, BITS)
    assert got.numel() == 0
    sc = torch.empty(int(wah.lib().wah_fetch_scratch_bytes(SEG, 0)), dtype=torch.uint8, device="cuda")
    table = wah.bitop_operand_table(t.dev)
    assert wah.lib().wah_fetch_indexed_device(FIRST, SEG, 2, table.data_ptr(), None, 0, None, sc.data_ptr(), sc.numel(), None) == WAH_OK
    assert wah.lib().wah_fetch_status(sc.data_ptr(), None) == WAH_OK


# ---- 3: what a table row holds in a touched segment -------------------------------------------------------------------------------
def _layout_rows(layout, segment, rng):
    """Listed rows of one segment for a layout of runs: the bit on both sides of every run edge, one in the middle of every run,
    and a few anywhere."""
    edges = np.cumsum([n for _, n in layout])
    rows = set(rng.integers(0, SEG_BITS, 12).tolist()) | {0, SEG_BITS - 1}
    start = 0
    for e in edges.tolist():
        rows |= {31 * start, 31 * e - 1, 31 * ((start + e) // 2) + 7}
        if e < sw.SEG_GROUPS:
            rows.add(31 * e)
        start = e
    return segment * SEG_BITS + np.array(sorted(rows), dtype=np.int64)


def test_operand_shapes_per_touched_segment(wah):
    """One zero fill (settled in the gather), one one-fill, 1024 literals, every LIST_SEGMENT_WORDS edge by every way
    (tests/_switch.py), a row inside a long fill, rows in the literal just before and just behind a fill: one layout per segment, a
    second bitmap with the layouts in another order, and both orders of the two as table rows."""
    rng = np.random.default_rng(77)
    layouts = [[("zeros", 1024)], [("ones", 1024)], [("lit", 1024)], [("lit", 1), ("zeros", 1022), ("lit", 1)], [("lit", 3), ("ones", 1000), ("lit", 21)],
               [("zeros", 500), ("lit", 1), ("ones", 523)]]
    layouts += [layout for _, _, _, layout in sw.list_words_probes()]
    layouts += sw.list_many_fills_layouts()[:4]
    s = len(layouts)
    n = s * SEG
    turned = layouts[s // 2:] + layouts[: s // 2]
    t = Table(wah, [sw.list_probe_bitmap(layouts, rng), sw.list_probe_bitmap(turned, rng), np.zeros(n, np.uint32)], n)
    rows = np.concatenate([np.union1d(_layout_rows(a, k, rng), _layout_rows(b, k, rng)) for k, (a, b) in enumerate(zip(layouts, turned))])
    assert np.all(rows[1:] > rows[:-1])
    for order in ([0, 1], [1, 0], [2, 0, 2, 1, 2]):
        want = t.check(rows, BITS, ("bits", order), order)
        assert len(set(want)) == 4 or 2 in order
        t.check(rows, FIRST, ("first", order), order)


# ---- 4: WAH_FETCH_BITS ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", [1, 4, 63, 64])
def test_bits_are_the_values_of_the_rows(wah, n_bits):
    n = SEG + 40
    rng = np.random.default_rng(n_bits)
    kinds = ("uniform", "low", "high", "clustered") if n_bits in (4, 63) else ("uniform",)
    for kind in kinds:
        values = _bsi.make_values(kind, rng, 32 * n, n_bits)
        values[5] = (1 << n_bits) - 1  # the top slice is set: bit n_bits - 1 is reached
        t = Table(wah, _bsi.build_slices(values, n_bits), n)
        rows = np.sort(np.concatenate([[5, 5], rng.integers(0, 32 * n, 300)]))
        got = wah.fetch_device(t.dev, _rows_dev(rows), n, BITS)
        assert _fetch.as_u64(got) == [int(v) for v in values[rows]], (n_bits, kind)
        assert max(_fetch.as_u64(got)) >> (n_bits - 1) == 1


@pytest.mark.parametrize("n_bits", [12, 63])
def test_values_at_rows_with_an_existence_bitmap(wah, n_bits):
    """Through columns.values_at_rows: the existence bitmap is the table's first row (with 63 slices: 64 rows, the top bit of the
    output), the slices are windows into the column matrix bsi_from_values compressed, and the rows come unsorted."""
    import torch

    n = 2 * SEG
    rng = np.random.default_rng(n_bits)
    count = 32 * n - 1000
    values = _bsi.uniform_values(rng, count, n_bits)
    exists = rng.random(count) < 0.7
    bsi = wah.columns.bsi_from_values(wah, torch.from_numpy(values.view(np.int64)).cuda(), n_bits, exists=torch.from_numpy(exists).cuda())
    assert bsi[2] == n and bsi[4]
    rows = rng.permutation(count)[:700]
    rows[:3] = rows[3]  # duplicates, unsorted
    got, have = wah.columns.values_at_rows(wah, bsi, _rows_dev(rows))
    assert np.array_equal(have.cpu().numpy(), exists[rows])
    assert np.array_equal(got.cpu().numpy().view(np.uint64), np.where(exists[rows], values[rows], np.uint64(0)))
    plain = wah.columns.bsi_from_values(wah, torch.from_numpy(values.view(np.int64)).cuda(), n_bits)
    got, have = wah.columns.values_at_rows(wah, plain, _rows_dev(rows))
    assert have is None and np.array_equal(got.cpu().numpy().view(np.uint64), values[rows])


# ---- 5: WAH_FETCH_FIRST -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_values", [1, 63, 64, 65, 129])
def test_first_is_the_key_of_the_row(wah, n_values):
    n = SEG
    rng = np.random.default_rng(n_values)
    keys = rng.integers(-1, n_values, 32 * n)  # -1: a row no column has
    t = Table(wah, _fetch.one_hot(keys, n_values, n), n)
    rows = np.sort(rng.integers(0, 32 * n, 400))
    got = wah.fetch_device(t.dev, _rows_dev(rows), n, FIRST)
    assert got.cpu().numpy().tolist() == keys[rows].tolist()  # none set: UINT64_MAX, which reads as -1
    assert (-1 in keys[rows]) or n_values == 1


def test_the_one_set_column_at_every_list_position(wah):
    n = 2 * SEG
    t = Table(wah, [np.zeros(n, np.uint32)] + _random_bitmaps(60, 2, n, 0.3), n)
    rng = np.random.default_rng(60)
    rows = np.sort(rng.integers(0, 32 * n, 150))
    for pos in sw.LIST_POSITIONS:
        k = max(pos + 1, sw.LIST_CHUNK + 1)
        order = [0] * k
        order[pos] = 1
        want = t.check(rows, FIRST, ("alone", pos), order)
        assert set(want) == {pos, _fetch.U64_MAX}
        if pos + 2 < k:
            order[pos + 2] = 1  # the same bitmap again behind it: the lower row wins
            order[k - 1] = 2
            assert set(t.check(rows, FIRST, ("two", pos), order)) == {pos, k - 1, _fetch.U64_MAX}
    assert set(t.check(rows, FIRST, "none set", [0] * 130)) == {_fetch.U64_MAX}


def test_keys_round_trip(wah):
    """values -> index -> values: keys_at_rows(index_from_keys(keys)) == keys, and -1 behind the key column's own rows."""
    import torch

    rng = np.random.default_rng(300)
    keys = torch.from_numpy(rng.integers(0, 300, 5000)).cuda()
    index = wah.columns.index_from_keys(wah, keys, 300)
    assert torch.equal(wah.columns.keys_at_rows(wah, index, torch.arange(5000, device="cuda")), keys)
    behind = torch.tensor([31743, 5000, 4999, 0], device="cuda")
    assert wah.columns.keys_at_rows(wah, index, behind).tolist() == [-1, -1, int(keys[4999]), int(keys[0])]


# ---- 6: more items than the items pass has wavefronts -----------------------------------------------------------------------------
def test_the_stride_loop_takes_a_second_turn(wah):
    """grid + 1 listed rows, one per segment, over bitmaps built from row lists (a few words per segment: nothing of the bitmaps'
    size exists): some wavefront handles two items."""
    import torch

    items = _fetch.grid_waves() + 1
    n = items * SEG
    s = np.arange(items, dtype=np.int64)
    rows = s * SEG_BITS + (s * 7919) % SEG_BITS
    in_a, in_b = s % 2 == 0, s % 3 == 0
    stream, offsets = wah.columns.bitmaps_from_rows(wah, [_rows_dev(rows[in_a]), _rows_dev(rows[in_b])], n)
    assert stream.numel() < 8 * items
    table = wah.columns.column_operand_table(stream, offsets, n, [0, 1])
    d_rows = _rows_dev(rows)
    assert len(_fetch.items_of(rows, n)) == items
    got = wah.fetch_device(table, d_rows, n, BITS)
    assert np.array_equal(got.cpu().numpy(), 2 * in_a + in_b)
    got = wah.fetch_device(table, d_rows, n, FIRST)
    assert np.array_equal(got.cpu().numpy(), np.where(in_a, 0, np.where(in_b, 1, -1)))
    neighbours = torch.clamp(d_rows + 1, max=32 * n - 1)
    assert not wah.fetch_device(table, neighbours, n, BITS).any()


# ---- 7: what only the device can refuse ---------------------------------------------------------------------------------------------
def _status(wah, table, rows, n, mode=BITS):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    d_rows = _rows_dev(rows)
    sc = torch.empty(int(wah.lib().wah_fetch_scratch_bytes(n, d_rows.numel())), dtype=torch.uint8, device="cuda")
    out = wah.fetch_device(table, d_rows, n, mode, scratch=sc, check=False)
    return int(wah.lib().wah_fetch_status(sc.data_ptr(), None)), out


def test_refused_rows(wah, three_segments):
    n = 3 * SEG
    table = wah.bitop_operand_table(three_segments.dev)
    rng = np.random.default_rng(5)
    good = np.sort(rng.integers(0, 32 * n, 130))
    assert _status(wah, table, good, n)[0] == WAH_OK
    assert _status(wah, table, [32 * n - 1], n)[0] == WAH_OK
    for what, bad in (("a row at 32 n", [32 * n]), ("behind good rows", list(good) + [32 * n]), ("far beyond", [5, 1 << 62]), ("negative", [-1])):
        assert _status(wah, table, bad, n)[0] == WAH_ERR_STREAM, what
    for at in (0, 63, len(good) - 2):
        rows = good.copy()
        rows[at], rows[at + 1] = good[at + 1] + 1, good[at]  # a descending pair at indices at | at + 1
        assert rows[at] > rows[at + 1]
        assert _status(wah, table, rows, n)[0] == WAH_ERR_STREAM, at
    with pytest.raises(wah.WahError):
        wah.fetch_device(table, _rows_dev([7, 3]), n, BITS)
    # many more heads than the item list has room for: refused, nothing is put outside it
    zigzag = np.tile([0, 2 * SEG_BITS], 400)
    assert _status(wah, table, zigzag, n)[0] == WAH_ERR_STREAM


def test_a_refused_stream_only_where_it_is_touched(wah, three_segments):
    """The documented contract: a malformed segment is refused when a listed row lies in it, and never seen otherwise."""
    import torch

    n = 3 * SEG
    rng = np.random.default_rng(6)
    oracle = _oracle.load()
    bitmap = _random_bitmaps(20, 3, n)[1]
    valid = [oracle.compress(bitmap[lo: lo + SEG]) for lo in range(0, n, SEG)]
    name, words = sw.list_refusals(rng)[1]
    assert name.startswith("1025 groups")
    stream, index = sw.list_refused_stream(valid, 1, words)
    bad = (_dev(stream), torch.from_numpy(index).cuda())
    for place in (0, 1, 2):
        ops = list(three_segments.dev)
        ops[place] = bad
        table = wah.bitop_operand_table(ops)
        for mode in (BITS, FIRST):
            assert _status(wah, table, [5, SEG_BITS + 9, 2 * SEG_BITS + 1], n, mode)[0] == WAH_ERR_STREAM, place
            assert _status(wah, table, [SEG_BITS], n, mode)[0] == WAH_ERR_STREAM, place
            rows = np.sort(np.concatenate([rng.integers(0, SEG_BITS, 70), rng.integers(2 * SEG_BITS, 3 * SEG_BITS, 70)]))
            status, out = _status(wah, table, rows, n, mode)
            assert status == WAH_OK, place
            streams = list(three_segments.streams)
            streams[place] = three_segments.streams[1]  # (segments 0 and 2 of the bad operand are bitmap 1's)
            assert _fetch.as_u64(out) == _fetch.ref_fetch(streams, rows, mode)
    empty = wah.bitop_operand_table(three_segments.dev)
    empty[1, 2] = 0  # a row without an index
    assert _status(wah, empty, [5], n)[0] == WAH_ERR_STREAM


# ---- 8: replay and the column front ends ------------------------------------------------------------------------------------------
def test_rows_overwritten_in_place(wah, three_segments):
    """Rows are read by the device only: the same call again, same scratch and out, after d_rows was overwritten in place."""
    import torch

    n = 3 * SEG
    rng = np.random.default_rng(8)
    table = wah.bitop_operand_table(three_segments.dev)
    d_rows = torch.zeros(200, dtype=torch.int64, device="cuda")
    sc = torch.empty(int(wah.lib().wah_fetch_scratch_bytes(n, 200)), dtype=torch.uint8, device="cuda")
    out = torch.empty(200, dtype=torch.int64, device="cuda")
    seen = set()
    for lo, hi in ((0, 32 * n), (0, 100), (SEG_BITS - 50, SEG_BITS + 50), (2 * SEG_BITS, 3 * SEG_BITS)):
        rows = np.sort(rng.integers(lo, hi, 200))
        d_rows.copy_(torch.from_numpy(rows))
        got = wah.fetch_device(table, d_rows, n, BITS, scratch=sc, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert _fetch.as_u64(got) == _fetch.ref_fetch(three_segments.streams, rows, BITS), (lo, hi)
        seen.add(tuple(got.tolist()))
    assert len(seen) == 4


@pytest.fixture(scope="module")
def small_table(wah):
    """32 * 992 * 2 rows: a 20-bit price with an existence bitmap, a 6-bit rating without, a city of 8 keys."""
    import torch

    n = 2 * SEG
    rng = np.random.default_rng(12)
    count = 32 * n
    price, rating = _bsi.uniform_values(rng, count, 20), _bsi.uniform_values(rng, count, 6)
    exists = rng.random(count) < 0.9
    city = rng.integers(0, 8, count)
    c = wah.columns
    return dict(n=n, price=price, rating=rating, exists=exists, city=city,
                bsi_price=c.bsi_from_values(wah, torch.from_numpy(price.view(np.int64)).cuda(), 20, exists=torch.from_numpy(exists).cuda()),
                bsi_rating=c.bsi_from_values(wah, torch.from_numpy(rating.view(np.int64)).cuda(), 6),
                index_city=c.index_from_keys(wah, torch.from_numpy(city).cuda(), 8))


def test_select_values_against_the_numpy_model(wah, small_table):
    """SELECT price, rating, city WHERE city IN (1, 3) AND rating == 5 LIMIT 100 OFFSET 7."""
    t = small_table
    n = t["n"]
    five = wah.columns.compare_column(wah, t["bsi_rating"], "==", 5)
    predicates = [(t["index_city"][0], t["index_city"][1], [1, 3], False), (five[0], five[1], [0], False)]
    rows, (price, rating, city), matching = wah.columns.select_values(wah, predicates, n, [t["bsi_price"], t["bsi_rating"], t["index_city"]], first=7, limit=100)
    match = np.flatnonzero(np.isin(t["city"], [1, 3]) & (t["rating"] == 5))
    want = match[7:107]
    assert matching == match.size and want.size == 100 and np.array_equal(rows.cpu().numpy(), want)
    assert np.array_equal(price[0].cpu().numpy().view(np.uint64), np.where(t["exists"][want], t["price"][want], np.uint64(0)))
    assert np.array_equal(price[1].cpu().numpy(), t["exists"][want])
    assert rating[1] is None and np.array_equal(rating[0].cpu().numpy().view(np.uint64), t["rating"][want])
    assert np.array_equal(city.cpu().numpy(), t["city"][want])


@pytest.mark.parametrize("largest", [True, False])
def test_values_of_top_rows(wah, small_table, largest):
    """top_rows gives the rows of ORDER BY price LIMIT k -- the strictly better ones, then the ties: not in row order --, and
    values_at_rows takes them as they are."""
    t = small_table
    rows = wah.columns.top_rows(wah, t["bsi_price"], 150, largest=largest)
    values, have = wah.columns.values_at_rows(wah, t["bsi_price"], rows)
    at = rows.cpu().numpy()
    assert have.all() and np.array_equal(values.cpu().numpy().view(np.uint64), t["price"][at])
    ranked = np.sort(t["price"][t["exists"]])
    want = ranked[::-1][:150] if largest else ranked[:150]
    assert np.array_equal(np.sort(values.cpu().numpy().view(np.uint64)), np.sort(want))
