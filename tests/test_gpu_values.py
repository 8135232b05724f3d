"""GPU tests of wah_values_indexed_device: the values of a row range, a whole attribute read back out of the index (include/wah.h),
and its front ends in api.py and columns.py.  Every case compares all outputs with tests/_values.py -- the fetch call's reference
over arange, a walk over the same streams on the CPU, proven by tests/test_values_reference.py -- or with the values / keys the
index was built from; everything is exact.  Every output lies in a buffer pre-filled with a poison pattern, 64 guard elements
on either side of it: a byte nobody wrote shows in the comparison, a byte written outside d_out[0 .. n_rows) in the guards.

The shapes are the smallest at which the kernel can go wrong: a last segment of 2 and of some hundred groups, one and two items a
segment (32 / 33 table rows), tables across the 64 rows of a gather chunk, windows that begin and end on and beside group, word
and segment edges, one item more than the launch has workgroups, and windows behind row 2^32."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _fetch, _foreign as fg, _long as lg, _oracle, _select, _values as vl
from tests import _switch as sw

pytestmark = pytest.mark.gpu

WAH_OK, WAH_ERR_STREAM = 0, -6
SEG, SEG_BITS = vl.SEG_WORDS, vl.SEG_BITS
BITS, FIRST = vl.BITS, vl.FIRST
GUARD = 64
POISON64 = int.from_bytes(bytes([vl.POISON]) * 8, "little", signed=True)


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


def _dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).cuda()


def _operand(stream):
    """(stream, index) on the device of one whole compressed bitmap."""
    import torch

    return _dev(stream), torch.from_numpy(_select.index_of(stream)).cuda()


def _guarded(n):
    """(buffer, out): n poisoned elements with 64 poisoned guard elements on either side."""
    import torch

    buf = torch.full((n + 2 * GUARD,), POISON64, dtype=torch.int64, device="cuda")
    return buf, buf[GUARD: GUARD + n]


def _guards_kept(buf, n):
    return bool((buf[:GUARD] == POISON64).all()) and bool((buf[GUARD + n:] == POISON64).all())


def _run(wah, table, n_words, mode, first, n, **kw):
    """One call into a poisoned, guarded output: the window's values as uint64."""
    buf, out = _guarded(n)
    got = wah.values_device(table, n_words, mode, first, n, out=out, **kw)
    assert got.data_ptr() == out.data_ptr() and got.numel() == n
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == POISON64) and np.all(host[GUARD + n:] == POISON64), ("a guard element was written", first, n)
    return host[GUARD: GUARD + n].view(np.uint64)


class Table:
    """Streams of the oracle for a list of decoded bitmaps of n words, uploaded once; a table row may name any of them.  The
    reference is computed once: every stream's bit of every row, read from the STREAM by group and bit (tests/_fetch.py's bits_at);
    a window of a table is tests/_values.py's fold of their slices."""

    def __init__(self, wah, bitmaps, n):
        oracle = _oracle.load()
        self.wah, self.n = wah, n
        self.streams = [oracle.compress(np.ascontiguousarray(b, dtype=np.uint32)) for b in bitmaps]
        self.dev = [_operand(st) for st in self.streams]
        rows = np.arange(32 * n, dtype=np.int64)
        self.bits = [_fetch.bits_at(st, rows) for st in self.streams]

    def want(self, order, first, n, mode):
        return vl.fold([self.bits[j][first: first + n] for j in order], mode)

    def table(self, order):
        return self.wah.bitop_operand_table([self.dev[j] for j in order])

    def check(self, order, first, n, mode, what=None, table=None):
        got = _run(self.wah, self.table(order) if table is None else table, self.n, mode, first, n)
        want = self.want(order, first, n, mode)
        assert np.array_equal(got, want), (what, first, n, mode, np.flatnonzero(got != want)[:5])
        return want


def _pool(n, size, seed=0):
    """Bitmaps of n words: random at several densities, all zero, all one, clustered."""
    oracle = _oracle.load()
    maps = []
    for j in range(size):
        kind = j % 7
        if kind == 5:
            maps.append(np.zeros(n, np.uint32) if j % 2 else np.full(n, 0xFFFFFFFF, np.uint32))
        elif kind == 6:
            maps.append(oracle.gen_clustered(n, seed + j, 3000))
        else:
            maps.append(oracle.gen_uniform(n, seed + j, (0.5, 0.03, 0.9, 0.5, 0.3)[kind]))
    return maps


@pytest.fixture(scope="module")
def pools(wah):
    """One table of 65 bitmaps per size, made when first asked for."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = Table(wah, _pool(n, 65, seed=n), n)
        return made[n]

    return get


# ---- 1: sizes and widths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", vl.SIZES)
def test_every_width_of_every_size(wah, pools, n):
    """The whole bitmap; widths on both sides of the 32 rows of a half, each with and without an existence row in front (to the
    call it is one more table row: 64 slices leave no room for one)."""
    t = pools(n)
    for width in vl.BITS_WIDTHS:
        for front in ([], [64]):
            order = front + list(range(1, 1 + width))
            if len(order) > 64:
                continue
            want = t.check(order, 0, 32 * n, BITS, ("width", width, bool(front)))
            if width > 2 and n > 1:
                assert int(want.max()) >> (len(order) - 1) == 1  # the top bit is reached
    t.check(list(range(65)), 0, 32 * n, FIRST, "first")


@pytest.mark.parametrize("n", vl.SIZES)
def test_windows_on_and_beside_every_edge(wah, pools, n):
    t = pools(n)
    wins = vl.windows(n)
    assert (0, 32 * n) in wins and (32 * n - 1, 1) in wins and (0, 0) in wins
    narrow, wide, cols = t.table([3, 0, 4, 1, 2]), t.table(list(range(33))), t.table([5, 1, 8, 3, 7])
    seen = set()
    for first, count in wins:
        t.check([3, 0, 4, 1, 2], first, count, BITS, "one item a segment", narrow)
        want = t.check(list(range(33)), first, count, BITS, "two items a segment", wide)
        t.check([5, 1, 8, 3, 7], first, count, FIRST, "first", cols)
        seen.add(want.tobytes())
    assert len(seen) > len(wins) // 3  # (the windows see different data)


def test_no_row_at_all(wah, pools):
    import torch

    t = pools(SEG)
    table = t.table([0, 1])
    assert wah.values_device(table, SEG, BITS, 5, 0).numel() == 0
    sc = torch.full((int(wah.lib().wah_values_scratch_bytes(SEG, 2)),), 0xA5, dtype=torch.uint8, device="cuda")  # (no initialisation)
    for first in (0, 31, 32 * SEG):
        assert wah.lib().wah_values_indexed_device(FIRST, SEG, 2, table.data_ptr(), first, 0, None, sc.data_ptr(), sc.numel(), None) == WAH_OK
        assert wah.lib().wah_values_status(sc.data_ptr(), None) == WAH_OK


# ---- 2: WAH_FETCH_FIRST ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_values", vl.FIRST_COLUMNS)
def test_first_is_the_key_of_the_row(wah, n_values):
    """Columns across the gather's chunk of 64; rows no column sets, rows two columns set, a column that is one one-fill over a whole
    segment, columns that are all zero."""
    n = 2 * SEG
    rng = np.random.default_rng(n_values)
    keys = rng.integers(-1, n_values, 32 * n)  # -1: a row no column has
    empty = sorted({n_values // 2, n_values - 1}) if n_values > 2 else []
    keys[np.isin(keys, empty)] = -1  # columns that are all zero
    maps = _fetch.one_hot(keys, n_values, n)
    filled = 0 if n_values < 3 else n_values // 3
    maps[filled][SEG:] = 0xFFFFFFFF  # one one-fill over segment 1: there, rows of two columns wherever a lower or a higher one has the row
    maps[0][:40] |= maps[n_values - 2][:40] if n_values > 2 else 0
    t = Table(wah, maps, n)
    assert [int(t.streams[c].size) for c in empty] == [2] * len(empty) and t.streams[filled][-1] == 0xC0000400
    order = list(range(n_values))
    want = t.check(order, 0, 32 * n, FIRST, "whole")
    assert np.array_equal(want[:SEG_BITS].astype(np.int64)[40 * 32:], keys[40 * 32: SEG_BITS])
    if n_values > 2:
        assert vl.U64_MAX in want[:SEG_BITS] and vl.U64_MAX not in want[SEG_BITS:] and len(set(want[SEG_BITS:].tolist())) == min(filled + 1, n_values - len(empty))
    for first, count in ((SEG_BITS - 70, 140), (SEG_BITS, SEG_BITS), (7, 1)):
        t.check(order, first, count, FIRST, "window")


def test_the_one_set_column_at_every_table_position(wah, pools):
    t = pools(2 * SEG)
    zero = next(j for j, b in enumerate(t.bits) if not b.any())
    for pos in sw.LIST_POSITIONS:
        k = max(pos + 1, sw.LIST_CHUNK + 1)
        order = [zero] * k
        order[pos] = 3
        want = t.check(order, SEG_BITS - 500, 1000, FIRST, ("alone", pos))
        assert set(want.tolist()) == {pos, vl.U64_MAX}
        if pos + 2 < k:
            order[pos + 2], order[k - 1] = 3, 4  # the same bitmap again behind it: the lower row wins
            assert set(t.check(order, SEG_BITS - 500, 1000, FIRST, ("two", pos)).tolist()) == {pos, k - 1, vl.U64_MAX}
    assert set(t.check([zero] * 130, 0, 64 * SEG, FIRST, "none set").tolist()) == {vl.U64_MAX}


# ---- 3: operands ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (SEG, 2 * SEG, SEG + 1, 2 * SEG + 30))
def test_foreign_operands_of_every_way(wah, oracle, n):
    """Every re-encoding of tests/_foreign.py: fills of one group, split fills, fillable literals, a one-word segment as two fills, set
    pad bits.  Six bitmaps in ONE way per table, and one table of all ways mixed; the expectation is plain indexing of the bitmaps
    the ORACLE decodes from the foreign streams."""
    from tests.test_gpu_foreign_operands import Operands

    ops = Operands(wah, oracle)
    tables = [[ops.get(n, way, j) for j in range(6)] for way in fg.ways_for(n)]
    tables.append([ops.get(n, way, 1) for way in fg.ways_for(n)])
    wins = [(0, 32 * n), (32 * n - 1, 1), (29, 35)] + ([(SEG_BITS - 3, 6), (SEG_BITS + 1, 32 * n - SEG_BITS - 1)] if 32 * n > SEG_BITS + 8 else [])
    for table in tables:
        bits = [_bsi.unpack_bits(o.data)[: 32 * n] for o in table]
        d_table = wah.bitop_operand_table([(o.d, o.offs) for o in table])
        for first, count in wins:
            for mode in (BITS, FIRST):
                got = _run(wah, d_table, n, mode, first, count)
                assert np.array_equal(got, vl.fold([b[first: first + count] for b in bits], mode)), (n, table[0].way, first, count, mode)


def test_windows_into_a_column_matrix_and_unchecked_outputs(wah):
    """Table rows that are windows into a column matrix, in any order and repeated; the output buffer of a range_column call and of
    an add_columns call that were only enqueued: a length that is a capacity, a stream nobody has checked yet."""
    import torch

    n = 2 * SEG
    rng = np.random.default_rng(21)
    count = 32 * n - 77
    va, vb = _bsi.uniform_values(rng, count, 12), _bsi.uniform_values(rng, count, 9)
    a = wah.columns.bsi_from_values(wah, _dev64(va), 12)
    b = wah.columns.bsi_from_values(wah, _dev64(vb), 9)
    ids = [3, 0, 0, 11, 5]
    table = wah.columns.column_operand_table(a[0], a[1], n, ids)
    bits = [(va >> np.uint64(11 - i)) & np.uint64(1) for i in ids]
    for first, rows in ((0, count), (SEG_BITS - 9, 40), (count - 1, 1)):
        for mode in (BITS, FIRST):
            assert np.array_equal(_run(wah, table, n, mode, first, rows), vl.fold([x[first: first + rows] for x in bits], mode)), (first, rows, mode)
    lo, hi = 1000, 3000
    out, _, out_offsets = wah.columns.range_column(wah, a, lo, hi, check=False)
    assert out.numel() >= wah.max_compressed_words(n)
    got = _run(wah, [(out, out_offsets)], n, FIRST, 0, count)
    assert np.array_equal(got.view(np.int64), np.where((va >= lo) & (va <= hi), 0, -1))
    total = wah.columns.add_columns(wah, a, b, check=False)
    values, have = wah.columns.values_of_column(wah, total, 0, count)
    assert have is None and np.array_equal(values.cpu().numpy().view(np.uint64), va + vb)
    assert torch.is_tensor(values) and values.dtype == torch.int64


# ---- 4: what only the device can refuse -------------------------------------------------------------------------------------------------
def _status(wah, table, n, mode, first, count):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    sc = torch.empty(int(wah.lib().wah_values_scratch_bytes(n, table.shape[0])), dtype=torch.uint8, device="cuda")
    buf, out = _guarded(count)
    wah.values_device(table, n, mode, first, count, scratch=sc, out=out, check=False)
    status = int(wah.lib().wah_values_status(sc.data_ptr(), None))
    assert _guards_kept(buf, count)
    return status, out.cpu().numpy().view(np.uint64)


def test_a_refused_stream_only_where_the_window_touches_it(wah, pools):
    """A malformed segment inside the window is reported; the same one outside the window is never seen, and the values are right."""
    import torch

    n = 3 * SEG - 5
    t = pools(n)
    rng = np.random.default_rng(6)
    oracle = _oracle.load()
    bitmap = _pool(n, 65, seed=n)[1]
    valid = [oracle.compress(bitmap[lo: lo + SEG]) for lo in range(0, n, SEG)]
    name, words = sw.list_refusals(rng)[1]
    assert name.startswith("1025 groups")
    stream, index = sw.list_refused_stream(valid, 1, words)
    bad = (_dev(stream), torch.from_numpy(index).cuda())
    for k, place in ((3, 0), (3, 2), (40, 0), (40, 20), (40, 39), (65, 64)):
        ops = [t.dev[j] for j in range(k)]
        ops[place] = bad
        table = wah.bitop_operand_table(ops)
        order = list(range(k))
        order[place] = 1  # (segments 0 and 2 of the bad operand are bitmap 1's)
        for mode in ((BITS, FIRST) if k <= 64 else (FIRST,)):
            for first, count in ((0, 32 * n), (SEG_BITS, 1), (2 * SEG_BITS - 1, 1), (SEG_BITS - 1, 2), (5, 2 * SEG_BITS)):
                assert _status(wah, table, n, mode, first, count)[0] == WAH_ERR_STREAM, (k, place, mode, first, count)
            for first, count in ((0, SEG_BITS), (2 * SEG_BITS, 32 * n - 2 * SEG_BITS), (77, 1000)):
                status, out = _status(wah, table, n, mode, first, count)
                assert status == WAH_OK and np.array_equal(out, t.want(order, first, count, mode)), (k, place, mode, first, count)
    empty = t.table([0, 1, 2])
    empty[1, 2] = 0  # a row without an index
    assert _status(wah, empty, n, BITS, 5, 1)[0] == WAH_ERR_STREAM
    with pytest.raises(wah.WahError):
        wah.values_device(empty, n, BITS, 5, 1)


# ---- 5: more items than the launch has workgroups -----------------------------------------------------------------------------------------
def test_a_workgroup_takes_a_second_item(wah):
    """One item more than the grid's cap (read from the kernel source), over bitmaps built from row lists -- a few words a segment,
    nothing of the bitmaps' size exists but the output: FIRST has one item a segment; BITS over 33 table rows two, over the first
    half of the segments and one more."""
    import torch

    items = vl.grid_items() + 1
    n = items * SEG
    s = np.arange(items, dtype=np.int64)
    lists = [(s * SEG_BITS + (s * 7919 + c * 131) % SEG_BITS)[(s + c) % 3 == 0] for c in range(33)]
    stream, offsets = wah.columns.bitmaps_from_rows(wah, [_dev64(x) for x in lists], n)
    assert stream.numel() < 80 * items
    table = wah.columns.column_operand_table(stream, offsets, n, list(range(33)))
    for mode, segments in ((FIRST, items), (BITS, items // 2 + 1)):
        count = segments * SEG_BITS - 5
        assert len(vl.items(mode, 33, 3, count)) in (items, items + 1)
        want = torch.full((count,), -1 if mode == FIRST else 0, dtype=torch.int64, device="cuda")
        for c in range(32, -1, -1):
            at = _dev64(lists[c][(lists[c] >= 3) & (lists[c] < 3 + count)]) - 3
            want[at] = c if mode == FIRST else 1 << (32 - c)
        buf, out = _guarded(count)
        got = wah.values_device(table, n, mode, 3, count, out=out)
        assert torch.equal(got, want) and _guards_kept(buf, count), mode
        assert int((want != want[0]).sum()) > segments // 2
        del buf, out, got, want


# ---- 6: bitmaps of more than 2^32 rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_of_table", (5, 33))
def test_windows_behind_row_2_32(wah, oracle, rows_of_table):
    """A bitmap of 4.3e9 rows that exists only compressed (tests/_long.py): a window of a few segments that crosses row 2^32, and one
    that ends at the last row."""
    from tests.test_gpu_long_bitmaps import Uploads

    up = Uploads(oracle)
    a = lg.A_SEGMENTS
    n = a * SEG
    bitmaps = [lg.operand(a, j) for j in range(5)]
    order = [j % 5 for j in range(rows_of_table)]
    table = wah.bitop_operand_table([up.pair(bitmaps[j]) for j in order])
    last = a * SEG_BITS
    assert last == 32 * n > 2**32
    for first, count in ((2**32 - 40000, 80000), (last - 50000, 50000), (2**32, 1), (2**32 - 1, 1)):
        bits = [bitmaps[j].bits_range(first, first + count) for j in range(5)]
        for mode in (BITS, FIRST):
            got = _run(wah, table, n, mode, first, count)
            want = vl.fold([bits[j] for j in order], mode)
            assert np.array_equal(got, want), (first, count, mode)
            assert count < 10 or len(set(want.tolist())) > 3


# ---- 7: the front ends ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(wah):
    """Two segments less 1000 rows: a 20-bit price with an existence bitmap, a clustered 40-bit stamp without, a city of 300 keys."""
    import torch

    n = 2 * SEG
    rng = np.random.default_rng(12)
    count = 32 * n - 1000
    price = _bsi.uniform_values(rng, count, 20)
    stamp = _bsi.make_values("clustered", rng, count, 40)
    exists = rng.random(count) < 0.9
    city = rng.integers(0, 300, count)
    c = wah.columns
    return dict(n=n, count=count, price=price, stamp=stamp, exists=exists, city=city,
                bsi_price=c.bsi_from_values(wah, _dev64(price), 20, exists=torch.from_numpy(exists).cuda()),
                bsi_stamp=c.bsi_from_values(wah, _dev64(stamp), 40),
                index_city=c.index_from_keys(wah, _dev64(city), 300))


def test_values_and_keys_round_trip(wah, small):
    """values -> index -> values, the whole column in one call; the three roads agree."""
    import torch

    t, c = small, wah.columns
    n, count = t["n"], t["count"]
    got, have = c.values_of_column(wah, t["bsi_price"])
    assert got.numel() == 32 * n and np.array_equal(have.cpu().numpy()[:count], t["exists"]) and not have[count:].any()
    assert np.array_equal(got.cpu().numpy().view(np.uint64)[:count], np.where(t["exists"], t["price"], np.uint64(0))) and not got[count:].any()
    stamp, none = c.values_of_column(wah, t["bsi_stamp"], 0, count)
    assert none is None and np.array_equal(stamp.cpu().numpy().view(np.uint64), t["stamp"])
    keys = c.keys_of_column(wah, t["index_city"])
    assert np.array_equal(keys.cpu().numpy()[:count], t["city"]) and bool((keys[count:] == -1).all())
    for first, rows in ((0, count), (SEG_BITS - 100, 1234), (17, 0)):
        listed = torch.arange(first, first + rows, dtype=torch.int64, device="cuda")
        for bsi in (t["bsi_price"], t["bsi_stamp"]):
            one = c.values_of_column(wah, bsi, first, rows)
            for other in (c.values_at_rows(wah, bsi, listed), c._values_of_column_torch(wah, bsi, first, rows)):
                assert torch.equal(one[0], other[0]) and (one[1] is None and other[1] is None or torch.equal(one[1], other[1]))
        assert torch.equal(c.keys_of_column(wah, t["index_city"], first, rows), c.keys_at_rows(wah, t["index_city"], listed))


def test_values_of_computed_attributes(wah, small):
    """The result of multiply_columns and of set_values_where, against numpy."""
    t, c = small, wah.columns
    count = t["count"]
    product = c.multiply_columns(wah, t["bsi_price"], t["bsi_stamp"])
    assert product[3:] == (60, True)
    got, have = c.values_of_column(wah, product, 0, count)
    assert np.array_equal(have.cpu().numpy(), t["exists"])
    assert np.array_equal(got.cpu().numpy().view(np.uint64), np.where(t["exists"], t["price"] * t["stamp"], np.uint64(0)))
    lo, hi = 1 << 18, 1 << 19
    mask = c.range_column(wah, t["bsi_price"], lo, hi)
    changed = c.set_values_where(wah, t["bsi_price"], mask, count, 12345)
    got, have = c.values_of_column(wah, changed, 0, count)
    selected = t["exists"] & (t["price"] >= lo) & (t["price"] <= hi)
    assert selected.any() and np.array_equal(have.cpu().numpy(), t["exists"])
    assert np.array_equal(got.cpu().numpy().view(np.uint64), np.where(selected, np.uint64(12345), np.where(t["exists"], t["price"], np.uint64(0))))


def test_reorder_rows(wah, small):
    """A permutation, its inverse (the round trip is word for word the original index) and an order with repeats, for both kinds of
    index; after a reorder by argsort the values ascend and every column still has its set bits."""
    import torch

    t, c = small, wah.columns
    n, count = t["n"], t["count"]
    rng = np.random.default_rng(5)
    perm = rng.permutation(count)
    d_perm, d_inverse = _dev64(perm), _dev64(np.argsort(perm))
    repeats = rng.integers(0, count, 5000)
    for index, numbers in ((t["bsi_price"], np.where(t["exists"], t["price"], np.uint64(0))), (t["bsi_stamp"], t["stamp"]), (t["index_city"], t["city"].astype(np.uint64))):
        read = (lambda x, rows: c.keys_of_column(wah, x, 0, rows)) if len(index) == 3 else (lambda x, rows: c.values_of_column(wah, x, 0, rows)[0])
        moved = c.reorder_rows(wah, index, d_perm, count)
        assert moved[2:] == index[2:] and np.array_equal(read(moved, count).cpu().numpy().view(np.uint64), numbers[perm])
        back = c.reorder_rows(wah, moved, d_inverse, count)
        assert back[2:] == index[2:] and torch.equal(back[0], index[0]) and torch.equal(back[1], index[1])
        some = c.reorder_rows(wah, index, _dev64(repeats), count)
        assert some[2] == SEG and np.array_equal(read(some, 5000).cpu().numpy().view(np.uint64), numbers[repeats])
    have = c.values_of_column(wah, c.reorder_rows(wah, t["bsi_price"], d_perm, count), 0, count)[1]
    assert np.array_equal(have.cpu().numpy(), t["exists"][perm])
    rating = _bsi.uniform_values(rng, count, 12)
    unordered = c.bsi_from_values(wah, _dev64(rating), 12)
    values = c.values_of_column(wah, unordered, 0, count)[0]
    ordered = c.reorder_rows(wah, unordered, torch.argsort(values), count)
    ascending = c.values_of_column(wah, ordered, 0, count)[0]
    assert bool((ascending[1:] >= ascending[:-1]).all()) and np.array_equal(ascending.cpu().numpy().view(np.uint64), np.sort(rating))
    # clustered by its own key the attribute compresses better: the high slices of an ascending column are a few long runs, where
    # every slice of a uniform column is literals
    assert ordered[0].numel() < unordered[0].numel()
    every = list(range(12))
    assert torch.equal(c.count_columns(wah, ordered[0], ordered[1], n, every), c.count_columns(wah, unordered[0], unordered[1], n, every))
    with pytest.raises(ValueError):
        c.reorder_rows(wah, t["index_city"], _dev64([0, count]), count + 1)  # a row that no column has
    with pytest.raises(ValueError):
        c.reorder_rows(wah, t["index_city"], _dev64([0, count]), count)


# ---- 8: stream behaviour ------------------------------------------------------------------------------------------------------------------
def _two_factors(seed, count, ka, kb):
    rng = np.random.default_rng(seed)
    return _bsi.uniform_values(rng, count, ka), _bsi.uniform_values(rng, count, kb)


def test_a_chain_with_nothing_read_back_in_between(wah):
    """build -> build -> multiply -> values: only the last call's status is read."""
    n, ka, kb = 2 * SEG, 9, 14
    count = 32 * n - 333
    va, vb = _two_factors(1, count, ka, kb)
    c = wah.columns
    a = c.bsi_from_values(wah, _dev64(va), ka, check=False)
    b = c.bsi_from_values(wah, _dev64(vb), kb, check=False)
    product = c.multiply_columns(wah, a, b, check=False)
    got, have = c.values_of_column(wah, product, 5, count - 5)
    assert have is None and np.array_equal(got.cpu().numpy().view(np.uint64), (va * vb)[5:])


def test_the_chain_as_one_captured_graph(wah):
    """multiply -> values captured once (side stream, warm-up outside, check=False; one chain of launches, no parallel branches)
    and replayed: as captured; after the multiplication's table was overwritten in place with two other attributes; after the
    values call's own table was overwritten in place with another attribute's rows.  The window stays as captured."""
    import torch

    n, ka, kb, k_out = 2 * SEG, 9, 14, 23
    count = 32 * n - 333
    first, rows = SEG_BITS - 5000, 20000
    c = wah.columns
    va, vb = _two_factors(1, count, ka, kb)
    wa, wb = _two_factors(2, count, ka, kb)
    other_values = _bsi.uniform_values(np.random.default_rng(3), count, k_out)
    a, b, a2, b2 = (c.bsi_from_values(wah, _dev64(v), k) for v, k in ((va, ka), (vb, kb), (wa, ka), (wb, kb)))
    other = c.bsi_from_values(wah, _dev64(other_values), k_out)
    sc = torch.empty(int(wah.lib().wah_bsi_mul_scratch_bytes(n, ka, k_out, 0)), dtype=torch.uint8, device="cuda")
    res = torch.empty(wah.max_compressed_words(k_out * n), dtype=torch.int32, device="cuda")
    res_offs = torch.zeros(k_out * (n // SEG) + 1, dtype=torch.int64, device="cuda")
    table = torch.zeros((ka + kb, 3), dtype=torch.int64, device="cuda")
    reuse = dict(scratch=sc, out=res, out_offsets=res_offs, check=False)
    c.multiply_columns(wah, a, b, n_bits=k_out, table=table, **reuse)  # fills the table; the warm-up outside the capture
    table_v = c.column_operand_table(res, res_offs, n, list(range(k_out)))
    sc_v = torch.empty(int(wah.lib().wah_values_scratch_bytes(n, k_out)), dtype=torch.uint8, device="cuda")
    buf, out = _guarded(rows)
    wah.values_device(table_v, n, BITS, first, rows, scratch=sc_v, out=out, check=False)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            wah.bsi_mul_device(table, ka, kb, k_out, n, **reuse)
            wah.values_device(table_v, n, BITS, first, rows, scratch=sc_v, out=out, check=False)
    order = wah.bsi_mul_row_order(ka, kb, False, False)
    window = slice(first, first + rows)
    seen = set()
    for what, want in (("as captured", (va * vb)[window]), ("other factors", (wa * wb)[window]), ("another attribute", other_values[window])):
        if what == "other factors":
            c._two_attribute_table(order, a2, b2, table)  # rewrites the multiplication's table in place
        if what == "another attribute":
            table_v.copy_(c.column_operand_table(other[0], other[1], n, list(range(k_out))))
        torch.cuda.synchronize()
        buf.fill_(POISON64)
        sc_v.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bsi_mul_status(sc.data_ptr(), n, ka, k_out, 0, None) == WAH_OK
        assert wah.lib().wah_values_status(sc_v.data_ptr(), None) == WAH_OK
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want) and _guards_kept(buf, rows), what
        seen.add(want.tobytes())
    assert len(seen) == 3  # different answers from one captured chain
