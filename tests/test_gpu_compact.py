"""GPU tests of wah_compact_indexed_device (include/wah.h) and its front ends: the rows a mask bitmap selects -- or, under
WAH_COMPACT_DELETE, does not select -- of every column of an index, moved together into new indexed bitmaps.  Everything is exact:
the words, their count, every index entry and the number of selected rows against the CPU oracle's compress() of the rows picked
out of unpacked bits (tests/_compact.py: model, reference).  tests/test_compact_reference.py proves on the CPU that every named
case reaches what its name says.  Columns are one to five segments, but for three cases: 70 source segments of one selected row
each, a table of one column more than the capped grid has wavefronts, and one bitmap of more than 2^32 rows (tests/_long.py)."""
import importlib

import numpy as np
import pytest

from tests import _compact as cp, _foreign, _long as lg, _select

pytestmark = pytest.mark.gpu

WAH_OK, WAH_ERR_CAPACITY, WAH_ERR_STREAM = 0, -4, -6
SEG_WORDS, SEG_BITS = cp.SEG_WORDS, cp.SEG_BITS
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _dev(words):
    import torch

    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).cuda()


def _dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


class Operands:
    """The mask and the columns of a case in device memory, each stream with its index -- made on the host (_select.index_of) or,
    with device_index, by wah_build_index_device -- and the tables over them.  streams: {column: (stream, index)} to use instead."""

    def __init__(self, wah, oracle, case, device_index=False, streams=None):
        def pair(st, idx=None):
            d = _dev(np.concatenate([st, np.zeros(1, np.uint32)]))[: st.size]
            if idx is None:
                idx = wah.build_index_device(d)[0] if device_index else _dev64(_select.index_of(st))
            else:
                idx = _dev64(idx)
            assert idx.numel() == _select.segments_of(case.n_words) + 1, case.name
            return d, idx

        self.mask_pair = pair(case.mask_stream(oracle))
        self.pairs = [pair(*streams[c]) if streams and c in streams else pair(case.column_stream(oracle, c)) for c in range(case.n_columns)]
        self.mask = wah.bitop_operand_table([self.mask_pair])
        self.table = wah.bitop_operand_table(self.pairs)


def _run(wah, case, ops, **kw):
    return wah.compact_device(ops.mask, ops.table, case.n_words, case.n_rows, case.n_words_out, delete=case.delete, **kw)


def _check(case, got, want, what=None):
    stream, offs, rows = got
    want_stream, want_index, want_rows = want
    what = what or case.name
    assert int(rows.item()) == want_rows, (what, int(rows.item()), want_rows)
    assert stream.numel() == want_stream.size, (what, stream.numel(), want_stream.size)
    assert np.array_equal(_host(stream), want_stream), what
    assert offs.numel() == want_index.size and np.array_equal(offs.cpu().numpy(), want_index), what


def _run_guarded(wah, oracle, case, ops=None):
    """The call into an output of exactly wah_compact_max_words words for the column segments that are read, a guard word behind it."""
    import torch

    ops = ops or Operands(wah, oracle, case)
    cap = wah.compact_max_words(case.n_words_out, case.n_columns, cp.read_source_words(oracle, case))
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    got = _run(wah, case, ops, out=buf[:cap])
    assert int(buf[cap].item()) == GUARD, case.name
    return got


# ---- the named cases ---------------------------------------------------------------------------------------------------------------
CASES = cp.named_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_named_case(wah, oracle, case):
    _check(case, _run_guarded(wah, oracle, case), cp.reference(oracle, case))


@pytest.mark.parametrize("delete", (False, True))
def test_the_identity_is_compress_of_the_columns(wah, oracle, delete):
    case = cp.all_zeros(True) if delete else cp.all_ones(False)
    got = _run_guarded(wah, oracle, case)
    assert np.array_equal(_host(got[0]), np.concatenate([oracle.compress(c) for c in case.columns])) and int(got[2].item()) == case.n_rows


@pytest.mark.parametrize("delete", (False, True))
def test_no_selected_row_is_one_zero_fill_per_segment(wah, oracle, delete):
    case = cp.all_ones(True) if delete else cp.all_zeros(False)
    stream, offs, rows = _run_guarded(wah, oracle, case)
    segments = _select.segments_of(case.n_words_out)
    groups = _select.groups_of(case.n_words_out)
    fills = [cp.FILL0 | min(1024, groups - 1024 * s) for s in range(segments)] * case.n_columns
    assert int(rows.item()) == 0 and np.array_equal(_host(stream), np.array(fills, np.uint32))
    assert np.array_equal(offs.cpu().numpy(), np.arange(case.n_columns * segments + 1))


FOREIGN = [cp.foreign(way) for way in _foreign.WAYS[1:]]


@pytest.mark.parametrize("case", FOREIGN, ids=[c.name for c in FOREIGN])
def test_foreign_streams_indexed_on_the_device(wah, oracle, case):
    _check(case, _run_guarded(wah, oracle, case, Operands(wah, oracle, case, device_index=True)), cp.reference(oracle, case))


@pytest.mark.parametrize("way", _foreign.PAD_WAYS)
def test_set_pad_bits_indexed_on_the_device(wah, oracle, way):
    for delete in (False, True):
        case = cp.pad_rows(delete, way)
        _check(case, _run_guarded(wah, oracle, case, Operands(wah, oracle, case, device_index=True)), cp.reference(oracle, case))


def test_one_row_more_than_the_output_holds_is_a_stream_error(wah, oracle):
    import torch

    case = cp.overfull_output()
    ops = Operands(wah, oracle, case)
    sc = torch.empty(int(wah.lib().wah_compact_scratch_bytes(case.n_words, case.n_words_out, case.n_columns)), dtype=torch.uint8, device="cuda")
    _, _, _, rows = _run(wah, case, ops, scratch=sc, check=False)
    assert wah.lib().wah_compact_status(sc.data_ptr(), None) == WAH_ERR_STREAM
    assert int(rows.item()) == 32 * case.n_words_out + 1
    full = cp.full_output()  # ... and the same shape with one row fewer is accepted
    _check(full, _run(wah, full, Operands(wah, oracle, full), scratch=sc), cp.reference(oracle, full))


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def test_columns_as_windows_into_a_column_matrix(wah, oracle):
    """The columns of one matrix stream with its whole index, picked by number and out of order (columns.column_operand_table)."""
    n = 2 * SEG_WORDS
    matrix = [cp.random_words(n, 0.5, 61), cp.clustered_words(n, 62), cp.random_words(n, 0.01, 63), np.full(n, 0xFFFFFFFF, np.uint32)]
    streams = [np.ascontiguousarray(oracle.compress(c), dtype=np.uint32) for c in matrix]
    ends = np.cumsum([0] + [s.size for s in streams])
    index = np.concatenate([_select.index_of(s)[:-1] + at for s, at in zip(streams, ends)] + [[ends[-1]]])
    d_stream, d_index = _dev(np.concatenate(streams)), _dev64(index)
    picked = [2, 0, 3]
    table = wah.columns.column_operand_table(d_stream, d_index, n, picked)
    case = cp.Case("windows", n, 32 * n - 77, n, cp.random_words(n, 0.3, 64), [matrix[c] for c in picked])
    ops = Operands(wah, oracle, case)
    got = wah.compact_device(ops.mask_pair, table, n, case.n_rows, n)
    _check(case, got, cp.reference(oracle, case))


def test_an_output_that_is_not_8_byte_aligned(wah, oracle):
    import torch

    case = cp.half()
    want = cp.reference(oracle, case)
    buf = torch.full((want[0].size + 3,), GUARD, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 8 == 0
    got = _run(wah, case, Operands(wah, oracle, case), out=buf[1: 1 + want[0].size])
    assert got[0].data_ptr() % 8 == 4
    _check(case, got, want)
    assert int(buf[0].item()) == GUARD and bool((buf[1 + want[0].size:] == GUARD).all())


def test_a_wavefront_takes_a_second_item(wah, oracle):
    """A table that repeats three columns until it has one row more than the capped grid has wavefronts: every output column
    against its source column's reference."""
    base = cp.Case("full grid", SEG_WORDS, SEG_BITS - 9, SEG_WORDS, cp.random_words(SEG_WORDS, 0.5, 71),
                   [cp.random_words(SEG_WORDS, 0.02, 72), cp.clustered_words(SEG_WORDS, 73), cp.random_words(SEG_WORDS, 0.5, 74)])
    ops = Operands(wah, oracle, base)
    k = cp.full_grid_columns()
    table = ops.table.repeat(-(-k // 3), 1)[:k].contiguous()
    stream, offs, rows = wah.compact_device(ops.mask, table, base.n_words, base.n_rows, base.n_words_out)
    want_stream, want_index, want_rows = cp.reference(oracle, base)
    assert int(rows.item()) == want_rows and offs.numel() == k + 1
    words, index = _host(stream), offs.cpu().numpy()
    for c in range(k):
        want = want_stream[want_index[c % 3]: want_index[c % 3 + 1]]
        assert np.array_equal(words[index[c]: index[c + 1]], want), c
    assert index[-1] == words.size


# ---- refusals the device sees ------------------------------------------------------------------------------------------------------
def _status(wah, case, ops, cap=None):
    """The call with check=False and then its status: (code, out buffer, count, offsets, rows)."""
    import torch

    k, n = case.n_columns, case.n_words_out
    sc = torch.empty(int(wah.lib().wah_compact_scratch_bytes(case.n_words, n, k)), dtype=torch.uint8, device="cuda")
    full = k * wah.max_compressed_words(n)
    buf = torch.full((full + 1,), GUARD, dtype=torch.int32, device="cuda")
    out, count, offs, rows = _run(wah, case, ops, scratch=sc, out=buf[: full if cap is None else cap], check=False)
    code = wah.lib().wah_compact_status(sc.data_ptr(), None)
    return code, buf, int(count.item()), offs, int(rows.item())


def test_capacity(wah, oracle):
    case = cp.half()
    ops = Operands(wah, oracle, case)
    want = cp.reference(oracle, case)
    total = want[0].size
    code, buf, count, offs, rows = _status(wah, case, ops, cap=total)
    assert code == WAH_OK and count == total and np.array_equal(_host(buf[:total]), want[0]) and int(buf[total].item()) == GUARD
    code, buf, count, offs, rows = _status(wah, case, ops, cap=total - 1)
    assert code == WAH_ERR_CAPACITY and count == total and rows == want[2]
    assert bool((buf[total - 1:] == GUARD).all()), "a word at or behind the capacity was written"
    assert np.array_equal(_host(buf[: total - 1]), want[0][: total - 1])


def test_a_malformed_column_segment_is_refused_only_where_a_row_is_selected(wah, oracle):
    n = 2 * SEG_WORDS
    col = cp.clustered_words(n, 110)
    st = np.ascontiguousarray(oracle.compress(col), dtype=np.uint32)
    idx = _select.index_of(st)
    fills = np.flatnonzero(st[idx[1]:] & np.uint32(cp.FILL0)) + idx[1]
    bad = st.copy()
    bad[fills[fills.size // 2]] += 1  # a fill of segment 1 one group too long: the segment's words no longer make up its groups
    in_both = cp.random_words(n, 0.2, 111)
    in_first = in_both.copy()
    in_first[SEG_WORDS:] = 0
    reads = cp.Case("selects a row of segment 1", n, 32 * n, SEG_WORDS, in_both, [col])
    stays = cp.Case("selects rows of segment 0 only", n, 32 * n, SEG_WORDS, in_first, [col])
    assert _status(wah, reads, Operands(wah, oracle, reads, streams={0: (bad, idx)}))[0] == WAH_ERR_STREAM
    _check(stays, _run(wah, stays, Operands(wah, oracle, stays, streams={0: (bad, idx)})), cp.reference(oracle, stays))
    _check(reads, _run(wah, reads, Operands(wah, oracle, reads)), cp.reference(oracle, reads))


def test_a_malformed_mask_segment_is_refused_whatever_it_selects(wah, oracle):
    """The mask is checked in every segment: a broken fill in a segment behind n_rows, which selects nothing, is refused."""
    n = 2 * SEG_WORDS
    mask = cp.clustered_words(n, 112)
    st = np.ascontiguousarray(oracle.compress(mask), dtype=np.uint32)
    idx = _select.index_of(st)
    fills = np.flatnonzero(st[idx[1]:] & np.uint32(cp.FILL0)) + idx[1]
    bad = st.copy()
    bad[fills[fills.size // 2]] += 1
    case = cp.Case("rows of segment 0 only", n, SEG_BITS - 5, SEG_WORDS, mask, [cp.random_words(n, 0.5, 113)])
    ops = Operands(wah, oracle, case)
    _check(case, _run(wah, case, ops), cp.reference(oracle, case))
    ops.mask_pair = (_dev(bad), ops.mask_pair[1])
    ops.mask = wah.bitop_operand_table([ops.mask_pair])
    assert _status(wah, case, ops)[0] == WAH_ERR_STREAM


# ---- more than 2^32 rows -----------------------------------------------------------------------------------------------------------
def test_ranks_and_output_rows_beyond_2_32(wah, oracle):
    """Size A of tests/_long.py (4.3e9 rows, compressed only): a mask of ones fills with five deleted rows in its first segment, so
    that the ranks of all but the first source segment and the output's rows pass 2^32 -- and every output segment draws from two
    source segments.  Expected: the segment-sparse splice model over the six row ranges between the deleted rows."""
    import torch

    a = lg.A_SEGMENTS
    n, n_rows = a * SEG_WORDS, a * SEG_BITS
    deleted = [3, 64, 1000, 20000, 31743]
    bits = np.ones(SEG_BITS, np.uint8)
    bits[deleted] = 0
    mask = lg.LongBitmap(a, 1, {0: cp.words_of(bits)})
    columns = [lg.marked(a, lg.A_NAMED, lg.A_ROWS, 501), lg.marked(a, lg.A_NAMED, (), 502, default=1)]
    edges = [-1] + deleted + [n_rows]
    ranges = [(lo + 1, hi - lo - 1) for lo, hi in zip(edges[:-1], edges[1:])]
    want = [lg.splice([(col, first, rows) for first, rows in ranges], a) for col in columns]
    want_stream, want_index = lg.expected_streams(oracle, want)
    total = n_rows - len(deleted)
    assert total > 2**32 and want[0].bit(2**32 - 5) == 1 and want[0].bit(lg.A_ROWS[-1] - 5) == 1

    pairs = [tuple(f(x) for f, x in zip((_dev, _dev64), b.stream_index(oracle))) for b in [mask] + columns]
    source_words = sum(int(p[0].numel()) for p in pairs[1:])
    cap = wah.compact_max_words(n, 2, source_words)
    assert want_stream.size <= cap
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    stream, offs, rows = wah.compact_device(pairs[0], wah.bitop_operand_table(pairs[1:]), n, n_rows, n, out=buf[:cap])
    assert int(rows.item()) == total and int(buf[cap].item()) == GUARD
    assert stream.numel() == want_stream.size and torch.equal(offs, _dev64(want_index))
    assert torch.equal(stream, _dev(want_stream))


# ---- the front ends ----------------------------------------------------------------------------------------------------------------
N_ROWS = SEG_BITS + 9001  # two segments, the last one ragged in rows


def _key_tables(wah, seed):
    rng = np.random.default_rng(seed)
    keys, other = rng.integers(0, 7, N_ROWS), rng.integers(0, 5, N_ROWS)
    return keys, other, wah.columns.index_from_keys(wah, _dev64(keys), 7), wah.columns.index_from_keys(wah, _dev64(other), 5)


@pytest.mark.parametrize("negate", (False, True))
def test_keep_and_delete_rows_of_an_equality_encoded_index(wah, negate):
    """WHERE other [NOT] IN (1, 3): the kept rows' keys, the deleted rows' keys, and COUNT(*) GROUP BY key on the compacted index
    against the same count under the predicate on the original.  A NOT IN mask has every position behind the table's rows set."""
    import torch

    keys, other, index, filt = _key_tables(wah, 81)
    predicates = [(filt[0], filt[1], [1, 3], negate)]
    mask = wah.columns.filter_columns(wah, predicates, index[2])
    sel = np.isin(other, [1, 3]) != negate
    for fn, chosen in ((wah.columns.keep_rows, sel), (wah.columns.delete_rows, ~sel)):
        got, rows = fn(wah, index, mask, N_ROWS)
        total = int(chosen.sum())
        assert int(rows.item()) == total and len(got) == 3 and got[2] == max(-(-total // SEG_BITS), 1) * SEG_WORDS
        assert got[1].numel() == 7 * (got[2] // SEG_WORDS) + 1
        fetched = wah.columns.keys_at_rows(wah, got, torch.arange(32 * got[2], dtype=torch.int64, device="cuda")).cpu().numpy()
        assert np.array_equal(fetched[:total], keys[chosen]) and bool((fetched[total:] == -1).all())
        counts = wah.columns.count_columns(wah, *got, list(range(7))).cpu().numpy()
        assert np.array_equal(counts, np.bincount(keys[chosen], minlength=7))
    kept = wah.columns.keep_rows(wah, index, mask, N_ROWS)[0]
    where = wah.columns.count_columns_where(wah, predicates, *index, list(range(7))).cpu().numpy()
    assert np.array_equal(where, np.bincount(keys[sel], minlength=7))  # (no column has a bit behind the table's rows)
    assert np.array_equal(wah.columns.count_columns(wah, *kept, list(range(7))).cpu().numpy(), where)
    # a bound instead of the count: the same rows in columns of the bound's length, nothing read back for the size
    bounded, rows = wah.columns.keep_rows(wah, index, mask, N_ROWS, n_rows_out=N_ROWS)
    assert bounded[2] == index[2] and int(rows.item()) == int(sel.sum())
    assert np.array_equal(wah.columns.count_columns(wah, *bounded, list(range(7))).cpu().numpy(), where)


def test_keep_and_delete_rows_of_a_bit_sliced_index_with_existence(wah):
    import torch

    n_bits = 12
    rng = np.random.default_rng(82)
    values = rng.integers(0, 1 << n_bits, N_ROWS)
    exists = rng.random(N_ROWS) < 0.8
    bsi = wah.columns.bsi_from_values(wah, _dev64(values), n_bits, exists=torch.from_numpy(exists).cuda())
    lo, hi = 1000, 1700
    mask = wah.columns.range_column(wah, bsi, lo, hi)
    sel = exists & (values >= lo) & (values <= hi)
    stored = np.where(exists, values, 0)
    for fn, chosen in ((wah.columns.keep_rows, sel), (wah.columns.delete_rows, ~sel)):
        got, rows = fn(wah, bsi, mask, N_ROWS)
        total = int(chosen.sum())
        assert int(rows.item()) == total and len(got) == 5 and got[3:] == (n_bits, True) and got[2] == max(-(-total // SEG_BITS), 1) * SEG_WORDS
        fetched, have = wah.columns.values_at_rows(wah, got, torch.arange(32 * got[2], dtype=torch.int64, device="cuda"))
        assert np.array_equal(have.cpu().numpy()[:total], exists[chosen]) and not bool(have[total:].any())
        assert np.array_equal(fetched.cpu().numpy()[:total], stored[chosen]) and not bool(fetched[total:].any())
        # the result goes unchanged into the calls that read an index
        stream, offs = wah.columns.range_column(wah, got, 1200, 3000)
        positions, count = wah.positions_device(stream, offs, got[2])
        want = np.flatnonzero(exists[chosen] & (values[chosen] >= 1200) & (values[chosen] <= 3000))
        assert count == want.size and np.array_equal(positions.cpu().numpy(), want)


class Chain:
    """filter -> keep_rows -> range -> count as four calls that are only enqueued, every buffer made beforehand and every table
    filled beforehand: what a captured graph needs, and what reads nothing back."""

    def __init__(self, wah, seed):
        import torch

        self.wah, self.n_bits = wah, 10
        rng = np.random.default_rng(seed)
        self.values = rng.integers(0, 1 << self.n_bits, N_ROWS)
        self.exists = rng.random(N_ROWS) < 0.9
        self.other = rng.integers(0, 5, N_ROWS)
        self.bsi = wah.columns.bsi_from_values(wah, _dev64(self.values), self.n_bits, exists=torch.from_numpy(self.exists).cuda())
        self.filt = wah.columns.index_from_keys(wah, _dev64(self.other), 5)
        n, k = self.bsi[2], self.n_bits + 1
        self.n, self.k = n, k
        lib = wah.lib()

        def bytes_(size):
            return torch.empty(int(size), dtype=torch.uint8, device="cuda")

        def words(count):
            return torch.full((int(count),), GUARD, dtype=torch.int32, device="cuda")

        def index(entries):
            return torch.zeros(int(entries), dtype=torch.int64, device="cuda")

        segs = n // SEG_WORDS
        self.ids = torch.tensor([1, 3], dtype=torch.int64, device="cuda")
        self.filter_table = torch.empty((2, 3), dtype=torch.int64, device="cuda")
        self.filter_ends = torch.tensor([2], dtype=torch.int64, device="cuda")
        self.filter_reuse = dict(scratch=bytes_(lib.wah_bitop_clauses_scratch_bytes(n, 2, 1)), out=words(wah.max_compressed_words(n)), out_offsets=index(segs + 1))
        self.columns = wah.columns.column_operand_table(self.bsi[0], self.bsi[1], n, list(range(k)))
        self.mask = wah.bitop_operand_table([(self.filter_reuse["out"], self.filter_reuse["out_offsets"])])
        self.kept_reuse = dict(scratch=bytes_(lib.wah_compact_scratch_bytes(n, n, k)), out=words(k * wah.max_compressed_words(n)), out_offsets=index(k * segs + 1),
                               out_rows=index(1))
        self.kept_table = wah.columns.column_operand_table(self.kept_reuse["out"], self.kept_reuse["out_offsets"], n, list(range(k)))
        self.bounds = wah.bsi_bounds(300, 800, "cuda")
        self.range_reuse = dict(scratch=bytes_(lib.wah_bsi_range_scratch_bytes(n, k)), out=words(wah.max_compressed_words(n)), out_offsets=index(segs + 1))
        self.count_table = wah.bitop_operand_table([(self.range_reuse["out"], self.range_reuse["out_offsets"])])
        self.count_reuse = dict(scratch=bytes_(lib.wah_select_scratch_bytes(n, 1)), counts=index(1))
        self.write([1, 3])

    def write(self, ids):
        """The filter's table overwritten in place: other IN ids (two of them)."""
        self.ids.copy_(_dev64(ids))
        self.wah.columns.column_operand_table(self.filt[0], self.filt[1], self.n, self.ids, out=self.filter_table)
        self.named = list(ids)

    def enqueue(self):
        wah, n = self.wah, self.n
        wah.bitop_clauses_indexed_device((self.filter_table, self.filter_ends), n, check=False, **self.filter_reuse)
        wah.compact_device(self.mask, self.columns, n, N_ROWS, n, check=False, **self.kept_reuse)
        wah.bsi_range_device(self.kept_table, self.bounds, n, exists=True, check=False, **self.range_reuse)
        wah.count_device(self.count_table, n, check=False, **self.count_reuse)

    def verify(self):
        lib, n = self.wah.lib(), self.n
        assert lib.wah_bitop_clauses_status(self.filter_reuse["scratch"].data_ptr(), n, 2, 1, None) == WAH_OK
        assert lib.wah_compact_status(self.kept_reuse["scratch"].data_ptr(), None) == WAH_OK
        assert lib.wah_bsi_range_status(self.range_reuse["scratch"].data_ptr(), n, self.k, None) == WAH_OK
        assert lib.wah_select_status(self.count_reuse["scratch"].data_ptr(), None) == WAH_OK
        sel = np.isin(self.other, self.named)
        assert int(self.kept_reuse["out_rows"].item()) == int(sel.sum())
        want = int((self.exists[sel] & (self.values[sel] >= 300) & (self.values[sel] <= 800)).sum())
        assert int(self.count_reuse["counts"].item()) == want, (self.named, int(self.count_reuse["counts"].item()), want)


def test_a_chain_of_calls_with_nothing_read_back(wah):
    """filter_columns -> keep_rows(n_rows_out=n_rows) -> range_column -> count through the front ends, every one with check=False:
    the statuses and the answer are read once, at the end."""
    import torch

    chain = Chain(wah, 83)
    n = chain.n
    out, _, out_offsets = wah.columns.filter_columns(wah, [(chain.filt[0], chain.filt[1], [0, 4], False)], n, check=False, **chain.filter_reuse)
    kept, rows = wah.columns.keep_rows(wah, chain.bsi, (out, out_offsets), N_ROWS, n_rows_out=N_ROWS, check=False, **chain.kept_reuse)
    assert kept[2:] == (n, chain.n_bits, True) and kept[0] is chain.kept_reuse["out"]
    ranged, _, ranged_offsets = wah.columns.range_column(wah, kept, 300, 800, check=False, **chain.range_reuse)
    counts = wah.count_device([(ranged, ranged_offsets)], n, check=False, **chain.count_reuse)
    torch.cuda.synchronize()
    chain.named = [0, 4]
    chain.verify()
    assert counts is chain.count_reuse["counts"] and rows is chain.kept_reuse["out_rows"]


def test_the_chain_as_one_graph_replayed_over_a_rewritten_filter(wah):
    """The mask, the tables and the ranks are only ever read by the device: ONE captured chain, replayed after the filter's table
    was overwritten in place, compacts the new selection and counts in it (capture as tests/test_gpu_splice.py: side stream,
    warm-up outside, check=False; one chain of launches, no parallel branches)."""
    import torch

    chain = Chain(wah, 84)
    chain.enqueue()  # warm-up outside the capture
    torch.cuda.synchronize()
    chain.verify()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            chain.enqueue()
    for ids in ([0, 2], [4, 1], [1, 3]):
        chain.write(ids)
        chain.kept_reuse["out"].fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        chain.verify()
