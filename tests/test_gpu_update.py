"""GPU tests of wah_update_indexed_device (include/wah.h) and its front ends: per column the blend of two indexed bitmaps under
a mask bitmap -- then where the mask selects a row below n_rows, else everywhere else.  Everything is exact: the words, their count
and every index entry against the CPU oracle's compress() of the blend on unpacked bits (tests/_update.py: model, reference).
tests/test_update_reference.py proves on the CPU that every named case reaches what its name says.  Columns are one to three
segments, but for two cases: a table of one-segment columns with one column more than the capped grid has wavefronts, and one
bitmap of more than 2^32 rows (tests/_long.py)."""
import importlib

import numpy as np
import pytest

from tests import _foreign, _long as lg, _select, _update as up

pytestmark = pytest.mark.gpu

WAH_OK, WAH_ERR_CAPACITY, WAH_ERR_STREAM = 0, -4, -6
SEG_WORDS, SEG_BITS = up.SEG_WORDS, up.SEG_BITS
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
    """The mask and both sides of a case in device memory, each stream with its index -- made on the host (_select.index_of) or,
    with device_index, by wah_build_index_device -- and the tables over them; a constant stays the int it is.  odd: every stream
    begins 4 bytes behind an 8-byte boundary.  streams: {(side, column): (stream, index)} to use instead."""

    def __init__(self, wah, oracle, case, device_index=False, odd=False, streams=None):
        def pair(st, idx=None):
            first = 1 if odd else 0
            buf = _dev(np.concatenate([np.zeros(first, np.uint32), st, np.zeros(1, np.uint32)]))
            assert buf.data_ptr() % 8 == 0
            d = buf[first: first + st.size]
            assert d.data_ptr() % 8 == (4 if odd else 0)
            if idx is None:
                idx = wah.build_index_device(d)[0] if device_index else _dev64(_select.index_of(st))
            else:
                idx = _dev64(idx)
            assert idx.numel() == _select.segments_of(case.n_words) + 1, case.name
            return d, idx

        def entry(side, c):
            if streams and (side, c) in streams:
                return pair(*streams[(side, c)])
            k = case.constant(side, c)
            return k if k is not None else pair(case.stream(oracle, side, c))

        self.mask_pair = pair(case.mask_stream(oracle))
        self.sides = {side: [entry(side, c) for c in range(case.n_columns)] for side in ("else", "then")}
        self.mask = wah.bitop_operand_table([self.mask_pair])
        self.tables = {side: wah.update_operand_table(self.sides[side], device="cuda") for side in ("else", "then")}


def _run(wah, case, ops, **kw):
    return wah.update_device(ops.mask, ops.tables["else"], ops.tables["then"], case.n_words, case.n_rows, **kw)


def _check(case, got, want, what=None):
    stream, offs = got
    want_stream, want_index = want
    what = what or case.name
    assert stream.numel() == want_stream.size, (what, stream.numel(), want_stream.size)
    assert np.array_equal(_host(stream), want_stream), what
    assert offs.numel() == want_index.size and np.array_equal(offs.cpu().numpy(), want_index), what


def _run_guarded(wah, oracle, case, ops=None):
    """The call into an output of exactly wah_update_max_words words for what is read, a guard word behind it."""
    import torch

    ops = ops or Operands(wah, oracle, case)
    cap = wah.update_max_words(case.n_words, case.n_columns, *up.read_words(oracle, case))
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    got = _run(wah, case, ops, out=buf[:cap])
    assert int(buf[cap].item()) == GUARD, case.name
    return got


# ---- the named cases ---------------------------------------------------------------------------------------------------------------
CASES = up.named_cases()
FOREIGN = up.foreign_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_named_case(wah, oracle, case):
    _check(case, _run_guarded(wah, oracle, case), up.reference(oracle, case))


def test_a_mask_of_zeros_leaves_compress_of_the_else_columns(wah, oracle):
    case = up.mask_of_zeros()
    got = _run_guarded(wah, oracle, case)
    assert np.array_equal(_host(got[0]), np.concatenate([oracle.compress(case.words("else", c)) for c in range(case.n_columns)]))


@pytest.mark.parametrize("case", FOREIGN, ids=[c.name for c in FOREIGN])
def test_foreign_streams(wah, oracle, case):
    _check(case, _run_guarded(wah, oracle, case), up.reference(oracle, case))


@pytest.mark.parametrize("case", FOREIGN, ids=[c.name for c in FOREIGN])
def test_foreign_streams_indexed_on_the_device(wah, oracle, case):
    _check(case, _run_guarded(wah, oracle, case, Operands(wah, oracle, case, device_index=True)), up.reference(oracle, case))


@pytest.mark.parametrize("way", _foreign.PAD_WAYS)
def test_set_pad_bits_indexed_on_the_device(wah, oracle, way):
    case = up.set_pad_bits(way)
    _check(case, _run_guarded(wah, oracle, case, Operands(wah, oracle, case, device_index=True)), up.reference(oracle, case))


@pytest.mark.parametrize("case", [up.seam_rows(), up.constants("then"), up.foreign("mixed", "mask")], ids=lambda c: c.name)
def test_streams_at_odd_4_byte_placements(wah, oracle, case):
    _check(case, _run_guarded(wah, oracle, case, Operands(wah, oracle, case, odd=True)), up.reference(oracle, case))


def test_an_output_that_is_not_8_byte_aligned(wah, oracle):
    import torch

    case = up.seam_rows()
    want = up.reference(oracle, case)
    buf = torch.full((want[0].size + 3,), GUARD, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 8 == 0
    got = _run(wah, case, Operands(wah, oracle, case), out=buf[1: 1 + want[0].size])
    assert got[0].data_ptr() % 8 == 4
    _check(case, got, want)
    assert int(buf[0].item()) == GUARD and bool((buf[1 + want[0].size:] == GUARD).all())


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def test_a_table_of_pairs_and_constants(wah):
    """A pair becomes the row of bitop_operand_table, a constant the row (0, bit, 0)."""
    st, offs = _dev(np.zeros(4, np.uint32)), _dev64(np.zeros(2, np.int64))
    table = wah.update_operand_table([0, (st, offs), 1])
    assert table.is_cuda and table.tolist() == [[0, 0, 0], [st.data_ptr(), 4, offs.data_ptr()], [0, 1, 0]]
    assert wah.update_operand_table([(st, offs)]).tolist() == wah.bitop_operand_table([(st, offs)]).tolist()
    assert wah.update_operand_table([1, 0], device="cuda").tolist() == [[0, 1, 0], [0, 0, 0]]
    for bad in ([], [2], [0, 1]):  # nothing; neither 0 nor 1; constants only and no device
        with pytest.raises(wah.WahError):
            wah.update_operand_table(bad)


def _wide(k, n_words, n_rows, seed):
    """k columns: sources of every kind and constants in turn on both sides."""
    pool = [up.random_words(n_words, 0.5, seed), up.random_words(n_words, 0.002, seed + 1), up.clustered_words(n_words, seed + 2), 0, 1,
            np.zeros(n_words, np.uint32), np.full(n_words, up.ONES, np.uint32)]
    else_ = [pool[c % len(pool)] for c in range(k)]
    then = [pool[(3 * c + 1) % len(pool)] for c in range(k)]
    return up.Case(f"{k} columns", n_words, n_rows, up.random_words(n_words, 0.3, seed + 3), else_, then)


@pytest.mark.parametrize("k", (1, 5, 65))
def test_column_counts(wah, oracle, k):
    """One, a few, and more than a wavefront has lanes; two segments and a ragged third, so that a wavefront's run of items crosses
    segments and keeps or walks the mask image as it should."""
    case = _wide(k, 2 * SEG_WORDS + 1, 32 * (2 * SEG_WORDS + 1) - 9, 80 + k)
    _check(case, _run_guarded(wah, oracle, case), up.reference(oracle, case))


def test_columns_as_windows_into_a_column_matrix(wah, oracle):
    """Both sides picked by number, out of order, from one matrix stream with its whole index (columns.column_operand_table)."""
    n = 2 * SEG_WORDS
    matrix = [up.random_words(n, 0.5, 61), up.clustered_words(n, 62), up.random_words(n, 0.01, 63), np.full(n, up.ONES, np.uint32)]
    streams = [np.ascontiguousarray(oracle.compress(c), dtype=np.uint32) for c in matrix]
    ends = np.cumsum([0] + [s.size for s in streams])
    index = np.concatenate([_select.index_of(s)[:-1] + at for s, at in zip(streams, ends)] + [[ends[-1]]])
    d_stream, d_index = _dev(np.concatenate(streams)), _dev64(index)
    else_ids, then_ids = [2, 0, 3], [1, 3, 0]
    case = up.Case("windows", n, 32 * n - 77, up.random_words(n, 0.3, 64), [matrix[c] for c in else_ids], [matrix[c] for c in then_ids])
    ops = Operands(wah, oracle, case)
    table = wah.columns.column_operand_table
    got = wah.update_device(ops.mask_pair, table(d_stream, d_index, n, else_ids), table(d_stream, d_index, n, then_ids), n, case.n_rows)
    _check(case, got, up.reference(oracle, case))


def test_a_wavefront_takes_a_second_item(wah, oracle):
    """Tables that repeat three columns until they have one row more than the capped grid has wavefronts: every output column
    against its source columns' reference."""
    base = up.Case("full grid", SEG_WORDS, SEG_BITS - 9, up.random_words(SEG_WORDS, 0.5, 71),
                   [up.random_words(SEG_WORDS, 0.02, 72), up.clustered_words(SEG_WORDS, 73), 1],
                   [up.clustered_words(SEG_WORDS, 74), 0, up.random_words(SEG_WORDS, 0.5, 75)])
    ops = Operands(wah, oracle, base)
    k = up.full_grid_columns()
    tables = [ops.tables[side].repeat(-(-k // 3), 1)[:k].contiguous() for side in ("else", "then")]
    stream, offs = wah.update_device(ops.mask, tables[0], tables[1], base.n_words, base.n_rows)
    want_stream, want_index = up.reference(oracle, base)
    assert offs.numel() == k + 1
    words, index = _host(stream), offs.cpu().numpy()
    for c in range(k):
        want = want_stream[want_index[c % 3]: want_index[c % 3 + 1]]
        assert np.array_equal(words[index[c]: index[c + 1]], want), c
    assert index[-1] == words.size


# ---- refusals the device sees ------------------------------------------------------------------------------------------------------
def _status(wah, case, ops, cap=None, mask=None, tables=None):
    """The call with check=False and then its status: (code, out buffer, count, offsets)."""
    import torch

    k, n = case.n_columns, case.n_words
    sc = torch.empty(int(wah.lib().wah_update_scratch_bytes(n, k)), dtype=torch.uint8, device="cuda")
    full = k * wah.max_compressed_words(n)
    buf = torch.full((full + 1,), GUARD, dtype=torch.int32, device="cuda")
    tables = tables or ops.tables
    out, count, offs = wah.update_device(ops.mask if mask is None else mask, tables["else"], tables["then"], n, case.n_rows, scratch=sc,
                                         out=buf[: full if cap is None else cap], check=False)
    code = wah.lib().wah_update_status(sc.data_ptr(), None)
    return code, buf, int(count.item()), offs


def test_capacity(wah, oracle):
    case = up.seam_rows()
    ops = Operands(wah, oracle, case)
    want = up.reference(oracle, case)
    total = want[0].size
    code, buf, count, offs = _status(wah, case, ops, cap=total)
    assert code == WAH_OK and count == total and np.array_equal(_host(buf[:total]), want[0]) and int(buf[total].item()) == GUARD
    code, buf, count, offs = _status(wah, case, ops, cap=total - 1)
    assert code == WAH_ERR_CAPACITY and count == total
    assert bool((buf[total - 1:] == GUARD).all()), "a word at or behind the capacity was written"
    assert np.array_equal(_host(buf[: total - 1]), want[0][: total - 1])


def _broken(oracle, words, seg):
    """(stream, index) of a bitmap whose segment `seg` holds a fill one group too long: its words no longer make up its groups."""
    st = np.ascontiguousarray(oracle.compress(words), dtype=np.uint32)
    idx = _select.index_of(st)
    fills = np.flatnonzero(st[idx[seg]: idx[seg + 1]] & np.uint32(up.FILL0)) + idx[seg]
    bad = st.copy()
    bad[fills[fills.size // 2]] += 1
    return bad, idx


def test_a_malformed_then_segment_is_refused_only_where_the_mask_selects(wah, oracle):
    n = 2 * SEG_WORDS
    then, else_ = up.clustered_words(n, 110), up.random_words(n, 0.5, 109)
    bad = _broken(oracle, then, 1)
    in_both = up.random_words(n, 0.2, 111)
    in_first = in_both.copy()
    in_first[SEG_WORDS:] = 0
    reads = up.Case("selects a row of segment 1", n, 32 * n, in_both, [else_], [then])
    stays = up.Case("selects rows of segment 0 only", n, 32 * n, in_first, [else_], [then])
    clipped = up.Case("rows of segment 0 only", n, SEG_BITS - 5, in_both, [else_], [then])
    assert _status(wah, reads, Operands(wah, oracle, reads, streams={("then", 0): bad}))[0] == WAH_ERR_STREAM
    for case in (stays, clipped):  # a mask segment of zeros, and one whose set bits lie behind n_rows: the then segment is not read
        _check(case, _run(wah, case, Operands(wah, oracle, case, streams={("then", 0): bad})), up.reference(oracle, case))
    _check(reads, _run(wah, reads, Operands(wah, oracle, reads)), up.reference(oracle, reads))


def test_a_malformed_else_segment_is_always_refused(wah, oracle):
    n = 2 * SEG_WORDS
    else_ = up.clustered_words(n, 112)
    in_first = up.random_words(n, 0.2, 113)
    in_first[SEG_WORDS:] = 0
    case = up.Case("selects rows of segment 0 only", n, 32 * n, in_first, [else_], [1])
    assert _status(wah, case, Operands(wah, oracle, case, streams={("else", 0): _broken(oracle, else_, 1)}))[0] == WAH_ERR_STREAM
    assert _status(wah, case, Operands(wah, oracle, case))[0] == WAH_OK


def test_a_malformed_mask_segment_is_refused_whatever_it_selects(wah, oracle):
    """The mask is checked in every segment: a broken fill in a segment behind n_rows, which selects nothing, is refused."""
    n = 2 * SEG_WORDS
    mask = up.clustered_words(n, 114)
    case = up.Case("rows of segment 0 only", n, SEG_BITS - 5, mask, [up.random_words(n, 0.5, 115)], [0])
    ops = Operands(wah, oracle, case)
    _check(case, _run(wah, case, ops), up.reference(oracle, case))
    bad, idx = _broken(oracle, mask, 1)
    assert _status(wah, case, ops, mask=wah.bitop_operand_table([(_dev(bad), _dev64(idx))]))[0] == WAH_ERR_STREAM


def test_entries_that_are_neither_streams_nor_constants_are_refused(wah, oracle):
    """A half-null entry on either side, a constant with stream_words == 2 on either side, and a constant mask."""
    case = up.constants("then", n_rows=SEG_BITS)
    ops = Operands(wah, oracle, case)
    assert _status(wah, case, ops)[0] == WAH_OK

    def edited(side, row, column, value):
        tables = {s: t.clone() for s, t in ops.tables.items()}
        tables[side][row, column] = value
        return tables

    assert _status(wah, case, ops, tables=edited("else", 1, 0, 0))[0] == WAH_ERR_STREAM  # the stream pointer null, the index not
    assert _status(wah, case, ops, tables=edited("else", 1, 2, 0))[0] == WAH_ERR_STREAM  # the index pointer null, the stream not
    assert _status(wah, case, ops, tables=edited("then", 0, 0, ops.mask_pair[0].data_ptr()))[0] == WAH_ERR_STREAM
    assert _status(wah, case, ops, tables=edited("then", 1, 2, ops.mask_pair[1].data_ptr()))[0] == WAH_ERR_STREAM
    assert _status(wah, case, ops, tables=edited("then", 1, 1, 2))[0] == WAH_ERR_STREAM  # a constant of "2"
    both = up.constants("both")
    ops_both = Operands(wah, oracle, both)
    tables = {s: t.clone() for s, t in ops_both.tables.items()}
    tables["else"][3, 1] = 2
    assert _status(wah, both, ops_both, tables=tables)[0] == WAH_ERR_STREAM
    for bit in (0, 1):
        assert _status(wah, case, ops, mask=wah.update_operand_table([bit], device="cuda"))[0] == WAH_ERR_STREAM  # a constant mask


# ---- more than 2^32 rows -----------------------------------------------------------------------------------------------------------
def test_rows_beyond_2_32(wah, oracle):
    """Size A of tests/_long.py (4.3e9 rows, compressed only): a mask of ones fills with live segments, a row limit five rows
    behind 2^32, a then side of streams and of the constant 1.  Expected: the segment-sparse row-wise model."""
    import torch

    a = lg.A_SEGMENTS
    n = a * SEG_WORDS
    n_rows = 2**32 + 5
    mask = lg.marked(a, lg.A_NAMED, lg.A_ROWS, 601, default=1)
    else_ = [lg.marked(a, lg.A_NAMED, lg.A_ROWS, 602), lg.marked(a, lg.A_NAMED, (), 603, default=1)]
    then = lg.marked(a, lg.A_NAMED, (), 604, default=1, density=0.1)
    limit = lg.below(a, n_rows)
    want = [lg.rowwise(lambda r: [np.where(r[0] & r[1], r[3], r[2])], [mask, limit, else_[0], then])[0],
            lg.rowwise(lambda r: [np.where(r[0] & r[1], 1, r[2])], [mask, limit, else_[1]])[0]]
    want_stream, want_index = lg.expected_streams(oracle, want)
    assert mask.bit(2**32) == 1 and want[1].bit(2**32) == 1 and want[0].bit(2**32) == then.bit(2**32)  # the last rows below the limit
    assert want[1].bit(n_rows) == else_[1].bit(n_rows) and want[0].bit(lg.A_ROWS[-1]) == 1                # ... and rows behind it

    pairs = [tuple(f(x) for f, x in zip((_dev, _dev64), b.stream_index(oracle))) for b in [mask] + else_ + [then]]
    source_words = sum(int(p[0].numel()) for p in pairs[1:])
    cap = wah.update_max_words(n, 2, int(pairs[0][0].numel()), source_words)
    assert want_stream.size <= cap
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    stream, offs = wah.update_device(pairs[0], pairs[1:3], [pairs[3], 1], n, n_rows, out=buf[:cap])
    assert int(buf[cap].item()) == GUARD
    assert stream.numel() == want_stream.size and torch.equal(offs, _dev64(want_index))
    assert torch.equal(stream, _dev(want_stream))


# ---- the front ends ----------------------------------------------------------------------------------------------------------------
N_ROWS = SEG_BITS + 9001  # two segments, the last one ragged in rows


def _same_index(got, want):
    """Word for word and entry for entry."""
    import torch

    assert tuple(got[2:]) == tuple(want[2:]), (got[2:], want[2:])
    assert got[0].numel() == want[0].numel() and torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1])


def _bsi(wah, values, n_bits, exists=None):
    import torch

    return wah.columns.bsi_from_values(wah, _dev64(values), n_bits, exists=None if exists is None else torch.from_numpy(exists).cuda())


@pytest.mark.parametrize("has_exists", (False, True))
def test_set_values_where(wah, has_exists):
    n_bits = 12
    rng = np.random.default_rng(91)
    values = rng.integers(0, 1 << n_bits, N_ROWS)
    exists = rng.random(N_ROWS) < 0.8 if has_exists else None
    bsi = _bsi(wah, values, n_bits, exists)
    lo, hi = 1000, 1700
    mask = wah.columns.range_column(wah, bsi, lo, hi)
    sel = (values >= lo) & (values <= hi) & (exists if has_exists else True)
    more = rng.random(N_ROWS) < 0.3  # a mask that also selects rows without a value: they get one
    mask2 = wah.columns.bitmaps_from_rows(wah, [_dev64(np.flatnonzero(more))], bsi[2])
    for m, chosen in ((mask, sel), (mask2[:2], more)):
        for value in (0, 5, (1 << n_bits) - 1, 0b101010101010):
            got = wah.columns.set_values_where(wah, bsi, m, N_ROWS, value)
            have = None if exists is None else exists | chosen
            stored = np.where(chosen, value, values)
            _same_index(got, _bsi(wah, stored if have is None else np.where(have, stored, 0), n_bits, have))
    if has_exists:  # NULL: the rows lose their value
        got = wah.columns.set_values_where(wah, bsi, mask2[:2], N_ROWS, None)
        have = exists & ~more
        _same_index(got, _bsi(wah, np.where(have, values, 0), n_bits, have))
    # rows at or behind n_rows are not updated
    got = wah.columns.set_values_where(wah, bsi, mask2[:2], 20000, 7)
    chosen = more & (np.arange(N_ROWS) < 20000)
    have = None if exists is None else exists | chosen
    stored = np.where(chosen, 7, values)
    _same_index(got, _bsi(wah, stored if have is None else np.where(have, stored, 0), n_bits, have))


def test_update_rows_and_choose_columns(wah):
    rng = np.random.default_rng(92)
    a, b = rng.integers(0, 1 << 10, N_ROWS), rng.integers(0, 1 << 10, N_ROWS)
    xa, xb = rng.random(N_ROWS) < 0.9, rng.random(N_ROWS) < 0.7
    pick = rng.random(N_ROWS) < 0.4
    mask = wah.columns.bitmaps_from_rows(wah, [_dev64(np.flatnonzero(pick))], -(-N_ROWS // SEG_BITS) * SEG_WORDS)[:2]
    bsi_a, bsi_b = _bsi(wah, np.where(xa, a, 0), 10, xa), _bsi(wah, np.where(xb, b, 0), 10, xb)
    have = np.where(pick, xb, xa)
    merged = _bsi(wah, np.where(have, np.where(pick, b, a), 0), 10, have)
    _same_index(wah.columns.update_rows(wah, bsi_a, mask, N_ROWS, bsi_b), merged)
    _same_index(wah.columns.choose_columns(wah, mask, bsi_b, bsi_a, N_ROWS), merged)
    # different widths, one existence slice, a width of the caller's: the missing slices are zeros, the missing existence ones
    narrow = rng.integers(0, 1 << 6, N_ROWS)
    bsi_n = _bsi(wah, narrow, 6)
    for n_bits in (None, 13):
        got = wah.columns.choose_columns(wah, mask, bsi_n, bsi_a, N_ROWS, n_bits=n_bits)
        have = np.where(pick, True, xa)
        _same_index(got, _bsi(wah, np.where(have, np.where(pick, narrow, a), 0), n_bits or 10, have))
    # the else side without an existence slice has a value in EVERY position of its columns, those behind the table's rows too
    got = wah.columns.choose_columns(wah, mask, bsi_a, bsi_n, N_ROWS)
    behind = 32 * bsi_a[2] - N_ROWS
    have = np.concatenate([np.where(pick, xa, True), np.ones(behind, bool)])
    stored = np.concatenate([np.where(pick, a, narrow), np.zeros(behind, np.int64)])
    _same_index(got, _bsi(wah, np.where(have, stored, 0), 10, have))
    plain = _bsi(wah, b, 10)
    _same_index(wah.columns.choose_columns(wah, mask, bsi_n, plain, N_ROWS), _bsi(wah, np.where(pick, narrow, b), 10))
    # an equality-encoded index
    keys, other = rng.integers(0, 7, N_ROWS), rng.integers(0, 7, N_ROWS)
    index, source = wah.columns.index_from_keys(wah, _dev64(keys), 7), wah.columns.index_from_keys(wah, _dev64(other), 7)
    _same_index(wah.columns.update_rows(wah, index, mask, N_ROWS, source), wah.columns.index_from_keys(wah, _dev64(np.where(pick, other, keys)), 7))


def test_set_keys_where(wah):
    rng = np.random.default_rng(93)
    keys, other = rng.integers(0, 7, N_ROWS), rng.integers(0, 5, N_ROWS)
    index, filt = wah.columns.index_from_keys(wah, _dev64(keys), 7), wah.columns.index_from_keys(wah, _dev64(other), 5)
    for negate in (False, True):  # a NOT IN mask has every position behind the table's rows set: n_rows keeps them out
        mask = wah.columns.filter_columns(wah, [(filt[0], filt[1], [1, 3], negate)], index[2])
        sel = np.isin(other, [1, 3]) != negate
        for key in (0, 4, 6):
            got = wah.columns.set_keys_where(wah, index, mask, N_ROWS, key)
            _same_index(got, wah.columns.index_from_keys(wah, _dev64(np.where(sel, key, keys)), 7))
            counts = wah.columns.count_columns(wah, *got, list(range(7))).cpu().numpy()
            assert int(counts.sum()) == N_ROWS  # every row in exactly one column


def test_greatest_and_least_columns(wah):
    rng = np.random.default_rng(94)
    a, b = rng.integers(0, 1 << 9, N_ROWS), rng.integers(0, 1 << 12, N_ROWS)
    b[::3] = a[::3]  # ties
    bsi_a, bsi_b = _bsi(wah, a, 9), _bsi(wah, b, 12)
    _same_index(wah.columns.greatest_columns(wah, bsi_a, bsi_b, N_ROWS), _bsi(wah, np.maximum(a, b), 12))
    _same_index(wah.columns.least_columns(wah, bsi_a, bsi_b, N_ROWS), _bsi(wah, np.minimum(a, b), 12))
    _same_index(wah.columns.greatest_columns(wah, bsi_b, bsi_a, N_ROWS), _bsi(wah, np.maximum(a, b), 12))


class Chain:
    """range -> set_values_where -> count as three calls that are only enqueued, every buffer made beforehand and every table
    filled beforehand: what a captured graph needs, and what reads nothing back.  The count is over every slice of the updated
    attribute: the number of rows that hold each bit."""

    def __init__(self, wah, seed):
        import torch

        self.wah, self.n_bits = wah, 10
        rng = np.random.default_rng(seed)
        self.values = rng.integers(0, 1 << self.n_bits, N_ROWS)
        self.bsi = wah.columns.bsi_from_values(wah, _dev64(self.values), self.n_bits)
        n, k = self.bsi[2], self.n_bits
        self.n, self.k = n, k
        lib = wah.lib()

        def bytes_(size):
            return torch.empty(int(size), dtype=torch.uint8, device="cuda")

        def words(count):
            return torch.full((int(count),), GUARD, dtype=torch.int32, device="cuda")

        def index(entries):
            return torch.zeros(int(entries), dtype=torch.int64, device="cuda")

        segs = n // SEG_WORDS
        self.slices = wah.columns.column_operand_table(self.bsi[0], self.bsi[1], n, list(range(k)))
        self.bounds = wah.bsi_bounds(0, 0, "cuda")
        self.range_reuse = dict(scratch=bytes_(lib.wah_bsi_range_scratch_bytes(n, k)), out=words(wah.max_compressed_words(n)), out_offsets=index(segs + 1))
        self.mask = wah.bitop_operand_table([(self.range_reuse["out"], self.range_reuse["out_offsets"])])
        self.then = wah.update_operand_table([0] * k, device="cuda")
        self.set_reuse = dict(scratch=bytes_(lib.wah_update_scratch_bytes(n, k)), out=words(k * wah.max_compressed_words(n)), out_offsets=index(k * segs + 1))
        self.count_table = wah.columns.column_operand_table(self.set_reuse["out"], self.set_reuse["out_offsets"], n, list(range(k)))
        self.count_reuse = dict(scratch=bytes_(lib.wah_select_scratch_bytes(n, k)), counts=index(k))
        self.write(300, 800, 5)

    def write(self, lo, hi, value):
        """The bounds and the then table overwritten in place."""
        self.wah.bsi_bounds(lo, hi, "cuda", out=self.bounds)
        bits = [(value >> (self.n_bits - 1 - i)) & 1 for i in range(self.n_bits)]
        self.then.copy_(self.wah.update_operand_table(bits, device="cuda"))
        self.lo, self.hi, self.value = lo, hi, value

    def enqueue(self):
        wah, n = self.wah, self.n
        wah.bsi_range_device(self.slices, self.bounds, n, exists=False, check=False, **self.range_reuse)
        wah.update_device(self.mask, self.slices, self.then, n, N_ROWS, check=False, **self.set_reuse)
        wah.count_device(self.count_table, n, check=False, **self.count_reuse)

    def verify(self):
        lib, n = self.wah.lib(), self.n
        assert lib.wah_bsi_range_status(self.range_reuse["scratch"].data_ptr(), n, self.k, None) == WAH_OK
        assert lib.wah_update_status(self.set_reuse["scratch"].data_ptr(), None) == WAH_OK
        assert lib.wah_select_status(self.count_reuse["scratch"].data_ptr(), None) == WAH_OK
        new = np.where((self.values >= self.lo) & (self.values <= self.hi), self.value, self.values)
        want = [int(((new >> (self.n_bits - 1 - i)) & 1).sum()) for i in range(self.n_bits)]
        assert self.count_reuse["counts"].cpu().tolist() == want, (self.lo, self.hi, self.value)


def test_a_chain_of_calls_with_nothing_read_back(wah):
    """range_column -> set_values_where -> count_columns through the front ends, every one with check=False: the statuses and the
    answer are read once, at the end."""
    import torch

    chain = Chain(wah, 95)
    out, _, out_offsets = wah.columns.range_column(wah, chain.bsi, 100, 400, check=False, **chain.range_reuse)
    got = wah.columns.set_values_where(wah, chain.bsi, (out, out_offsets), N_ROWS, 777, check=False, **chain.set_reuse)
    assert got[2:] == (chain.n, chain.n_bits, False) and got[0] is chain.set_reuse["out"]
    counts = wah.columns.count_columns(wah, *got[:3], list(range(chain.k)), check=False, **chain.count_reuse)
    torch.cuda.synchronize()
    chain.lo, chain.hi, chain.value = 100, 400, 777
    chain.verify()
    assert counts is chain.count_reuse["counts"]


def test_the_chain_as_one_graph_replayed_over_rewritten_bounds_and_values(wah):
    """The mask and the tables are only ever read by the device: ONE captured chain, replayed after the bounds and the then table
    were overwritten in place, applies the new update (capture as tests/test_gpu_compact.py: side stream, warm-up outside,
    check=False; one chain of launches, no parallel branches)."""
    import torch

    chain = Chain(wah, 96)
    chain.enqueue()  # warm-up outside the capture
    torch.cuda.synchronize()
    chain.verify()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            chain.enqueue()
    for lo, hi, value in ((0, 1023, 1023), (500, 501, 0), (200, 900, 0b1010101010)):
        chain.write(lo, hi, value)
        chain.set_reuse["out"].fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        chain.verify()
