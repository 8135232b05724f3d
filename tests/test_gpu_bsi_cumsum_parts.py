"""GPU tests of wah_bsi_cumsum_parts_indexed_device: the running sum of a bit-sliced value that starts again at every row of a starts
bitmap, as a new bit-sliced attribute in one call (include/wah.h), and its front ends in api.py and columns.py.  Everything is exact:
the result's words, their count and its whole segment index against the oracle's compress() of the slice matrix that numpy builds
FROM THE VALUES, the unpacked bitmaps and the starts (tests/_cumsum_parts.py); tests/test_cumsum_parts_reference.py proves that
model against a restatement of the kernels' steps and that every wrong model is caught.  Outputs and scratch are poisoned and have a
guard behind them.

The named cases run at 992, 2 * 992 and 3 * 992 words -- one, two and three segments; 513 segments are one more than the grid has
workgroups; 8194 segments are two more than one round of the scan, with starts in the last four; the bitmap of more than 2^32 rows
and the 8194 segments are expected from tests/_long.py's run model."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _cumsum as cs, _cumsum_parts as cp, _foreign as fg, _long as lg
from tests.test_gpu_bsi_arith import Streams, _dev, _dev_values, _host

pytestmark = pytest.mark.gpu

WAH_ERR_STREAM = -6
SEG = 992
GUARD = 0x5A5A5A5A
POISON = 0xA5


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


@pytest.fixture(scope="module")
def cases():
    return cp.named_cases()


def _flags(wah, case):
    return ((wah.BSI_EXISTS if case["exists"] is not None else 0) | (wah.CUMSUM_EXCLUSIVE if case["exclusive"] else 0) |
            (wah.CUMSUM_ALL_ROWS if case["all_rows"] else 0))


def _operands(wah, case):
    """(value rows, filter rows, the starts row) as indexed compressed bitmaps."""
    streams = Streams(wah, case["n"])
    val = []
    if case["kv"]:
        val = [streams.of(row) for row in _bsi.build_slices(case["values"], case["kv"], case["exists"], zero_missing=True)]
    elif case["exists"] is not None:
        val = [streams.of(_bsi.pack_bits(case["exists"]))]
    return val, [streams.of(_bsi.pack_bits(f)) for f in case["filters"]], streams.of(_bsi.pack_bits(case["starts"]))


def _call(wah, case, val, filters, starts, check=True, scratch=None, plain=False):
    """The call into poisoned outputs and a poisoned scratch with a guard behind each; returns what bsi_cumsum_parts_device returns
    (plain: the call without partitions, for the comparison word for word)."""
    import torch

    n, rows_out = case["n"], cs.rows_out(case)
    cap, entries = wah.max_compressed_words(rows_out * n), rows_out * (n // SEG) + 1
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    offs = torch.full((entries + 1,), -1, dtype=torch.int64, device="cuda")
    size = wah.lib().wah_bsi_cumsum_scratch_bytes if plain else wah.lib().wah_bsi_cumsum_parts_scratch_bytes
    need = int(size(n, case["k_out"], _flags(wah, case)))
    if scratch is None:
        scratch = torch.full((need + 256,), POISON, dtype=torch.uint8, device="cuda")
    val, filters = (None if isinstance(x, list) and not x else x for x in (val, filters))
    kw = dict(filters=filters, exists=case["exists"] is not None, exclusive=case["exclusive"], all_rows=case["all_rows"], scratch=scratch[:need],
              out=buf[:cap], out_offsets=offs[:entries], check=check)
    if plain:
        got = wah.bsi_cumsum_device(val, n, case["n_rows"], case["kv"], case["k_out"], **kw)
    else:
        got = wah.bsi_cumsum_parts_device(val, n, case["n_rows"], case["kv"], case["k_out"], starts, **kw)
    torch.cuda.synchronize()
    assert int(buf[cap].item()) == GUARD and int(offs[entries].item()) == -1, "guard"
    assert scratch.numel() == need or bool((scratch[need:] == POISON).all()), "scratch guard"
    return got


def _same(oracle, got, offs, matrix, what):
    """(got, offs) is, word for word, compress(matrix as one bitmap) and its whole segment index."""
    want, index = cs.compressed(oracle, matrix)
    assert got.numel() == want.size, (what, got.numel(), want.size)
    assert np.array_equal(_host(got), want), what
    assert offs.numel() == index.size and np.array_equal(offs.cpu().numpy(), index), what


def _run(wah, oracle, case, what, tables=None):
    want = cp.expected(case)
    operands = _operands(wah, case) if tables is None else None  # (kept until the call is done: a table holds raw pointers)
    val, filters, starts = operands if tables is None else tables
    got, offs = _call(wah, case, val, filters, starts)
    del operands
    _same(oracle, got, offs, want, what)


# ---- 1: the named cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cp.named_cases()))
def test_named_case_vs_value_model(wah, oracle, cases, name):
    _run(wah, oracle, cases[name], name)


@pytest.mark.parametrize("name", ("no start, 1 segments", "no start, 2 segments", "no start, 3 segments", "widths 27 x 64", "widths 0 x 33"))
def test_without_a_start_the_plain_call_word_for_word(wah, cases, name):
    import torch

    case = dict(cases[name], starts=np.zeros(32 * cases[name]["n"], bool))
    val, filters, starts = _operands(wah, case)
    got, offs = _call(wah, case, val, filters, starts)
    want, want_offs = _call(wah, case, val, filters, None, plain=True)
    assert torch.equal(got, want) and torch.equal(offs, want_offs)


def test_the_starts_as_a_table_and_as_a_pair(wah, oracle, cases):
    case = cases["two starts in a step"]
    val, filters, starts = _operands(wah, case)
    _run(wah, oracle, case, "table", tables=(val, filters, wah.bitop_operand_table([starts])))
    _run(wah, oracle, case, "pair", tables=(wah.bitop_operand_table(val), wah.bitop_operand_table(filters), starts))


def test_one_segment_more_than_the_grid(wah, oracle):
    """513 segments, a 1-slice value under one filter and a 2-bit result: the first workgroup takes a second segment, and the scan of
    the records has 513 entries; a partition of every length from a few rows to a few segments."""
    n = (cs.GRID_ITEMS + 1) * SEG
    rng = np.random.default_rng(513)
    rows = 32 * n
    values = (rng.random(rows) < 0.5).astype(np.uint64)
    starts = np.zeros(rows, bool)
    starts[rng.integers(0, rows, 300)] = True
    starts[40 * cs.SEG_BITS: 45 * cs.SEG_BITS] = False       # a carry over five segments
    starts[[511 * cs.SEG_BITS + 9, 512 * cs.SEG_BITS, rows - 1]] = True
    case = cp.make_case(n, 1, 2, starts, n_rows=rows - 3, n_filters=1, values=values)
    _run(wah, oracle, case, "513 segments")


# ---- 2: long bitmaps, expected from the run model --------------------------------------------------------------------------------------
def _long_run(wah, oracle, filt, starts, n_rows):
    """The call on long bitmaps against tests/_cumsum_parts.py's long_expected (its docstring says what the operands are), the
    expected stream assembled on the device."""
    import torch

    a = filt.n_segments
    n = a * SEG
    want, want_index, incoming = cp.long_expected(oracle, filt, starts, n_rows, empty=lambda total: torch.empty(total, dtype=torch.int32, device="cuda"),
                                                  put=lambda words: torch.from_numpy(np.ascontiguousarray(words)).cuda())
    total = int(want_index[-1])
    tables = []
    for bitmap in (filt, starts):
        stream, index = bitmap.stream_index(oracle)
        tables.append((_dev(stream), torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).cuda()))
    cap = total + 64
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    offs = torch.full((2 * a + 2,), -1, dtype=torch.int64, device="cuda")
    got, got_offs = wah.bsi_cumsum_parts_device(None, n, n_rows, 0, 2, tables[1], filters=[tables[0]], all_rows=True, out=buf[:cap],
                                                out_offsets=offs[: 2 * a + 1])
    assert int(buf[cap].item()) == GUARD and int(offs[2 * a + 1].item()) == -1
    assert got.numel() == total
    assert torch.equal(got_offs, torch.from_numpy(want_index).cuda())
    assert torch.equal(got, want)
    return incoming


def test_the_scan_carries_a_pair_over_its_round_seam(wah, oracle):
    """8194 segments, two more than a round of the scan has entries, with starts in segments 17 and 8190 to 8193: what flows into
    segments 8192 and 8193 is folded from the carry of round 0, a pair whose flag is set and whose sum is segment 8191's tail."""
    a = 8194
    named = (0, 17, 8190, 8191, 8192, 8193)
    filt = lg.marked(a, named, (0,), 43, default=1)
    at = [17 * lg.SEG_BITS + 5, 8190 * lg.SEG_BITS + 300, 8190 * lg.SEG_BITS + 20000, 8191 * lg.SEG_BITS + 31743, 8192 * lg.SEG_BITS, 8193 * lg.SEG_BITS + 64]
    incoming = _long_run(wah, oracle, filt, lg.from_rows(a, at), a * lg.SEG_BITS - 70)
    assert incoming[8190] > 8000 * lg.SEG_BITS and incoming[8192] <= 1 and 0 < incoming[8193] <= lg.SEG_BITS


def test_a_bitmap_of_more_than_2_32_rows(wah, oracle):
    """135 400 segments (4.298e9 rows) and starts at row 5, behind row 2^32 and in the last segment, in front of n_rows and behind
    it: segment numbers, row numbers, the matrix's word offsets and the clip pass 2^32, the count that flows in passes 2^32 in
    front of the start and begins again behind it."""
    a = lg.A_SEGMENTS
    n_rows = a * lg.SEG_BITS - 11
    start = 2**32 + 2
    assert start // lg.SEG_BITS in lg.A_NAMED and a - 1 in lg.A_NAMED
    filt = lg.marked(a, lg.A_NAMED, lg.A_ROWS, 41, default=1)
    at = [5, start, n_rows - 1000, n_rows, n_rows + 3]
    incoming = _long_run(wah, oracle, filt, lg.from_rows(a, at), n_rows)
    cut = start // lg.SEG_BITS
    assert incoming[cut] > 2**32 - 6 * lg.SEG_BITS and incoming[cut + 1] <= lg.SEG_BITS and incoming[a - 1] > (a - cut - 3) * lg.SEG_BITS


# ---- 3: foreign streams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", range(len(fg.WAYS) - 1))
def test_every_operand_in_every_reencoding(wah, oracle, first):
    """The value's slices, its existence row, two filters and the starts row written in every way of tests/_foreign.py that compress()
    never emits, the ways rotating over the nine table rows and `first` over the ways: every row, the starts row too, is seen in
    every way; the result is the canonical one."""
    n, kv = 2 * SEG, 5
    rng = np.random.default_rng(12)
    rows = 32 * n
    values = _bsi.make_values("clustered", rng, rows, kv)
    exists = np.repeat(rng.random(rows // 992 + 1) < 0.8, 992)[:rows]  # runs: the existence row has fills too
    filters = [np.repeat(rng.random(rows // 500 + 1) < 0.7, 500)[:rows], rng.random(rows) < 0.8]
    starts = rng.random(rows) < 1 / 2000
    starts[3000:9000] = True   # fills of ones
    starts[9000:9100] = rng.random(100) < 0.5
    case = cp.make_case(n, kv, 20, starts, n_rows=rows - 100, values=values, filters=filters)
    case["exists"] = exists
    matrix = np.concatenate([_bsi.build_slices(values, kv, exists, zero_missing=True), np.stack([_bsi.pack_bits(f) for f in filters]),
                             _bsi.pack_bits(starts)[None]])
    ways = fg.WAYS[1:]
    foreign = fg.rows_foreign(matrix, n, np.random.default_rng(3), first=first)
    assert len(foreign) == kv + 4 and foreign[-1][0] == ways[(first + kv + 3) % len(ways)]
    operands = []
    for way, stream in foreign:
        assert np.array_equal(oracle.decompress(stream)[:n], matrix[len(operands)]), way
        d = _dev(stream)
        offs, _ = wah.build_index_device(d)
        operands.append((d, offs))
    _run(wah, oracle, case, ("foreign", first), tables=(operands[: kv + 1], operands[kv + 1: kv + 3], operands[kv + 3]))


def test_the_foreign_ways_reach_the_starts_row():
    ways = fg.WAYS[1:]
    assert {ways[(first + 8) % len(ways)] for first in range(len(ways))} == set(ways) == set(fg.ways_for(2 * SEG)[1:])


# ---- 4: what only the device sees -----------------------------------------------------------------------------------------------------
def _status(wah, case, val, filters, starts):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    flags = _flags(wah, case)
    sc = torch.empty(int(wah.lib().wah_bsi_cumsum_parts_scratch_bytes(case["n"], case["k_out"], flags)), dtype=torch.uint8, device="cuda")
    _call(wah, case, val, filters, starts, check=False, scratch=sc)
    return int(wah.lib().wah_bsi_cumsum_parts_status(sc.data_ptr(), case["n"], case["k_out"], flags, None))


def test_a_bad_starts_stream_is_refused_by_the_status_call_only(wah):
    runs = np.repeat(np.random.default_rng(2).random(32 * 2 * SEG // 992) < 0.3, 992)
    case = cp.make_case(2 * SEG, 12, 28, runs, with_exists=True, n_filters=2, seed=9)
    val, filters, starts = _operands(wah, case)
    val_table, filter_table, starts_table = wah.bitop_operand_table(val), wah.bitop_operand_table(filters), wah.bitop_operand_table([starts])
    assert _status(wah, case, val_table, filter_table, starts_table) == 0
    for col in (0, 2):  # a starts row without a stream, or without an index
        bad = starts_table.clone()
        bad[0, col] = 0
        assert _status(wah, case, val_table, filter_table, bad) == WAH_ERR_STREAM, col
    bad = val_table.clone()
    bad[5, 2] = 0
    assert _status(wah, case, bad, filter_table, starts_table) == WAH_ERR_STREAM
    bad = filter_table.clone()
    bad[1, 0] = 0
    assert _status(wah, case, val_table, bad, starts_table) == WAH_ERR_STREAM
    with pytest.raises(wah.WahError):
        bad = starts_table.clone()
        bad[0, 2] = 0
        _call(wah, case, val_table, filter_table, bad)
    # a fill of the starts row one group shorter: the segment's groups do not add up
    words = _host(starts[0]).copy()
    fills = np.flatnonzero((words >> 31 == 1) & ((words & 0x3FFFFFFF) >= 2))
    assert fills.size
    words[int(fills[-1])] -= 1  # (in the last segment: every segment of the row is walked)
    assert _status(wah, case, val, filters, (_dev(words), starts[1])) == WAH_ERR_STREAM
    assert _status(wah, case, val, filters, starts) == 0


def test_front_end_refuses_bad_arguments(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    pair = (stream, offs)
    with pytest.raises(wah.WahError):
        wah.bsi_cumsum_parts_device([pair] * 33, SEG, 0, 33, 40, pair)
    with pytest.raises(wah.WahError):
        wah.bsi_cumsum_parts_device([pair] * 3, SEG, 0, 3, 65, pair)
    with pytest.raises(wah.WahError):
        wah.bsi_cumsum_parts_device([pair] * 3, SEG + 1, 0, 3, 8, pair)
    with pytest.raises(wah.WahError):
        wah.bsi_cumsum_parts_device([pair] * 3, SEG, 0, 2, 8, pair)  # a table that does not go with the width
    with pytest.raises(wah.WahError):
        wah.bsi_cumsum_parts_device([pair] * 3, SEG, 0, 3, 8, [pair, pair])  # two starts rows
    with pytest.raises(ValueError):
        wah.columns.cumsum_column_by(wah, (stream, offs, SEG, 33, False), 0, pair)
    with pytest.raises(ValueError):
        wah.columns.cumsum_column_by(wah, (stream, offs, SEG, 8, False), 0, pair, n_bits=65)
    with pytest.raises(ValueError):
        wah.columns.partition_starts(wah, (stream, offs, SEG, 8, True), 5)


# ---- 5: the front ends ----------------------------------------------------------------------------------------------------------------
def _clustered_key(rng, rows, n_keys, mean_run):
    """A key column clustered by key: runs of random lengths, neighbouring runs of different keys."""
    lengths = rng.geometric(1.0 / mean_run, rows // mean_run + 64)
    keys = rng.integers(0, n_keys - 1, lengths.size)
    keys[1:] = np.where(keys[1:] == keys[:-1], n_keys - 1, keys[1:])  # (n_keys - 1 never drawn: a neighbour's stand-in)
    return np.repeat(keys, lengths)[:rows].astype(np.uint64)


@pytest.fixture(scope="module")
def table(wah):
    """A table of 2 * 992 * 32 - 50 rows clustered by a 6-bit key, with a 9-bit quantity (an existence bitmap), a 32-bit amount and
    two filter bitmaps."""
    import torch

    n = 2 * SEG
    rows = 32 * n - 50
    rng = np.random.default_rng(2026)
    key = _clustered_key(rng, rows, 64, 700)
    qty, amount = _bsi.uniform_values(rng, rows, 9), _bsi.uniform_values(rng, rows, 32)
    qty_exists = rng.random(rows) < 0.9
    f = [rng.random(rows) < 0.7, np.repeat(rng.random(rows // 300 + 1) < 0.6, 300)[:rows]]
    streams = Streams(wah, n)

    def padded(a, dtype):
        out = np.zeros(32 * n, dtype)
        out[: a.size] = a
        return out

    starts = np.zeros(rows, bool)
    starts[1:] = key[1:] != key[:-1]
    return dict(n=n, rows=rows, key=key, starts=starts, qty=qty, amount=amount, qty_exists=qty_exists, f=f,
                d_key=wah.columns.bsi_from_values(wah, _dev_values(key), 6, n_words_per_column=n),
                d_qty=wah.columns.bsi_from_values(wah, _dev_values(qty), 9, n_words_per_column=n, exists=torch.from_numpy(qty_exists).cuda()),
                d_amount=wah.columns.bsi_from_values(wah, _dev_values(amount), 32, n_words_per_column=n),
                d_f=[streams.of(_bsi.pack_bits(padded(x, bool))) for x in f],
                d_starts=streams.of(_bsi.pack_bits(padded(starts, bool))))


def _np_cumsum_by(values, mask, starts, exclusive=False):
    """The segmented running sum of the masked values, uint64."""
    x = np.where(mask, values, np.uint64(0)).astype(np.uint64)
    run = np.cumsum(x, dtype=np.uint64)
    last = np.maximum.accumulate(np.where(starts, np.arange(x.size), 0))
    run = run - np.where(np.cumsum(starts) > 0, (run - x)[last], np.uint64(0))
    return run - x if exclusive else run


def _decoded(wah, pair, n):
    return _bsi.unpack_bits(_host(wah.decompress_segments_device(pair[0], pair[1], n))[:n])


def test_partition_starts_on_a_clustered_key(wah, table):
    t = table
    assert 50 < t["starts"].sum() < 500
    got = wah.columns.partition_starts(wah, t["d_key"], t["rows"])
    bits = _decoded(wah, got, t["n"])
    assert np.array_equal(bits[: t["rows"]], t["starts"]) and not bits[t["rows"]:].any() and not bits[0]
    # fewer rows than the key's columns hold: the rows in front of n_rows are right, and what the columns hold behind them does
    # not matter to a call with the same n_rows
    cut = int(np.flatnonzero(t["starts"])[7])
    some = wah.columns.partition_starts(wah, t["d_key"], cut)
    assert np.array_equal(_decoded(wah, some, t["n"])[:cut], t["starts"][:cut])
    values, have = wah.columns.values_of_column(wah, wah.columns.row_numbers_by(wah, some, t["n"], cut), 0, t["rows"])
    want = np.zeros(t["rows"], np.uint64)
    want[:cut] = _np_cumsum_by(np.ones(cut, np.uint64), np.ones(cut, bool), t["starts"][:cut])
    assert np.array_equal(values.cpu().numpy().view(np.uint64), want) and np.array_equal(have.cpu().numpy(), np.arange(t["rows"]) < cut)
    assert not _decoded(wah, wah.columns.partition_starts(wah, t["d_key"], 1), t["n"])[0]  # one row: no start


def test_cumsum_column_by_against_numpy(wah, table):
    t = table
    n, rows, starts = t["n"], t["rows"], t["starts"]
    # SUM(qty) OVER (PARTITION BY key ORDER BY rowid) WHERE f0 AND f1, the attribute's own existence bitmap in the selection
    mask = t["qty_exists"] & t["f"][0] & t["f"][1]
    total = wah.columns.cumsum_column_by(wah, t["d_qty"], rows, t["d_starts"], where=t["d_f"])
    assert total[2:] == (n, 9 + rows.bit_length(), True)
    values, have = wah.columns.values_of_column(wah, total, 0, rows)
    assert np.array_equal(have.cpu().numpy(), mask)
    want = _np_cumsum_by(t["qty"], mask, starts)
    assert np.array_equal(values.cpu().numpy().view(np.uint64), np.where(mask, want, 0))
    assert int(want.max()) < int(np.cumsum(np.where(mask, t["qty"], 0)).max()) // 10  # (the partitions matter)
    values, have = wah.columns.values_of_column(wah, total, rows, 50)
    assert not bool(have.any()) and not bool(values.any())  # rows behind n_rows have no value
    # the starts made on the device from the key; a 32-bit amount without a filter, exclusive, every row
    made = wah.columns.partition_starts(wah, t["d_key"], rows)
    total = wah.columns.cumsum_column_by(wah, t["d_amount"], rows, made, exclusive=True, all_rows=True)
    assert total[2:] == (n, 32 + rows.bit_length(), False)
    values, _ = wah.columns.values_of_column(wah, total, 0, rows)
    want = _np_cumsum_by(t["amount"], np.ones(rows, bool), starts, exclusive=True)
    assert int(want.max()) > 1 << 36 and np.array_equal(values.cpu().numpy().view(np.uint64), want)
    # a single filter as a pair, a width of the caller's, the starts as a one-row table
    narrow = wah.columns.cumsum_column_by(wah, t["d_amount"], rows, wah.bitop_operand_table([made]), where=t["d_f"][0], n_bits=16)
    values, have = wah.columns.values_of_column(wah, narrow, 0, rows)
    assert np.array_equal(have.cpu().numpy(), t["f"][0])
    assert np.array_equal(values.cpu().numpy().view(np.uint64), np.where(t["f"][0], _np_cumsum_by(t["amount"], t["f"][0], starts) & np.uint64(0xFFFF), 0))


def test_row_numbers_by_against_numpy(wah, table):
    t = table
    n, rows, starts = t["n"], t["rows"], t["starts"]
    one = np.ones(rows, np.uint64)
    numbers = wah.columns.row_numbers_by(wah, t["d_starts"], n, rows)  # no filter at all
    assert numbers[2:] == (n, rows.bit_length(), True)
    values, have = wah.columns.values_of_column(wah, numbers, 0, rows)
    want = _np_cumsum_by(one, np.ones(rows, bool), starts)
    assert bool(have.all()) and np.array_equal(values.cpu().numpy().view(np.uint64), want)
    assert (want[starts] == 1).all() and want[0] == 1  # ROW_NUMBER() starts at 1 in every partition
    mask = t["f"][0] & t["f"][1]
    numbers = wah.columns.row_numbers_by(wah, t["d_starts"], n, rows, where=t["d_f"])
    values, have = wah.columns.values_of_column(wah, numbers, 0, rows)
    assert np.array_equal(have.cpu().numpy(), mask)
    assert np.array_equal(values.cpu().numpy().view(np.uint64), np.where(mask, _np_cumsum_by(one, mask, starts), 0))
    ranks = wah.columns.row_numbers_by(wah, t["d_starts"], n, rows, where=t["d_f"][1], exclusive=True, all_rows=True)
    assert ranks[2:] == (n, rows.bit_length(), False)
    values, _ = wah.columns.values_of_column(wah, ranks, 0, rows)
    assert np.array_equal(values.cpu().numpy().view(np.uint64), _np_cumsum_by(one, t["f"][1], starts, exclusive=True))


def test_streak_lengths_against_numpy(wah, table):
    t = table
    n, rows = t["n"], t["rows"]
    mask = t["f"][1]  # runs of 300 rows
    streak = wah.columns.streak_lengths(wah, t["d_f"][1], n, rows)
    values, have = wah.columns.values_of_column(wah, streak, 0, rows)
    want = _np_cumsum_by(np.ones(rows, np.uint64), mask, ~mask)
    assert np.array_equal(have.cpu().numpy(), mask) and np.array_equal(values.cpu().numpy().view(np.uint64), np.where(mask, want, 0))
    assert int(want[mask].max()) >= 600 and int(want[mask].min()) == 1
    loop, run = np.zeros(rows, np.uint64), 0
    for p in range(5000):
        run = run + 1 if mask[p] else 0
        loop[p] = run
    assert np.array_equal(np.where(mask, want, 0)[:5000], loop[:5000])
    # the mask as a conjunction of predicates
    both = t["f"][0] & t["f"][1]
    predicates = [(s, o, [0], False) for s, o in t["d_f"]]
    values, have = wah.columns.values_of_column(wah, wah.columns.streak_lengths(wah, predicates, n, rows), 0, rows)
    assert np.array_equal(have.cpu().numpy(), both)
    assert np.array_equal(values.cpu().numpy().view(np.uint64), np.where(both, _np_cumsum_by(np.ones(rows, np.uint64), both, ~both), 0))


# ---- 6: a chain with nothing read back, and the same as one captured graph -----------------------------------------------------------------
def _chain_want(key, qty, limit):
    starts = np.zeros(key.size, bool)
    starts[1:] = key[1:] != key[:-1]
    return int((_np_cumsum_by(qty, np.ones(key.size, bool), starts) <= np.uint64(limit)).sum())


def test_chain_without_a_read_back_and_its_graph_replay(wah, table):
    """bsi_from_values(key) -> partition_starts -> cumsum_column_by -> compare_column(<=, L) -> count_columns, "the rows in front of
    which their partition's running quantity has not passed L", every call with check=False into tensors made beforehand: the
    statuses are read once at the end.  Then the six calls as ONE captured graph, replayed after the key column was rebuilt in
    place (capture as the plain call's test: side stream, warm-up outside, check=False; one chain of launches, no parallel
    branches)."""
    import torch

    t = table
    n, rows, kk, kv, limit = t["n"], t["rows"], 6, 9, 40_000
    k_out = kv + rows.bit_length()
    rng = np.random.default_rng(33)
    keys = [t["key"], _clustered_key(rng, rows, 64, 150), _clustered_key(rng, rows, 64, 3000)]
    d_qty = wah.columns.bsi_from_values(wah, _dev_values(t["qty"]), kv, n_words_per_column=n)
    values = _dev_values(keys[0])
    lib = wah.lib()
    one = wah.max_compressed_words(n)
    segs = (one + 1023) // 1024

    def u8(size):
        return torch.empty(int(size), dtype=torch.uint8, device="cuda")

    def words(count):
        return torch.empty(count, dtype=torch.int32, device="cuda")

    def index(entries):
        return torch.zeros(entries, dtype=torch.int64, device="cuda")

    sc_build, sc_splice, sc_cmp = u8(lib.wah_bsi_build_scratch_bytes(n, kk)), u8(lib.wah_splice_scratch_bytes(n, kk, 2)), u8(lib.wah_bsi_compare_scratch_bytes(n, kk, kk))
    sc_sum, sc_range, sc_count = u8(lib.wah_bsi_cumsum_parts_scratch_bytes(n, k_out, 0)), u8(lib.wah_bsi_range_scratch_bytes(n, k_out)), u8(lib.wah_select_scratch_bytes(n, 1))
    out_key, offs_key = words(wah.max_compressed_words(kk * n)), index(kk * (n // SEG) + 1)
    out_shift, offs_shift = words(kk * one), index(kk * segs + 1)
    out_starts, offs_starts = words(one), index(segs + 1)
    out_sum, offs_sum = words(wah.max_compressed_words((k_out + 1) * n)), index((k_out + 1) * (n // SEG) + 1)
    out_range, offs_range = words(one), index(segs + 1)
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")

    def statuses():
        return (int(lib.wah_bsi_build_status(sc_build.data_ptr(), n, kk, None)), int(lib.wah_splice_status(sc_splice.data_ptr(), None)),
                int(lib.wah_bsi_compare_status(sc_cmp.data_ptr(), n, kk, kk, None)), int(lib.wah_bsi_cumsum_parts_status(sc_sum.data_ptr(), n, k_out, 0, None)),
                int(lib.wah_bsi_range_status(sc_range.data_ptr(), n, k_out + 1, None)), int(lib.wah_select_status(sc_count.data_ptr(), None)))

    # the front ends (they build their tables on the device); this is the warm-up outside the capture, too
    wah.bsi_build_device(values, kk, n, scratch=sc_build, out=out_key, out_offsets=offs_key, check=False)
    key = (out_key, offs_key, n, kk, False)
    starts = wah.columns.partition_starts(wah, key, rows, shift=dict(scratch=sc_splice, out=out_shift, out_offsets=offs_shift), scratch=sc_cmp,
                                          out=out_starts, out_offsets=offs_starts, check=False)
    assert starts[0].data_ptr() == out_starts.data_ptr()
    total = wah.columns.cumsum_column_by(wah, d_qty, rows, starts, scratch=sc_sum, out=out_sum, out_offsets=offs_sum, check=False)
    assert total[2:] == (n, k_out, True) and total[0].data_ptr() == out_sum.data_ptr()
    hit, _, hit_offs = wah.columns.compare_column(wah, total, "<=", limit, scratch=sc_range, out=out_range, out_offsets=offs_range, check=False)
    wah.columns.count_columns(wah, hit, hit_offs, n, [0], scratch=sc_count, counts=counts, check=False)
    assert statuses() == (0,) * 6
    assert 0 < int(counts.item()) == _chain_want(keys[0], t["qty"], limit) < rows
    # the same six calls over tables made beforehand: inside a capture nothing is copied from the host
    key_columns = wah.columns.column_operand_table(out_key, offs_key, n, list(range(kk)))
    pieces = wah.splice_pieces([(n, 0, 1), (n, 0, rows - 1)], torch.device("cuda:0"))
    splice_table = torch.cat([key_columns, key_columns])
    cmp_table = wah.columns._two_attribute_table(wah.bsi_compare_row_order(kk, kk), key, (out_shift, offs_shift, n, kk, False))
    val_table = wah.columns._slice_table(d_qty)
    starts_table = wah.bitop_operand_table([(out_starts, offs_starts)])
    range_table = wah.columns.column_operand_table(out_sum, offs_sum, n, list(range(k_out + 1)))
    count_table = wah.bitop_operand_table([(out_range, offs_range)])
    bounds = wah.bsi_bounds(0, limit, torch.device("cuda:0"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            wah.bsi_build_device(values, kk, n, scratch=sc_build, out=out_key, out_offsets=offs_key, check=False)
            wah.splice_device(pieces, splice_table, kk, n, scratch=sc_splice, out=out_shift, out_offsets=offs_shift, check=False)
            wah.bsi_compare_device(cmp_table, kk, kk, "!=", n, scratch=sc_cmp, out=out_starts, out_offsets=offs_starts, check=False)
            wah.bsi_cumsum_parts_device(val_table, n, rows, kv, k_out, starts_table, scratch=sc_sum, out=out_sum, out_offsets=offs_sum, check=False)
            wah.bsi_range_device(range_table, bounds, n, exists=True, scratch=sc_range, out=out_range, out_offsets=offs_range, check=False)
            wah.count_device(count_table, n, scratch=sc_count, counts=counts, check=False)
    seen = set()
    for other in keys[1:] + keys[:1]:
        values.copy_(_dev_values(other))  # rewritten in place: the captured calls hold its address
        counts.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert statuses() == (0,) * 6
        assert int(counts.item()) == _chain_want(other, t["qty"], limit)
        seen.add(int(counts.item()))
    assert len(seen) == 3  # different answers from one captured chain
