"""GPU tests of wah_bsi_total_parts_indexed_device: the total of a row's partition in every one of its rows, as a new bit-sliced
attribute in one call (include/wah.h), and its front ends in api.py and columns.py.  Everything is exact: the result's words, their
count and its whole segment index against the oracle's compress() of the slice matrix that numpy builds FROM THE VALUES, the unpacked
bitmaps and the starts (tests/_total_parts.py); tests/test_total_parts_reference.py proves that model against a restatement of the
kernels' steps and that every wrong model is caught.  Outputs and scratch are poisoned and have a guard behind them.

The named cases run at 992, 2 * 992 and 3 * 992 words -- one, two and three segments; 513 segments are one more than the grid has
workgroups; 8194 segments are two more than one round of either scan, with starts in the first four and the last four; the bitmap
of more than 2^32 rows and the 8194 segments are expected from tests/_long.py's run model."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _cumsum as cs, _foreign as fg, _long as lg, _total_parts as tp, test_gpu_bsi_cumsum_parts as gp
from tests.test_gpu_bsi_arith import Streams, _dev, _dev_values, _host

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6
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
    return tp.named_cases()


def _flags(wah, case):
    return (wah.BSI_EXISTS if case["exists"] is not None else 0) | (wah.CUMSUM_ALL_ROWS if case["all_rows"] else 0)


_operands = gp._operands  # (value rows, filter rows, the starts row) as indexed compressed bitmaps
_same = gp._same


def _call(wah, case, val, filters, starts, check=True, scratch=None, cap=None):
    """The call into poisoned outputs and a poisoned scratch with a guard behind each; returns what bsi_total_parts_device returns."""
    import torch

    n, rows_out = case["n"], cs.rows_out(case)
    cap, entries = wah.max_compressed_words(rows_out * n) if cap is None else cap, rows_out * (n // SEG) + 1
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    offs = torch.full((entries + 1,), -1, dtype=torch.int64, device="cuda")
    need = int(wah.lib().wah_bsi_total_parts_scratch_bytes(n, case["k_out"], _flags(wah, case)))
    if scratch is None:
        scratch = torch.full((need + 256,), POISON, dtype=torch.uint8, device="cuda")
    val, filters = (None if isinstance(x, list) and not x else x for x in (val, filters))
    got = wah.bsi_total_parts_device(val, n, case["n_rows"], case["kv"], case["k_out"], starts, filters=filters, exists=case["exists"] is not None,
                                     all_rows=case["all_rows"], scratch=scratch[:need], out=buf[:cap], out_offsets=offs[:entries], check=check)
    torch.cuda.synchronize()
    assert int(buf[cap].item()) == GUARD and int(offs[entries].item()) == -1, "guard"
    assert scratch.numel() == need or bool((scratch[need:] == POISON).all()), "scratch guard"
    return got


def _run(wah, oracle, case, what, tables=None):
    want = tp.expected(case)
    operands = _operands(wah, case) if tables is None else None  # (kept until the call is done: a table holds raw pointers)
    val, filters, starts = operands if tables is None else tables
    got, offs = _call(wah, case, val, filters, starts)
    del operands
    _same(oracle, got, offs, want, what)


# ---- 1: the named cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tp.named_cases()))
def test_named_case_vs_value_model(wah, oracle, cases, name):
    _run(wah, oracle, cases[name], name)


def test_the_starts_as_a_table_and_as_a_pair(wah, oracle, cases):
    case = cases["two starts in a step"]
    val, filters, starts = _operands(wah, case)
    _run(wah, oracle, case, "table", tables=(val, filters, wah.bitop_operand_table([starts])))
    _run(wah, oracle, case, "pair", tables=(wah.bitop_operand_table(val), wah.bitop_operand_table(filters), starts))


def test_one_segment_more_than_the_grid(wah, oracle):
    """513 segments, a 1-slice value under one filter and a 2-bit result: the first workgroup takes a second segment, and both scans
    of the records have 513 entries; a partition of every length from a few rows to a few segments."""
    n = (cs.GRID_ITEMS + 1) * SEG
    rng = np.random.default_rng(513)
    rows = 32 * n
    values = (rng.random(rows) < 0.5).astype(np.uint64)
    starts = np.zeros(rows, bool)
    starts[rng.integers(0, rows, 300)] = True
    starts[40 * cs.SEG_BITS: 45 * cs.SEG_BITS] = False       # an inflow from behind over five segments
    starts[[511 * cs.SEG_BITS + 9, 512 * cs.SEG_BITS, rows - 1]] = True
    case = tp.make_case(n, 1, 2, starts, n_rows=rows - 3, n_filters=1, values=values)
    _run(wah, oracle, case, "513 segments")


# ---- 2: long bitmaps, expected from the run model --------------------------------------------------------------------------------------
def _long_run(wah, oracle, filt, starts, n_rows):
    """The call on long bitmaps against tests/_total_parts.py's long_expected (its docstring says what the operands are), the expected
    stream assembled on the device."""
    import torch

    a = filt.n_segments
    n = a * SEG
    want, want_index, sizes = tp.long_expected(oracle, filt, starts, n_rows, empty=lambda total: torch.empty(total, dtype=torch.int32, device="cuda"),
                                               put=lambda words: torch.from_numpy(np.ascontiguousarray(words)).cuda())
    total = int(want_index[-1])
    tables = []
    for bitmap in (filt, starts):
        stream, index = bitmap.stream_index(oracle)
        tables.append((_dev(stream), torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).cuda()))
    cap = total + 64
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    offs = torch.full((2 * a + 2,), -1, dtype=torch.int64, device="cuda")
    got, got_offs = wah.bsi_total_parts_device(None, n, n_rows, 0, 2, tables[1], filters=[tables[0]], all_rows=True, out=buf[:cap],
                                               out_offsets=offs[: 2 * a + 1])
    assert int(buf[cap].item()) == GUARD and int(offs[2 * a + 1].item()) == -1
    assert got.numel() == total
    assert torch.equal(got_offs, torch.from_numpy(want_index).cuda())
    assert torch.equal(got, want)
    return sizes


def test_both_scans_carry_a_pair_over_their_round_seams(wah, oracle):
    """8194 segments, two more than a round of either scan has entries, with starts in the first four and the last four: the one long
    partition from segment 3 to segment 8190 crosses the forward scan's seam behind segment 8191 and the backward scan's seam in
    front of segment 2, where the short last round takes the carry of round 0."""
    a = tp.ROUND_SEGMENTS
    named = (0, 1, 2, 3, 8190, 8191, 8192, 8193)
    filt = lg.marked(a, named, (0,), 43, default=1)
    at = [700, lg.SEG_BITS + 5, 2 * lg.SEG_BITS + 31000, 3 * lg.SEG_BITS + 64, 8190 * lg.SEG_BITS + 300, 8190 * lg.SEG_BITS + 20000, 8191 * lg.SEG_BITS + 31743,
          8192 * lg.SEG_BITS, 8193 * lg.SEG_BITS + 64]
    sizes = _long_run(wah, oracle, filt, lg.from_rows(a, at), a * lg.SEG_BITS - 70)
    assert sizes.size == len(at) + 1 and int(sizes.max()) > 8000 * lg.SEG_BITS and 0 < int(sizes[1]) < lg.SEG_BITS and 0 < int(sizes[2]) < 2 * lg.SEG_BITS


def test_a_bitmap_of_more_than_2_32_rows(wah, oracle):
    """135 400 segments (4.298e9 rows) and starts at row 5, behind row 2^32 and in the last segment, in front of n_rows and behind
    it: segment numbers, row numbers, the matrix's word offsets and the clip pass 2^32, and so does the size of the partition
    that rows 5 .. 2^32 + 1 lie in, which reaches row 5 from behind over 135 000 records."""
    a = lg.A_SEGMENTS
    n_rows = a * lg.SEG_BITS - 11
    start = 2**32 + 2
    assert start // lg.SEG_BITS in lg.A_NAMED and a - 1 in lg.A_NAMED
    filt = lg.marked(a, lg.A_NAMED, lg.A_ROWS, 41, default=1)
    at = [5, start, n_rows - 1000, n_rows, n_rows + 3]
    sizes = _long_run(wah, oracle, filt, lg.from_rows(a, at), n_rows)
    assert sizes.size == 4 and int(sizes[1]) > 2**32 - 6 * lg.SEG_BITS and 0 < int(sizes[3]) <= 1000


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
    case = tp.make_case(n, kv, 20, starts, n_rows=rows - 100, values=values, filters=filters)
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


# ---- 4: what only the device sees -----------------------------------------------------------------------------------------------------
def _status(wah, case, val, filters, starts, cap=None):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    flags = _flags(wah, case)
    sc = torch.empty(int(wah.lib().wah_bsi_total_parts_scratch_bytes(case["n"], case["k_out"], flags)), dtype=torch.uint8, device="cuda")
    _call(wah, case, val, filters, starts, check=False, scratch=sc, cap=cap)
    return int(wah.lib().wah_bsi_total_parts_status(sc.data_ptr(), case["n"], case["k_out"], flags, None))


def test_a_bad_operand_is_refused_by_the_status_call_only(wah):
    runs = np.repeat(np.random.default_rng(2).random(32 * 2 * SEG // 992) < 0.3, 992)
    case = tp.make_case(2 * SEG, 12, 28, runs, with_exists=True, n_filters=2, seed=9)
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


def test_too_small_a_capacity_is_refused_and_the_guard_stays(wah, oracle, cases):
    case = cases["widths 26 x 32"]
    val, filters, starts = _operands(wah, case)
    want, _ = cs.compressed(oracle, tp.expected(case))
    assert _status(wah, case, val, filters, starts, cap=want.size) == 0
    for cap in (want.size - 1, want.size // 2):
        assert _status(wah, case, val, filters, starts, cap=cap) == WAH_ERR_CAPACITY, cap  # (_call looks at the word behind the capacity)


def test_front_end_refuses_bad_arguments(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    pair = (stream, offs)
    with pytest.raises(wah.WahError):
        wah.bsi_total_parts_device([pair] * 33, SEG, 0, 33, 40, pair)
    with pytest.raises(wah.WahError):
        wah.bsi_total_parts_device([pair] * 3, SEG, 0, 3, 65, pair)
    with pytest.raises(wah.WahError):
        wah.bsi_total_parts_device([pair] * 3, SEG + 1, 0, 3, 8, pair)
    with pytest.raises(wah.WahError):
        wah.bsi_total_parts_device([pair] * 3, SEG, 0, 2, 8, pair)  # a table that does not go with the width
    with pytest.raises(wah.WahError):
        wah.bsi_total_parts_device([pair] * 3, SEG, 0, 3, 8, [pair, pair])  # two starts rows
    with pytest.raises(TypeError):
        wah.bsi_total_parts_device([pair] * 3, SEG, 0, 3, 8, pair, exclusive=True)  # there is no exclusive total
    with pytest.raises(ValueError):
        wah.columns.total_column_by(wah, (stream, offs, SEG, 33, False), 0, pair)
    with pytest.raises(ValueError):
        wah.columns.total_column_by(wah, (stream, offs, SEG, 8, False), 0, pair, n_bits=65)


# ---- 5: the front ends ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(wah):
    """A table of 2 * 992 * 32 - 50 rows clustered by a 6-bit key, with a 9-bit quantity (an existence bitmap), a 32-bit amount and
    two filter bitmaps, the second in runs that leave whole partitions without a selected row."""
    import torch

    n = 2 * SEG
    rows = 32 * n - 50
    rng = np.random.default_rng(2027)
    key = gp._clustered_key(rng, rows, 64, 700)
    qty, amount = _bsi.uniform_values(rng, rows, 9), _bsi.uniform_values(rng, rows, 32)
    qty_exists = rng.random(rows) < 0.9
    f = [rng.random(rows) < 0.7, np.repeat(rng.random(rows // 3000 + 1) < 0.6, 3000)[:rows]]
    streams = Streams(wah, n)

    def padded(a, dtype):
        out = np.zeros(32 * n, dtype)
        out[: a.size] = a
        return out

    starts = np.zeros(rows, bool)
    starts[1:] = key[1:] != key[:-1]
    return dict(n=n, rows=rows, key=key, starts=starts, part=np.cumsum(starts), qty=qty, amount=amount, qty_exists=qty_exists, f=f,
                d_key=wah.columns.bsi_from_values(wah, _dev_values(key), 6, n_words_per_column=n),
                d_qty=wah.columns.bsi_from_values(wah, _dev_values(qty), 9, n_words_per_column=n, exists=torch.from_numpy(qty_exists).cuda()),
                d_amount=wah.columns.bsi_from_values(wah, _dev_values(amount), 32, n_words_per_column=n),
                d_f=[streams.of(_bsi.pack_bits(padded(x, bool))) for x in f],
                d_starts=streams.of(_bsi.pack_bits(padded(starts, bool))))


def _np_total_by(values, mask, part):
    """Every row's partition total of the masked values, uint64."""
    x = np.where(mask, values, np.uint64(0)).astype(np.uint64)
    totals = np.zeros(int(part[-1]) + 1, np.uint64)
    np.add.at(totals, part, x)
    return totals[part]


def _values(wah, bsi, rows):
    values, have = wah.columns.values_of_column(wah, bsi, 0, rows)
    return values.cpu().numpy().view(np.uint64), np.ones(rows, bool) if have is None else have.cpu().numpy()


def test_total_column_by_against_numpy(wah, table):
    t = table
    n, rows, part = t["n"], t["rows"], t["part"]
    # SUM(qty) OVER (PARTITION BY key) WHERE f0 AND f1, the attribute's own existence bitmap in the selection
    mask = t["qty_exists"] & t["f"][0] & t["f"][1]
    total = wah.columns.total_column_by(wah, t["d_qty"], rows, t["d_starts"], where=t["d_f"])
    assert total[2:] == (n, 9 + rows.bit_length(), True)
    values, have = _values(wah, total, rows)
    want = _np_total_by(t["qty"], mask, part)
    assert np.array_equal(have, mask) and np.array_equal(values, np.where(mask, want, 0))
    assert len(set(want[mask].tolist())) > 20  # (the partitions matter)
    values, have = wah.columns.values_of_column(wah, total, rows, 50)
    assert not bool(have.any()) and not bool(values.any())  # rows behind n_rows have no value
    # the starts made on the device from the key; a 32-bit amount without a filter, every row
    made = wah.columns.partition_starts(wah, t["d_key"], rows)
    total = wah.columns.total_column_by(wah, t["d_amount"], rows, made, all_rows=True)
    assert total[2:] == (n, 32 + rows.bit_length(), False)
    want = _np_total_by(t["amount"], np.ones(rows, bool), part)
    assert int(want.max()) > 1 << 36 and np.array_equal(_values(wah, total, rows)[0], want)
    # every row under a filter: a partition without a selected row holds 0
    total = wah.columns.total_column_by(wah, t["d_amount"], rows, made, where=t["d_f"][1], all_rows=True)
    want = _np_total_by(t["amount"], t["f"][1], part)
    assert (want == 0).any() and np.array_equal(_values(wah, total, rows)[0], want)
    # a single filter as a pair, a width of the caller's, the starts as a one-row table
    narrow = wah.columns.total_column_by(wah, t["d_amount"], rows, wah.bitop_operand_table([made]), where=t["d_f"][0], n_bits=16)
    values, have = _values(wah, narrow, rows)
    assert np.array_equal(have, t["f"][0])
    assert np.array_equal(values, np.where(t["f"][0], _np_total_by(t["amount"], t["f"][0], part) & np.uint64(0xFFFF), 0))
    # no starts at all: SUM(x) OVER ()
    grand = wah.columns.total_column_by(wah, t["d_qty"], rows, None, where=t["d_f"][0])
    values, have = _values(wah, grand, rows)
    mask = t["qty_exists"] & t["f"][0]
    assert np.array_equal(have, mask) and np.array_equal(values, np.where(mask, np.uint64(t["qty"][mask].sum()), np.uint64(0)))


def test_partition_sizes_against_numpy(wah, table):
    t = table
    n, rows, part = t["n"], t["rows"], t["part"]
    one = np.ones(rows, np.uint64)
    sizes = wah.columns.partition_sizes(wah, t["d_starts"], n, rows)  # no filter at all: COUNT(*) OVER (PARTITION BY key)
    assert sizes[2:] == (n, rows.bit_length(), True)
    values, have = _values(wah, sizes, rows)
    want = np.bincount(part)[part].astype(np.uint64)
    assert bool(have.all()) and np.array_equal(values, want) and int(want.min()) >= 1
    mask = t["f"][0] & t["f"][1]
    values, have = _values(wah, wah.columns.partition_sizes(wah, t["d_starts"], n, rows, where=t["d_f"]), rows)
    assert np.array_equal(have, mask) and np.array_equal(values, np.where(mask, _np_total_by(one, mask, part), 0))
    every = wah.columns.partition_sizes(wah, t["d_starts"], n, rows, where=t["d_f"][1], all_rows=True)
    assert every[2:] == (n, rows.bit_length(), False)
    assert np.array_equal(_values(wah, every, rows)[0], _np_total_by(one, t["f"][1], part))


def test_mean_column_by_against_numpy(wah, table):
    t = table
    n, rows, part = t["n"], t["rows"], t["part"]
    for where, all_rows in ((None, False), (t["d_f"][1], True), (t["d_f"], False)):
        mask = t["qty_exists"].copy()
        for f in ([] if where is None else [t["f"][1]] if isinstance(where, tuple) else t["f"]):
            mask &= f
        mean = wah.columns.mean_column_by(wah, t["d_qty"], rows, t["d_starts"], where=where, all_rows=all_rows)
        assert mean[2:] == (n, 9, True)
        values, have = _values(wah, mean, rows)
        total, size = _np_total_by(t["qty"], mask, part), _np_total_by(np.ones(rows, np.uint64), mask, part)
        exists = (size > 0) & (mask | all_rows)
        assert np.array_equal(have, exists), all_rows
        assert np.array_equal(values, np.where(exists, total // np.maximum(size, 1), 0)), all_rows
        assert not all_rows or bool((size == 0).any())  # (a partition without a selected row is NULL)


def test_rows_of_partitions_where_against_numpy(wah, table):
    t = table
    n, rows, part = t["n"], t["rows"], t["part"]
    mask = t["qty_exists"] & t["f"][0]
    total = _np_total_by(t["qty"], mask, part)
    bound = int(np.sort(total[mask])[mask.sum() // 2])
    for op, fn in (("<", np.less), ("<=", np.less_equal), (">", np.greater), (">=", np.greater_equal), ("==", np.equal)):
        got = wah.columns.rows_of_partitions_where(wah, t["d_qty"], rows, t["d_starts"], op, bound, where=t["d_f"][0])
        bits = gp._decoded(wah, got, n)
        want = mask & fn(total, np.uint64(bound))
        assert np.array_equal(bits[:rows], want) and not bits[rows:].any(), op
    assert 0 < want.sum() < mask.sum()  # ("==": the median is some partition's total)


def test_the_result_goes_into_the_other_calls(wah, table):
    """compare_column, divide_columns and values_of_column take the result as it is: the share of total x * 100 / SUM(x), and the rows
    of the groups whose total passes a bound, against numpy."""
    t = table
    n, rows, part = t["n"], t["rows"], t["part"]
    total = wah.columns.total_column_by(wah, t["d_amount"], rows, t["d_starts"], where=t["d_f"][0])
    want = _np_total_by(t["amount"], t["f"][0], part)
    bound = int(np.sort(want)[rows // 2])
    hit = wah.columns.compare_column(wah, total, ">", bound)
    assert np.array_equal(gp._decoded(wah, hit, n)[:rows], t["f"][0] & (want > np.uint64(bound)))
    ratio = wah.columns.divide_columns(wah, total, t["d_amount"])  # the total in units of the row's own amount
    values, have = _values(wah, ratio, rows)
    exists = t["f"][0] & (t["amount"] > 0)
    assert np.array_equal(have, exists) and np.array_equal(values, np.where(exists, want // np.maximum(t["amount"], 1), 0))


def test_the_total_is_the_running_sum_at_the_partitions_last_row(wah, table):
    """The cross-check against the existing call on the device: the total equals cumsum_column_by(all_rows=True) read at each
    partition's last row."""
    import torch

    t = table
    n, rows, starts = t["n"], t["rows"], t["starts"]
    for bsi, where in ((t["d_qty"], t["d_f"]), (t["d_amount"], None)):
        running = wah.columns.cumsum_column_by(wah, bsi, rows, t["d_starts"], where=where, all_rows=True)
        total = wah.columns.total_column_by(wah, bsi, rows, t["d_starts"], where=where, all_rows=True)
        assert running[2:] == total[2:]
        r, _ = wah.columns.values_of_column(wah, running, 0, rows)
        got, _ = wah.columns.values_of_column(wah, total, 0, rows)
        nxt = np.append(np.flatnonzero(starts), rows)  # the partitions' ends, then the gather on the device
        end = torch.from_numpy(nxt[np.searchsorted(nxt, np.arange(rows), side="right")] - 1).cuda()
        assert torch.equal(got, r[end])


# ---- 6: a chain with nothing read back, and the same as one captured graph -----------------------------------------------------------------
def _chain_want(key, qty, limit):
    starts = np.zeros(key.size, bool)
    starts[1:] = key[1:] != key[:-1]
    return int((_np_total_by(qty, np.ones(key.size, bool), np.cumsum(starts)) > np.uint64(limit)).sum())


def test_chain_without_a_read_back_and_its_graph_replay(wah, table):
    """partition_starts -> total_column_by -> compare_column(>, L) -> count_columns, "the rows of the groups whose total quantity
    passes L", every call with check=False into tensors made beforehand: the statuses are read once at the end.  Then the chain with
    the value column's build in front as ONE captured graph, replayed after the value column was rebuilt in place (capture as the
    partitioned running sum's test: side stream, warm-up outside, check=False; one chain of launches, no parallel branches)."""
    import torch

    t = table
    n, rows, kk, kv, limit = t["n"], t["rows"], 6, 9, 150_000
    k_out = kv + rows.bit_length()
    rng = np.random.default_rng(34)
    quantities = [t["qty"], _bsi.uniform_values(rng, rows, kv), _bsi.uniform_values(rng, rows, kv) >> np.uint64(1)]
    values = _dev_values(quantities[0])
    lib = wah.lib()
    one = wah.max_compressed_words(n)
    segs = (one + 1023) // 1024

    def u8(size):
        return torch.empty(int(size), dtype=torch.uint8, device="cuda")

    def words(count):
        return torch.empty(count, dtype=torch.int32, device="cuda")

    def index(entries):
        return torch.zeros(entries, dtype=torch.int64, device="cuda")

    sc_build, sc_splice, sc_cmp = u8(lib.wah_bsi_build_scratch_bytes(n, kv)), u8(lib.wah_splice_scratch_bytes(n, kk, 2)), u8(lib.wah_bsi_compare_scratch_bytes(n, kk, kk))
    sc_sum, sc_range, sc_count = u8(lib.wah_bsi_total_parts_scratch_bytes(n, k_out, 0)), u8(lib.wah_bsi_range_scratch_bytes(n, k_out)), u8(lib.wah_select_scratch_bytes(n, 1))
    out_qty, offs_qty = words(wah.max_compressed_words(kv * n)), index(kv * (n // SEG) + 1)
    out_shift, offs_shift = words(kk * one), index(kk * segs + 1)
    out_starts, offs_starts = words(one), index(segs + 1)
    out_sum, offs_sum = words(wah.max_compressed_words((k_out + 1) * n)), index((k_out + 1) * (n // SEG) + 1)
    out_range, offs_range = words(one), index(segs + 1)
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")

    def statuses():
        return (int(lib.wah_bsi_build_status(sc_build.data_ptr(), n, kv, None)), int(lib.wah_splice_status(sc_splice.data_ptr(), None)),
                int(lib.wah_bsi_compare_status(sc_cmp.data_ptr(), n, kk, kk, None)), int(lib.wah_bsi_total_parts_status(sc_sum.data_ptr(), n, k_out, 0, None)),
                int(lib.wah_bsi_range_status(sc_range.data_ptr(), n, k_out + 1, None)), int(lib.wah_select_status(sc_count.data_ptr(), None)))

    # the front ends (they build their tables on the device); this is the warm-up outside the capture, too
    wah.bsi_build_device(values, kv, n, scratch=sc_build, out=out_qty, out_offsets=offs_qty, check=False)
    qty = (out_qty, offs_qty, n, kv, False)
    key = t["d_key"]
    starts = wah.columns.partition_starts(wah, key, rows, shift=dict(scratch=sc_splice, out=out_shift, out_offsets=offs_shift), scratch=sc_cmp,
                                          out=out_starts, out_offsets=offs_starts, check=False)
    assert starts[0].data_ptr() == out_starts.data_ptr()
    total = wah.columns.total_column_by(wah, qty, rows, starts, scratch=sc_sum, out=out_sum, out_offsets=offs_sum, check=False)
    assert total[2:] == (n, k_out, True) and total[0].data_ptr() == out_sum.data_ptr()
    hit, _, hit_offs = wah.columns.compare_column(wah, total, ">", limit, scratch=sc_range, out=out_range, out_offsets=offs_range, check=False)
    wah.columns.count_columns(wah, hit, hit_offs, n, [0], scratch=sc_count, counts=counts, check=False)
    assert statuses() == (0,) * 6
    assert 0 < int(counts.item()) == _chain_want(t["key"], quantities[0], limit) < rows
    # the same calls over tables made beforehand: inside a capture nothing is copied from the host
    key_columns = wah.columns.column_operand_table(key[0], key[1], n, list(range(kk)))
    pieces = wah.splice_pieces([(n, 0, 1), (n, 0, rows - 1)], torch.device("cuda:0"))
    splice_table = torch.cat([key_columns, key_columns])
    cmp_table = wah.columns._two_attribute_table(wah.bsi_compare_row_order(kk, kk), key, (out_shift, offs_shift, n, kk, False))
    val_table = wah.columns._slice_table(qty)
    starts_table = wah.bitop_operand_table([(out_starts, offs_starts)])
    range_table = wah.columns.column_operand_table(out_sum, offs_sum, n, list(range(k_out + 1)))
    count_table = wah.bitop_operand_table([(out_range, offs_range)])
    bounds = wah.bsi_bounds(limit + 1, (1 << k_out) - 1, torch.device("cuda:0"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            wah.bsi_build_device(values, kv, n, scratch=sc_build, out=out_qty, out_offsets=offs_qty, check=False)
            wah.splice_device(pieces, splice_table, kk, n, scratch=sc_splice, out=out_shift, out_offsets=offs_shift, check=False)
            wah.bsi_compare_device(cmp_table, kk, kk, "!=", n, scratch=sc_cmp, out=out_starts, out_offsets=offs_starts, check=False)
            wah.bsi_total_parts_device(val_table, n, rows, kv, k_out, starts_table, scratch=sc_sum, out=out_sum, out_offsets=offs_sum, check=False)
            wah.bsi_range_device(range_table, bounds, n, exists=True, scratch=sc_range, out=out_range, out_offsets=offs_range, check=False)
            wah.count_device(count_table, n, scratch=sc_count, counts=counts, check=False)
    seen = set()
    for other in quantities[1:] + quantities[:1]:
        values.copy_(_dev_values(other))  # rewritten in place: the captured calls hold its address
        counts.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert statuses() == (0,) * 6
        assert int(counts.item()) == _chain_want(t["key"], other, limit)
        seen.add(int(counts.item()))
    assert len(seen) == 3  # different answers from one captured chain
