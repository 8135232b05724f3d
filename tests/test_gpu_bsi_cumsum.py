"""GPU tests of wah_bsi_cumsum_indexed_device: the running sum of a bit-sliced value over the rows the filters select, as a new
bit-sliced attribute in one call (include/wah.h), and its front ends in api.py and columns.py.  Everything is exact: the result's
words, their count and its whole segment index against the oracle's compress() of the slice matrix that numpy builds FROM THE VALUES
and the unpacked bitmaps (tests/_cumsum.py); tests/test_cumsum_reference.py proves that model against a restatement of the kernel's
steps and that every named case can fail.  Outputs and scratch are poisoned and have a guard behind them.

The named cases run at 992, 2 * 992 and 3 * 992 words -- one, two and three segments: the segments' bases, the half block's 32
words in front of the next segment's first -- over the row counts, widths, sums, selections, flags and filter counts of
tests/_cumsum.py; 513 segments are one more than the grid has workgroups; the bitmap of more than 2^32 rows comes from
tests/_long.py."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _cumsum as cs, _foreign as fg, _long as lg
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
    return cs.named_cases()


def _flags(wah, case):
    return ((wah.BSI_EXISTS if case["exists"] is not None else 0) | (wah.CUMSUM_EXCLUSIVE if case["exclusive"] else 0) |
            (wah.CUMSUM_ALL_ROWS if case["all_rows"] else 0))


def _operands(wah, case):
    """(value rows, filter rows) as indexed compressed bitmaps: the value's slices as the index holds them (a row outside the
    existence bitmap is stored as 0), its existence row, and every filter."""
    streams = Streams(wah, case["n"])
    val = []
    if case["kv"]:
        val = [streams.of(row) for row in _bsi.build_slices(case["values"], case["kv"], case["exists"], zero_missing=True)]
    elif case["exists"] is not None:
        val = [streams.of(_bsi.pack_bits(case["exists"]))]
    return val, [streams.of(_bsi.pack_bits(f)) for f in case["filters"]]


def _call(wah, case, val, filters, check=True, scratch=None):
    """The call into poisoned outputs and a poisoned scratch with a guard behind each; returns what bsi_cumsum_device returns."""
    import torch

    n, rows_out = case["n"], cs.rows_out(case)
    cap, entries = wah.max_compressed_words(rows_out * n), rows_out * (n // SEG) + 1
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    offs = torch.full((entries + 1,), -1, dtype=torch.int64, device="cuda")
    need = int(wah.lib().wah_bsi_cumsum_scratch_bytes(n, case["k_out"], _flags(wah, case)))
    if scratch is None:
        scratch = torch.full((need + 256,), POISON, dtype=torch.uint8, device="cuda")
    val, filters = (None if isinstance(x, list) and not x else x for x in (val, filters))
    got = wah.bsi_cumsum_device(val, n, case["n_rows"], case["kv"], case["k_out"], filters=filters,
                                exists=case["exists"] is not None, exclusive=case["exclusive"], all_rows=case["all_rows"], scratch=scratch[:need],
                                out=buf[:cap], out_offsets=offs[:entries], check=check)
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
    want = cs.expected(case)
    operands = _operands(wah, case) if tables is None else None  # (kept until the call is done: a table holds raw pointers)
    val, filters = operands if tables is None else tables
    got, offs = _call(wah, case, val, filters)
    del operands
    _same(oracle, got, offs, want, what)


# ---- 1: the named cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cs.named_cases()))
def test_named_case_vs_value_model(wah, oracle, cases, name):
    _run(wah, oracle, cases[name], name)


def test_one_segment_more_than_the_grid(wah, oracle):
    """513 segments, a 1-slice value under one filter and a 1-bit result: the first workgroup takes a second segment, and the scan
    of the totals has 513 entries."""
    n = (cs.GRID_ITEMS + 1) * SEG
    rng = np.random.default_rng(513)
    values = (rng.random(32 * n) < 0.5).astype(np.uint64)
    values[-cs.SEG_BITS:] = np.where(rng.random(cs.SEG_BITS) < 0.9, 1, 0)  # the last segment differs from the first
    case = cs.make_case(n, 1, 1, 32 * n - 3, False, 1, values=values)
    _run(wah, oracle, case, "513 segments")


def test_a_bitmap_of_more_than_2_32_rows(wah, oracle):
    """135 400 segments (4.298e9 rows), a filter of constant ones with a few live segments, no value slices, a 2-bit result and
    all_rows: every row in front of n_rows = 2^32 + 5 holds the number of selected rows up to it mod 4, zeros behind -- segment
    numbers, row numbers, the word offsets of the matrix and the clip pass 2^32, and the bases pass 2^32 too.  Expected from
    tests/_long.py's run model: a segment of ones adds 31 744, a multiple of 4, so between two live segments every constant segment
    of a result slice is the same 1024 literals, given by the count mod 4 in front of it; behind n_rows it is one zero fill."""
    import torch

    a = lg.A_SEGMENTS
    n = a * SEG
    n_rows = 2**32 + 5
    cut = n_rows // lg.SEG_BITS
    assert cut in lg.A_NAMED and n_rows < 32 * n and lg.SEG_BITS % 4 == 0
    filt = lg.marked(a, lg.A_NAMED, lg.A_ROWS, 41, default=1)
    assert set(filt.defaults().tolist()) == {1} and len(filt.live) >= len(lg.A_NAMED)
    front = np.concatenate([[0], np.cumsum(filt.segment_counts())]).astype(np.int64)  # the selected rows in front of every segment
    assert front[cut] > 2**32 - 6 * lg.SEG_BITS
    stream, index = filt.stream_index(oracle)
    d_stream, d_index = _dev(stream), torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).cuda()

    def segment(s, bits):  # the two result slices' words of segment s whose filter bits are `bits`
        run = (front[s] + np.cumsum(bits.astype(np.int64))) & 3
        run[max(min(n_rows - s * lg.SEG_BITS, lg.SEG_BITS), 0):] = 0
        return [np.asarray(oracle.compress(_bsi.pack_bits(((run >> b) & 1).astype(bool))), dtype=np.uint32) for b in (1, 0)]

    ones = np.ones(lg.SEG_BITS, np.uint8)
    phase_words = {p: [torch.from_numpy(w.view(np.int32)).cuda() for w in segment_words] for p, segment_words in
                   ((p, [np.asarray(oracle.compress(_bsi.pack_bits((((p + 1 + np.arange(lg.SEG_BITS)) >> b) & 1).astype(bool))), dtype=np.uint32)
                         for b in (1, 0)]) for p in range(4))}
    assert all(w.numel() == 1024 for ws in phase_words.values() for w in ws)
    live = {s: segment(s, filt.seg_bits(s)) for s in filt.live}
    assert np.array_equal(segment(1, ones)[0], phase_words[int(front[1]) & 3][0].cpu().numpy().view(np.uint32))
    # the lengths of all 2 a segments of the result, slice 1 first
    lengths = np.where(np.arange(a) < cut, 1024, 1).astype(np.int64)
    lengths = np.stack([lengths, lengths.copy()])
    for s, pair in live.items():
        lengths[0, s], lengths[1, s] = pair[0].size, pair[1].size
    want_index = np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64)
    total = int(want_index[-1])
    want = torch.empty(total, dtype=torch.int32, device="cuda")
    zero_fill = int(np.array([lg.FILL | lg.SEG_GROUPS], np.uint32).view(np.int32)[0])
    for j in range(2):
        first = 0
        for s in sorted(live) + [a]:  # the constant segments [first, s) -- all in front of the cut or all behind it -- then the live segment s
            if s > first:
                lo, hi = int(want_index[j * a + first]), int(want_index[j * a + s])
                if first < cut:
                    want[lo:hi].view(-1, 1024)[:] = phase_words[int(front[first]) & 3][j]
                else:
                    want[lo:hi] = zero_fill
            if s < a:
                at = int(want_index[j * a + s])
                want[at: at + live[s][j].size] = torch.from_numpy(live[s][j].view(np.int32)).cuda()
            first = s + 1

    table = wah.bitop_operand_table([(d_stream, d_index)])
    cap = total + 64
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    offs = torch.full((2 * a + 2,), -1, dtype=torch.int64, device="cuda")
    got, got_offs = wah.bsi_cumsum_device(None, n, n_rows, 0, 2, filters=table, all_rows=True, out=buf[:cap], out_offsets=offs[: 2 * a + 1])
    assert int(buf[cap].item()) == GUARD and int(offs[2 * a + 1].item()) == -1
    assert got.numel() == total
    assert torch.equal(got_offs, torch.from_numpy(want_index).cuda())
    assert torch.equal(got, want)


# ---- 2: foreign streams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", (0, 5))
def test_every_operand_in_every_reencoding(wah, oracle, first):
    """The value's slices, its existence row and two filters written in every way of tests/_foreign.py that compress() never emits,
    the ways rotating over the fifteen table rows: the result is the canonical one."""
    n, kv = 2 * SEG, 12
    rng = np.random.default_rng(12)
    rows = 32 * n
    values = _bsi.make_values("clustered", rng, rows, kv)
    exists = np.repeat(rng.random(rows // 992 + 1) < 0.8, 992)[:rows]  # runs: the existence row has fills too
    filters = [np.repeat(rng.random(rows // 500 + 1) < 0.7, 500)[:rows], rng.random(rows) < 0.8]
    case = cs.make_case(n, kv, 30, rows - 100, values=values, filters=filters)
    case["exists"] = exists
    matrix = np.concatenate([_bsi.build_slices(values, kv, exists, zero_missing=True), np.stack([_bsi.pack_bits(f) for f in filters])])
    foreign = fg.rows_foreign(matrix, n, np.random.default_rng(3), first=first)
    assert {way for way, _ in foreign} == set(fg.WAYS[1:]) and len(foreign) == kv + 3
    operands = []
    for way, stream in foreign:
        assert np.array_equal(oracle.decompress(stream)[:n], matrix[len(operands)]), way
        d = _dev(stream)
        offs, _ = wah.build_index_device(d)
        operands.append((d, offs))
    _run(wah, oracle, case, ("foreign", first), tables=(operands[: kv + 1], operands[kv + 1:]))


# ---- 3: what only the device sees -----------------------------------------------------------------------------------------------------
def _status(wah, case, val, filters):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    flags = _flags(wah, case)
    sc = torch.empty(int(wah.lib().wah_bsi_cumsum_scratch_bytes(case["n"], case["k_out"], flags)), dtype=torch.uint8, device="cuda")
    _call(wah, case, val, filters, check=False, scratch=sc)
    return int(wah.lib().wah_bsi_cumsum_status(sc.data_ptr(), case["n"], case["k_out"], flags, None))


def test_a_bad_operand_is_refused_by_the_status_call_only(wah):
    case = cs.make_case(2 * SEG, 12, 28, None, True, 2, seed=9)
    val, filters = _operands(wah, case)
    val_table, filter_table = wah.bitop_operand_table(val), wah.bitop_operand_table(filters)
    assert _status(wah, case, val_table, filter_table) == 0
    for r, col in ((0, 2), (5, 2), (11, 0), (12, 2), (12, 0)):  # a slice or the existence row without an index, or without a stream
        bad = val_table.clone()
        bad[r, col] = 0
        assert _status(wah, case, bad, filter_table) == WAH_ERR_STREAM, (r, col)
    for r, col in ((0, 0), (1, 2)):
        bad = filter_table.clone()
        bad[r, col] = 0
        assert _status(wah, case, val_table, bad) == WAH_ERR_STREAM, (r, col)
    with pytest.raises(wah.WahError):
        bad = filter_table.clone()
        bad[1, 2] = 0
        _call(wah, case, val_table, bad)
    # a fill of a filter one group shorter: the segment's groups do not add up
    run = np.repeat(np.random.default_rng(2).random(32 * case["n"] // 992) < 0.7, 992)
    case = dict(case, filters=[run])
    val, filters = _operands(wah, case)
    assert _status(wah, case, val, filters) == 0
    words = _host(filters[0][0]).copy()
    fills = np.flatnonzero((words >> 31 == 1) & ((words & 0x3FFFFFFF) >= 2))
    assert fills.size
    words[int(fills[0])] -= 1
    assert _status(wah, case, val, [(_dev(words), filters[0][1])]) == WAH_ERR_STREAM


def test_front_end_refuses_bad_arguments(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(wah.WahError):
        wah.bsi_cumsum_device([(stream, offs)] * 33, SEG, 0, 33, 40)
    with pytest.raises(wah.WahError):
        wah.bsi_cumsum_device([(stream, offs)] * 3, SEG, 0, 3, 65)
    with pytest.raises(wah.WahError):
        wah.bsi_cumsum_device([(stream, offs)] * 3, SEG + 1, 0, 3, 8)
    with pytest.raises(wah.WahError):
        wah.bsi_cumsum_device([(stream, offs)] * 3, SEG, 0, 2, 8)  # a table that does not go with the width
    with pytest.raises(wah.WahError):
        wah.bsi_cumsum_device(None, SEG, 0, 0, 8)                  # nothing that names a device
    with pytest.raises(ValueError):
        wah.columns.cumsum_column(wah, (stream, offs, SEG, 33, False), 0)
    with pytest.raises(ValueError):
        wah.columns.cumsum_column(wah, (stream, offs, SEG, 8, False), 0, n_bits=65)
    with pytest.raises(ValueError):
        wah.columns.row_numbers_where(wah, [], SEG, 0)


# ---- 4: the front ends ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(wah):
    """A table of 2 * 992 * 32 - 50 rows with a 9-bit quantity (an existence bitmap), a 32-bit amount and two filter bitmaps."""
    import torch

    n = 2 * SEG
    rows = 32 * n - 50
    rng = np.random.default_rng(2025)
    qty, amount = _bsi.uniform_values(rng, rows, 9), _bsi.uniform_values(rng, rows, 32)
    qty_exists = rng.random(rows) < 0.9
    f = [rng.random(rows) < 0.7, np.repeat(rng.random(rows // 300 + 1) < 0.6, 300)[:rows]]
    streams = Streams(wah, n)

    def padded(a, dtype):
        out = np.zeros(32 * n, dtype)
        out[: a.size] = a
        return out

    return dict(n=n, rows=rows, qty=qty, amount=amount, qty_exists=qty_exists, f=f,
                d_qty=wah.columns.bsi_from_values(wah, _dev_values(qty), 9, n_words_per_column=n, exists=torch.from_numpy(qty_exists).cuda()),
                d_amount=wah.columns.bsi_from_values(wah, _dev_values(amount), 32, n_words_per_column=n),
                d_f=[streams.of(_bsi.pack_bits(padded(x, bool))) for x in f])


def _np_cumsum(values, mask, exclusive=False):
    x = np.where(mask, values, np.uint64(0)).astype(np.uint64)
    run = np.cumsum(x, dtype=np.uint64)
    return run - x if exclusive else run


def test_cumsum_column_against_numpy(wah, table):
    t = table
    n, rows = t["n"], t["rows"]
    # SUM(qty) OVER (ORDER BY rowid) WHERE f0 AND f1, the attribute's own existence bitmap in the selection
    mask = t["qty_exists"] & t["f"][0] & t["f"][1]
    total = wah.columns.cumsum_column(wah, t["d_qty"], rows, where=t["d_f"])
    assert total[2:] == (n, 9 + rows.bit_length(), True)
    values, have = wah.columns.values_of_column(wah, total, 0, rows)
    assert np.array_equal(have.cpu().numpy(), mask)
    assert np.array_equal(values.cpu().numpy().view(np.uint64), np.where(mask, _np_cumsum(t["qty"], mask), 0))
    values, have = wah.columns.values_of_column(wah, total, rows, 50)
    assert not bool(have.any()) and not bool(values.any())  # rows behind n_rows have no value
    # a 32-bit amount without a filter, exclusive, every row: beyond 2^32 after two rows
    every = np.ones(rows, bool)
    total = wah.columns.cumsum_column(wah, t["d_amount"], rows, exclusive=True, all_rows=True)
    assert total[2:] == (n, 32 + rows.bit_length(), False)
    values, have = wah.columns.values_of_column(wah, total, 0, rows)
    want = _np_cumsum(t["amount"], every, exclusive=True)
    assert int(want[-1]) > 1 << 40 and np.array_equal(values.cpu().numpy().view(np.uint64), want)
    # a single filter as a pair, a width of the caller's: the low 16 bits
    narrow = wah.columns.cumsum_column(wah, t["d_amount"], rows, where=t["d_f"][0], n_bits=16)
    values, have = wah.columns.values_of_column(wah, narrow, 0, rows)
    assert np.array_equal(have.cpu().numpy(), t["f"][0])
    assert np.array_equal(values.cpu().numpy().view(np.uint64), np.where(t["f"][0], _np_cumsum(t["amount"], t["f"][0]) & np.uint64(0xFFFF), 0))
    # the result goes into range_column, compare_columns, kth_column_where and another cumsum_column as it is
    total = wah.columns.cumsum_column(wah, t["d_qty"], rows, where=t["d_f"])
    run = _np_cumsum(t["qty"], mask)
    assert int(run[-1]) > 1 << 20  # (the default width holds it)
    hit, hit_offs = wah.columns.range_column(wah, total, 1000, 200000)
    want_bits = mask & (run >= 1000) & (run <= 200000)
    assert want_bits.any() and int(wah.columns.count_columns(wah, hit, hit_offs, n, [0])[0].item()) == int(want_bits.sum())
    above, above_offs = wah.columns.compare_columns(wah, total, ">", t["d_amount"])
    assert int(wah.columns.count_columns(wah, above, above_offs, n, [0])[0].item()) == int((mask & (run > t["amount"])).sum()) > 0
    again = wah.columns.cumsum_column(wah, total, rows, n_bits=40)
    values, have = wah.columns.values_of_column(wah, again, 0, rows)
    assert np.array_equal(have.cpu().numpy(), mask) and np.array_equal(values.cpu().numpy().view(np.uint64), np.where(mask, _np_cumsum(run, mask), 0))
    assert wah.columns.kth_column_where(wah, total, 0) == (int(run[mask].min()), int(mask.sum()))


def test_row_numbers_where_against_numpy(wah, table):
    t = table
    n, rows = t["n"], t["rows"]
    mask = t["f"][0] & t["f"][1]
    numbers = wah.columns.row_numbers_where(wah, t["d_f"], n, rows)
    assert numbers[2:] == (n, rows.bit_length(), True)
    values, have = wah.columns.values_of_column(wah, numbers, 0, rows)
    want = np.cumsum(mask).astype(np.uint64)
    assert np.array_equal(have.cpu().numpy(), mask) and np.array_equal(values.cpu().numpy().view(np.uint64), np.where(mask, want, 0))
    assert int(values.cpu().numpy().view(np.uint64)[np.flatnonzero(mask)[0]]) == 1  # ROW_NUMBER() starts at 1
    ranks = wah.columns.row_numbers_where(wah, t["d_f"][1], n, rows, exclusive=True, all_rows=True)
    assert ranks[2:] == (n, rows.bit_length(), False)
    values, _ = wah.columns.values_of_column(wah, ranks, 0, rows)
    assert np.array_equal(values.cpu().numpy().view(np.uint64), (np.cumsum(t["f"][1]) - t["f"][1]).astype(np.uint64))


# ---- 5: a chain with nothing read back, and the same as one captured graph -----------------------------------------------------------------
def _chain_want(qty, limit):
    return int((np.cumsum(qty.astype(np.uint64), dtype=np.uint64) <= np.uint64(limit)).sum())


def test_chain_without_a_read_back_and_its_graph_replay(wah, table):
    """bsi_from_values -> cumsum_column -> compare_column(<=, L) -> count_columns, "the rows until the running total passes L", every
    call with check=False into tensors made beforehand: the statuses are read once at the end.  Then the four calls as ONE captured
    graph, replayed after the value column was rewritten in place (capture as the map call's test: side stream, warm-up outside,
    check=False; one chain of launches, no parallel branches)."""
    import torch

    t = table
    n, rows, kv, limit = t["n"], t["rows"], 9, 3_000_000
    k_out = kv + rows.bit_length()
    rng = np.random.default_rng(32)
    columns = [t["qty"], _bsi.uniform_values(rng, rows, kv) >> np.uint64(1), _bsi.uniform_values(rng, rows, kv) | np.uint64(256)]
    values = _dev_values(columns[0])
    lib = wah.lib()
    sc_build = torch.empty(int(lib.wah_bsi_build_scratch_bytes(n, kv)), dtype=torch.uint8, device="cuda")
    sc_sum = torch.empty(int(lib.wah_bsi_cumsum_scratch_bytes(n, k_out, 0)), dtype=torch.uint8, device="cuda")
    sc_range = torch.empty(int(lib.wah_bsi_range_scratch_bytes(n, k_out)), dtype=torch.uint8, device="cuda")
    sc_count = torch.empty(int(lib.wah_select_scratch_bytes(n, 1)), dtype=torch.uint8, device="cuda")
    out_build = torch.empty(wah.max_compressed_words(kv * n), dtype=torch.int32, device="cuda")
    offs_build = torch.zeros(kv * (n // SEG) + 1, dtype=torch.int64, device="cuda")
    out_sum = torch.empty(wah.max_compressed_words((k_out + 1) * n), dtype=torch.int32, device="cuda")
    offs_sum = torch.zeros((k_out + 1) * (n // SEG) + 1, dtype=torch.int64, device="cuda")
    out_range = torch.empty(wah.max_compressed_words(n), dtype=torch.int32, device="cuda")
    offs_range = torch.zeros((wah.max_compressed_words(n) + 1023) // 1024 + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")

    def statuses():
        return (int(lib.wah_bsi_build_status(sc_build.data_ptr(), n, kv, None)), int(lib.wah_bsi_cumsum_status(sc_sum.data_ptr(), n, k_out, 0, None)),
                int(lib.wah_bsi_range_status(sc_range.data_ptr(), n, k_out + 1, None)), int(lib.wah_select_status(sc_count.data_ptr(), None)))

    # the front ends (they build their tables on the device); this is the warm-up outside the capture, too
    wah.bsi_build_device(values, kv, n, scratch=sc_build, out=out_build, out_offsets=offs_build, check=False)
    key = (out_build, offs_build, n, kv, False)
    total = wah.columns.cumsum_column(wah, key, rows, scratch=sc_sum, out=out_sum, out_offsets=offs_sum, check=False)
    assert total[2:] == (n, k_out, True) and total[0].data_ptr() == out_sum.data_ptr()
    hit, _, hit_offs = wah.columns.compare_column(wah, total, "<=", limit, scratch=sc_range, out=out_range, out_offsets=offs_range, check=False)
    wah.columns.count_columns(wah, hit, hit_offs, n, [0], scratch=sc_count, counts=counts, check=False)
    assert statuses() == (0, 0, 0, 0)
    assert 0 < int(counts.item()) == _chain_want(columns[0], limit) < rows
    # the same four calls over tables made beforehand: inside a capture nothing is copied from the host
    val_table = wah.columns._slice_table(key)
    range_table = wah.columns.column_operand_table(out_sum, offs_sum, n, list(range(k_out + 1)))
    count_table = wah.bitop_operand_table([(out_range, offs_range)])
    bounds = wah.bsi_bounds(0, limit, torch.device("cuda:0"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            wah.bsi_build_device(values, kv, n, scratch=sc_build, out=out_build, out_offsets=offs_build, check=False)
            wah.bsi_cumsum_device(val_table, n, rows, kv, k_out, scratch=sc_sum, out=out_sum, out_offsets=offs_sum, check=False)
            wah.bsi_range_device(range_table, bounds, n, exists=True, scratch=sc_range, out=out_range, out_offsets=offs_range, check=False)
            wah.count_device(count_table, n, scratch=sc_count, counts=counts, check=False)
    seen = set()
    for other in columns[1:] + columns[:1]:
        values.copy_(_dev_values(other))  # rewritten in place: the captured calls hold its address
        counts.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert statuses() == (0, 0, 0, 0)
        assert int(counts.item()) == _chain_want(other, limit)
        seen.add(int(counts.item()))
    assert len(seen) == 3  # different answers from one captured chain
