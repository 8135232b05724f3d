"""GPU tests of wah_bsi_kth_grouped_indexed_device: MIN, MAX, the median, the k-th value and quantiles of a bit-sliced attribute PER
GROUP, for every (group, query) pair in one call (include/wah.h), and its front ends in api.py and columns.py.  Every case compares
the five result words of every pair -- found, value, total, less, equal -- with the model that answers from the VALUES
(tests/_kthg.py); everything is exact.  tests/test_kthg_reference.py shows with numpy alone that the shapes used here reach what
they are meant to reach: answers that differ between groups and between the queries of a group, every bucket, both outcomes of
`found`, items that take the short cut and items that do not within one pass, and a wavefront that takes a second item."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _kth, _kthg, _select

pytestmark = pytest.mark.gpu

WAH_ERR_STREAM = -6
SEG = _kthg.SEG_WORDS
U64 = _kth.U64_MAX


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


def _host(t):
    return t.cpu().numpy().view(np.uint32)


class Streams:
    """One indexed compressor of n_words, reused for every row."""

    def __init__(self, wah, n_words):
        self.comp = wah.DeviceCompressor(n_words, indexed=True)

    def of(self, words):
        self.comp.run(_dev(words))
        return self.comp.result().clone(), self.comp.seg_offsets.clone()

    def of_rows(self, selected):
        return self.of(_bsi.pack_bits(selected))


def _hand(stream):
    import torch

    return _dev(stream), torch.from_numpy(_select.index_of(stream)).cuda()


def _tuples(results):
    """[G][Q] five-tuples of Python ints in 0 .. 2^64 - 1"""
    return [[tuple(int(v) & U64 for v in row) for row in group] for group in results.tolist()]


def _operands(wah, case):
    """(filters, groups flat, slices) as lists of (stream, seg_offsets), kept alive by the caller."""
    streams = Streams(wah, case.n_words)
    filters = [streams.of_rows(r) for r in case.filters]
    groups = [streams.of_rows(r) for g in case.groups for r in g]
    slices = [streams.of_rows(r) for r in case.slices()]
    return filters, groups, slices


def _check_case(wah, case):
    filters, groups, slices = _operands(wah, case)
    got = wah.bsi_kth_grouped_device(filters, groups, slices, case.queries, case.n_words, rows_per_group=case.rows_per_group)
    assert tuple(got.shape) == (len(case.groups), len(case.queries), 5)
    got, want = _tuples(got), case.model()
    for g in range(len(want)):
        for q in range(len(case.queries)):
            assert got[g][q] == want[g][q], (case.name, g, case.queries[q])


# ---- 1: sizes x widths, three groups of one row, MIN / median / MAX ---------------------------------------------------------------------
@pytest.mark.parametrize("n", _kthg.SIZES)
@pytest.mark.parametrize("n_bits", _kthg.WIDTHS)
def test_sizes_and_widths_vs_value_model(wah, n, n_bits):
    """No filter, the existence bitmap, existence and a mask."""
    for n_filters in (0, 1, 2):
        _check_case(wah, _kthg.keyed(n, n_bits, n_filters))


def test_one_group_one_query_equals_the_ungrouped_call(wah):
    """G = 1 with Q = 1: the five words of bsi_kth_device over the filter, the group's row and the slices, for every query the
    interface names."""
    import torch

    case = _kthg.keyed(1000, 9, 1, (1,), "min")
    filters, groups, slices = _operands(wah, case)
    assert len(groups) == 1
    table = wah.bitop_operand_table(filters + groups + slices)
    total = int(case.selected(0).sum())
    model = _kth.Model(case.values, case.selected(0))
    for name, kind, a, b in _kth.query_cases(total):
        alone = wah.bsi_kth_device(table, (kind, a, b), case.n_words, 2)
        grouped = wah.bsi_kth_grouped_device(filters, groups, slices, [(kind, a, b)], case.n_words)
        assert torch.equal(grouped.view(5), alone), name
        assert tuple(int(v) & U64 for v in alone.tolist()) == model(kind, a, b), name


def test_two_keys_of_two_rows_per_group(wah):
    _check_case(wah, _kthg.keyed(_kthg.SIZES[-1], 9, 1, (2, 3)))


def test_every_named_query_over_three_groups(wah):
    case = _kthg.keyed(SEG * 2 + 5, 9, 1, (3,), "spread")
    assert case.lanes == 3 * 35
    _check_case(wah, case)


def test_overlapping_repeated_and_empty_groups(wah):
    _check_case(wah, _kthg.overlapping())


@pytest.mark.parametrize("n_filters", [0, 1])
def test_clustered_keys(wah, n_filters):
    """Values sorted by key: a group's row is one zero-fill in most segments, and most items end behind it; one group lives in
    the ragged last segment alone."""
    _check_case(wah, _kthg.clustered(n_filters))


def test_a_wavefront_takes_a_second_item_of_another_lane(wah):
    case = _kthg.second_item()
    assert _kthg.assert_second_item(case) > 0
    _check_case(wah, case)


def test_empty_bitmap(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    queries = [(kind, a, b) for _, kind, a, b in _kth.query_cases(0)]
    for n_filters in (0, 2):
        got = wah.bsi_kth_grouped_device([(stream, offs)] * n_filters, [(stream, offs)] * 4, [(stream, offs)] * 3, queries, 0, rows_per_group=2)
        assert tuple(got.shape) == (2, len(queries), 5) and not got.any()


# ---- 2: pad bits ------------------------------------------------------------------------------------------------------------------
def test_pad_bits_are_never_selected(wah):
    """Hand-built streams that SET pad bits of the last group (tests/_select.py), as a filter, as a group's row and as a slice:
    the selected rows are the positions below 32 * n_words, whatever a stream holds behind them."""
    for what, n, stream, bits in _select.pad_streams():
        rows = 32 * n
        values = _bsi.uniform_values(np.random.default_rng(n), rows, 8)
        selected = np.zeros(rows, bool)
        selected[_select.stream_positions(stream, n)] = True
        assert int(selected.sum()) == bits, what
        streams = Streams(wah, n)
        slices = [streams.of(row) for row in _bsi.build_slices(values, 8)]
        pad, ones = _hand(stream), streams.of_rows(np.ones(rows, bool))
        model = _kth.Model(values, selected)
        want = [model(*q) for q in _kthg.MIN_MEDIAN_MAX]
        for filters, groups, r in (([pad], [ones, pad], 1), ([], [pad, pad], 1), ([pad, pad], [pad, pad, ones, pad], 2)):
            got = _tuples(wah.bsi_kth_grouped_device(filters, groups, slices, _kthg.MIN_MEDIAN_MAX, n, rows_per_group=r))
            assert got == [want, want], (what, len(filters), r)
        # as the ONE slice of a 1-bit attribute, under no filter and a group row that sets the pad bits too: `equal` counts rows
        got = _tuples(wah.bsi_kth_grouped_device(None, [pad], [pad], [(_kth.QUANTILE, 1, 1), (_kth.QUANTILE, 0, 1)], n))
        assert got == [[(1, 1, bits, 0, bits), (1, 1, bits, 0, bits)]] if bits else got[0][0][2] == 0, what
        got = _tuples(wah.bsi_kth_grouped_device(None, [ones], [pad], [(_kth.QUANTILE, 1, 1)], n))
        assert got == [[(1, 1, rows, rows - bits, bits) if bits else (1, 0, rows, 0, rows)]], what


# ---- 3: refusals ------------------------------------------------------------------------------------------------------------------
def _status(wah, filters, groups, slices, queries, n):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    g, q = groups.shape[0], len(queries)
    sc = torch.empty(int(wah.lib().wah_bsi_kth_grouped_scratch_bytes(n, slices.shape[0], g, q)), dtype=torch.uint8, device="cuda:0")
    wah.bsi_kth_grouped_device(filters, groups, slices, queries, n, scratch=sc, check=False)
    return int(wah.lib().wah_bsi_kth_grouped_status(sc.data_ptr(), None))


def _fills(operand, segment):
    """(words, indices of the fills of at least two groups in `segment`)"""
    words, offs = _host(operand[0]).copy(), operand[1].cpu().numpy()
    lo, hi = int(offs[segment]), int(offs[segment + 1])
    return words, lo + np.flatnonzero((words[lo:hi] >> 31 == 1) & ((words[lo:hi] & 0x3FFFFFFF) >= 2))


def _has_fill(operand, segment):
    return _fills(operand, segment)[1].size > 0


def _short_fill(wah, operand, segment):
    """The operand with one fill of `segment` one group short (the segment's words no longer make up its groups)."""
    words, fills = _fills(operand, segment)
    assert fills.size, "no fill to break in that segment"
    words[int(fills[0])] -= 1
    return _dev(words), operand[1]


def test_refusals_depend_neither_on_data_nor_on_queries(wah):
    """Four segments, two groups clustered in segments 0 - 1 and in segment 2; NO group selects anything in segment 3.  A broken
    segment in the filter, in one group's row and in a slice is WAH_ERR_STREAM -- for the slice also in segment 3, and also under
    queries that name no row; the clean tables under the same queries give 0."""
    n, n_bits = SEG * 4, 12
    rng = np.random.default_rng(41)
    rows = 32 * n
    values = _bsi.make_values("clustered", rng, rows, n_bits)
    in_group = [np.zeros(rows, bool), np.zeros(rows, bool)]
    in_group[0][100: 2 * _kthg.SEG_BITS - 50] = True
    in_group[1][2 * _kthg.SEG_BITS + 7: 3 * _kthg.SEG_BITS - 9] = True
    runs = np.repeat(rng.random(rows // 4000 + 1) < 0.7, 4000)[:rows]
    streams = Streams(wah, n)
    f_ops, g_ops = [streams.of_rows(runs)], [streams.of_rows(r) for r in in_group]
    s_ops = [streams.of(row) for row in _bsi.build_slices(values, n_bits)]
    filters, groups, slices = wah.bitop_operand_table(f_ops), wah.bitop_operand_table(g_ops), wah.bitop_operand_table(s_ops)
    query_sets = ([(_kth.QUANTILE, 1, 2), (_kth.DESCENDING, 0, 1)], [(_kth.ASCENDING, U64, 1), (7, 0, 0)])
    for queries in query_sets:
        assert _status(wah, filters, groups, slices, queries, n) == 0
        assert _status(wah, None, groups, slices, queries, n) == 0
    keep = []
    # the last slice with a fill in segment 3 (and in segment 0), broken there
    last = max(i for i in range(n_bits) if _has_fill(s_ops[i], 0) and _has_fill(s_ops[i], 3))
    assert last >= n_bits - 4, "the broken slice lies in the last digit"
    for segment in (3, 0):
        bad = list(s_ops)
        bad[last] = _short_fill(wah, s_ops[last], segment)
        keep.append(bad)
        for queries in query_sets:
            assert _status(wah, filters, groups, wah.bitop_operand_table(bad), queries, n) == WAH_ERR_STREAM, ("slice", segment, queries)
    # a slice of the FIRST digit broken in segment 3, where nothing is selected: only the checking items walk it there
    first_digit = [i for i in range(4) if _has_fill(s_ops[i], 3)]
    assert first_digit
    bad = list(s_ops)
    bad[first_digit[0]] = _short_fill(wah, s_ops[first_digit[0]], 3)
    for queries in query_sets:
        assert _status(wah, filters, groups, wah.bitop_operand_table(bad), queries, n) == WAH_ERR_STREAM, ("first digit", queries)
    # the filter, and group 1's row in a segment where it is one zero-fill
    for queries in query_sets:
        for segment in (0, 3):
            assert _status(wah, wah.bitop_operand_table([_short_fill(wah, f_ops[0], segment)]), groups, slices, queries, n) == WAH_ERR_STREAM
        for g, segment in ((1, 0), (0, 3), (1, 2)):
            bad_groups = list(g_ops)
            bad_groups[g] = _short_fill(wah, g_ops[g], segment)
            assert _status(wah, filters, wah.bitop_operand_table(bad_groups), slices, queries, n) == WAH_ERR_STREAM, (g, segment)
    # a row without an index or a stream, in every table
    for which, r, col in (("f", 0, 2), ("g", 1, 0), ("g", 0, 2), ("s", n_bits - 1, 2), ("s", 0, 0)):
        tables = {"f": filters.clone(), "g": groups.clone(), "s": slices.clone()}
        tables[which][r, col] = 0
        assert _status(wah, tables["f"], tables["g"], tables["s"], query_sets[0], n) == WAH_ERR_STREAM, (which, r, col)
    with pytest.raises(wah.WahError):
        wah.bsi_kth_grouped_device(filters, groups, wah.bitop_operand_table(bad), query_sets[0], n)


def test_front_end_refuses_bad_tables(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    one = [(stream, offs)]
    for filters, groups, slices, queries, r in ((None, one * 3, one * 4, [(0, 0, 1)], 2),      # 3 rows are no groups of 2
                                                (None, one * 9, one * 4, [(0, 0, 1)], 9),      # 9 rows per group
                                                (None, one, one * 65, [(0, 0, 1)], 1),         # 65 slices
                                                (one * 65, one, one, [(0, 0, 1)], 1),          # 65 filters
                                                (None, one * 65, one, [(0, 0, 1)] * 64, 1),    # 4160 lanes
                                                (None, one, one, torch.zeros(3, dtype=torch.int64, device="cuda"), 1),
                                                (None, one, one, torch.zeros((1, 3), dtype=torch.int32, device="cuda"), 1)):
        with pytest.raises(wah.WahError):
            wah.bsi_kth_grouped_device(filters, groups, slices, queries, 0, rows_per_group=r)
    with pytest.raises(wah.WahError):
        wah.bsi_kth_grouped_device(None, one, one, [(0, 0, 1)], 0, results=torch.zeros((1, 1, 4), dtype=torch.int64, device="cuda"))


# ---- 4: pointer placement, graph replay ---------------------------------------------------------------------------------------------
def test_pointer_placement(wah):
    """The three tables, the queries and the results at 8-byte offsets that are not 16-byte aligned."""
    import torch

    case = _kthg.keyed(SEG + 8, 9, 1, (2, 3))
    filters, groups, slices = _operands(wah, case)

    def moved(t):
        flat = torch.zeros(t.numel() + 1, dtype=torch.int64, device="cuda")
        view = flat[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 8
        return view

    tables = [moved(wah.bitop_operand_table(ops)) for ops in (filters, groups, slices)]
    queries = moved(wah.bsi_kth_queries(case.queries, "cuda:0"))
    results = moved(torch.zeros((len(case.groups), len(case.queries), 5), dtype=torch.int64, device="cuda"))
    got = wah.bsi_kth_grouped_device(tables[0], tables[1], tables[2], queries, case.n_words, rows_per_group=2, results=results)
    assert got is results and _tuples(got) == case.model()


def test_graph_replay_with_other_queries_and_another_group_row(wah):
    """Tables and queries are only ever read by the device: ONE captured call, replayed after the queries AND one group's row were
    overwritten in place, answers the new question (a linear capture on a side stream, warm-up outside, check=False)."""
    import torch

    n, n_bits = SEG * 2 + 3, 20
    rng = np.random.default_rng(2)
    rows = 32 * n
    values = _bsi.uniform_values(rng, rows, n_bits)
    key = rng.integers(0, 5, rows)
    mask = rng.random(rows) < 0.6
    streams = Streams(wah, n)
    f_ops, s_ops = [streams.of_rows(mask)], [streams.of(row) for row in _bsi.build_slices(values, n_bits)]
    k_ops = [streams.of_rows(key == v) for v in range(5)]
    filters, slices = wah.bitop_operand_table(f_ops), wah.bitop_operand_table(s_ops)
    every = wah.bitop_operand_table(k_ops)
    groups = every[:3].clone()
    queries = wah.bsi_kth_queries(_kthg.MIN_MEDIAN_MAX, "cuda:0")
    sc = torch.empty(int(wah.lib().wah_bsi_kth_grouped_scratch_bytes(n, n_bits, 3, 3)), dtype=torch.uint8, device="cuda:0")
    res = torch.zeros((3, 3, 5), dtype=torch.int64, device="cuda:0")
    call = lambda: wah.bsi_kth_grouped_device(filters, groups, slices, queries, n, scratch=sc, results=res, check=False)  # noqa: E731
    call()  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    seen = set()
    for own, asked in (((0, 1, 2), _kthg.MIN_MEDIAN_MAX), ((0, 4, 2), [(_kth.DESCENDING, 3, 1), (_kth.QUANTILE, 99, 100), (_kth.ASCENDING, U64, 1)]),
                       ((3, 4, 2), [(_kth.ASCENDING, 17, 1), (_kth.QUANTILE, 1, 3), (_kth.DESCENDING, 0, 1)])):
        wah.bsi_kth_queries(asked, out=queries)
        for g, v in enumerate(own):
            groups[g].copy_(every[v])
        torch.cuda.synchronize()
        res.fill_(0x5A5A5A5A)
        graph.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bsi_kth_grouped_status(sc.data_ptr(), None) == 0
        want = [[_kth.Model(values, mask & (key == v))(*q) for q in asked] for v in own]
        assert _tuples(res) == want, (own, asked)
        seen.add(str(want))
    assert len(seen) == 3


# ---- 5: the column front end --------------------------------------------------------------------------------------------------------
def test_quantiles_by_end_to_end(wah):
    """SELECT a, b, MIN(y), MAX(y) WHERE lo <= x <= hi GROUP BY a, b over 100 000 rows (the shape of test_gpu_group_sum.py's end to
    end test): quantiles_by(["min", "max"]) equals extremes_by, and with more queries it equals the value model."""
    import torch

    rows = 100_000
    rng = np.random.default_rng(21)
    a, b = rng.integers(0, 3, rows), rng.integers(0, 2, rows)
    x, y = rng.integers(0, 1 << 12, rows), rng.integers(0, 1 << 20, rows)
    lo, hi = 300, 3500
    x[a == 2] = rng.integers(0, lo, int((a == 2).sum()))
    y_exists = rng.random(rows) < 0.7
    chosen = (x >= lo) & (x <= hi)
    cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64)).cuda()  # noqa: E731
    st_a, offs_a, n = wah.columns.index_from_keys(wah, cuda(a), 3)
    st_b, offs_b, _ = wah.columns.index_from_keys(wah, cuda(b), 2)
    bsi_x = wah.columns.bsi_from_values(wah, cuda(x), 12)
    bsi_y = wah.columns.bsi_from_values(wah, cuda(y), 20, exists=torch.from_numpy(y_exists).cuda())
    where = wah.columns.range_column(wah, bsi_x, lo, hi)
    keys = [(st_a, offs_a, [0, 1, 2]), (st_b, offs_b, torch.arange(2, dtype=torch.int64, device="cuda"))]
    low, high = wah.columns.extremes_by(wah, keys, bsi_y, n, where=where)
    got = wah.columns.quantiles_by(wah, keys, bsi_y, n, ["min", "max"], where=where)
    assert got["values"].shape == (3, 2, 2) and got["values"].dtype == object
    assert np.array_equal(got["values"][..., 0], low) and np.array_equal(got["values"][..., 1], high)
    assert low[2, 0] is None and low[0, 0] is not None
    asked = ["min", "median", (99, 100), (_kth.DESCENDING, 2, 1), "max", (_kth.ASCENDING, 1 << 40, 1)]
    got = wah.columns.quantiles_by(wah, keys, bsi_y, n, asked, where=[where, where])
    triples = wah.columns._quantile_queries(wah, asked)
    for name in ("totals", "less", "equal"):
        assert str(got[name].dtype) == "torch.int64" and tuple(got[name].shape) == (3, 2, len(asked)), name
    for i in range(3):
        for j in range(2):
            model = _kth.Model(y.astype(np.uint64), chosen & y_exists & (a == i) & (b == j))
            for q, triple in enumerate(triples):
                found, value, total, less, equal = model(*triple)
                assert got["values"][i, j, q] == (value if found else None), (i, j, triple)
                assert (int(got["totals"][i, j, q]), int(got["less"][i, j, q]), int(got["equal"][i, j, q])) == (total, less, equal), (i, j, triple)
    # one key, no where, an attribute without an existence bitmap: the column's rows behind the table's belong to no group
    got = wah.columns.quantiles_by(wah, keys[1:], bsi_x, n, ["min", "max"])
    assert [tuple(got["values"][j]) for j in range(2)] == [(int(x[b == j].min()), int(x[b == j].max())) for j in range(2)]
    assert got["totals"].cpu().tolist() == [[int((b == j).sum())] * 2 for j in range(2)]
