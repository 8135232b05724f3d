"""GPU tests of wah_bsi_kth_indexed_device: MIN, MAX, the k-th value and quantiles of a bit-sliced attribute among the rows a set of
filters selects, in one call (include/wah.h), and its front ends in api.py and columns.py.  Every case compares the five result
words -- found, value, total, less, equal -- with the model that answers from the VALUES (tests/_kth.py); everything is exact.

Sizes: 31, 992, 1000 and 992 * 9 + 17 words -- less than a segment, exactly one, a ragged one, several workgroups with a ragged
end.  Widths: 1, 3, 4, 5, 8, 9, 20, 63 and 64 slices -- a single short digit, and a digit boundary and one slice to either side of
it for every digit width from 2 to 4.  tests/test_kth_reference.py shows with numpy alone that these cases reach every kind of
query, every bucket and both outcomes of `found`."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _kth, _select

pytestmark = pytest.mark.gpu

WAH_ERR_STREAM = -6
SEG = 992
U64 = _kth.U64_MAX
SIZES = [31, SEG, 1000, SEG * 9 + 17]
WIDTHS = [1, 3, 4, 5, 8, 9, 20, 63, 64]


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


def _answers(wah, table, n, n_filters, queries):
    """The result words of every query (name, kind, a, b) over one table, each call checked, read back together."""
    import torch

    results = torch.empty((len(queries), 5), dtype=torch.int64, device="cuda")
    scratch = torch.empty(int(wah.lib().wah_bsi_kth_scratch_bytes(n, table.shape[0] - n_filters)), dtype=torch.uint8, device="cuda")
    for row, (_, kind, a, b) in zip(results, queries):
        wah.bsi_kth_device(table, (kind, a, b), n, n_filters, scratch=scratch, result=row)
    return [tuple(int(v) & U64 for v in row) for row in results.tolist()]


def _check(wah, ops, n, n_filters, values, selected, what, queries=None):
    """ops: the filters' and the slices' (stream, seg_offsets), kept alive here; selected: the bool rows the filters select."""
    model = _kth.Model(values, selected)
    queries = _kth.query_cases(model.total) if queries is None else queries
    table = wah.bitop_operand_table(ops)
    for (name, kind, a, b), got in zip(queries, _answers(wah, table, n, n_filters, queries)):
        assert got == model(kind, a, b), (what, name, kind, a, b)


# ---- 1: sizes x widths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("n_bits", WIDTHS)
def test_sizes_and_widths_vs_value_model(wah, n, n_bits):
    """Uniform values over the full width, every query the interface names: without a filter, under the existence bitmap, and
    under existence and a mask (two filters).  64 slices do not go through bsi_from_values: the slice matrix is compressed here."""
    rng = np.random.default_rng(31 * n + n_bits)
    rows = 32 * n
    values = _bsi.uniform_values(rng, rows, n_bits)
    exists, mask = rng.random(rows) < 0.9, rng.random(rows) < 0.4
    streams = Streams(wah, n)
    slices = [streams.of(row) for row in _bsi.build_slices(values, n_bits)]
    _check(wah, slices, n, 0, values, None, (n, n_bits, "no filter"))
    d_exists, d_mask = streams.of_rows(exists), streams.of_rows(mask)
    _check(wah, [d_exists] + slices, n, 1, values, exists, (n, n_bits, "existence"))
    _check(wah, [d_mask, d_exists] + slices, n, 2, values, exists & mask, (n, n_bits, "two filters"))


# ---- 2: kinds of values, kinds of masks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["low", "high", "clustered", "equal", "ties"])
@pytest.mark.parametrize("n_bits", [9, 20])
def test_value_kinds(wah, kind, n_bits):
    """low / high: the top slices are one fill per segment (settled in the gather, or a fill with an effect); clustered: fills in
    every slice; all rows equal; two values whose ties straddle the boundary between segments 3 and 4."""
    n = SIZES[-1]
    rng = np.random.default_rng(n_bits + len(kind))
    rows = 32 * n
    values = _kth.value_sets(rng, rows, n_bits, 4 * 32 * SEG)[kind]
    if kind == "ties":
        assert values[4 * 32 * SEG - 1] != values[4 * 32 * SEG + 7] and values[4 * 32 * SEG] == values[4 * 32 * SEG - 1]
    sparse = rng.random(rows) < 0.01
    streams = Streams(wah, n)
    slices = [streams.of(row) for row in _bsi.build_slices(values, n_bits)]
    _check(wah, slices, n, 0, values, None, (kind, n_bits, "no filter"))
    _check(wah, [streams.of_rows(sparse)] + slices, n, 1, values, sparse, (kind, n_bits, "sparse mask"))


@pytest.mark.parametrize("n", [SEG, SIZES[-1]])
def test_masks(wah, n):
    """A mask of one row (total 1), a dense one, an all-zero fill (total 0), all ones."""
    n_bits = 20
    rng = np.random.default_rng(n)
    rows = 32 * n
    values = _bsi.make_values("uniform", rng, rows, n_bits)
    streams = Streams(wah, n)
    slices = [streams.of(row) for row in _bsi.build_slices(values, n_bits)]
    masks = _kth.mask_sets(rng, rows)
    assert masks["one row"].sum() == 1 and not masks["zeros"].any() and masks["ones"].all()
    for name in ("one row", "dense", "zeros", "ones"):
        _check(wah, [streams.of_rows(masks[name])] + slices, n, 1, values, masks[name], (n, name))


def test_empty_bitmap(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    for n_filters in (0, 2):
        table = wah.bitop_operand_table([(stream, offs)] * (n_filters + 3))
        for got in _answers(wah, table, 0, n_filters, _kth.query_cases(0)):
            assert got == (0, 0, 0, 0, 0)


def test_pad_bits_are_never_selected(wah):
    """Hand-built filter streams that SET pad bits of the last group (tests/_select.py): the selected rows are the positions below
    32 * n_words, whatever the stream holds behind them."""
    import torch

    for what, n, stream, bits in _select.pad_streams():
        rows = 32 * n
        values = _bsi.uniform_values(np.random.default_rng(n), rows, 8)
        selected = np.zeros(rows, bool)
        selected[_select.stream_positions(stream, n)] = True
        assert int(selected.sum()) == bits, what
        streams = Streams(wah, n)
        slices = [streams.of(row) for row in _bsi.build_slices(values, 8)]
        pad_filter = (_dev(stream), torch.from_numpy(_select.index_of(stream)).cuda())
        _check(wah, [pad_filter] + slices, n, 1, values, selected, what)
        _check(wah, [pad_filter, pad_filter] + slices, n, 2, values, selected, (what, "twice"))


def test_unchecked_filter_output_as_mask(wah):
    """The mask is the not-yet-checked output of filter_columns on the stream, named with the buffer's capacity as its length."""
    import torch

    n, n_bits = SEG * 2, 12
    rng = np.random.default_rng(77)
    rows = 32 * n
    values = _bsi.uniform_values(rng, rows, n_bits)
    keys = rng.integers(0, 8, rows)
    key_stream, key_offsets, key_n = wah.columns.index_from_keys(wah, torch.from_numpy(keys).cuda(), 8)
    assert key_n == n
    streams = Streams(wah, n)
    slices = [streams.of(row) for row in _bsi.build_slices(values, n_bits)]
    out, _, out_offsets = wah.columns.filter_columns(wah, [(key_stream, key_offsets, [1, 3, 6], False)], n, check=False)
    assert out.numel() == wah.max_compressed_words(n)  # the whole buffer: its capacity is the row's length
    _check(wah, [(out, out_offsets)] + slices, n, 1, values, np.isin(keys, [1, 3, 6]), "unchecked filter output")


def test_pointer_placement(wah):
    """Streams shifted by 4 bytes, the table, the query and the result at 8-byte offsets."""
    import torch

    n, n_bits = SEG + 8, 9
    rng = np.random.default_rng(5)
    rows = 32 * n
    values = _bsi.uniform_values(rng, rows, n_bits)
    mask = rng.random(rows) < 0.5
    streams = Streams(wah, n)
    ops = []
    for words in [_bsi.pack_bits(mask)] + list(_bsi.build_slices(values, n_bits)):
        stream, offs = streams.of(words)
        shifted = torch.empty(stream.numel() + 1, dtype=torch.int32, device="cuda")
        shifted[1:] = stream
        assert shifted[1:].data_ptr() % 8 == 4
        ops.append((shifted[1:], offs))
    table = wah.bitop_operand_table(ops)
    flat = torch.zeros(table.numel() + 1, dtype=torch.int64, device="cuda")
    moved = flat[1:].view(-1, 3)
    moved.copy_(table)
    pool = torch.zeros(16, dtype=torch.int64, device="cuda")
    query, result = pool[1:4], pool[5:10]
    assert moved.data_ptr() % 16 != table.data_ptr() % 16 and query.data_ptr() % 16 == 8 and result.data_ptr() % 16 == 8
    model = _kth.Model(values, mask)
    for _, kind, a, b in _kth.query_cases(model.total):
        wah.bsi_kth_query(kind, a, b, out=query)
        got = wah.bsi_kth_device(moved, query, n, 1, result=result)
        assert tuple(int(v) & U64 for v in got.tolist()) == model(kind, a, b), (kind, a, b)


# ---- 3: graph replay ------------------------------------------------------------------------------------------------------------
def test_graph_replay_with_another_query(wah):
    """The query is only ever read by the device: ONE captured call, replayed after it was overwritten in place, answers the new
    query (capture as the range call's test: side stream, warm-up outside, check=False; one chain of launches)."""
    import torch

    n, n_bits = SEG * 2 + 3, 20
    rng = np.random.default_rng(2)
    rows = 32 * n
    values = _bsi.uniform_values(rng, rows, n_bits)
    mask = rng.random(rows) < 0.3
    streams = Streams(wah, n)
    ops = [streams.of_rows(mask)] + [streams.of(row) for row in _bsi.build_slices(values, n_bits)]
    table = wah.bitop_operand_table(ops)
    query = wah.bsi_kth_query(_kth.QUANTILE, 1, 2, "cuda:0")
    sc = torch.empty(int(wah.lib().wah_bsi_kth_scratch_bytes(n, n_bits)), dtype=torch.uint8, device="cuda:0")
    res = torch.zeros(5, dtype=torch.int64, device="cuda:0")
    wah.bsi_kth_device(table, query, n, 1, scratch=sc, result=res, check=False)  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            wah.bsi_kth_device(table, query, n, 1, scratch=sc, result=res, check=False)
    model = _kth.Model(values, mask)
    seen = set()
    for kind, a, b in ((_kth.QUANTILE, 0, 1), (_kth.DESCENDING, 0, 1), (_kth.ASCENDING, model.total // 5, 1), (_kth.ASCENDING, model.total, 1),
                       (_kth.QUANTILE, 1, 2), (_kth.DESCENDING, 99, 1)):
        wah.bsi_kth_query(kind, a, b, out=query)
        torch.cuda.synchronize()
        res.fill_(0x5A5A5A5A)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bsi_kth_status(sc.data_ptr(), None) == 0
        got = tuple(int(v) & U64 for v in res.tolist())
        assert got == model(kind, a, b), (kind, a, b)
        seen.add(got)
    assert len(seen) == 6  # six different answers from one captured call


# ---- 4: refusals ----------------------------------------------------------------------------------------------------------------
def _status(wah, table, query, n, n_filters):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    sc = torch.empty(int(wah.lib().wah_bsi_kth_scratch_bytes(n, table.shape[0] - n_filters)), dtype=torch.uint8, device="cuda:0")
    wah.bsi_kth_device(table, query, n, n_filters, scratch=sc, check=False)
    return int(wah.lib().wah_bsi_kth_status(sc.data_ptr(), None))


def test_refusals_depend_neither_on_data_nor_on_query(wah):
    """A malformed segment in a slice of the LAST digit, under a mask that selects nothing, is still WAH_ERR_STREAM, whatever the
    query; so are a bad filter row, an empty fill and a row without an index or a stream."""
    n, n_bits = SEG * 4, 12
    rng = np.random.default_rng(41)
    rows = 32 * n
    values = _bsi.make_values("clustered", rng, rows, n_bits)
    streams = Streams(wah, n)
    for mask in (np.zeros(rows, bool), rng.random(rows) < 0.5):
        ops = [streams.of_rows(mask)] + [streams.of(row) for row in _bsi.build_slices(values, n_bits)]
        table = wah.bitop_operand_table(ops)
        queries = [(_kth.QUANTILE, 1, 2), (_kth.ASCENDING, U64, 1), (7, 0, 0), (_kth.DESCENDING, 0, 1)]
        for q in queries:
            assert _status(wah, table, q, n, 1) == 0
        source = n_bits  # the last slice: table row 1 + n_bits - 1
        words = _host(ops[source][0]).copy()
        fills = np.flatnonzero((words >> 31 == 1) & ((words & 0x3FFFFFFF) >= 2))
        assert fills.size, "a clustered slice has fills"
        at = int(fills[fills.size // 2])
        for name, word in (("short fill", words[at] - 1), ("empty fill", words[at] & 0xC0000000)):
            broken = words.copy()
            broken[at] = word
            for r in (n_bits, n_bits - 2, 5, 1, 0):  # the last slice, another one of the last digit, one of the middle digit, the first, the filter
                bad_rows = list(ops)
                bad_rows[r] = (_dev(broken), ops[source][1])
                bad_table = wah.bitop_operand_table(bad_rows)
                for q in queries:
                    assert _status(wah, bad_table, q, n, 1) == WAH_ERR_STREAM, (name, r, q)
            with pytest.raises(wah.WahError):
                wah.bsi_kth_device(bad_table, queries[0], n, 1)
        for r, col in ((0, 2), (1, 2), (n_bits, 2), (n_bits, 0), (0, 0)):
            t = table.clone()
            t[r, col] = 0
            for q in queries[:2]:
                assert _status(wah, t, q, n, 1) == WAH_ERR_STREAM, (r, col, q)


def test_front_end_refuses_bad_tables(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(wah.WahError):
        wah.bsi_kth_device([(stream, offs)] * 66, (0, 0, 1), 0, 1)  # 65 slices
    with pytest.raises(wah.WahError):
        wah.bsi_kth_device([(stream, offs)] * 66, (0, 0, 1), 0, 65)  # 65 filters
    with pytest.raises(wah.WahError):
        wah.bsi_kth_device([(stream, offs)], (0, 0, 1), 0, 1)  # no slice
    with pytest.raises(wah.WahError):
        wah.bsi_kth_device([(stream, offs)], torch.zeros(3, dtype=torch.int32, device="cuda"), 0, 0)


# ---- 5: the column front ends ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attribute(wah):
    """Over the same 32 * 992 * 2 rows: a 20-bit attribute with an existence bitmap, a 6-bit one without (many ties), and an
    equality-encoded attribute of 8 bins whose bins 1 and 3 are the mask."""
    import torch

    n = SEG * 2
    rng = np.random.default_rng(3)
    rows = 32 * n
    values = _bsi.uniform_values(rng, rows, 20)
    small = _bsi.uniform_values(rng, rows, 6)
    exists = rng.random(rows) < 0.9
    keys = rng.integers(0, 8, rows)
    bsi = wah.columns.bsi_from_values(wah, torch.from_numpy(values.view(np.int64)).cuda(), 20, exists=torch.from_numpy(exists).cuda())
    bsi_small = wah.columns.bsi_from_values(wah, torch.from_numpy(small.view(np.int64)).cuda(), 6)
    index = wah.columns.index_from_keys(wah, torch.from_numpy(keys).cuda(), 8)
    mask = wah.columns.filter_columns(wah, [(index[0], index[1], [1, 3], False)], n)
    return dict(n=n, values=values, small=small, exists=exists, in_mask=np.isin(keys, [1, 3]), bsi=bsi, bsi_small=bsi_small, mask=mask, index=index)


def test_min_max_median_kth(wah, attribute):
    c = wah.columns
    values, exists, in_mask = attribute["values"], attribute["exists"], attribute["in_mask"]
    for mask, selected in ((None, exists), (attribute["mask"], exists & in_mask)):
        chosen = np.sort(values[selected])
        total = int(chosen.size)
        assert c.min_column_where(wah, attribute["bsi"], mask) == (int(chosen[0]), total)
        assert c.max_column_where(wah, attribute["bsi"], mask) == (int(chosen[-1]), total)
        assert c.median_column_where(wah, attribute["bsi"], mask) == (int(chosen[(total - 1) // 2]), total)
        assert c.quantile_column_where(wah, attribute["bsi"], 99, 100, mask) == (int(chosen[99 * (total - 1) // 100]), total)
        for k in (0, 7, total - 1):
            assert c.kth_column_where(wah, attribute["bsi"], k, mask) == (int(chosen[k]), total)
            assert c.kth_column_where(wah, attribute["bsi"], k, mask, largest=True) == (int(chosen[total - 1 - k]), total)
        assert c.kth_column_where(wah, attribute["bsi"], total, mask) == (None, total)
    # an attribute without an existence bitmap: every row counts
    small = np.sort(attribute["small"])
    assert c.median_column_where(wah, attribute["bsi_small"]) == (int(small[(small.size - 1) // 2]), small.size)
    nothing = wah.columns.filter_columns(wah, [(attribute["index"][0], attribute["index"][1], [1], False), (attribute["index"][0], attribute["index"][1], [2], False)], attribute["n"])
    assert c.min_column_where(wah, attribute["bsi"], nothing) == (None, 0)


@pytest.mark.parametrize("largest", [True, False])
def test_top_rows(wah, attribute, largest):
    """ORDER BY value LIMIT k against a stable argsort of the model: the rows strictly beyond the threshold come first (as a set:
    they are listed in row order), then the first ties in row order -- exactly the rows a stable sort takes."""
    cases = ((attribute["bsi"], attribute["values"], attribute["exists"], 20), (attribute["bsi_small"], attribute["small"], np.ones(attribute["small"].size, bool), 6))
    for bsi, values, have, n_bits in cases:
        for mask, selected in ((None, have), (attribute["mask"], have & attribute["in_mask"])):
            rows = np.flatnonzero(selected)
            key = values[rows] if not largest else np.uint64((1 << n_bits) - 1) - values[rows]
            order = rows[np.argsort(key, kind="stable")]
            for k in (1, 10, 1000, rows.size, rows.size + 5):
                got = wah.columns.top_rows(wah, bsi, k, mask, largest=largest).cpu().numpy()
                want = order[:k]
                assert got.size == want.size, (n_bits, k)
                threshold = values[want[-1]]
                better = int((values[want] != threshold).sum())
                assert np.array_equal(np.sort(got[:better]), np.sort(want[:better])), (n_bits, k, "strictly better")
                assert np.array_equal(got[better:], want[better:]), (n_bits, k, "ties in row order")
                assert np.array_equal(got[:better], np.sort(got[:better]))
            assert wah.columns.top_rows(wah, bsi, 0, mask, largest=largest).numel() == 0
    nothing = wah.columns.filter_columns(wah, [(attribute["index"][0], attribute["index"][1], [1], False), (attribute["index"][0], attribute["index"][1], [2], False)], attribute["n"])
    assert wah.columns.top_rows(wah, attribute["bsi"], 5, nothing, largest=largest).numel() == 0
