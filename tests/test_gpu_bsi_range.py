"""GPU tests of wah_bsi_range_indexed_device: `lo <= value <= hi` over a bit-sliced attribute in one call (include/wah.h), and its
front ends in api.py and columns.py.  Everything is exact: the result's words, their count and its segment index against
compress() of the bitmap computed with numpy FROM THE VALUES (tests/_bsi.py) -- the CPU oracle and an indexed compress of it.

The sweeps run at 1, 31, 992 and 992 * 3 + 5 words and 1, 2, 20, 63 and 64 slices, without and with an existence row (64 slices
and an existence row are 65 table rows: the existence row alone in the second chunk of 64; 63 and one are exactly one chunk),
over every bound edge the interface names.  For the headline case of a size the test first asserts, with numpy alone, that it can
fail: the expected bitmap is neither all zeros nor all ones, every single bit of either bound changes it, and so does the
existence row."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _kth

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6
SEG = 992


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
    """One indexed compressor of n_words, reused for the operands and for the expected results' segment indexes."""

    def __init__(self, wah, n_words):
        self.comp = wah.DeviceCompressor(n_words, indexed=True)

    def of(self, words):
        self.comp.run(_dev(words))
        return self.comp.result().clone(), self.comp.seg_offsets.clone()


def _same(streams, oracle, got, offs, combined, what):
    """(got, offs) is exactly compress(combined) and its segment index."""
    combined = np.ascontiguousarray(combined, dtype=np.uint32)
    want = oracle.compress(combined)
    assert got.numel() == want.size, (what, got.numel(), want.size)
    assert np.array_equal(_host(got), want), what
    _, ref_offs = streams.of(combined)
    assert np.array_equal(offs.cpu().numpy(), ref_offs.cpu().numpy()), what


def _check_cases(wah, oracle, streams, values, n_bits, exists, cases, n, what):
    ops = [streams.of(row) for row in _bsi.build_slices(values, n_bits, exists)]  # (the table holds raw pointers: ops stays alive)
    table = wah.bitop_operand_table(ops)
    for name, lo, hi in cases:
        got, offs = wah.bsi_range_device(table, (lo, hi), n, exists=exists is not None)
        _same(streams, oracle, got, offs, _bsi.expected_range(values, lo, hi, exists), (what, name, lo, hi))


# ---- 1: the sweeps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, SEG, SEG * 3 + 5])
@pytest.mark.parametrize("n_bits,with_exists", [(1, False), (2, False), (2, True), (20, False), (20, True), (63, False), (63, True), (64, False), (64, True)])
def test_sweep_vs_value_model(wah, oracle, n, n_bits, with_exists):
    """Uniform values over the full width (incompressible slices: 8 batches of 128 literals per segment), every bound edge case; the
    headline range first, shown to be able to fail before anything is launched."""
    what = (n, n_bits, with_exists)
    if n >= 31:
        values, exists, lo, hi = _bsi.headline(n, n_bits, with_exists)
        _bsi.assert_range_matters(values, n_bits, lo, hi, exists, what)
        cases = [("headline", lo, hi)]
    else:  # 32 rows have no room for the bounds' neighbours
        rng = np.random.default_rng(n_bits)
        values = _bsi.uniform_values(rng, 32 * n, n_bits)
        exists = rng.random(32 * n) < 0.9 if with_exists else None
        cases = []
    _check_cases(wah, oracle, Streams(wah, n), values, n_bits, exists, cases + _bsi.bound_cases(values, n_bits), n, what)


@pytest.mark.parametrize("kind", ["low", "high", "clustered"])
@pytest.mark.parametrize("n_bits", [20, 64])
@pytest.mark.parametrize("existence", ["none", "dense", "empty segment"])
def test_value_kinds(wah, oracle, kind, n_bits, existence):
    """low: the top 10 slices are all zero -- settled in the gather, and still folded, under bound bits 0 and 1; high: the top 10 are
    all ones (one fill with an effect per segment); clustered: values constant over runs of some thousand rows, fills with an
    effect in every slice.  Existence: none, density 0.9, and 0.9 with a whole segment of rows that do not exist."""
    n = SEG * 3 + 5
    what = (kind, n_bits, existence)
    values, exists, lo, hi = _bsi.headline(n, n_bits, existence != "none", kind, empty=(32 * SEG, 64 * SEG) if existence == "empty segment" else None)
    if existence == "empty segment":
        assert not _bsi.pack_bits(exists)[SEG: 2 * SEG].any() and _bsi.pack_bits(exists)[2 * SEG:].any()
    top, half = (1 << n_bits) - 1, 1 << (n_bits - 1)
    cases = [("headline", lo, hi)] + _bsi.bound_cases(values, n_bits)
    present = int(values[17])
    low10 = (1 << (n_bits - 10)) - 1
    # bounds whose top bits are 0 and 1 against slices that are all zero / all one there
    cases += [("top bits 0", present & low10, (present & low10) + 1000), ("top bits 1", (present & low10) | (top - low10), top),
              ("lo top bit", half, top), ("hi top bit", present >> 1, half | (present >> 1)), ("below all of high", 0, top - low10 - 1),
              ("above all of low", low10 + 1, top)]
    _bsi.assert_range_matters(values, n_bits, lo, hi, exists, what)
    # (the headline range of the full width selects little besides the planted rows of low and high values: one inside the values too)
    ordered = np.sort(values)
    inner_lo, inner_hi = int(ordered[values.size // 3]), int(ordered[2 * values.size // 3])
    want = _bsi.expected_range(values, inner_lo, inner_hi, exists)
    assert want.any() and not (want == _bsi.ONES).all()
    cases.append(("inner thirds", inner_lo, inner_hi))
    _check_cases(wah, oracle, Streams(wah, n), values, n_bits, exists, cases, n, what)


def test_empty_bitmap(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    for exists in (False, True):
        got, out_offs = wah.bsi_range_device([(stream, offs)] * (3 + exists), (0, 5), 0, exists=exists)
        assert got.numel() == 0 and int(out_offs[0].item()) == 0


def test_rows_without_existence_match_zero(wah, oracle):
    """Without an existence bitmap a row whose slices are all zero has the value 0: it matches exactly when lo == 0."""
    n = SEG + 7
    values = np.zeros(32 * n, np.uint64)
    values[:1000] = np.arange(1, 1001, dtype=np.uint64)  # the caller's own 1000 rows, none of value 0
    streams = Streams(wah, n)
    _check_cases(wah, oracle, streams, values, 12, None, [("lo 0", 0, 500), ("lo 1", 1, 500), ("all", 0, 4095), ("eq 0", 0, 0)], n, "no existence")
    exists = np.arange(32 * n) < 1000
    _check_cases(wah, oracle, streams, values, 12, exists, [("lo 0", 0, 500), ("lo 1", 1, 500), ("all", 0, 4095), ("eq 0", 0, 0)], n, "existence")


def test_settled_rows_on_both_sides_of_the_chunk_edge_are_folded(wah, oracle):
    """The one property the shared walk (list_walk, wah_list_walk.hpp) keeps for its four callers at once: a row whose segment
    was settled in the gather -- one zero fill, never a batch -- is still folded, on either side of the edge between two chunks
    of 64 table rows.  992 + 31 words: two segments, the second one ragged.  Values are 64-bit multiples of 16, so slices 60 .. 63
    are all zero.
      range    64 slices + existence, 65 rows: rows 60 .. 63 are zero fills, row 64, the first of the second chunk, folds them;
               bounds whose low four bits are not zero, so that a zero slice skipped changes the result;
      k-th     two filters + 64 slices, 66 rows: the zero slices are rows 62 .. 65, the last digit of the last pass;
      clauses  ends 63, 64 and 66, operands 62 .. 65 empty: the second clause is one empty operand, the third two;
      list     OR of 66 operands of which 62 .. 65 are empty.
    Expected: tests/_bsi.py and tests/_kth.py from the values, the numpy fold of the operands through the oracle."""
    n = SEG + 31
    rows = 32 * n
    rng = np.random.default_rng(6466)
    values = _bsi.uniform_values(rng, rows, 64) & np.uint64(~0xF & _bsi.U64_MAX)
    exists, mask = rng.random(rows) < 0.9, rng.random(rows) < 0.4
    streams = Streams(wah, n)
    matrix = _bsi.build_slices(values, 64, exists)
    assert matrix.shape[0] == 65 and matrix[:60].any(axis=1).all() and not matrix[60:64].any()
    ops = [streams.of(row) for row in matrix]
    assert all(st.numel() == 2 for st, _ in ops[60:64])  # one fill word per segment

    # range: a present value a is below a + 1 and b is above b - 1 only if the zero slices under the bounds' low bits are folded
    ordered = np.sort(values[exists])
    a, b = int(ordered[ordered.size // 4]), int(ordered[3 * ordered.size // 4])
    cases = [("low bits 0001 / 1111", a + 1, b - 1), ("low bits 1111 / 0001", a - 1, b + 1), ("present bounds", a, b), ("one value", a, a)]
    assert not np.array_equal(_bsi.expected_range(values, a + 1, b - 1, exists), _bsi.expected_range(values, a, b, exists))
    table = wah.bitop_operand_table(ops)
    for name, lo, hi in cases:
        got, offs = wah.bsi_range_device(table, (lo, hi), n, exists=True)
        _same(streams, oracle, got, offs, _bsi.expected_range(values, lo, hi, exists), ("range", name))

    # k-th: every answer's low four bits come from the four settled slices
    model = _kth.Model(values, exists & mask)
    d_mask = streams.of(_bsi.pack_bits(mask))  # (the table holds raw pointers: d_mask stays alive)
    rows_table = wah.bitop_operand_table([d_mask, ops[64]] + ops[:64])
    assert rows_table.shape[0] == 66 and model.total > 16
    for name, kind, qa, qb in _kth.query_cases(model.total):
        got = wah.bsi_kth_device(rows_table, (kind, qa, qb), n, 2)
        assert tuple(int(v) & _bsi.U64_MAX for v in got.tolist()) == model(kind, qa, qb), ("k-th", name)

    # clauses and list: 62 sparse operands, then four empty ones
    sparse = [_bsi.pack_bits(rng.random(rows) < 1 / 128) for _ in range(62)]
    union = np.bitwise_or.reduce(sparse)
    assert union.any() and not (union == _bsi.ONES).all()
    empty = streams.of(np.zeros(n, np.uint32))
    assert empty[0].numel() == 2
    operands = [streams.of(words) for words in sparse] + [empty] * 4
    got, offs = wah.bitop_list_indexed_device("or", operands, n)
    _same(streams, oracle, got, offs, union, "list")
    for negate, want in (((False, True, True), union), ((True, True, True), ~union), ((False, False, True), np.zeros(n, np.uint32))):
        clauses = [(operands[:63], negate[0]), (operands[63:64], negate[1]), (operands[64:], negate[2])]
        got, offs = wah.bitop_clauses_indexed_device(clauses, n)
        _same(streams, oracle, got, offs, want, ("clauses", negate))


# ---- 2: chaining and the column front ends --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attribute(wah):
    """A 20-bit attribute with an existence bitmap and an equality-encoded attribute of 8 bins over the same 32 * 992 * 2 rows."""
    import torch

    n = SEG * 2
    values, exists, lo, hi = _bsi.headline(n, 20, True)
    keys = np.random.default_rng(3).integers(0, 8, 32 * n)
    d_values = torch.from_numpy(values.view(np.int64)).cuda()
    bsi = wah.columns.bsi_from_values(wah, d_values, 20, exists=torch.from_numpy(exists).cuda())
    index = wah.columns.index_from_keys(wah, torch.from_numpy(keys).cuda(), 8)
    return dict(n=n, values=values, exists=exists, lo=lo, hi=hi, keys=keys, bsi=bsi, index=index, d_values=d_values)


def test_bsi_from_values_builds_the_slices(wah, oracle, attribute):
    stream, seg_offsets, n, n_bits, has_exists = attribute["bsi"]
    assert (n, n_bits, has_exists) == (attribute["n"], 20, True)
    slices = _bsi.build_slices(attribute["values"], 20, attribute["exists"], zero_missing=True)
    assert slices.shape == (21, n)
    assert np.array_equal(_host(stream), oracle.compress(slices.reshape(-1)))  # whole segments: the rows' streams back to back
    assert seg_offsets.numel() >= 21 * 2 + 1
    for i in (0, 7, 19, 20):  # ... and every row a window of the index
        first, last = int(seg_offsets[2 * i].item()), int(seg_offsets[2 * i + 2].item())
        assert np.array_equal(_host(stream[first:last]), oracle.compress(slices[i])), i
    # no existence bitmap, a column length of its own, values out of range
    plain = wah.columns.bsi_from_values(wah, attribute["d_values"][:5000], 20, n_words_per_column=SEG)
    assert plain[2:] == (SEG, 20, False)
    padded = np.zeros(32 * SEG, np.uint64)
    padded[:5000] = attribute["values"][:5000]
    assert np.array_equal(_host(plain[0]), oracle.compress(_bsi.build_slices(padded, 20).reshape(-1)))
    with pytest.raises(ValueError):
        wah.columns.bsi_from_values(wah, attribute["d_values"], 19)
    with pytest.raises(ValueError):
        wah.columns.bsi_from_values(wah, attribute["d_values"], 64)


def test_range_column_chains_into_filter_columns(wah, oracle, attribute):
    """`key IN (1, 3, 6) AND lo <= value <= hi`: the range result is one more operand of the clause call; negated, = is !=."""
    n, values, exists, keys = attribute["n"], attribute["values"], attribute["exists"], attribute["keys"]
    lo, hi = attribute["lo"], attribute["hi"]
    streams = Streams(wah, n)
    in_range = _bsi.assert_range_matters(values, 20, lo, hi, exists, "front ends")
    got, offs = wah.columns.range_column(wah, attribute["bsi"], lo, hi)
    _same(streams, oracle, got, offs, in_range, "range_column")
    key_stream, key_offsets, key_n = attribute["index"]
    assert key_n == n
    in_list = _bsi.pack_bits(np.isin(keys, [1, 3, 6]))
    want = in_list & in_range
    assert want.any() and not np.array_equal(want, in_list) and not np.array_equal(want, in_range)
    both, both_offs = wah.columns.filter_columns(wah, [(key_stream, key_offsets, [1, 3, 6], False), (got, offs, [0], False)], n)
    _same(streams, oracle, both, both_offs, want, "IN and BETWEEN")
    # value != c: = through a negated clause (NOT is over all 32 * n_words rows; the existence bitmap is then a clause of its own)
    c = int(values[np.flatnonzero(exists)[5]])
    eq, eq_offs = wah.columns.compare_column(wah, attribute["bsi"], "==", c)
    bsi_stream, bsi_offsets = attribute["bsi"][0], attribute["bsi"][1]
    ne, ne_offs = wah.columns.filter_columns(wah, [(eq, eq_offs, [0], True), (bsi_stream, bsi_offsets, [20], False)], n)
    _same(streams, oracle, ne, ne_offs, _bsi.pack_bits((values != np.uint64(c)) & exists), "!=")
    only_not, only_not_offs = wah.columns.filter_columns(wah, [(eq, eq_offs, [0], True)], n)
    _same(streams, oracle, only_not, only_not_offs, ~_bsi.pack_bits((values == np.uint64(c)) & exists), "NOT =")


def test_compare_column(wah, oracle, attribute):
    n, values, exists = attribute["n"], attribute["values"], attribute["exists"]
    streams = Streams(wah, n)
    top = (1 << 20) - 1
    model = {"<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal, "==": np.equal}
    present = int(values[np.flatnonzero(exists)[11]])
    for op, f in model.items():
        for c in (present, 0, top, top // 3):
            got, offs = wah.columns.compare_column(wah, attribute["bsi"], op, c)
            _same(streams, oracle, got, offs, _bsi.pack_bits(f(values, np.uint64(c)) & exists), (op, c))
    for op, c in (("<", 0), (">", top), (">", top + 5), ("==", top + 1), (">=", top + 1)):  # empty ranges, not errors
        got, offs = wah.columns.compare_column(wah, attribute["bsi"], op, c)
        _same(streams, oracle, got, offs, np.zeros(n, np.uint32), (op, c))
    got, offs = wah.columns.compare_column(wah, attribute["bsi"], "<=", top + 5)
    _same(streams, oracle, got, offs, _bsi.pack_bits(exists), ("<=", top + 5))
    with pytest.raises(ValueError):
        wah.columns.compare_column(wah, attribute["bsi"], "!=", 3)


def test_sum_column_where(wah, attribute):
    """SUM(value) over the rows of a mask, in Python ints: a range over the attribute itself, a bin of the other attribute, and a
    60-bit attribute whose sum does not fit 64 bits."""
    import torch

    n, values, exists, keys = attribute["n"], attribute["values"], attribute["exists"], attribute["keys"]
    got, offs = wah.columns.range_column(wah, attribute["bsi"], attribute["lo"], attribute["hi"])
    mask = (values >= np.uint64(attribute["lo"])) & (values <= np.uint64(attribute["hi"])) & exists
    assert wah.columns.sum_column_where(wah, attribute["bsi"], got, offs) == int(values[mask].sum()) > 0
    key_stream, key_offsets, _ = attribute["index"]
    bin4 = wah.bitop_list_indexed_device("or", wah.columns.column_operand_table(key_stream, key_offsets, n, [4]), n)
    assert wah.columns.sum_column_where(wah, attribute["bsi"], *bin4) == int(values[(keys == 4) & exists].sum()) > 0
    wide = _bsi.uniform_values(np.random.default_rng(9), 32 * n, 60)
    bsi = wah.columns.bsi_from_values(wah, torch.from_numpy(wide.view(np.int64)).cuda(), 60)
    want = sum(int(v) for v in wide[keys == 4])
    assert want >= 1 << 64
    assert wah.columns.sum_column_where(wah, bsi, *bin4) == want


# ---- 3: graph replay ------------------------------------------------------------------------------------------------------------
def test_graph_replay_with_other_bounds(wah, oracle, attribute):
    """The bounds are only ever read by the device: ONE captured call, replayed after they were overwritten in place, answers the
    new range (capture as the clause call's test: side stream, warm-up outside, check=False; one chain of launches)."""
    import torch

    n, values, exists = attribute["n"], attribute["values"], attribute["exists"]
    stream, seg_offsets, _, n_bits, _ = attribute["bsi"]
    streams = Streams(wah, n)
    table = wah.columns.column_operand_table(stream, seg_offsets, n, list(range(n_bits + 1)))
    bounds = wah.bsi_bounds(attribute["lo"], attribute["hi"], "cuda:0")
    sc = torch.empty(int(wah.lib().wah_bsi_range_scratch_bytes(n, n_bits)), dtype=torch.uint8, device="cuda:0")
    res = torch.empty(wah.max_compressed_words(n), dtype=torch.int32, device="cuda:0")
    res_offs = torch.zeros(n // SEG + 2, dtype=torch.int64, device="cuda:0")
    wah.bsi_range_device(table, bounds, n, exists=True, scratch=sc, out=res, out_offsets=res_offs, check=False)  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _, count, _ = wah.bsi_range_device(table, bounds, n, exists=True, scratch=sc, out=res, out_offsets=res_offs, check=False)
    top = (1 << 20) - 1
    seen = set()
    for lo, hi in ((top // 5, top // 2), (0, 1000), (attribute["lo"], attribute["hi"]), (5, 4), (top // 2, _bsi.U64_MAX)):
        want = _bsi.expected_range(values, lo, hi, exists)
        seen.add(want.tobytes())
        wah.bsi_bounds(lo, hi, "cuda:0", out=bounds)
        torch.cuda.synchronize()
        res.fill_(0x5A5A5A5A)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bsi_range_status(sc.data_ptr(), n, n_bits, None) == 0
        _same(streams, oracle, res[: int(count.item())], res_offs[: n // SEG + 1], want, (lo, hi))
    assert len(seen) == 5  # five different answers from one captured call


# ---- 4: refusals ----------------------------------------------------------------------------------------------------------------
def _status(wah, table, bounds, n, exists, **kw):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    k = table.shape[0] - (1 if exists else 0)
    sc = torch.empty(int(wah.lib().wah_bsi_range_scratch_bytes(n, k)), dtype=torch.uint8, device="cuda:0")
    wah.bsi_range_device(table, bounds, n, exists=exists, scratch=sc, check=False, **kw)
    return int(wah.lib().wah_bsi_range_status(sc.data_ptr(), n, k, None))


def test_refusals_come_from_the_status_call(wah, oracle):
    """What only the device sees -- a row whose segment does not add up, an empty fill, a row without an index, too small an output --
    is reported by the status call, whatever the bounds are: an empty range checks as much as a full one."""
    import torch

    n, n_bits = SEG * 4, 12
    rng = np.random.default_rng(41)
    values = _bsi.make_values("clustered", rng, 32 * n, n_bits)
    exists = rng.random(32 * n) < 0.9
    streams = Streams(wah, n)
    ops = [streams.of(row) for row in _bsi.build_slices(values, n_bits, exists)]
    top = (1 << n_bits) - 1
    all_bounds = ((5, 4), (0, top), (top // 3, top // 2), (1 << n_bits, _bsi.U64_MAX))
    table = wah.bitop_operand_table(ops)
    for bounds in all_bounds:
        assert _status(wah, table, bounds, n, True) == 0
    # a fill of a slice, one group shorter: the segment's groups do not add up; and the same fill emptied
    row = 3
    words = _host(ops[row][0]).copy()
    fills = np.flatnonzero((words >> 31 == 1) & ((words & 0x3FFFFFFF) >= 2))
    assert fills.size, "a clustered slice has fills"
    at = int(fills[fills.size // 2])
    for name, word in (("short fill", words[at] - 1), ("empty fill", words[at] & 0xC0000000)):
        broken = words.copy()
        broken[at] = word
        for r in (row, 0, n_bits - 1, n_bits):  # any slice, the first, the last, and the existence row
            rows = list(ops)
            rows[r] = (_dev(broken), ops[row][1])
            bad_table = wah.bitop_operand_table(rows)
            for bounds in all_bounds:
                assert _status(wah, bad_table, bounds, n, True) == WAH_ERR_STREAM, (name, r, bounds)
        with pytest.raises(wah.WahError):
            wah.bsi_range_device(bad_table, (0, top), n, exists=True)
    # a row without an index, or without a stream
    for r, col in ((0, 2), (7, 2), (n_bits, 2), (5, 0)):
        t = table.clone()
        t[r, col] = 0
        for bounds in all_bounds[:2]:
            assert _status(wah, t, bounds, n, True) == WAH_ERR_STREAM, (r, col, bounds)
    # an output one word too small, for a result of many words
    lo, hi = top // 4, (3 * top) // 4
    need = int(oracle.compress(_bsi.expected_range(values, lo, hi, exists)).size)
    assert need > 200
    out, count, _ = wah.bsi_range_device(table, (lo, hi), n, exists=True, check=False)
    torch.cuda.synchronize()
    assert int(count.item()) == need
    small = torch.full((need + 63,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert _status(wah, table, (lo, hi), n, True, out=small[:need]) == 0
    assert bool((small[:need] == out[:need]).all()) and bool((small[need:] == 0x5A5A5A5A).all())
    small.fill_(0x5A5A5A5A)
    assert _status(wah, table, (lo, hi), n, True, out=small[: need - 1]) == WAH_ERR_CAPACITY
    assert bool((small[need - 1:] == 0x5A5A5A5A).all())


def test_front_end_refuses_bad_tables(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(wah.WahError):
        wah.bsi_range_device([(stream, offs)] * 65, (0, 1), 0)
    with pytest.raises(wah.WahError):
        wah.bsi_range_device([(stream, offs)], (0, 1), 0, exists=True)
    with pytest.raises(wah.WahError):
        wah.bsi_range_device([(stream, offs)], torch.zeros(2, dtype=torch.int32, device="cuda"), 0)
