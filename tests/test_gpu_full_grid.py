"""GPU tests of the three newest ways into the index and of the fetch call's row check at the sizes where a wavefront takes a
SECOND item: from_positions_kernel (contiguous runs of (list, segment) items, the slice end and the list's bounds carried from
one item to the next), from_positions_check_kernel and fetch_check_kernel (grid-stride loops over ends and rows),
bsi_slices_kernel (a grid-stride loop over blocks of 2048 rows with the sticky "value too wide" register carried across).
Every other test of these calls stops where each wavefront of the launch has exactly one item.

tests/_grid.py reads the grid caps out of the sources and builds the shapes and references; tests/test_grid_reference.py proves
them on the CPU, the conditions that keep these tests from being vacuous included.  Everything is exact.  Every output buffer
the api lets the caller pass comes in filled with 0x5A5A... and with 64 entries of guard behind it, the scratch filled with
0xA5 bytes: no freshly allocated zero page hides a word that was not written.

That the tests bite: libraries with ONE token changed, built from a scratch copy of the sources, this file run once against each
on an MI355X.  runs[shape] = test_builder_runs_of_more_than_one_item[shape], capacity = test_builder_capacity_with_runs_of_two,
keys = test_index_from_keys_past_both_thresholds; the three mutants of a check loop ran without the "behind_the_bitmap" tests
(only defects whose rows lie inside the bitmap go past a blinded check pass into the builder).

  from_positions_kernel: `: slice_end` -> `: lb`        runs[two] runs[three], capacity, keys (not runs[lists]: one segment a
                                                        list, every item is the `seg == 0 ? lb` arm)
  ... the crossing without `have_list = false`          runs[two] runs[three] runs[lists], capacity, and the three tests of the
                                                        ends loop (trip + 12 lists are runs of 65 lists)
  from_positions_check_kernel: rows loop, first trip    test_check_pass_refuses_rows_of_a_second_trip (all three places),
    only (`i += stride` -> `i += a.n_rows`)             test_check_pass_refuses_an_end_off_a_descent_of_a_second_trip
  ... ends loop, first trip only (`j += a.n_lists`)     test_check_pass_refuses_a_decreasing_end_of_a_second_trip (both places),
                                                        test_check_pass_refuses_a_last_end_that_is_not_the_row_count
  fetch_check_kernel: first trip only                   test_fetch_heads_of_a_second_trip,
    (`base += a.n_rows`)                                test_fetch_refuses_a_descending_pair_of_a_second_trip (all three places)
  bsi_slices_kernel: first trip only                    test_bsi_build_blocks_of_a_second_trip, ..._upper_halves_in_a_second_trip,
    (`blk += n_blocks`)                                 test_bsi_build_refuses_a_wide_value_of_a_second_trip (all three rows)
  ... `over = 0u` at the top of the loop body           test_bsi_build_keeps_a_refusal_of_the_first_trip_across_the_second (both
                                                        blocks) and nothing else: a value that is too wide in a wavefront's LAST
                                                        block is still seen, so the rows of the second trip do not catch it

Not built: `seg == 0 ? lb` -> the slice end carried across a list end (the same program: lists lie back to back, the last
segment's slice ends at the list's `le`, which is the next list's `lb`); anything that touches a clamp of an end, of a row's
place or of a store, an address, a buffer size or the bound of a loop that loads.
"""
import importlib

import numpy as np
import pytest

from tests import _fetch, _grid, _rows, _select, _slices

pytestmark = pytest.mark.gpu

WAH_OK, WAH_ERR_CAPACITY, WAH_ERR_STREAM = 0, -4, -6
SENTINEL, SENTINEL64, GUARD = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A, 64
SEG = _select.SEG_WORDS


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


def _dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _dev_values(values):
    import torch

    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64)).cuda()


def _dev_words(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _words(n):
    import torch

    return torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")


def _longs(n):
    import torch

    return torch.full((n + GUARD,), SENTINEL64, dtype=torch.int64, device="cuda:0")


def _scratch(n_bytes):
    import torch

    return torch.full((int(n_bytes),), 0xA5, dtype=torch.uint8, device="cuda:0")


def _kept(buf, n, sentinel):
    return bool((buf[n:] == sentinel).all()) and buf.numel() == n + GUARD


# ---- the builder ----------------------------------------------------------------------------------------------------------------
def _fp_status(wah, d_rows, d_ends, n, out=None, out_offsets=None):
    """Enqueue only, into sentinel-filled buffers; the verdict comes from the status call.  Returns (status, count, out, offsets)."""
    sc = _scratch(wah.lib().wah_from_positions_scratch_bytes(n, d_ends.numel()))
    out, count, offs = wah.from_positions_device(d_rows, d_ends, n, scratch=sc, out=out, out_offsets=out_offsets, check=False)
    return int(wah.lib().wah_from_positions_status(sc.data_ptr(), None)), int(count.item()), out, offs


def _built_is(wah, d_rows, d_ends, n, want, want_index, what):
    """One call into buffers of exactly the reference's sizes: WAH_OK, the words, their count, every index entry, both guards."""
    out, offs = _words(want.size), _longs(want_index.size)
    status, count, _, _ = _fp_status(wah, d_rows, d_ends, n, out=out[: want.size], out_offsets=offs[: want_index.size])
    assert status == WAH_OK and count == want.size, (what, status, count, want.size)
    assert np.array_equal(offs[: want_index.size].cpu().numpy(), want_index), what
    assert np.array_equal(_host(out[: want.size]), want), what
    assert _kept(out, want.size, SENTINEL) and _kept(offs, want_index.size, SENTINEL64), what
    return out, offs


def _list_table(stream, index, n_lists, segments):
    """The operand table of all lists of one call, built on the device."""
    import torch

    table = torch.empty((n_lists, 3), dtype=torch.int64, device=stream.device)
    table[:, 0] = stream.data_ptr()
    table[:, 1] = stream.numel()
    table[:, 2] = torch.arange(n_lists, dtype=torch.int64, device=stream.device) * (8 * segments) + index.data_ptr()
    return table


_REFERENCES = {}


def _shape_reference(oracle, name):
    if name not in _REFERENCES:
        sh = _grid.shape(name)
        _REFERENCES[name] = _rows.reference(oracle, sh.lists, sh.n_words)
    return _REFERENCES[name]


@pytest.mark.parametrize("name", _grid.SHAPES)
def test_builder_runs_of_more_than_one_item(wah, oracle, name):
    """Runs of two, three and four items: the slice end carried inside a list, the list's bounds read anew behind a list end, runs
    that begin in a later segment, the ragged last segment in every place of a run."""
    sh = _grid.shape(name)
    assert sh.per >= 2 and sh.n_items > _grid.thresholds()["items"]
    want, want_index = _shape_reference(oracle, name)
    rows, ends = _rows.flatten(sh.lists)
    out, offs = _built_is(wah, _dev64(rows), _dev64(ends), sh.n_words, want, want_index, name)
    table = _list_table(out, offs, sh.n_lists, sh.segments)
    counts = _longs(sh.n_lists)
    sc = _scratch(wah.lib().wah_select_scratch_bytes(sh.n_words, sh.n_lists))
    wah.count_device(table, sh.n_words, scratch=sc, counts=counts[: sh.n_lists])
    assert np.array_equal(counts[: sh.n_lists].cpu().numpy(), [r.size for r in sh.lists]) and _kept(counts, sh.n_lists, SENTINEL64)


def test_builder_capacity_with_runs_of_two(wah, oracle):
    sh = _grid.shape("two")
    want, want_index = _shape_reference(oracle, "two")
    rows, ends = _rows.flatten(sh.lists)
    d_rows, d_ends = _dev64(rows), _dev64(ends)
    total = want.size
    buf = _words(total)
    status, count, _, _ = _fp_status(wah, d_rows, d_ends, sh.n_words, out=buf[: total - 1])
    assert status == WAH_ERR_CAPACITY and count == total
    assert bool((buf[total - 1:] == SENTINEL).all())
    status, count, _, offs = _fp_status(wah, d_rows, d_ends, sh.n_words, out=buf[:total])
    assert status == WAH_OK and count == total
    assert np.array_equal(_host(buf[:total]), want) and _kept(buf, total, SENTINEL)
    assert np.array_equal(offs.cpu().numpy(), want_index)


def test_index_from_keys_past_both_thresholds(wah, oracle):
    """An ordinary column: 300 values over 28 segments are 8400 items (runs of two), 888 732 rows a second trip of the check pass."""
    import torch

    n_values, n = 300, 28 * SEG
    n_rows = 32 * n - 100
    t = _grid.thresholds()
    assert n_values * 28 > t["items"] and n_rows > t["check_threads"]
    rng = np.random.default_rng(300)
    keys = rng.integers(0, n_values, n_rows)
    d_keys = torch.from_numpy(keys).cuda()
    stream, seg_offsets, got_n = wah.columns.index_from_keys(wah, d_keys, n_values)
    assert got_n == n
    lists = [np.flatnonzero(keys == v).astype(np.int64) for v in range(n_values)]
    want, want_index = _rows.reference(oracle, lists, n)
    assert stream.numel() == want.size and np.array_equal(seg_offsets.cpu().numpy(), want_index)
    assert np.array_equal(_host(stream), want)
    counts = wah.columns.count_columns(wah, stream, seg_offsets, n, list(range(n_values)))
    assert counts.tolist() == np.bincount(keys, minlength=n_values).tolist()
    at = np.concatenate([rng.integers(0, n_rows, 1000), [0, n_rows - 1]])
    got = wah.columns.keys_at_rows(wah, (stream, seg_offsets, n), torch.from_numpy(at).cuda())
    assert np.array_equal(got.cpu().numpy(), keys[at])


# ---- the builder's check pass: the rows loop ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_rows(wah):
    lists = _grid.check_rows_lists()
    rows, ends = _rows.flatten(lists)
    return dict(lists=lists, rows=rows, ends=ends, d_rows=_dev64(rows), d_ends=_dev64(ends), n=_grid.CHECK_ROWS_WORDS,
                trip=_grid.thresholds()["check_threads"])


def _patched(wah, c, at, values, ends=None):
    """The status of the call with rows[at] = values (device-side, put back afterwards) or with other ends."""
    at = _dev64(np.asarray(at, np.int64).reshape(-1))
    before = c["d_rows"][at].clone()
    c["d_rows"][at] = _dev64(np.asarray(values, np.int64).reshape(-1))
    try:
        return _fp_status(wah, c["d_rows"], c["d_ends"] if ends is None else _dev64(ends), c["n"])[0]
    finally:
        c["d_rows"][at] = before


def test_check_pass_accepts_rows_of_a_second_trip(wah, oracle, check_rows):
    c = check_rows
    assert c["rows"].size > c["trip"] + 4096 and c["ends"][2] > c["trip"]  # a legal descent behind the first trip
    want, want_index = _rows.reference(oracle, c["lists"], c["n"])
    _built_is(wah, c["d_rows"], c["d_ends"], c["n"], want, want_index, "valid")
    assert _patched(wah, c, c["rows"].size - 1, 32 * c["n"] - 1) == WAH_OK  # the last position inside the bitmap, in the last row
    assert np.array_equal(c["d_rows"].cpu().numpy(), c["rows"])


def _places(c):
    return {"first of the second trip": c["trip"], "second": c["trip"] + 1, "last row": c["rows"].size - 1}


@pytest.mark.parametrize("place", ("first of the second trip", "second", "last row"))
def test_check_pass_refuses_rows_of_a_second_trip(wah, check_rows, place):
    """Each defect alone, all rows inside the bitmap: a duplicate of the row in front (at the first index of the second trip that
    row belongs to the first trip) and a descending pair."""
    c = check_rows
    i, rows = _places(c)[place], c["rows"]
    assert i >= c["trip"] and _fp_status(wah, c["d_rows"], c["d_ends"], c["n"])[0] == WAH_OK
    assert _patched(wah, c, i, rows[i - 1]) == WAH_ERR_STREAM
    assert _patched(wah, c, [i - 1, i], [rows[i], rows[i - 1]]) == WAH_ERR_STREAM
    assert _fp_status(wah, c["d_rows"], c["d_ends"], c["n"])[0] == WAH_OK


@pytest.mark.parametrize("place", ("first of the second trip", "second", "last row"))
def test_check_pass_refuses_a_row_behind_the_bitmap_in_a_second_trip(wah, check_rows, place):
    c = check_rows
    i = _places(c)[place]
    assert _patched(wah, c, i, 32 * c["n"]) == WAH_ERR_STREAM


def test_check_pass_refuses_an_end_off_a_descent_of_a_second_trip(wah, check_rows):
    """The ends stay legal by themselves (never decreasing, the last one n_rows): only the rows loop, which meets the descent at an
    index that is no end any more, can refuse."""
    c = check_rows
    assert c["ends"][2] > c["trip"]
    for off in (-1, 1):
        ends = c["ends"].copy()
        ends[2] += off
        assert _fp_status(wah, c["d_rows"], _dev64(ends), c["n"])[0] == WAH_ERR_STREAM, off


# ---- the builder's check pass: the ends loop -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_ends(wah):
    p = _grid.check_ends_positions()
    rows, ends = p[p >= 0].astype(np.int64), np.cumsum(p >= 0).astype(np.int64)
    return dict(p=p, rows=rows, ends=ends, d_rows=_dev64(rows), n=_grid.CHECK_ENDS_WORDS, trip=_grid.thresholds()["check_threads"])


def test_check_pass_accepts_ends_of_a_second_trip(wah, check_ends):
    c = check_ends
    assert c["ends"].size == c["trip"] + 12
    want, want_index = _grid.one_row_reference(c["p"], c["n"])
    assert want_index.size * 8 > 4 << 20  # (an index of 4 MiB)
    _built_is(wah, c["d_rows"], _dev64(c["ends"]), c["n"], want, want_index, "valid")


@pytest.mark.parametrize("place", ("first of the second trip", "last but one"))
def test_check_pass_refuses_a_decreasing_end_of_a_second_trip(wah, check_ends, place):
    """ends[j] one below ends[j - 1]; the rows around list j ascend from list to list, so the rows loop asks no end there."""
    c = check_ends
    j = c["trip"] if place == "first of the second trip" else c["ends"].size - 2
    ends = c["ends"].copy()
    assert ends[j - 2] < ends[j - 1] < ends[j] < ends[j + 1]
    ends[j] = ends[j - 1] - 1
    assert _fp_status(wah, c["d_rows"], _dev64(ends), c["n"])[0] == WAH_ERR_STREAM
    assert _fp_status(wah, c["d_rows"], _dev64(c["ends"]), c["n"])[0] == WAH_OK


def test_check_pass_refuses_a_last_end_that_is_not_the_row_count(wah, check_ends):
    c = check_ends
    ends = c["ends"].copy()
    assert ends[-2] == ends[-1] - 1 and c["rows"][-2] < c["rows"][-1]
    ends[-1] -= 1  # (still not below the end in front of it)
    assert _fp_status(wah, c["d_rows"], _dev64(ends), c["n"])[0] == WAH_ERR_STREAM


# ---- the fetch call's check pass -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fetch(wah):
    import torch

    values, exists, keys, rows = _grid.fetch_case()
    n = _grid.FETCH_WORDS
    stream, offs = wah.bsi_build_device(_dev_values(values), _grid.FETCH_BITS_WIDE, n, exists=torch.from_numpy(exists).cuda())
    bits = _grid.FETCH_BITS_WIDE
    table = wah.columns.column_operand_table(stream, offs, n, [bits] + list(range(bits)))  # the existence bitmap on top
    index = wah.columns.index_from_keys(wah, torch.from_numpy(keys).cuda(), _grid.FETCH_KEYS)
    key_table = wah.columns.column_operand_table(index[0], index[1], n, list(range(_grid.FETCH_KEYS)))
    return dict(values=values, exists=exists, keys=keys, rows=rows, n=n, keep=(stream, offs, index), table=table, key_table=key_table,
                d_rows=_dev64(rows), trip=_grid.thresholds()["fetch_check_rows"])


def _fetch_status(wah, f, d_rows, table, mode, out=None):
    sc = _scratch(wah.lib().wah_fetch_scratch_bytes(f["n"], d_rows.numel()))
    out = wah.fetch_device(table, d_rows, f["n"], mode, scratch=sc, out=out, check=False)
    return int(wah.lib().wah_fetch_status(sc.data_ptr(), None)), out


def test_fetch_heads_of_a_second_trip(wah, fetch):
    f = fetch
    rows, r = f["rows"], f["rows"].size
    items = _fetch.items_of(rows, f["n"])
    assert r > f["trip"] and _fetch.grid_waves() < len(items) <= _fetch.item_bound(r, f["n"])
    buf = _longs(r)
    status, _ = _fetch_status(wah, f, f["d_rows"], f["table"], wah.FETCH_BITS, out=buf[:r])
    assert status == WAH_OK
    want = np.where(f["exists"][rows], f["values"][rows] | np.uint64(1 << _grid.FETCH_BITS_WIDE), np.uint64(0))
    assert np.array_equal(buf[:r].cpu().numpy().view(np.uint64), want) and _kept(buf, r, SENTINEL64)
    buf = _longs(r)
    status, _ = _fetch_status(wah, f, f["d_rows"], f["key_table"], wah.FETCH_FIRST, out=buf[:r])
    assert status == WAH_OK
    assert np.array_equal(buf[:r].cpu().numpy(), f["keys"][rows]) and _kept(buf, r, SENTINEL64)


def _fetch_places(f):
    return {"first of the second trip": f["trip"], "second": f["trip"] + 1, "last row": f["rows"].size - 1}


@pytest.mark.parametrize("place", ("first of the second trip", "second", "last row"))
def test_fetch_refuses_a_descending_pair_of_a_second_trip(wah, fetch, place):
    """Both rows inside the bitmap.  (Nothing is asserted about the output of a refused call: it is unspecified.)"""
    f = fetch
    i = _fetch_places(f)[place]
    bad = f["d_rows"].clone()
    assert f["rows"][i - 1] > 0
    bad[i] = int(f["rows"][i - 1]) - 1
    assert _fetch_status(wah, f, bad, f["table"], wah.FETCH_BITS)[0] == WAH_ERR_STREAM
    assert _fetch_status(wah, f, f["d_rows"], f["table"], wah.FETCH_BITS)[0] == WAH_OK


@pytest.mark.parametrize("place", ("first of the second trip", "second", "last row"))
def test_fetch_refuses_a_row_behind_the_bitmap_in_a_second_trip(wah, fetch, place):
    f = fetch
    i = _fetch_places(f)[place]
    bad = f["d_rows"].clone()
    bad[i:] = 32 * f["n"]  # (it and every row behind it: the list still does not descend)
    assert _fetch_status(wah, f, bad, f["table"], wah.FETCH_BITS)[0] == WAH_ERR_STREAM
    if place == "last row":
        assert f["rows"][i] == 32 * f["n"] - 1  # ... and the last position inside it was accepted there


# ---- the slices kernel -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def column(wah):
    """The column of _grid.bsi_shape with two bits and existence bytes, on the device once (134 MB)."""
    import torch

    values, exists = _grid.bsi_case(2, True)
    n_words, n_rows = _grid.bsi_shape()
    return dict(values=values, exists=exists, n=n_words, n_rows=n_rows, d_values=_dev_values(values), d_exists=torch.from_numpy(exists).cuda(),
                trip=_grid.thresholds()["bsi_rows"])


def _bsi_status(wah, d_values, n_bits, n, d_exists=None, out=None, out_offsets=None):
    k = n_bits + (d_exists is not None)
    sc = _scratch(wah.lib().wah_bsi_build_scratch_bytes(n, k))
    out, count, offs = wah.bsi_build_device(d_values, n_bits, n, exists=d_exists, scratch=sc, out=out, out_offsets=out_offsets, check=False)
    return int(wah.lib().wah_bsi_build_status(sc.data_ptr(), n, k, None)), int(count.item()), out, offs


def test_bsi_build_blocks_of_a_second_trip(wah, oracle, column):
    c = column
    n = c["n"]
    matrix = _slices.expected_matrix(c["values"], c["exists"], 2, n)
    for i, row in enumerate(matrix):
        _grid.assert_second_trip_matters(row, i)
    want = _slices.expected_stream(oracle, matrix)
    entries = 3 * (n // SEG) + 1
    out, offs = _words(want.size), _longs(entries)
    status, count, _, _ = _bsi_status(wah, c["d_values"], 2, n, c["d_exists"], out=out[: want.size], out_offsets=offs[:entries])
    assert status == WAH_OK and count == want.size
    assert np.array_equal(_host(out[: want.size]), want)
    assert _kept(out, want.size, SENTINEL) and _kept(offs, entries, SENTINEL64)
    comp = wah.DeviceCompressor(matrix.size, indexed=True)  # the index: an indexed compress of the expected matrix
    comp.run(_dev_words(matrix.reshape(-1)))
    assert np.array_equal(_host(comp.result()), want)
    assert comp.seg_offsets.numel() == entries and np.array_equal(offs[:entries].cpu().numpy(), comp.seg_offsets.cpu().numpy())
    assert int(offs[entries - 1].item()) == want.size


def test_bsi_build_upper_halves_in_a_second_trip(wah, oracle):
    """34 bits: the loop over the upper halves runs in the second trip too.  Four slices are held against the oracle as windows of
    the index: the two of the upper halves, the first and the last of the lower ones."""
    n, n_rows = _grid.bsi_shape()
    values, _ = _grid.bsi_case(34, False)
    entries = 34 * (n // SEG) + 1
    cap = wah.max_compressed_words(34 * n)
    out, offs = _words(cap), _longs(entries)
    status, count, _, _ = _bsi_status(wah, _dev_values(values), 34, n, out=out[:cap], out_offsets=offs[:entries])
    assert status == WAH_OK and _kept(out, cap, SENTINEL) and _kept(offs, entries, SENTINEL64)
    index = offs[:entries].cpu().numpy()
    assert index[0] == 0 and index[-1] == count and np.all(np.diff(index) > 0)
    segs = n // SEG
    for i in (0, 1, 2, 33):
        row = _grid.bsi_slice_row(values, 34, i, n)
        _grid.assert_second_trip_matters(row, i)
        first, last = int(index[i * segs]), int(index[(i + 1) * segs])
        assert np.array_equal(_host(out[first:last]), oracle.compress(row)), i


def _second_trip_rows(c):
    missing = c["trip"] + int(np.flatnonzero(~c["exists"][c["trip"]:])[7])
    return {"first row of the second trip": c["trip"], "last row": c["n_rows"] - 1, "a missing row of the second trip": missing}


@pytest.mark.parametrize("place", ("first row of the second trip", "last row", "a missing row of the second trip"))
def test_bsi_build_refuses_a_wide_value_of_a_second_trip(wah, column, place):
    """One value of 2^n_bits alone; the same row with 2^n_bits - 1 is accepted."""
    c = column
    row = _second_trip_rows(c)[place]
    assert row >= c["trip"] and (place != "a missing row of the second trip" or not c["exists"][row])
    before = int(c["d_values"][row].item())
    try:
        c["d_values"][row] = 4
        assert _bsi_status(wah, c["d_values"], 2, c["n"], c["d_exists"])[0] == WAH_ERR_STREAM
        c["d_values"][row] = 3
        assert _bsi_status(wah, c["d_values"], 2, c["n"], c["d_exists"])[0] == WAH_OK
    finally:
        c["d_values"][row] = before


@pytest.mark.parametrize("block", (0, 7))
def test_bsi_build_keeps_a_refusal_of_the_first_trip_across_the_second(wah, column, block):
    """Wavefronts 0 to 7 take a second block: what they found too wide in their first one must outlast it."""
    c = column
    t = _grid.thresholds()
    row = block * t["bsi_block_rows"] + 100
    assert (block + t["bsi_blocks"]) * t["bsi_block_words"] < c["n"]  # the wavefront of this block has a second one
    before = int(c["d_values"][row].item())
    try:
        c["d_values"][row] = 4
        assert _bsi_status(wah, c["d_values"], 2, c["n"], c["d_exists"])[0] == WAH_ERR_STREAM
    finally:
        c["d_values"][row] = before
    assert _bsi_status(wah, c["d_values"], 2, c["n"], c["d_exists"])[0] == WAH_OK
