"""CPU proof of tests/_grid.py, the thresholds, shapes and references of tests/test_gpu_full_grid.py: the grid caps are found in
the sources and are what the shapes assume, runs() partitions the items, every condition that keeps a shape from being vacuous
holds, the two defect models change at least a hundred segments -- and what they change reaches the words --, the closed form
for lists of no row or one row is the oracle's, and the slices kernel's shape has a set and a clear bit in every slice among
the rows of the second trip."""
import numpy as np
import pytest

from tests import _fetch, _grid, _rows, _select, _slices


def test_thresholds_are_found_and_are_what_the_shapes_assume():
    t = _grid.thresholds()
    assert t["items"] == 8192, "from_positions_kernel's grid moved: revisit shapes two, three and lists (_grid._shape_table)"
    assert t["check_threads"] == 524288, "from_positions_check_kernel's grid moved: revisit check_rows_lists and check_ends_positions"
    assert t["fetch_check_rows"] == 524288, "fetch_check_kernel's grid moved: revisit fetch_case"
    assert t["bsi_blocks"] == 8192 and t["bsi_rows"] == 16777216, "bsi_slices_kernel's grid moved: revisit bsi_shape"
    assert _grid.bsi_shape() == (524768, 8192 * 2048 + 3 * 2048 + 77)
    assert {n: _grid._shape_table()[n] for n in _grid.SHAPES} == {"two": (2976, 2740, 2), "three": (2981, 4100, 3), "lists": (992, 3 * 8192 + 5, 4)}


@pytest.mark.parametrize("n_lists,segments", ((1, 1), (5, 3), (2048, 4), (2049, 4), (2740, 3), (4100, 4), (24581, 1), (8193, 1)))
def test_runs_partition_the_items(n_lists, segments):
    per, runs = _grid.runs(n_lists, segments)
    flat = [item for run in runs for item in run]
    assert flat == [divmod(i, segments) for i in range(n_lists * segments)]
    assert all(len(run) <= per for run in runs) and len(runs) <= _grid.thresholds()["items"]
    assert (per == 1) == (n_lists * segments <= _grid.thresholds()["items"])
    # a run goes on in the list it is in, or begins the next one at segment 0
    for run in runs:
        for (c0, s0), (c1, s1) in zip(run, run[1:]):
            assert (c1, s1) == ((c0, s0 + 1) if s0 + 1 < segments else (c0 + 1, 0))


@pytest.mark.parametrize("name", _grid.SHAPES)
def test_shape_conditions(name):
    sh = _grid.shape(name)
    figures = _grid.assert_shape(sh)
    assert sh.n_items > _grid.thresholds()["items"] and len(sh.lists) == sh.n_lists
    rows, ends = _rows.flatten(sh.lists)
    assert rows.size == ends[-1] and all(np.all(np.diff(r) > 0) for r in sh.lists)
    assert all(r.size == 0 or (r[0] >= 0 and r[-1] < 32 * sh.n_words) for r in sh.lists)
    per_segment = {_rows.route_of(int(r.size)) for r in sh.item_rows}
    assert per_segment == {_rows.EMPTY, _rows.REGISTERS, _rows.IMAGE}
    assert figures["stale"] >= 100 and (figures["lo"] >= 100 or sh.segments == 1)


def test_what_the_models_change_reaches_the_words(oracle):
    """The models are held against the rows, segment by segment; here a sample of the lists they change goes through the oracle:
    the modelled list's stream differs from the reference's in the segments whose rows differ."""
    sh = _grid.shape("two")
    s = sh.segments
    for model in (_grid.model_lo_is_list_start, _grid.model_stale_list):
        modelled = model(sh)
        changed = [i for i in range(sh.n_items) if not np.array_equal(modelled[i], sh.item_rows[i])]
        assert len(changed) >= 100
        for item in changed[:: len(changed) // 20]:
            c = item // s
            rows = np.concatenate(modelled[c * s: (c + 1) * s])
            assert rows.size == 0 or rows[-1] < 32 * sh.n_words
            got, got_index = _rows.reference(oracle, [np.unique(rows)], sh.n_words)
            want, want_index = _rows.reference(oracle, [sh.lists[c]], sh.n_words)
            k = item % s
            assert not np.array_equal(got[got_index[k]: got_index[k + 1]], want[want_index[k]: want_index[k + 1]]), (model.__name__, item)


@pytest.mark.parametrize("n_words", (992, 2976, 2981, 993))
def test_one_row_closed_form_is_the_oracles(oracle, n_words):
    rng = np.random.default_rng(n_words)
    groups = _select.groups_of(n_words)
    edges = [0, 30, 31, 31743, 31744, 32 * n_words - 1, 31 * (groups - 1), 31 * (groups - 1) - 1, 31 * 1023 - 1, 31 * 1023]
    p = np.concatenate([[q for q in edges if 0 <= q < 32 * n_words], [-1, -1], rng.integers(0, 32 * n_words, 60), [-1]])
    stream, index = _grid.one_row_reference(p, n_words)
    want, want_index = _rows.reference(oracle, _grid.one_row_lists(p), n_words)
    assert np.array_equal(index, want_index) and np.array_equal(stream, want)
    segments = _select.segments_of(n_words)
    assert stream.size == sum(_rows.one_row_words(int(q), n_words) if q >= 0 else segments for q in p)


def test_check_pass_inputs(oracle):
    trip = _grid.thresholds()["check_threads"]
    lists = _grid.check_rows_lists()
    rows, ends = _rows.flatten(lists)
    assert len(lists) == 4 and rows.size > trip + 4096 and trip + 1 < ends[2] < rows.size - 2
    descents = np.flatnonzero(rows[1:] <= rows[:-1]) + 1
    assert list(descents) == list(ends[:-1])  # the list boundaries and nothing else
    for i in (trip, trip + 1, rows.size - 1):  # where the defects go: inside a list, both neighbours at a distance
        assert i not in ends and i - 1 not in ends and rows[i - 2] < rows[i - 1] < rows[i] < 32 * _grid.CHECK_ROWS_WORDS - 1
    p = _grid.check_ends_positions()
    assert p.size == trip + 12 and 0.3 < np.mean(p < 0) < 0.37
    for j in (trip, p.size - 2):
        assert 0 <= p[j - 1] < p[j] < p[j + 1]
    stream, index = _grid.one_row_reference(p, _grid.CHECK_ENDS_WORDS)
    assert index.size == p.size + 1 and index[-1] == stream.size
    sample = np.concatenate([np.arange(40), np.arange(trip - 20, trip + 12)])
    want, want_index = _rows.reference(oracle, _grid.one_row_lists(p[sample[:40]]), _grid.CHECK_ENDS_WORDS)
    assert np.array_equal(stream[: index[40]], want) and np.array_equal(index[:41], want_index)
    want, want_index = _rows.reference(oracle, _grid.one_row_lists(p[sample[40:]]), _grid.CHECK_ENDS_WORDS)
    assert np.array_equal(stream[index[trip - 20]:], want) and np.array_equal(index[trip - 20:] - index[trip - 20], want_index)


def test_fetch_case():
    trip = _grid.thresholds()["fetch_check_rows"]
    values, exists, keys, rows = _grid.fetch_case()
    n = _grid.FETCH_WORDS
    assert rows.size == trip + 200 and np.all(rows[1:] >= rows[:-1]) and np.any(rows[1:] == rows[:-1])
    assert rows[0] == 0 and rows[-1] == 32 * n - 1 and set(rows // _select.SEG_BITS) == {0, 1, 2}
    items = _fetch.items_of(rows, n)
    assert _fetch.grid_waves() < len(items) <= _fetch.item_bound(rows.size, n)
    assert any(head >= trip for head, _ in items)  # heads that only a second trip appends
    for i in (trip, trip + 1, rows.size - 1):
        assert rows[i - 1] > 0  # a row below it lies inside the bitmap
    assert not (values >> np.uint64(_grid.FETCH_BITS_WIDE)).any() and exists.any() and not exists.all()
    assert set(keys) == set(range(_grid.FETCH_KEYS))


def test_bsi_shape_has_a_second_trip_that_matters():
    t = _grid.thresholds()
    n_words, n_rows = _grid.bsi_shape()
    assert n_words % _slices.SEG == 0 and n_words > t["bsi_blocks"] * t["bsi_block_words"] and t["bsi_rows"] < n_rows < 32 * n_words
    values, exists = _grid.bsi_case(2, True)
    assert values.size == n_rows and not (values >> np.uint64(2)).any()
    matrix = _slices.expected_matrix(values, exists, 2, n_words)
    assert matrix.shape == (3, n_words)
    for i, row in enumerate(matrix):
        _grid.assert_second_trip_matters(row, i)
        assert not row[-(-n_rows // 32):].any()
    assert not np.array_equal(matrix[:2], _slices.expected_matrix(values, None, 2, n_words))  # zeroing the missing rows changes the slices
    assert np.flatnonzero(~exists[t["bsi_rows"]:]).size > 0  # a row of the second trip that does not exist
    wide, none = _grid.bsi_case(34, False)
    assert none is None and wide.size == n_rows and (wide >> np.uint64(33)).any() and not (wide >> np.uint64(34)).any()
    for i in (0, 1, 2, 33):
        row = _grid.bsi_slice_row(wide, 34, i, n_words)
        _grid.assert_second_trip_matters(row, i)
        assert np.array_equal(row[:2048], _slices.expected_matrix(wide[:65536], None, 34, 2048)[i])
