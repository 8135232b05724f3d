"""CPU proof of tests/_rows.py, the reference and the input builders of the GPU tests of wah_from_positions_device: every
builder's claimed words per segment and its route (no row / at most 64 rows / more) hold under the CPU oracle, the reference's
index is the one the segment walk gives, and the size bound of include/wah.h holds for every input the GPU tests use -- and is
met with equality where it says so."""
import numpy as np
import pytest

from tests import _rows, _select

CASES = _rows.switch_cases()


def test_case_names_are_unique_and_rows_ascend_inside_the_bitmap():
    assert len({c[0] for c in CASES}) == len(CASES)
    for name, n, rows, words in CASES:
        assert np.all(np.diff(rows) > 0), name
        assert rows.size == 0 or (rows[0] >= 0 and rows[-1] < 32 * n), name
        assert len(words) == _select.segments_of(n), name


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_claimed_words_per_segment(oracle, case):
    name, n, rows, words = case
    stream, index = _rows.reference(oracle, [rows], n)
    assert list(_rows.segment_words(index)) == words
    assert index[-1] == stream.size
    # the stream is the bitmap's: it decodes to it, and its set bits are the rows
    assert np.array_equal(_select.stream_positions(stream, n), rows)
    assert np.array_equal(oracle.decompress(stream)[:n], _select.bitmap_of(rows, n))


def test_every_route_is_taken_on_both_sides_of_its_switch_point():
    per_segment = {name: list(_rows.rows_per_segment(rows, n)) for name, n, rows, _ in CASES}
    for k, route in ((0, _rows.EMPTY), (1, _rows.REGISTERS), (2, _rows.REGISTERS), (63, _rows.REGISTERS), (64, _rows.REGISTERS), (65, _rows.IMAGE)):
        assert per_segment[f"{k} rows in one segment"] == [k] and _rows.route_of(k) == route
    assert per_segment["31743 rows: all but one"] == [31743] and per_segment["31744 rows: the whole segment"] == [31744]
    assert _rows.route_of(31744) == _rows.IMAGE
    for groups, route in ((1, _rows.REGISTERS), (2, _rows.REGISTERS), (3, _rows.IMAGE)):
        assert per_segment[f"run of {31 * groups} alone"] == [31 * groups] and _rows.route_of(31 * groups) == route
    assert per_segment["run of 62 across a segment edge"] == [31, 31]
    assert per_segment["run of 93 across a segment edge"] == [31, 62]
    assert per_segment["run of 93 across a segment edge, two groups in front"] == [62, 31]
    assert per_segment["31 rows across a segment edge, not group aligned"] == [15, 16]
    assert per_segment["the last real bit of a ragged bitmap"] == [0, 1]
    for name in ("64 rows in 64 neighbouring groups", "64 rows in 3 groups: two all ones that touch, and two bits",
                 "64 rows in 3 groups: all ones, two bits, all ones"):
        assert per_segment[name] == [64], name
        rows = [c for c in CASES if c[0] == name][0][2]
        assert np.unique(rows // 31).size == (64 if "64 neighbouring" in name else 3)


def test_reference_index_of_several_lists(oracle):
    """Lists back to back: every list's index shifted by the words in front of it, one total at the end."""
    n = 2981
    lists = [np.array([0, 5, 31744, 95000], np.int64), np.empty(0, np.int64), np.arange(100, 32 * n, 977, dtype=np.int64)]
    stream, index = _rows.reference(oracle, lists, n)
    segments = _select.segments_of(n)
    assert index.size == 3 * segments + 1 and index[0] == 0 and index[-1] == stream.size and np.all(np.diff(index) > 0)
    for c, rows in enumerate(lists):
        own = stream[index[c * segments]: index[(c + 1) * segments]]
        assert np.array_equal(own, oracle.compress(_select.bitmap_of(rows, n)))
        assert np.array_equal(_select.stream_positions(own, n), rows)
    assert list(np.diff(index)[segments: 2 * segments]) == [1] * segments  # the empty list: one zero-fill per segment
    rows, ends = _rows.flatten(lists)
    assert list(ends) == [4, 4, 4 + len(lists[2])] and rows.size == ends[-1]


def _inputs(oracle):
    for name, n, rows, _ in CASES:
        yield name, n, [rows]
    for n, lists in _rows.switch_cases_by_length().items():
        yield f"all switch cases of {n} words as lists of one call", n, lists
    for n in (1, 30, 31, 992, 993, 2976, 2981):
        yield f"parity {n}", n, _rows.parity_lists(oracle, n)
    for k, n in _rows.MANY_LISTS:
        yield f"{k} lists", n, _rows.many_lists(k)


def test_size_bound_holds_and_is_met(oracle):
    met = {}
    for name, n, lists in _inputs(oracle):
        if name.endswith(" lists"):  # one row each: a literal, and a gap on either side of it unless it sits in the first or last group
            words = sum(_rows.one_row_words(int(r[0]), n) for r in lists)
        else:
            words = _rows.reference(oracle, lists, n)[0].size
        bound = _rows.max_words(n, len(lists), sum(len(r) for r in lists))
        assert words <= bound, (name, words, bound)
        met[name] = words == bound
    g, s = _select.groups_of(_select.SEG_WORDS), 1
    n_rows = [c for c in CASES if c[0] == _rows.BOUND_MET_BY_ROWS][0][2].size
    assert met[_rows.BOUND_MET_BY_ROWS] and s + 2 * n_rows < g
    assert met[_rows.BOUND_MET_BY_GROUPS]


def test_many_lists_formula_is_the_oracles(oracle):
    """(the bound test counts the many-list inputs by formula: here the formula is held against the oracle on a sample)"""
    for k, n in ((70, _select.SEG_WORDS), (40, 3 * _select.SEG_WORDS)):
        lists = [np.array([(c * 1019) % _select.SEG_BITS], np.int64) for c in range(k)] + [np.array([0], np.int64), np.array([31 * 1023 + 5], np.int64)]
        want = sum(_rows.one_row_words(int(r[0]), n) for r in lists)
        assert _rows.reference(oracle, lists, n)[0].size == want
