"""CPU tests of tests/_kthg.py: the numpy restatement of the lane-wise radix select (the items, the short cut of an item that
selects nothing, the item that checks the slices, one histogram and one decision per lane) equals the model that answers from the
VALUES on every shape the GPU tests use, and the inputs have what keeps those tests from being vacuous."""
import numpy as np
import pytest

from tests import _kth, _kthg

SHAPES = _kthg.shapes()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_restatement_equals_the_value_model(name):
    case = SHAPES[name]
    assert _kthg.restate(case) == case.model(), name


def test_the_grid_cap_is_read_from_the_source():
    assert _kthg.grid_cap() == 1024  # 256 CUs x four resident workgroups; a cap that moves: revisit second_item() and DESIGN.md
    assert _kthg.digit_bits() == 4
    items = _kthg.wave_items(10)
    assert [r for r in items if r] == [[i] for i in range(10)] and len(items) == 12
    cap_waves = _kthg.grid_cap() * _kthg.PASS_WAVES
    runs = _kthg.wave_items(cap_waves + 3)
    assert len(runs) == cap_waves and runs[0] == [0, cap_waves] and runs[2] == [2, cap_waves + 2] and runs[3] == [3]


def test_answers_differ_between_groups():
    for name in ("two keys", "no filter", "clustered", "second item", "width 20"):
        _kthg.assert_groups_differ(SHAPES[name])
    # overlapping: the group given twice through a repeated row answers as the first one, the empty one finds nothing
    m = SHAPES["overlapping"].model()
    assert m[0] == m[2] and m[0] != m[1] and all(r == (0, 0, 0, 0, 0) for r in m[3])


def test_two_queries_of_one_group_leave_pass_0_with_different_prefixes():
    trace = {}
    case = SHAPES["width 9"]
    _kthg.restate(case, trace)
    n_q = len(case.queries)
    for g in range(len(case.groups)):
        prefixes = trace["prefix0"][g * n_q: (g + 1) * n_q]
        assert len(set(prefixes)) == n_q, (g, prefixes)  # MIN, median and MAX part in the first digit


def test_every_bucket_is_picked_and_both_outcomes_of_found_occur():
    trace = {}
    case = SHAPES["spread"]
    got = _kthg.restate(case, trace)
    assert {b for width, b in trace["picks"] if width == 4} == set(range(16))
    assert {b for width, b in trace["picks"] if width == 1} == {0, 1}  # 9 slices: the last digit is one slice
    found = {r[0] for rows in got for r in rows}
    assert found == {0, 1}
    assert len(case.queries) == len(_kth.query_cases(0, spread=True)) and case.lanes == 3 * len(case.queries)


def test_the_clustered_shape_has_items_with_and_without_a_selection_in_every_pass():
    trace = {}
    case = SHAPES["clustered"]
    _kthg.restate(case, trace)
    n_seg = -(-case.rows // _kthg.SEG_BITS)
    for p, (counted, skipped) in enumerate(zip(trace["counted"], trace["skipped"])):
        assert counted and skipped and len(counted) + len(skipped) == n_seg * case.lanes, p
        assert len(skipped) > len(counted), p  # most items end behind their group's row
    # the checking items: lane 0 in the last pass, every segment, also where group 0 has no row
    assert trace["checked"] == set(range(n_seg))
    last = len(trace["counted"]) - 1
    empty_for_lane_0 = [seg for seg in range(n_seg) if not case.selected(0)[seg * _kthg.SEG_BITS: (seg + 1) * _kthg.SEG_BITS].any()]
    assert empty_for_lane_0 and all((seg, 0) in trace["counted"][last] and (seg, 0) in trace["skipped"][0] for seg in empty_for_lane_0)
    # the last group lives in the ragged last segment alone
    rows_of_last = np.flatnonzero(case.groups[-1][0])
    assert rows_of_last.size == _kthg.CLUSTERED_TAIL and rows_of_last[0] >= (n_seg - 1) * _kthg.SEG_BITS and case.n_words % _kthg.SEG_WORDS
    assert all(r[0] == 1 for r in case.model()[-1])


def test_a_wavefront_does_not_keep_one_lane():
    """Every (segment, lane) pair is exactly one item; and where the lanes divide the grid's wavefronts -- 128 lanes, 4096
    wavefronts: without the turn a wavefront would have ONE lane in all its items -- the items of lane 0, which walk every slice in
    the last pass, lie in as many wavefronts as there are segments."""
    for lanes, n_seg in ((1, 9), (2, 9), (3, 9), (12, 700), (70, 59), (128, 529), (4096, 3)):
        n_items = n_seg * lanes
        pairs = [_kthg.item_of(i, lanes, n_items) for i in range(n_items)]
        assert sorted(pairs) == [(s, l) for s in range(n_seg) for l in range(lanes)], lanes
    lanes, n_seg = 128, 529
    n_items = lanes * n_seg
    waves = _kthg.grid_waves(n_items)
    assert waves == _kthg.grid_cap() * _kthg.PASS_WAVES and waves % lanes == 0
    of_lane_0 = [i % waves for i in range(n_items) if _kthg.item_of(i, lanes, n_items)[1] == 0]
    assert len(of_lane_0) == n_seg == len(set(of_lane_0))


def test_the_second_item_shape_is_above_the_cap():
    case = SHAPES["second item"]
    assert _kthg.assert_second_item(case) > 0
    assert case.lanes == 70


def test_wrong_kernels_would_fail():
    """What a kernel that shares state between lanes would answer differs from the model: lane 0's answers for everybody."""
    case = SHAPES["two keys"]
    m = case.model()
    assert any(m[g] != m[0] for g in range(1, len(m)))
    # a short cut taken by the checking item too would leave slice segments unwalked
    trace = {}
    _kthg.restate(SHAPES["clustered"], trace)
    assert any((seg, 0) in trace["skipped"][0] for seg in trace["checked"])
