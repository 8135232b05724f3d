"""CPU tests of the group-by tests' own reference (tests/_groupby.py): the value model and the restatement of the kernel's steps
agree on every named case and on random draws, every wrong model changes the answer of the named case that is meant to catch it,
and the two thresholds the restatement states are the ones in csrc/wah_group_by.hip."""
import os
import re

import numpy as np
import pytest

from tests import _groupby as gb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return gb.named_cases()


@pytest.fixture(scope="module")
def answers(cases):
    """The model's answer of every named case, computed once."""
    return {name: gb.expected(case) for name, case in cases.items()}


def test_named_cases_cover_what_the_interface_names(cases):
    for n in gb.SIZES:
        assert any(c["n"] == n for c in cases.values()), n
    for ks in gb.KEY_WIDTHS:
        for vs in gb.VALUE_WIDTHS:
            assert any(c["ks"] == ks and c["vs"] == vs for c in cases.values()), (ks, vs)
    for n_filters in gb.FILTER_COUNTS:
        for with_exists in (False, True):
            assert any(len(c["filters"]) == n_filters and (c["exists"] is not None) == with_exists for c in cases.values())
    for nb in (1, gb.LDS_BUCKETS - 1, gb.LDS_BUCKETS, 1 << 12):
        assert any(c["n_buckets"] == nb for c in cases.values()), nb
    big = 32 * gb.BIG
    assert {c["n_rows"] for c in cases.values()} >= {big, big - 1, 0, gb.SEG_BITS, gb.SEG_BITS - 1, gb.SEG_BITS + 1, 31 * 1000, 31 * 1000 + 1}
    assert set(gb.CAUGHT_BY) == set(gb.WRONG) and len(gb.WRONG) >= 6


def test_model_and_restatement_agree_on_the_named_cases(cases, answers):
    for name, case in cases.items():
        assert gb.kernel(case) == answers[name], name


def test_the_named_cases_are_not_vacuous(cases, answers):
    """Counts in more than one bucket wherever there is more than one, rows in "other" where the case is about it, and a carry where
    the case is about that."""
    for name, (counts, sums) in answers.items():
        case = cases[name]
        if case["n_rows"] > 64 and case["prefill"] is None:
            assert sum(counts) > 0, name
            assert sums is None or sum(sums) > 0, name
    assert answers["buckets 4096 under a 32-slice key"][0][-1] > sum(answers["buckets 4096 under a 32-slice key"][0][:-1]) > 0
    assert answers["buckets 1 x 17"][0][1] > 0 and answers["map: n_keys below the domain"][0][-1] > 0
    for name in ("carry lds", "carry global"):
        counts, sums = answers[name]
        assert any(s >> 64 == 4 for s in sums) and all(c >= 7 for c in counts), name


@pytest.mark.parametrize("seed", range(40))
def test_model_and_restatement_agree_on_random_draws(seed):
    case = gb.random_case(seed)
    assert gb.kernel(case) == gb.expected(case), seed


@pytest.mark.parametrize("wrong", gb.WRONG)
def test_every_wrong_model_is_caught(cases, answers, wrong):
    name = gb.CAUGHT_BY[wrong]
    assert gb.kernel(cases[name], wrong) != answers[name], (wrong, name)


def test_buckets_of_a_lookup():
    case = dict(n_buckets=4, lookup=np.array([0, 3, 4, gb.DROP, 2], np.uint32))
    assert gb.buckets_of(case, np.array([0, 1, 2, 3, 4, 5, 1 << 31], np.uint64)).tolist() == [0, 3, 4, 4, 2, 4, 4]
    assert gb.buckets_of(dict(n_buckets=4, lookup=None), np.array([0, 3, 4, 1 << 31], np.uint64)).tolist() == [0, 3, 4, 4]


def test_thresholds_are_the_kernels():
    text = open(os.path.join(ROOT, "gpu-wah_amd", "csrc", "wah_group_by.hip")).read()
    grid = re.search(r"constexpr u32 kGroupByGridItems = (\d+);", text)
    lds = re.search(r"constexpr u32 kGroupByLdsBuckets = (\d+);", text)
    assert grid and lds
    assert (int(grid.group(1)), int(lds.group(1))) == (gb.GRID_ITEMS, gb.LDS_BUCKETS)
    assert re.search(r"a\.n_buckets \+ 1u <= kGroupByLdsBuckets", text)
