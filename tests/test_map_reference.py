"""CPU tests of the map tests' own reference (tests/_map.py): the value model and the restatement of the kernel's steps agree on
every named case and on random draws, every wrong model changes the answer of the named case that is meant to catch it, the cases
the device tests call refused are refused by both and the others by neither, and the grid cap the tests state is the one in
csrc/wah_map.hip."""
import os
import re

import numpy as np
import pytest

from tests import _map as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return mp.named_cases()


@pytest.fixture(scope="module")
def answers(cases):
    """The model's answer of every named case, computed once."""
    return {name: mp.expected(case) for name, case in cases.items()}


def _same(a, b):
    return a[1] == b[1] and (a[0] is None) == (b[0] is None) and (a[0] is None or (a[0].shape == b[0].shape and np.array_equal(a[0], b[0])))


def test_named_cases_cover_what_the_interface_names(cases):
    for n in mp.SIZES:
        for with_exists, partial in mp.MODES:
            assert any(c["n"] == n and (c["exists"] is not None) == with_exists and c["partial"] == partial for c in cases.values()), (n, with_exists, partial)
    for ks in mp.KEY_WIDTHS:
        for k_out in mp.OUT_WIDTHS:
            assert any(c["ks"] == ks and c["k_out"] == k_out for c in cases.values()), (ks, k_out)
    want = {0, 1, 63, 64, 65, 31, 32, 33, 31 * 1000, 2047, 2048, 2049, mp.HALF_START - 1, mp.HALF_START, mp.HALF_START + 1, mp.SEG_BITS - 1,
            mp.SEG_BITS, mp.SEG_BITS + 1, 32 * mp.BIG - 1, 32 * mp.BIG}
    assert {c["n_rows"] for c in cases.values()} >= want
    sizes = {(c["lookup"].size, 1 << c["ks"]) for c in cases.values()}
    assert any(k == 1 for k, _ in sizes) and any(1 < k < d for k, d in sizes) and any(k == d for k, d in sizes) and any(k > d for k, d in sizes)
    assert any((c["lookup"] == mp.NULL).any() for c in cases.values())
    assert any(c["k_out"] == 32 and (c["lookup"] == mp.NULL - 1).all() for c in cases.values())  # the largest storable value
    assert set(mp.CAUGHT_BY) == set(mp.WRONG) and len(mp.WRONG) >= 5


def test_model_and_restatement_agree_on_the_named_cases(cases, answers):
    for name, case in cases.items():
        assert not answers[name][1], (name, "a named case is not refused")
        assert _same(mp.kernel(case), answers[name]), name


def test_the_named_cases_are_not_vacuous(cases, answers):
    """Values in every result slice wherever rows can have one, rows without a value where the case is partial, and a result of
    fills only under the constant lookup."""
    for name, (matrix, _) in answers.items():
        case = cases[name]
        assert matrix.shape == (case["k_out"] + mp.has_exists_row(case), case["n"]), name
        if case["n_rows"] >= 64:
            assert matrix.any(), name
        if case["partial"] and case["n_rows"] >= 2048 and not name.startswith("constant") and case["lookup"].size >= 64:
            values, has, _ = mp.values_of(case)
            assert not has[: case["n_rows"]].all(), name
    constant = answers["constant lookup"][0]
    assert all((row == 0xFFFFFFFF).all() for row in constant)
    first = answers["n_rows 1"][0]
    assert sum(int(np.unpackbits(row.view(np.uint8)).sum()) for row in first) <= first.shape[0] and not first[:, 1:].any()
    assert not answers["n_rows 0"][0].any()


@pytest.mark.parametrize("seed", range(24))
def test_model_and_restatement_agree_on_random_draws(seed):
    case = mp.random_case(seed)
    assert _same(mp.kernel(case), mp.expected(case)), seed


@pytest.mark.parametrize("wrong", mp.WRONG)
def test_every_wrong_model_is_caught(cases, answers, wrong):
    name = mp.CAUGHT_BY[wrong]
    assert not _same(mp.kernel(cases[name], wrong), answers[name]), (wrong, name)


def test_refusals_of_the_model_and_the_restatement():
    refused, fine = mp.refused_cases()
    assert len(refused) >= 4 and len(fine) >= 3
    for name, case in refused.items():
        assert mp.expected(case) == (None, True) and mp.kernel(case) == (None, True), name
    for name, case in fine.items():
        want = mp.expected(case)
        assert not want[1] and _same(mp.kernel(case), want), name


def test_the_grid_cap_and_the_blocks_are_the_kernels():
    text = open(os.path.join(ROOT, "gpu-wah_amd", "csrc", "wah_map.hip")).read()
    grid = re.search(r"constexpr u32 kMapGridItems = (\d+);", text)
    blocks = re.search(r"constexpr u32 kMapBlocks = (\d+);", text)
    assert grid and blocks and (int(grid.group(1)), int(blocks.group(1))) == (mp.GRID_ITEMS, mp.BLOCKS)
    assert re.search(r"constexpr u32 kMapBlockRows = %d;" % mp.BLOCK_ROWS, text) and re.search(r"constexpr u32 kMapBlockWords = %d;" % mp.BLOCK_WORDS, text)
