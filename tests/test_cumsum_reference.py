"""CPU tests of the running-sum tests' own reference (tests/_cumsum.py): the value model, its slice matrix through the oracle's
compress() and the restatement of the kernel's steps agree on every named case and on random draws, every wrong model changes the
answer of the named case that is meant to catch it, the default width holds every sum, and the constants the tests state are the
ones in csrc/wah_cumsum.hip."""
import os
import re

import numpy as np
import pytest

from tests import _bsi, _cumsum as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return cs.named_cases()


@pytest.fixture(scope="module")
def answers(cases):
    """The model's answer of every named case, computed once."""
    return {name: cs.expected(case) for name, case in cases.items()}


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def test_named_cases_cover_what_the_interface_names(cases):
    assert {c["n_rows"] for c in cases.values()} >= set(cs.ROW_EDGES) | {32 * cs.BIG}
    for kv in cs.VAL_WIDTHS:
        for k_out in cs.OUT_WIDTHS:
            assert any(c["kv"] == kv and c["k_out"] == k_out for c in cases.values()), (kv, k_out)
    for with_exists in (False, True):
        for exclusive, all_rows in cs.MODES:
            assert any((c["exists"] is not None) == with_exists and c["exclusive"] == exclusive and c["all_rows"] == all_rows and c["kv"] and c["filters"]
                       for c in cases.values()), (with_exists, exclusive, all_rows)
    assert {len(c["filters"]) for c in cases.values()} >= {0, 1, cs.MAX_FILTERS}
    assert {c["n"] for c in cases.values()} == set(cs.SIZES)
    assert set(cs.CAUGHT_BY) == set(cs.WRONG) and len(cs.WRONG) >= 6


def test_the_three_statements_agree_on_the_named_cases(oracle, cases, answers):
    for name, case in cases.items():
        matrix = answers[name]
        assert matrix.shape == (cs.rows_out(case), case["n"]), name
        assert _same(cs.kernel(case), matrix), name
        stream, index = cs.compressed(oracle, matrix)
        assert index.size == matrix.shape[0] * (case["n"] // cs.SEG_WORDS) + 1 and index[0] == 0 and index[-1] == stream.size, name
        assert (np.diff(index) >= 1).all(), name
        assert np.array_equal(np.asarray(oracle.decompress(stream))[: matrix.size], matrix.reshape(-1)), name
        values, exists = _bsi.values_of_slices(matrix, case["k_out"])
        want, sel = cs.values_of(case)
        assert np.array_equal(values, want) and (exists is None) == case["all_rows"] and (exists is None or np.array_equal(exists, sel)), name


def test_the_named_cases_are_not_vacuous(cases, answers):
    for name, matrix in answers.items():
        case = cases[name]
        sel = cs.selection(case)
        if name.startswith("empty selection"):
            assert not sel.any() and not matrix.any(), name
            continue
        assert sel.any() and matrix.any(), name
        if (case["filters"] or case["exists"] is not None) and not name.startswith("every row") and case["n_rows"] > 64:
            assert not sel[: case["n_rows"]].all(), name
    # the sums the issue names: past 2^32 inside the first block and past 2^46 at the end; 2^32 exactly at segment 1's first row
    ones = cases["all ones of 32 bits"]
    run, _ = cs.values_of(ones)
    assert int(run[cs.BLOCK_ROWS - 1]) > 1 << 32 and int(run[-1]) > 1 << 46 and ones["k_out"] == 48 and ones["n"] == 3 * cs.SEG_WORDS
    run, _ = cs.values_of(cases["2^32 at a segment's first row"])
    assert int(run[:cs.SEG_BITS].max()) == (1 << 32) - 1 and int(run[cs.SEG_BITS]) == 1 << 32
    # a result narrower than the true sum
    cut = cases["truncated sum"]
    wide, _ = cs.values_of(dict(cut, k_out=64))
    assert int(wide.max()) >> cut["k_out"] and np.array_equal(cs.values_of(cut)[0], wide & np.uint64((1 << cut["k_out"]) - 1))
    # the base passes through a zero total
    middle = cases["empty middle segment values"]
    assert not cs.selection(middle)[cs.SEG_BITS: 2 * cs.SEG_BITS].any() and cs.selection(middle)[2 * cs.SEG_BITS:].any()


def test_sums_beyond_2_63_stay_exact():
    """The model against Python ints where the 64-bit sum wraps: 2^32 - 1 in 3 * 31 744 rows does not, so the carry is tested on the
    model's own arithmetic with a start near 2^64."""
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 32, 5000, dtype=np.uint64)
    x[0] = np.uint64((1 << 64) - 5)
    run = np.cumsum(x, dtype=np.uint64)
    total = 0
    for i, v in enumerate(x.tolist()):
        total = (total + v) % (1 << 64)
        assert int(run[i]) == total
    assert total < (1 << 63)  # (it wrapped)


@pytest.mark.parametrize("seed", range(24))
def test_the_three_statements_agree_on_random_draws(oracle, seed):
    case = cs.random_case(seed)
    matrix = cs.expected(case)
    assert _same(cs.kernel(case), matrix), seed
    stream, index = cs.compressed(oracle, matrix)
    assert np.array_equal(np.asarray(oracle.decompress(stream))[: matrix.size], matrix.reshape(-1)) and index[-1] == stream.size, seed


@pytest.mark.parametrize("wrong", cs.WRONG)
def test_every_wrong_model_is_caught(cases, answers, wrong):
    name = cs.CAUGHT_BY[wrong]
    assert not _same(cs.kernel(cases[name], wrong), answers[name]), (wrong, name)


def test_the_size_bound_holds():
    """min(64, value width + bit_length(n_rows)) holds the sum of n_rows largest values, and one bit less does not (below 64)."""
    for kv in (0, 1, 7, 31, 32):
        for n_rows in (1, 2, 3, 63, 64, 65, cs.SEG_BITS, 1 << 24, (1 << 32) - 1, 1 << 32, (1 << 32) + 5):
            bound = cs.size_bound(kv, n_rows)
            top = n_rows * ((1 << kv) - 1 if kv else 1)
            assert top < 1 << bound or bound == 64, (kv, n_rows)
            assert bound == min(64, kv + n_rows.bit_length())
    assert cs.size_bound(0, 5) == 3 and 5 >= 1 << 2           # a count needs all of them
    assert cs.size_bound(32, 1 << 32) == 64
    for case in cs.named_cases().values():
        if case["k_out"] >= cs.size_bound(case["kv"], case["n_rows"]):
            wide, _ = cs.values_of(dict(case, k_out=64))
            assert case["k_out"] == 64 or not int(wide.max()) >> case["k_out"]


def test_the_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "gpu-wah_amd", "csrc", "wah_cumsum.hip")).read()
    for name, value in (("kCumsumGridItems", cs.GRID_ITEMS), ("kCumsumBlocks", cs.BLOCKS), ("kCumsumBlockRows", cs.BLOCK_ROWS),
                        ("kCumsumBlockWords", cs.BLOCK_WORDS)):
        assert re.search(r"constexpr u32 %s = %d;" % (name, value), text), name
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    assert re.search(r"#define WAH_GROUP_MAX_FILTERS %du" % cs.MAX_FILTERS, header)
