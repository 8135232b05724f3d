"""CPU proof of the membership tests' own references (tests/_member.py), no library and no device: the value model (np.isin on the
values) and the restatement of the kernel's steps (items, fold, search, groups, halves) agree on every named case and on random
draws; every wrong model of the restatement changes an answer on the named case that is there to catch it; and the headline
cases can fail -- neither all zeros nor all ones, and one set entry less is another answer."""
import numpy as np
import pytest

from tests import _bsi, _member as mb


@pytest.fixture(scope="module")
def cases():
    return mb.named_cases()


def test_model_and_restatement_agree_on_every_named_case(cases):
    assert len(cases) > 150
    for name, case in cases.items():
        assert np.array_equal(mb.kernel(case), mb.expected(case)), name


def test_model_and_restatement_agree_on_random_draws():
    rng = np.random.default_rng(2718)
    for draw in range(60):
        k = int(rng.integers(1, 65))
        n = int(rng.choice([1, 7, 31, 500, 992, 993, 1500, 992 * 2 + 3]))
        values, exists, _ = mb.attribute(n, k, bool(rng.integers(0, 2)), seed=draw, domain=None if draw % 3 else 50)
        negate = bool(rng.integers(0, 2))
        if draw % 2:
            case = mb.bitset_case(n, k, values, exists, int(rng.integers(0, min(1 << k, 5000) + 1)), rng, negate)
        else:
            pool = np.concatenate([values[: int(rng.integers(0, 200))], _bsi.uniform_values(rng, 20, 64)])
            case = mb.list_case(n, k, values, exists, pool.tolist(), negate, poison=values[200:230].tolist() if draw % 4 == 0 else ())
        assert np.array_equal(mb.kernel(case), mb.expected(case)), (draw, n, k)


@pytest.mark.parametrize("wrong", mb.WRONG)
def test_every_wrong_model_changes_an_answer(cases, wrong):
    case = cases[mb.CAUGHT_BY[wrong]]
    want = mb.expected(case)
    assert np.array_equal(mb.kernel(case), want)
    assert not np.array_equal(mb.kernel(case, wrong), want), (wrong, mb.CAUGHT_BY[wrong])


def test_headline_cases_can_fail(cases):
    for name, case in cases.items():
        if not name.startswith("headline") or case["n"] < 31:
            continue
        want = mb.expected(case)
        assert want.any() and not (want == _bsi.ONES).all(), name
        if mb.is_bitset(case):
            held = case["values"][case["values"] < np.uint64(case["set_bits"])] if case["exists"] is None else \
                case["values"][(case["values"] < np.uint64(case["set_bits"])) & case["exists"]]
            at = int(next(v for v in held if case["words"][int(v) >> 5] >> (int(v) & 31) & 1))
            words = case["words"].copy()
            words[at >> 5] &= np.uint32(~(1 << (at & 31)) & 0xFFFFFFFF)
            less = dict(case, words=words)
        else:
            held = case["values"] if case["exists"] is None else case["values"][case["exists"]]
            at = int(np.flatnonzero(np.isin(case["members"], held))[0])
            less = dict(case, members=np.delete(case["members"], at))
        assert not np.array_equal(mb.expected(less), want), name


def test_the_seam_case_plants_what_it_says():
    case = mb.seam_case()
    want = _bsi.unpack_bits(mb.expected(case))
    groups = (32 * case["n"] + 30) // 31
    for row in (31 * 511 + 30, 31 * 512, 2 * mb.SEG_BITS + 31 * 511 + 7, 2 * mb.SEG_BITS + 31 * 512 + 3, 31 * (groups - 1), 32 * case["n"] - 1):
        assert want[row], row
    assert not want[100] and not want[mb.SEG_BITS: 2 * mb.SEG_BITS].any() and not case["exists"][mb.SEG_BITS: 2 * mb.SEG_BITS].any()
