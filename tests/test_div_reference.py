"""CPU tests of the column division helpers (tests/_div.py): the restoring long division over the slice matrices, with its
lazily blended remainder and its skip of the dividend's leading zero slices, equals the model that answers from the VALUES for
every width triple, both results and all four existence combinations; A == Q * B + R and R < B hold in Python ints; every wrong
model changes an answer on a named case; the package's statement of the table order equals the tests' own; and the value pairs
the GPU tests use hold their planted rows and pass the vacuity guard."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _div

SIZES = (31, 992)
GPU_SIZES = (992, 2 * 992, 5 * 992)  # tests/test_gpu_bsi_div.py


@pytest.mark.parametrize("n_words", SIZES)
@pytest.mark.parametrize("ka,kb,n_out", _div.WIDTHS)
def test_sweep_equals_the_value_model(n_words, ka, kb, n_out):
    va, vb, xa, xb, _, _ = _div.case(n_words, ka, kb, True, True)
    for have_a, have_b in _div.EXISTENCE:
        ea, eb = (xa if have_a else None), (xb if have_b else None)
        slices_a, slices_b = _bsi.build_slices(va, ka, ea), _bsi.build_slices(vb, kb, eb)
        zeroed_a, zeroed_b = _bsi.build_slices(va, ka, ea, zero_missing=True), _bsi.build_slices(vb, kb, eb, zero_missing=True)
        for remainder in (False, True):
            want = _div.expected_matrix(va, vb, n_out, remainder, ea, eb)
            got = _div.sweep(slices_a, ka, slices_b, kb, n_out, remainder, have_a, have_b)
            assert got.shape == want.shape == (n_out + 1, n_words), (have_a, have_b, remainder)
            assert np.array_equal(got, want), (have_a, have_b, remainder)
            # the skip changes nothing
            assert np.array_equal(_div.sweep(slices_a, ka, slices_b, kb, n_out, remainder, have_a, have_b, skip=False), want), (have_a, have_b)
            # rows that do not exist may hold anything in the operands: the result stores them as 0 all the same
            assert np.array_equal(_div.sweep(zeroed_a, ka, zeroed_b, kb, n_out, remainder, have_a, have_b), want), (have_a, have_b)


@pytest.mark.parametrize("ka,kb,n_out", _div.WIDTHS)
def test_quotient_times_divisor_plus_remainder(ka, kb, n_out):
    """With all slices kept, A == Q * B + R and R < B in every row that exists, in Python ints; a row with B = 0 does not exist."""
    n_words = 31
    va, vb, _, _, _, _ = _div.case(n_words, ka, kb, False, False, seed=1)
    slices_a, slices_b = _bsi.build_slices(va, ka), _bsi.build_slices(vb, kb)
    quotient, qx = _bsi.values_of_slices(_div.sweep(slices_a, ka, slices_b, kb, ka, False), ka)
    rest, rx = _bsi.values_of_slices(_div.sweep(slices_a, ka, slices_b, kb, min(ka, kb), True), min(ka, kb))
    assert np.array_equal(qx, rx) and np.array_equal(qx, vb != 0) and qx.any() and not qx.all()
    for a, b, q, r, x in zip(va.tolist(), vb.tolist(), quotient.tolist(), rest.tolist(), qx.tolist()):
        if x:
            assert a == q * b + r and r < b, (a, b, q, r)
        else:
            assert b == 0 and q == 0 and r == 0


# the case on which each wrong model shows: (ka, kb, n_out, remainder)
SHOWS = {
    "zero_divisor_kept": (8, 8, 8, False),
    "narrow_ripple": (20, 13, 20, False),  # (needs ka > kb: a partial remainder of i steps is below 2^i)
    "not_restored": (8, 8, 8, False),
    "a_least_significant_first": (5, 3, 5, False),
    "skip_after_nonzero": (20, 13, 20, False),
    "truncated_dividend": (40, 41, 20, False),
    "unblended_remainder": (8, 8, 8, True),
}


@pytest.mark.parametrize("wrong", _div.WRONG)
def test_every_wrong_model_changes_an_answer(wrong):
    ka, kb, n_out, remainder = SHOWS[wrong]
    n_words = 31
    va, vb, _, _, _, _ = _div.case(n_words, ka, kb, False, False)
    if wrong == "skip_after_nonzero":  # a slice of A that is all zero below a non-zero one
        va = va & ~np.uint64(1 << 7)
    slices_a, slices_b = _bsi.build_slices(va, ka), _bsi.build_slices(vb, kb)
    want = _div.expected_matrix(va, vb, n_out, remainder)
    assert np.array_equal(_div.sweep(slices_a, ka, slices_b, kb, n_out, remainder), want)
    assert not np.array_equal(_div.sweep(slices_a, ka, slices_b, kb, n_out, remainder, wrong=wrong), want), wrong


def test_the_skip_runs_where_leading_slices_are_zero():
    ka, kb, n_words = 20, 13, 31
    va, vb, _, _, _, _ = _div.case(n_words, ka, kb, False, False, seed=2)
    slices_b = _bsi.build_slices(vb, kb)
    for zero_top, zero_mid in ((0, False), (3, False), (3, True), (ka, False)):
        wa = va & np.uint64((1 << (ka - zero_top)) - 1)
        if zero_mid:
            wa = wa & ~np.uint64(1 << 5)
        slices_a = _bsi.build_slices(wa, ka)
        for remainder in (False, True):
            stats = {}
            want = _div.expected_matrix(wa, vb, ka, remainder)
            assert np.array_equal(_div.sweep(slices_a, ka, slices_b, kb, ka, remainder, stats=stats), want)
            assert stats["skipped"] == zero_top, (zero_top, zero_mid)  # a zero slice below a non-zero one is not skipped
            assert np.array_equal(_div.sweep(slices_a, ka, slices_b, kb, ka, remainder, skip=False, stats=stats), want)
            assert stats["skipped"] == 0


def test_a_divisor_below_its_declared_width():
    """B's slices above its last one that is not all zero are left out of every ripple: the answers do not change, with the
    dividend wider than the divisor's real width and narrower, and with a divisor that is zero everywhere."""
    ka, kb, n_words = 20, 13, 31
    va, vb, _, _, _, _ = _div.case(n_words, ka, kb, False, False, seed=3)
    slices_a = _bsi.build_slices(va, ka)
    for real in (0, 1, 5, 12):
        wb = vb & np.uint64((1 << real) - 1)
        slices_b = _bsi.build_slices(wb, kb)
        for n_out in (3, ka):
            for remainder in (False, True):
                want = _div.expected_matrix(va, wb, n_out, remainder)
                assert np.array_equal(_div.sweep(slices_a, ka, slices_b, kb, n_out, remainder), want), (real, n_out, remainder)
                assert np.array_equal(_div.sweep(slices_a, ka, slices_b, kb, n_out, remainder, skip=False), want), (real, n_out, remainder)


@pytest.mark.parametrize("n_words", GPU_SIZES)
@pytest.mark.parametrize("ka,kb,n_out", _div.WIDTHS)
def test_value_pairs_hold_their_planted_rows_and_can_fail(n_words, ka, kb, n_out):
    combos = _div.EXISTENCE if n_words == GPU_SIZES[0] else ((False, False), (True, True))
    for have_a, have_b in combos:
        va, vb, xa, xb, planted, absent = _div.case(n_words, ka, kb, have_a, have_b)
        assert va.size == vb.size == 32 * n_words and (xa is not None) == have_a and (xb is not None) == have_b
        assert len(set(planted.values()) | set(absent)) == len(planted) + 2
        for (pa, pb), row in planted.items():
            assert int(va[row]) == pa and int(vb[row]) == pb
            assert (xa is None or xa[row]) and (xb is None or xb[row])
        top = ((1 << ka) - 1, (1 << kb) - 1)
        for wanted in ((top[0], 1), (0, top[1]), top, (top[0], 0), (0, 0), (1 << (ka - 1), 1), (1, top[1]), (top[0], 1 << (kb - 1))):
            assert wanted in planted, wanted
        assert kb == 1 or kb > ka or (top[1] - 1, top[1]) in planted
        assert xa is None or (not xa[absent[0]] and (xb is None or xb[absent[0]]))
        assert xb is None or (not xb[absent[1]] and (xa is None or xa[absent[1]]))
        for remainder in (False, True):
            _div.assert_div_matters(va, vb, ka, kb, n_out, remainder, xa, xb, (ka, kb, n_out, remainder, have_a, have_b))


def test_the_guard_refuses_vacuous_inputs():
    rows = 32 * 31
    rng = np.random.default_rng(3)
    va, vb, _, _, _, _ = _div.case(31, 8, 8, False, False)
    _div.assert_div_matters(va, vb, 8, 8, 8, False, None, None, "headline")
    _div.assert_div_matters(va, vb, 8, 8, 8, True, None, None, "headline")
    with pytest.raises(AssertionError):  # half the divisors are zero
        _div.assert_div_matters(va, np.where(np.arange(rows) % 2 == 0, vb, np.uint64(0)), 8, 8, 8, False, None, None, "zeros")
    with pytest.raises(AssertionError):  # no divisor is zero: the existence row is that of the operands
        _div.assert_div_matters(va, vb | np.uint64(1), 8, 8, 8, False, None, None, "no zero divisor")
    with pytest.raises(AssertionError):  # uniform operands of one width: the quotient's top slices are all but empty -- here empty
        _div.assert_div_matters(_bsi.uniform_values(rng, rows, 8) | np.uint64(128), vb | np.uint64(128), 8, 8, 8, False, None, None, "uniform")
    with pytest.raises(AssertionError):  # an existence row that is full changes nothing when it is dropped
        _div.assert_div_matters(va, vb, 8, 8, 8, False, np.ones(rows, bool), None, "full existence")


def test_row_order_is_the_packages():
    pkg = importlib.import_module("gpu-wah_amd")
    for ka in (1, 2, 3, 13, 20, 40, 41, 63, 64):
        for kb in (1, 2, 5, 13, 20, 40, 41, 63, 64):
            for have_a, have_b in _div.EXISTENCE:
                order = _div.row_order(ka, kb, have_a, have_b)
                assert pkg.bsi_div_row_order(ka, kb, have_a, have_b) == order, (ka, kb, have_a, have_b)
                assert len(order) == ka + kb + have_a + have_b
                assert sorted(i for who, i in order if who == "a") == list(range(ka + have_a))
                assert sorted(i for who, i in order if who == "b") == list(range(kb + have_b))
    # XA, XB, B0, B1, A2, A1, A0 in significances
    assert _div.row_order(3, 2, True, True) == [("a", 3), ("b", 2), ("b", 1), ("b", 0), ("a", 0), ("a", 1), ("a", 2)]
    assert _div.row_order(1, 3, False, True) == [("b", 3), ("b", 2), ("b", 1), ("b", 0), ("a", 0)]
    # (40, 41) with A's existence row: A starts in table row 42, and the second chunk of 64 rows begins with its slice of significance 17
    order = _div.row_order(40, 41, True, False)
    assert order[1] == ("b", 40) and order[41] == ("b", 0) and order[42] == ("a", 0) and order[64] == ("a", 22) and len(order) == 82
    assert len(_div.row_order(64, 64, True, True)) == 130
    for bad in ((0, 5), (5, 0), (65, 1), (1, 65)):
        with pytest.raises(pkg.WahError):
            pkg.bsi_div_row_order(*bad)


def test_semantics_of_the_edges():
    """Unsigned operands at 64 bits; ka slices lose nothing of the quotient and min(ka, kb) nothing of the remainder; fewer truncate,
    more zero-extend; x / 0 is NULL."""
    top = (1 << 64) - 1
    va = np.array([0, 5, 5, top, 1 << 63, 3, 7, 255, top, 1 << 32, top, top - 1] + [0] * 20, dtype=np.uint64)
    vb = np.array([0, 4, 6, 1, 2, 3, 0, 255, top, 1 << 31, 1 << 63, top] + [0] * 20, dtype=np.uint64)
    ints = [(int(a), int(b)) for a, b in zip(va, vb)]
    for n_out in (1, 8, 63, 64):
        assert [int(v) for v in _div.expected_values(va, vb, n_out, False)] == [(a // b) % (1 << n_out) if b else 0 for a, b in ints]
        assert [int(v) for v in _div.expected_values(va, vb, n_out, True)] == [(a % b) % (1 << n_out) if b else 0 for a, b in ints]
    s64a, s64b = _bsi.build_slices(va, 64), _bsi.build_slices(vb, 64)
    for remainder in (False, True):
        got = _div.sweep(s64a, 64, s64b, 64, 64, remainder)
        assert np.array_equal(got, _div.expected_matrix(va, vb, 64, remainder))
        assert np.array_equal(_bsi.unpack_bits(got[64]), vb != 0)
    small_a, small_b = va & np.uint64(0xFF), vb & np.uint64(0x0F)
    sa, sb = _bsi.build_slices(small_a, 8), _bsi.build_slices(small_b, 4)
    full = _div.sweep(sa, 8, sb, 4, 8, False)
    wide = _div.sweep(sa, 8, sb, 4, 20, False)
    assert not wide[:12].any() and np.array_equal(wide[12:], full)  # zero extension
    assert np.array_equal(_div.sweep(sa, 8, sb, 4, 5, False)[:5], full[3:8])  # truncation keeps the low slices
    rest = _div.sweep(sa, 8, sb, 4, 4, True)
    assert np.array_equal(_div.sweep(sa, 8, sb, 4, 9, True)[5:], rest) and not _div.sweep(sa, 8, sb, 4, 9, True)[:5].any()
