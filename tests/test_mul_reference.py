"""CPU tests of the column multiplication helpers (tests/_mul.py): the shift-and-add sweep over the slice matrices, with its
accumulator whose carry slot nobody has written yet and its skip of a zero slice of B, equals the model that answers from the
VALUES for every width triple and all four existence combinations; the package's statement of the table order equals the tests'
own; and the value pairs the GPU tests use hold their planted rows and pass the vacuity guard."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _mul

SIZES = (31, 992)


@pytest.mark.parametrize("n_words", SIZES)
@pytest.mark.parametrize("ka,kb,n_out", _mul.WIDTHS)
def test_sweep_equals_the_value_model(n_words, ka, kb, n_out):
    va, vb, xa, xb, _, _ = _mul.case(n_words, ka, kb, True, True)
    for have_a, have_b in _mul.EXISTENCE:
        ea, eb = (xa if have_a else None), (xb if have_b else None)
        slices_a, slices_b = _bsi.build_slices(va, ka, ea), _bsi.build_slices(vb, kb, eb)
        want = _mul.expected_matrix(va, vb, n_out, ea, eb)
        got = _mul.sweep(slices_a, ka, slices_b, kb, n_out, have_a, have_b)
        assert got.shape == want.shape == (n_out + (have_a or have_b), n_words), (have_a, have_b)
        assert np.array_equal(got, want), (have_a, have_b)
        # the skip of a zero slice changes nothing
        assert np.array_equal(_mul.sweep(slices_a, ka, slices_b, kb, n_out, have_a, have_b, skip_zero=False), want), (have_a, have_b)
        # rows that do not exist may hold anything in the operands: the result stores them as 0 all the same
        zeroed_a, zeroed_b = _bsi.build_slices(va, ka, ea, zero_missing=True), _bsi.build_slices(vb, kb, eb, zero_missing=True)
        assert np.array_equal(_mul.sweep(zeroed_a, ka, zeroed_b, kb, n_out, have_a, have_b), want), (have_a, have_b)


@pytest.mark.parametrize("ka,kb,n_out", _mul.WIDTHS)
def test_sweep_with_zero_slices_of_b(ka, kb, n_out):
    """Every slice of B but one zeroed in turn (the first, a middle one, the last), and B a constant of all-ones and zero slices:
    the skipped steps write their carry slots, every slice a later step reads has been written."""
    n_words = 31
    va, vb, _, _, _, _ = _mul.case(n_words, ka, kb, False, False, seed=1)
    slices_a = _bsi.build_slices(va, ka)
    for cleared in sorted({0, kb // 2, kb - 1}):
        wb = vb & ~np.uint64(1 << cleared)
        assert np.array_equal(_mul.sweep(slices_a, ka, _bsi.build_slices(wb, kb), kb, n_out), _mul.expected_matrix(va, wb, n_out)), cleared
    for c in (0, 1, (1 << kb) - 1, 0x8000000000000421 & ((1 << kb) - 1)):
        wb = np.full(va.shape, c, dtype=np.uint64)
        assert np.array_equal(_mul.sweep(slices_a, ka, _bsi.build_slices(wb, kb), kb, n_out), _mul.expected_matrix(va, wb, n_out)), c


@pytest.mark.parametrize("ka,kb,n_out", _mul.WIDTHS)
def test_value_pairs_hold_their_planted_rows_and_can_fail(ka, kb, n_out):
    n_words = 992
    for have_a, have_b in _mul.EXISTENCE:
        va, vb, xa, xb, planted, absent = _mul.case(n_words, ka, kb, have_a, have_b)
        assert va.size == vb.size == 32 * n_words and (xa is not None) == have_a and (xb is not None) == have_b
        assert len(set(planted.values()) | set(absent)) == len(planted) + 2
        for (pa, pb), row in planted.items():
            assert int(va[row]) == pa and int(vb[row]) == pb
            assert (xa is None or xa[row]) and (xb is None or xb[row])
        top = ((1 << ka) - 1, (1 << kb) - 1)
        for wanted in (top, (0, top[1]), (top[0], 0), (1 << (ka - 1), top[1]), (top[0], 1 << (kb - 1))):
            assert wanted in planted, wanted
        assert xa is None or (not xa[absent[0]] and (xb is None or xb[absent[0]]))
        assert xb is None or (not xb[absent[1]] and (xa is None or xa[absent[1]]))
        _mul.assert_mul_matters(va, vb, ka, kb, n_out, xa, xb, (ka, kb, n_out, have_a, have_b))


def test_the_guard_refuses_vacuous_inputs():
    rows = 32 * 31
    rng = np.random.default_rng(3)
    va, vb = _bsi.uniform_values(rng, rows, 8), _bsi.uniform_values(rng, rows, 8)
    _mul.assert_mul_matters(va, vb, 8, 8, 16, None, None, "uniform")
    with pytest.raises(AssertionError):  # B == 0: every slice is empty
        _mul.assert_mul_matters(va, np.zeros(rows, np.uint64), 8, 8, 16, None, None, "zero")
    with pytest.raises(AssertionError):  # B even: slice 0 of the product is empty
        _mul.assert_mul_matters(va, vb & np.uint64(0xFE), 8, 8, 16, None, None, "even")
    with pytest.raises(AssertionError):  # no row of A and B exists at once
        _mul.assert_mul_matters(va, vb, 8, 8, 16, np.arange(rows) % 2 == 0, np.arange(rows) % 2 == 1, "disjoint existence")
    with pytest.raises(AssertionError):  # an existence row that is full changes nothing when it is dropped
        _mul.assert_mul_matters(va, vb, 8, 8, 16, np.ones(rows, bool), None, "full existence")


def test_row_order_is_the_packages():
    pkg = importlib.import_module("gpu-wah_amd")
    for ka in (1, 2, 3, 13, 20, 40, 41, 63, 64):
        for kb in (1, 2, 5, 13, 20, 40, 41, 63, 64):
            for have_a, have_b in _mul.EXISTENCE:
                order = _mul.row_order(ka, kb, have_a, have_b)
                assert pkg.bsi_mul_row_order(ka, kb, have_a, have_b) == order, (ka, kb, have_a, have_b)
                assert len(order) == ka + kb + have_a + have_b
                assert sorted(i for who, i in order if who == "a") == list(range(ka + have_a))
                assert sorted(i for who, i in order if who == "b") == list(range(kb + have_b))
    # XA, XB, A0, A1, A2, B0, B1 in significances: no interleaving
    assert _mul.row_order(3, 2, True, True) == [("a", 3), ("b", 2), ("a", 2), ("a", 1), ("a", 0), ("b", 1), ("b", 0)]
    assert _mul.row_order(1, 3, False, True) == [("b", 3), ("a", 0), ("b", 2), ("b", 1), ("b", 0)]
    # (40, 41) with A's existence row: B starts in table row 41, inside the first chunk of 64 rows, and crosses the edge at slice 23
    order = _mul.row_order(40, 41, True, False)
    assert order[40] == ("a", 0) and order[41] == ("b", 40) and order[63] == ("b", 41 - 1 - 22) and order[64] == ("b", 41 - 1 - 23)
    assert len(_mul.row_order(64, 64, True, True)) == 130
    for bad in ((0, 5), (5, 0), (65, 1), (1, 65)):
        with pytest.raises(pkg.WahError):
            pkg.bsi_mul_row_order(*bad)


def test_semantics_of_the_edges():
    """Unsigned operands; ka + kb slices lose nothing; fewer truncate, more zero-extend; the product is right at 64 bits, where
    ka + kb reaches 128."""
    top = (1 << 64) - 1
    va = np.array([0, 5, 5, top, 1 << 63, 3, 0, 255, top, 1 << 32] + [0] * 22, dtype=np.uint64)
    vb = np.array([0, 4, 6, 1, 2, 3, 1, 255, top, 1 << 32] + [0] * 22, dtype=np.uint64)
    ints = [(int(a), int(b)) for a, b in zip(va, vb)]
    for n_out in (1, 8, 63, 64):
        assert [int(v) for v in _mul.expected_values(va, vb, n_out)] == [(a * b) % (1 << n_out) for a, b in ints]
    small_a, small_b = va & np.uint64(0xFF), vb & np.uint64(0x0F)
    sa, sb = _bsi.build_slices(small_a, 8), _bsi.build_slices(small_b, 4)
    full = _mul.sweep(sa, 8, sb, 4, 12)
    values, _ = _bsi.values_of_slices(full, 12)
    assert np.array_equal(values, small_a * small_b) and int(values.max()) == 255 * 15  # nothing lost
    wide = _mul.sweep(sa, 8, sb, 4, 20)
    assert not wide[:8].any() and np.array_equal(wide[8:], full)  # zero extension
    assert np.array_equal(_mul.sweep(sa, 8, sb, 4, 5), full[7:])  # truncation keeps the low slices
    assert np.array_equal(_mul.sweep(sb, 4, sa, 8, 12), full)  # commutative
    s64a, s64b = _bsi.build_slices(va, 64), _bsi.build_slices(vb, 64)
    assert np.array_equal(_mul.sweep(s64a, 64, s64b, 64, 64), _mul.expected_matrix(va, vb, 64))
