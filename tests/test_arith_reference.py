"""CPU tests of the column arithmetic helpers (tests/_arith.py): the ex / carry / hold sweep over the slice matrices equals the
model that answers from the VALUES, for both operations, every width triple and all four existence combinations; the package's
statement of the table order equals the tests' own; and the value pairs the GPU tests use pass the vacuity guard."""
import importlib

import numpy as np
import pytest

from tests import _arith, _bsi

SIZES = (31, 992 * 2)


@pytest.mark.parametrize("n_words", SIZES)
@pytest.mark.parametrize("ka,kb,n_out", _arith.WIDTHS)
def test_sweep_equals_the_value_model(n_words, ka, kb, n_out):
    for op in _arith.OPS:
        va, vb, xa, xb, _ = _arith.case(n_words, ka, kb, op, True, True)
        for have_a, have_b in _arith.EXISTENCE:
            ea, eb = (xa if have_a else None), (xb if have_b else None)
            slices_a, slices_b = _bsi.build_slices(va, ka, ea), _bsi.build_slices(vb, kb, eb)
            want = _arith.expected_matrix(va, vb, op, n_out, ea, eb)
            got = _arith.sweep(slices_a, ka, slices_b, kb, op, n_out, have_a, have_b)
            assert got.shape == want.shape == (n_out + (have_a or have_b), n_words), (op, have_a, have_b)
            assert np.array_equal(got, want), (op, have_a, have_b)
            # rows that do not exist may hold anything in the operands: the result stores them as 0 all the same
            zeroed_a, zeroed_b = _bsi.build_slices(va, ka, ea, zero_missing=True), _bsi.build_slices(vb, kb, eb, zero_missing=True)
            assert np.array_equal(_arith.sweep(zeroed_a, ka, zeroed_b, kb, op, n_out, have_a, have_b), want), (op, have_a, have_b)


@pytest.mark.parametrize("n_words", (992, 992 * 2))
@pytest.mark.parametrize("ka,kb,n_out", _arith.WIDTHS)
def test_value_pairs_can_fail(n_words, ka, kb, n_out):
    for op in _arith.OPS:
        for have_a, have_b in _arith.EXISTENCE:
            va, vb, xa, xb, planted = _arith.case(n_words, ka, kb, op, have_a, have_b)
            assert va.size == vb.size == 32 * n_words and (xa is not None) == have_a and (xb is not None) == have_b
            assert len(set(planted.values())) == len(planted)
            for (pa, pb), row in planted.items():
                assert int(va[row]) == pa and int(vb[row]) == pb
            _arith.assert_arith_matters(va, vb, ka, kb, n_out, xa, xb, (n_words, ka, kb, n_out, op, have_a, have_b))


def test_the_guard_refuses_vacuous_inputs():
    rows = 32 * 31
    rng = np.random.default_rng(3)
    va, vb = _bsi.uniform_values(rng, rows, 8), _bsi.uniform_values(rng, rows, 8)
    _arith.assert_arith_matters(va, vb, 8, 8, 9, None, None, "uniform")
    with pytest.raises(AssertionError):  # B == 0: ADD and SUB give one answer, and no slice of the carry is set
        _arith.assert_arith_matters(va, np.zeros(rows, np.uint64), 8, 8, 9, None, None, "zero")
    with pytest.raises(AssertionError):  # A == B: every slice of the difference is empty
        _arith.assert_arith_matters(va, va, 8, 8, 9, None, None, "equal")
    with pytest.raises(AssertionError):  # no row of A and B exists at once: every slice is empty
        _arith.assert_arith_matters(va, vb, 8, 8, 9, np.arange(rows) % 2 == 0, np.arange(rows) % 2 == 1, "disjoint existence")
    with pytest.raises(AssertionError):  # an existence row that is full changes nothing when it is dropped
        _arith.assert_arith_matters(va, vb, 8, 8, 9, np.ones(rows, bool), None, "full existence")


def test_row_order_is_the_packages():
    pkg = importlib.import_module("gpu-wah_amd")
    for ka in (1, 2, 13, 20, 40, 41, 63, 64):
        for kb in (1, 2, 13, 20, 40, 41, 63, 64):
            for have_a, have_b in _arith.EXISTENCE:
                order = _arith.row_order(ka, kb, have_a, have_b)
                assert pkg.bsi_arith_row_order(ka, kb, have_a, have_b) == order, (ka, kb, have_a, have_b)
                assert len(order) == ka + kb + have_a + have_b
                assert sorted(i for who, i in order if who == "a") == list(range(ka + have_a))
                assert sorted(i for who, i in order if who == "b") == list(range(kb + have_b))
    # existence rows first, then least significant first: XA, XB, A0, B0, A1, B1, A2 in significances
    assert _arith.row_order(3, 2, True, True) == [("a", 3), ("b", 2), ("a", 2), ("b", 1), ("a", 1), ("b", 0), ("a", 0)]
    assert _arith.row_order(1, 3, False, True) == [("b", 3), ("a", 0), ("b", 2), ("b", 1), ("b", 0)]
    # (40, 41) with A's existence row: the held A slice of significance 31 in table row 63, its B slice in row 64, the first of the
    # second chunk of 64 rows
    order = _arith.row_order(40, 41, True, False)
    assert order[63] == ("a", 40 - 1 - 31) and order[64] == ("b", 41 - 1 - 31)
    assert len(_arith.row_order(64, 64, True, True)) == 130
    assert pkg.ARITH_OPS == {"+": 0, "-": 1}
    for bad in ((0, 5), (5, 0), (65, 1), (1, 65)):
        with pytest.raises(pkg.WahError):
            pkg.bsi_arith_row_order(*bad)


def test_semantics_of_the_edges():
    """Unsigned operands; max(ka, kb) + 1 slices lose no carry; the top slice of a difference is set exactly where A < B; a smaller
    width truncates, a larger one zero-extends a sum and sign-extends a difference; arithmetic is right at 64 bits."""
    top = (1 << 64) - 1
    va = np.array([0, 5, 5, top, 1 << 63, 3, 0, 255] + [0] * 24, dtype=np.uint64)
    vb = np.array([0, 4, 6, 1, (1 << 63) - 1, 3, 1, 1] + [0] * 24, dtype=np.uint64)
    ints = [(int(a), int(b)) for a, b in zip(va, vb)]
    for n_out in (1, 8, 63, 64):
        assert [int(v) for v in _arith.expected_values(va, vb, "+", n_out)] == [(a + b) % (1 << n_out) for a, b in ints]
        assert [int(v) for v in _arith.expected_values(va, vb, "-", n_out)] == [(a - b) % (1 << n_out) for a, b in ints]
    small_a, small_b = va & np.uint64(0xFF), vb & np.uint64(0x0F)
    sa, sb = _bsi.build_slices(small_a, 8), _bsi.build_slices(small_b, 4)
    full = _arith.sweep(sa, 8, sb, 4, "+", 9)
    values, _ = _bsi.values_of_slices(full, 9)
    assert np.array_equal(values, small_a + small_b)  # no carry lost
    diff = _arith.sweep(sa, 8, sb, 4, "-", 9)
    assert np.array_equal(_bsi.unpack_bits(diff[0]), small_a < small_b)  # the borrow is the sign
    wide = _arith.sweep(sa, 8, sb, 4, "-", 20)
    for row in wide[:12]:
        assert np.array_equal(row, diff[0])  # sign extension
    wide_sum = _arith.sweep(sa, 8, sb, 4, "+", 20)
    assert not wide_sum[:11].any() and np.array_equal(wide_sum[11:], full)  # zero extension
    assert np.array_equal(_arith.sweep(sa, 8, sb, 4, "+", 5), full[4:])  # truncation keeps the low slices
    assert np.array_equal(_arith.sweep(sa, 8, sb, 4, "-", 5), diff[4:])
    s64a, s64b = _bsi.build_slices(va, 64), _bsi.build_slices(vb, 64)
    for op in _arith.OPS:
        assert np.array_equal(_arith.sweep(s64a, 64, s64b, 64, op, 64), _arith.expected_matrix(va, vb, op, 64)), op
