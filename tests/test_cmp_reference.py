"""CPU tests of the column-to-column comparison helpers (tests/_cmp.py): the eq / gt / hold sweep over the slice matrices equals
the model that answers from the VALUES, for all six operators and all four existence combinations; the package's statement of the
table order equals the tests' own; and the value pairs the GPU tests use pass the vacuity guard."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _cmp

SIZES = (31, 992 * 2 + 5)


@pytest.mark.parametrize("n_words", SIZES)
@pytest.mark.parametrize("ka,kb", _cmp.WIDTHS)
def test_sweep_equals_the_value_model(n_words, ka, kb):
    va, vb, xa, xb = _cmp.case(n_words, ka, kb, True, True)
    for have_a, have_b in _cmp.EXISTENCE:
        ea, eb = (xa if have_a else None), (xb if have_b else None)
        slices_a, slices_b = _bsi.build_slices(va, ka, ea), _bsi.build_slices(vb, kb, eb)
        for op in _cmp.OPS:
            want = _cmp.expected_compare(va, vb, op, ea, eb)
            assert np.array_equal(_cmp.sweep(slices_a, ka, slices_b, kb, op, have_a, have_b), want), (op, have_a, have_b)


@pytest.mark.parametrize("n_words", SIZES)
@pytest.mark.parametrize("ka,kb", _cmp.WIDTHS)
def test_value_pairs_can_fail(n_words, ka, kb):
    for have_a, have_b in _cmp.EXISTENCE:
        va, vb, xa, xb = _cmp.case(n_words, ka, kb, have_a, have_b)
        assert va.size == vb.size == 32 * n_words and (xa is not None) == have_a and (xb is not None) == have_b
        _cmp.assert_compare_matters(va, vb, ka, kb, xa, xb, (n_words, ka, kb, have_a, have_b))


def test_row_order_is_the_packages():
    pkg = importlib.import_module("gpu-wah_amd")
    for ka in (1, 2, 13, 20, 40, 41, 63, 64):
        for kb in (1, 2, 13, 20, 40, 41, 63, 64):
            for have_a, have_b in _cmp.EXISTENCE:
                order = _cmp.row_order(ka, kb, have_a, have_b)
                assert pkg.bsi_compare_row_order(ka, kb, have_a, have_b) == order, (ka, kb, have_a, have_b)
                assert len(order) == ka + kb + have_a + have_b
                assert sorted(i for who, i in order if who == "a") == list(range(ka + have_a))
                assert sorted(i for who, i in order if who == "b") == list(range(kb + have_b))
    assert _cmp.row_order(3, 2, True, True) == [("a", 0), ("a", 1), ("b", 0), ("a", 2), ("b", 1), ("a", 3), ("b", 2)]
    assert _cmp.row_order(1, 3, False, True) == [("b", 0), ("b", 1), ("a", 0), ("b", 2), ("b", 3)]
    # the held A slice in table row 63 and its B slice in row 64, the first of the second chunk of 64 rows
    for ka, kb in ((41, 40), (40, 41), (1, 64)):
        order = _cmp.row_order(ka, kb, False, False)
        assert order[63][0] == "a" and order[64][0] == "b" and ka - order[63][1] == kb - order[64][1], (ka, kb)
    assert len(_cmp.row_order(64, 64, True, True)) == 130
    for bad in ((0, 5), (5, 0), (65, 1), (1, 65)):
        with pytest.raises(pkg.WahError):
            pkg.bsi_compare_row_order(*bad)


def test_semantics_of_the_edges():
    """Unsigned values; a narrower attribute counts as zero above its width; without existence equal rows match ==, <= and >=."""
    va = np.array([0, 5, 5, (1 << 64) - 1, 1 << 63, 3] + [0] * 26, dtype=np.uint64)
    vb = np.array([0, 4, 6, 1, (1 << 63) - 1, 3] + [0] * 26, dtype=np.uint64)
    assert list(_bsi.unpack_bits(_cmp.expected_compare(va, vb, ">"))[:6]) == [False, True, False, True, True, False]
    sa, sb = _bsi.build_slices(va, 64), _bsi.build_slices(vb, 63)
    for op in _cmp.OPS:
        assert np.array_equal(_cmp.sweep(sa, 64, sb, 63, op), _cmp.expected_compare(va, vb, op)), op
    for op, matches in (("<", False), ("<=", True), (">", False), (">=", True), ("==", True), ("!=", False)):
        tail = _bsi.unpack_bits(_cmp.sweep(sa, 64, sb, 63, op))[6:]  # rows of value 0 in both
        assert tail.all() if matches else not tail.any(), op
