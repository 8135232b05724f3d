"""CPU tests of the inputs of tests/test_gpu_bsi_build.py (tests/_slices.py): every generated case can fail -- no expected slice is
constant over the caller's rows, no two are equal, and the existence bytes change what is stored --, and the expected matrix is
the slice matrix of the column: _bsi.values_of_slices reads the (zeroed) values and the existence row back from it."""
import numpy as np
import pytest

from tests import _bsi, _slices


@pytest.mark.parametrize("n_words", _slices.N_WORDS)
@pytest.mark.parametrize("n_bits", _slices.N_BITS)
@pytest.mark.parametrize("with_exists", (False, True), ids=("plain", "exists"))
def test_cases_can_fail_and_invert(n_words, n_bits, with_exists):
    counts = _slices.row_counts(n_words)
    assert counts[0] == 0 and counts[-1] == 32 * n_words and 2049 in counts and 31744 in counts
    for n_rows in counts:
        what = (n_words, n_rows, n_bits, with_exists)
        values, exists = _slices.case(n_words, n_rows, n_bits, with_exists)
        assert values.size == n_rows and values.dtype == np.uint64
        if n_bits < 64:
            assert not (values >> np.uint64(n_bits)).any(), what
        if n_rows >= _slices.GUARD_FROM:
            matrix = _slices.assert_case_matters(values, exists, n_bits, n_words, what)
        else:
            matrix = _slices.expected_matrix(values, exists, n_bits, n_words)
        assert matrix.shape == (n_bits + with_exists, n_words) and matrix.dtype == np.uint32
        back, have = _bsi.values_of_slices(matrix, n_bits)
        v, e = _slices.padded(values, exists, n_words)
        assert np.array_equal(back, v if e is None else np.where(e, v, np.uint64(0))), what
        assert (have is None) == (e is None) and (e is None or np.array_equal(have, e)), what
        assert not back[n_rows:].any() and (have is None or not have[n_rows:].any()), what


def test_all_cases_is_the_whole_product():
    cases = _slices.all_cases()
    assert len(cases) == len(set(cases)) == sum(len(_slices.row_counts(n)) for n in _slices.N_WORDS) * len(_slices.N_BITS) * 2
    assert (_slices.SEG, 0, 64, True) in cases and (_slices.SEG * 3, 32 * _slices.SEG * 3, 1, False) in cases
