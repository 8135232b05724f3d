"""CPU tests of the order-statistics helpers (tests/_kth.py): the numpy restatement of the digit-wise radix select over the slices
equals the model that answers from the VALUES, for every digit width from 1 to 4, on the widths, values, filters and queries the GPU
tests use; and the cases are not vacuous -- every kind of query, every bucket of a full digit and both outcomes of `found`
actually occur among them."""
import numpy as np
import pytest

from tests import _bsi, _kth

WIDTHS = (1, 3, 4, 5, 8, 9, 20, 63, 64)
ROWS = 32 * 61


@pytest.mark.parametrize("n_bits", WIDTHS)
def test_radix_select_equals_the_value_model(n_bits):
    rng = np.random.default_rng(100 + n_bits)
    seen = {d: set() for d in (1, 2, 3, 4)}
    outcomes, kinds = set(), set()
    masks = _kth.mask_sets(rng, ROWS)
    for name, values in _kth.value_sets(rng, ROWS, n_bits, ROWS // 2).items():
        slices = _bsi.build_slices(values, n_bits)
        for mask_name in ("none", "dense", "one row", "zeros") if name == "uniform" else ("none", "sparse"):
            selected = None if mask_name == "none" else masks[mask_name]
            filters = [] if selected is None else [_bsi.pack_bits(selected)]
            total = ROWS if selected is None else int(selected.sum())
            fast = _kth.Model(values, selected)
            for what, kind, a, b in _kth.query_cases(total, spread=True):
                want = _kth.model(values, selected, kind, a, b)
                assert fast(kind, a, b) == want, (name, mask_name, what)
                outcomes.add(want[0])
                kinds.add(kind)
                for digit in (1, 2, 3, 4):
                    got = _kth.radix_select(slices, n_bits, filters, kind, a, b, digit, seen[digit])
                    assert got == want, (name, mask_name, what, digit, got, want)
    assert outcomes == {0, 1} and {_kth.ASCENDING, _kth.DESCENDING, _kth.QUANTILE, 3} <= kinds
    if n_bits >= 8:  # every bucket position of a full digit was picked at least once, for every width
        for digit in (1, 2, 3, 4):
            assert {bucket for width, bucket in seen[digit] if width == digit} == set(range(1 << digit)), (digit, sorted(seen[digit]))


def test_two_filters_are_anded():
    rng = np.random.default_rng(5)
    values = _bsi.uniform_values(rng, ROWS, 12)
    f1, f2 = rng.random(ROWS) < 0.5, rng.random(ROWS) < 0.5
    slices = _bsi.build_slices(values, 12)
    for what, kind, a, b in _kth.query_cases(int((f1 & f2).sum())):
        want = _kth.model(values, f1 & f2, kind, a, b)
        assert _kth.radix_select(slices, 12, [_bsi.pack_bits(f1), _bsi.pack_bits(f2)], kind, a, b, 4) == want, what
    assert _kth.model(values, f1 & f2, _kth.QUANTILE, 1, 2) != _kth.model(values, f1, _kth.QUANTILE, 1, 2)


def test_model_semantics():
    values = np.array([5, 1, 5, 9, 5, 0, 7, 7], dtype=np.uint64)
    assert _kth.model(values, None, _kth.ASCENDING, 0, 1) == (1, 0, 8, 0, 1)
    assert _kth.model(values, None, _kth.ASCENDING, 3, 1) == (1, 5, 8, 2, 3)
    assert _kth.model(values, None, _kth.DESCENDING, 0, 1) == (1, 9, 8, 7, 1)
    assert _kth.model(values, None, _kth.DESCENDING, 2, 1) == (1, 7, 8, 5, 2)
    assert _kth.model(values, None, _kth.QUANTILE, 1, 2) == (1, 5, 8, 2, 3)  # floor(7 / 2) = 3: the lower median
    assert _kth.model(values, None, _kth.QUANTILE, _kth.U64_MAX, _kth.U64_MAX) == (1, 9, 8, 7, 1)
    assert _kth.model(values, None, _kth.ASCENDING, 8, 1) == (0, 0, 8, 0, 0)
    assert _kth.model(values, None, _kth.QUANTILE, 0, 0) == (0, 0, 8, 0, 0)
    assert _kth.model(values, None, _kth.QUANTILE, 3, 2) == (0, 0, 8, 0, 0)
    assert _kth.model(values, None, 7, 0, 1) == (0, 0, 8, 0, 0)
    assert _kth.model(values, np.zeros(8, bool), _kth.QUANTILE, 0, 1) == (0, 0, 0, 0, 0)
    one = np.zeros(8, bool)
    one[3] = True
    assert _kth.model(values, one, _kth.QUANTILE, 1, 2) == (1, 9, 1, 0, 1)
