"""CPU tests of the bit-sliced index helpers (tests/_bsi.py): both numpy restatements of the slice sweep -- the four-bitmap
O'Neil & Quass step as include/wah.h states it, and the three-bitmap state the kernel keeps -- equal the model that answers from
the VALUES, over every kind of value and every bound edge case the GPU tests use; the slice builder round-trips; and the headline
choices of the GPU tests pass the vacuity guard."""
import numpy as np
import pytest

from tests import _bsi

WIDTHS = (1, 2, 3, 8, 20, 63, 64)


@pytest.mark.parametrize("n_bits", WIDTHS)
@pytest.mark.parametrize("kind", ["uniform", "low", "high", "clustered"])
def test_sweeps_equal_the_value_model(n_bits, kind):
    rng = np.random.default_rng(1000 * n_bits + len(kind))
    rows = 32 * 331
    values = _bsi.make_values(kind, rng, rows, n_bits)
    exists = rng.random(rows) < 0.9
    cases = _bsi.bound_cases(values, n_bits)
    names = {name for name, _, _ in cases}
    assert {"eq present", "lo 0", "hi max", "lo > hi", "lo = hi + 1"} <= names
    assert ("hi = 2^k" in names and "lo = 2^k" in names) if n_bits < 64 else "eq 2^64 - 1" in names
    for have in (None, exists):
        slices = _bsi.build_slices(values, n_bits, have)
        for name, lo, hi in cases:
            want = _bsi.expected_range(values, lo, hi, have)
            assert np.array_equal(_bsi.sweep(slices, n_bits, lo, hi, have is not None), want), (name, lo, hi)
            assert np.array_equal(_bsi.sweep_three(slices, n_bits, lo, hi, have is not None), want), (name, lo, hi)


@pytest.mark.parametrize("n_bits", (1, 2, 5))
def test_sweeps_over_every_pair_of_bounds(n_bits):
    """Narrow widths exhaustively: every (lo, hi) up to two beyond the width, every value present."""
    rng = np.random.default_rng(n_bits)
    values = rng.integers(0, 1 << n_bits, 32 * 8).astype(np.uint64)
    slices = _bsi.build_slices(values, n_bits)
    for lo in range((1 << n_bits) + 2):
        for hi in range((1 << n_bits) + 2):
            want = _bsi.expected_range(values, lo, hi)
            assert np.array_equal(_bsi.sweep(slices, n_bits, lo, hi), want), (lo, hi)
            assert np.array_equal(_bsi.sweep_three(slices, n_bits, lo, hi), want), (lo, hi)


def test_bound_edge_semantics():
    """lo > hi: nothing; hi beyond the width: the maximum; lo beyond the width: nothing; rows of value 0 match when lo == 0."""
    values = np.array([0, 1, 5, 7] * 8, dtype=np.uint64)
    slices = _bsi.build_slices(values, 3)
    assert not _bsi.sweep(slices, 3, 5, 4).any() and not _bsi.sweep_three(slices, 3, 5, 4).any()
    for f in (_bsi.sweep, _bsi.sweep_three):
        assert np.array_equal(f(slices, 3, 5, 8), _bsi.pack_bits(values >= 5))
        assert np.array_equal(f(slices, 3, 5, _bsi.U64_MAX), _bsi.pack_bits(values >= 5))
        assert not f(slices, 3, 8, _bsi.U64_MAX).any()
        assert np.array_equal(f(slices, 3, 0, 0), _bsi.pack_bits(values == 0))


@pytest.mark.parametrize("n_bits", WIDTHS)
def test_slice_builder_round_trips(n_bits):
    rng = np.random.default_rng(n_bits)
    rows = 32 * 77
    values = _bsi.uniform_values(rng, rows, n_bits)
    exists = rng.random(rows) < 0.5
    slices = _bsi.build_slices(values, n_bits)
    assert slices.shape == (n_bits, 77) and slices.dtype == np.uint32
    back, have = _bsi.values_of_slices(slices, n_bits)
    assert have is None and np.array_equal(back, values)
    # row 0 is the most significant bit, position 32 * word + bit
    assert np.array_equal(_bsi.unpack_bits(slices[0]), (values >> np.uint64(n_bits - 1)).astype(bool))
    with_rows = _bsi.build_slices(values, n_bits, exists, zero_missing=True)
    back, have = _bsi.values_of_slices(with_rows, n_bits)
    assert np.array_equal(have, exists) and np.array_equal(back, np.where(exists, values, np.uint64(0)))
    kept = _bsi.build_slices(values, n_bits, exists)
    assert np.array_equal(kept[:n_bits], slices) and np.array_equal(kept[n_bits], _bsi.pack_bits(exists))


def test_pack_bits_layout():
    bits = np.zeros(64, bool)
    bits[[0, 31, 33]] = True
    assert list(_bsi.pack_bits(bits)) == [0x80000001, 0x00000002]
    assert np.array_equal(_bsi.unpack_bits(_bsi.pack_bits(bits)), bits)


@pytest.mark.parametrize("n_words", (31, 992, 992 * 2, 992 * 3 + 5))
@pytest.mark.parametrize("n_bits", (1, 2, 20, 63, 64))
def test_headline_choices_can_fail(n_words, n_bits):
    """The values and bounds the GPU tests use for their headline cases pass the vacuity guard, with and without existence."""
    for kind in ("uniform", "low", "high", "clustered"):
        for with_exists in (False, True):
            values, exists, lo, hi = _bsi.headline(n_words, n_bits, with_exists, kind)
            assert values.size == 32 * n_words and int(values.max()) < 1 << n_bits
            _bsi.assert_range_matters(values, n_bits, lo, hi, exists, (n_words, n_bits, with_exists, kind))
