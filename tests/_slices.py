"""Inputs and expected results for wah_bsi_build_device (include/wah.h): the bit-sliced index of a value column.  No GPU, no
library: tests/test_slices_reference.py proves the cases can fail, tests/test_gpu_bsi_build.py holds the kernel against them.

The kernel hands a wavefront blocks of 2048 rows (64 words of every slice), loads them in steps of 64 rows and keeps the two
32-bit halves of a value apart, so the switch points are: columns of 992 words (15.5 blocks: the last one half full) and of three
times that; row counts around a step, a block and a segment of 31744 rows, an empty and a full column; widths around the halves'
boundary and the widest ones; without and with existence bytes (64 bits and existence are 65 slices)."""
import numpy as np

from tests import _bsi

SEG = 992
N_WORDS = (SEG, SEG * 3)
N_BITS = (1, 2, 31, 32, 33, 63, 64)
GUARD_FROM = 64  # rows from which the vacuity guard holds


def row_counts(n_words):
    top = 32 * n_words
    wanted = (0, 1, 63, 64, 65, 2047, 2048, 2049, 31743, 31744, top - 1, top)
    return sorted(set(min(r, top) for r in wanted))


def case(n_words, n_rows, n_bits, with_exists):
    """(values uint64 [n_rows], exists bool [n_rows] or None): uniform over [0, 2^n_bits), existence Bernoulli 0.7; deterministic."""
    rng = np.random.default_rng([n_words, n_rows, n_bits, int(with_exists)])
    values = _bsi.uniform_values(rng, n_rows, n_bits)
    exists = rng.random(n_rows) < 0.7 if with_exists else None
    return values, exists


def padded(values, exists, n_words):
    """The column as the index sees it: 32 * n_words rows, those behind the caller's hold 0 and do not exist."""
    v = np.zeros(32 * n_words, np.uint64)
    v[: values.size] = values
    if exists is None:
        return v, None
    e = np.zeros(32 * n_words, bool)
    e[: exists.size] = exists
    return v, e


def expected_matrix(values, exists, n_bits, n_words):
    v, e = padded(values, exists, n_words)
    return _bsi.build_slices(v, n_bits, e, zero_missing=True)


def expected_stream(oracle, matrix):
    return np.ascontiguousarray(oracle.compress(np.ascontiguousarray(matrix.reshape(-1), dtype=np.uint32)), dtype=np.uint32)


def assert_case_matters(values, exists, n_bits, n_words, what):
    """The vacuity guard, numpy alone (n_rows >= GUARD_FROM): every expected slice row has a set and a clear bit among the first
    n_rows rows, no two slice rows are equal, and with existence zeroing the missing rows changes at least one slice."""
    n_rows = values.size
    assert n_rows >= GUARD_FROM, what
    matrix = expected_matrix(values, exists, n_bits, n_words)
    for i, row in enumerate(matrix):
        bits = _bsi.unpack_bits(row)[:n_rows]
        assert bits.any() and not bits.all(), (what, "slice", i, "is constant")
    assert np.unique(matrix, axis=0).shape[0] == matrix.shape[0], (what, "two slices are equal")
    if exists is not None:
        v, e = padded(values, exists, n_words)
        assert not np.array_equal(_bsi.build_slices(v, n_bits, e, zero_missing=False), matrix), (what, "zeroing the missing rows changes nothing")
    return matrix


def all_cases():
    """Every (n_words, n_rows, n_bits, with_exists) of the switch points."""
    return [(n, r, b, e) for n in N_WORDS for b in N_BITS for e in (False, True) for r in row_counts(n)]
