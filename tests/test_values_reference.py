"""CPU proof of the range call's reference and rules (tests/_values.py): ref_values -- tests/_fetch.py's ref_fetch over arange, which
reads the STREAMS by group and bit -- agrees with plain indexing of the bitmaps the oracle decodes (word p // 32, bit p % 32), with
values[first: first + n] for a bit-sliced attribute and with the keys of one-hot columns; values_of is the same numbers; the
model that restates the kernel's rules gives them too; its items tile d_out[0 .. n) exactly once for every shape the GPU tests
use; and each of the four wrong models, one error each, changes an answer on the cases named for it."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _fetch, _values as vl

SEG, SEG_BITS = vl.SEG_WORDS, vl.SEG_BITS
BITS, FIRST = vl.BITS, vl.FIRST


def _streams(oracle, bitmaps):
    return [oracle.compress(np.ascontiguousarray(b, dtype=np.uint32)) for b in bitmaps]


def _plain(oracle, streams, n_words, first, n, mode):
    """The answer by plain indexing of the decoded bitmaps."""
    bits = np.stack([_bsi.unpack_bits(oracle.decompress(st)[:n_words])[first: first + n] for st in streams])
    k = len(streams)
    if mode == BITS:
        return [sum(int(bits[j, i]) << (k - 1 - j) for j in range(k)) for i in range(n)]
    return [int(np.argmax(bits[:, i])) if bits[:, i].any() else vl.U64_MAX for i in range(n)]


def test_the_rules_read_the_kernel_and_the_library():
    assert vl.grid_items() >= 1
    pkg = importlib.import_module("gpu-wah_amd")
    assert "wah_values_indexed_device" in pkg.ABI_SYMBOLS and callable(pkg.values_device)
    assert callable(pkg.columns.values_of_column) and callable(pkg.columns.keys_of_column) and callable(pkg.columns.reorder_rows)
    assert callable(pkg.columns._values_of_column_torch)


@pytest.mark.parametrize("n_words", [1, 31, SEG + 1, 3 * SEG - 5])
def test_the_reference_is_plain_indexing_of_the_decoded_bitmaps(oracle, n_words):
    rng = np.random.default_rng(n_words)
    streams = _streams(oracle, [oracle.gen_uniform(n_words, 10 + j, p) for j, p in enumerate((0.5, 0.02, 0.9, 0.5, 0.0))])
    n_bits = 32 * n_words
    wins = [(0, min(n_bits, 200)), (n_bits - 1, 1), (0, 0)]
    if n_bits > SEG_BITS + 100:
        wins += [(SEG_BITS - 40, 80), (SEG_BITS, 33), (n_bits - 70, 70)]
    wins.append((int(rng.integers(0, n_bits // 2)), min(n_bits // 2, 150)))
    for first, n in wins:
        for mode in (BITS, FIRST):
            want = _plain(oracle, streams, n_words, first, n, mode)
            assert vl.ref_values(streams, first, n, mode) == want, (first, n, mode)
            assert vl.values_of(streams, first, n, mode).tolist() == want, (first, n, mode)
            got, writes = vl.model(streams, first, n, mode)
            assert got.tolist() == want and np.all(writes == 1), (first, n, mode)


@pytest.mark.parametrize("n_bits", [1, 2, 31, 32, 33, 63])
@pytest.mark.parametrize("with_exists", [False, True])
def test_bits_are_the_values_with_the_existence_bit_on_top(oracle, n_bits, with_exists):
    n_words = SEG + 1
    rng = np.random.default_rng(n_bits)
    values = _bsi.uniform_values(rng, 32 * n_words, n_bits)
    exists = rng.random(32 * n_words) < 0.8 if with_exists else None
    slices = _bsi.build_slices(values, n_bits, exists, zero_missing=True)
    streams = _streams(oracle, ([slices[n_bits]] if with_exists else []) + list(slices[:n_bits]))
    first, n = SEG_BITS - 100, 132  # across the seam, into the ragged last segment of two groups
    want = np.where(exists, values, 0)[first: first + n].astype(np.uint64) if with_exists else values[first: first + n].astype(np.uint64)
    if with_exists:
        want = want | (exists[first: first + n].astype(np.uint64) << np.uint64(n_bits))
    assert np.array_equal(vl.values_of(streams, first, n, BITS), want)
    assert vl.ref_values(streams, first, n, BITS) == want.tolist()
    got, writes = vl.model(streams, first, n, BITS)
    assert np.array_equal(got, want) and np.all(writes == 1)


@pytest.mark.parametrize("n_values", vl.FIRST_COLUMNS)
def test_first_is_the_key(oracle, n_values):
    n_words = 40
    rng = np.random.default_rng(n_values)
    keys = rng.integers(-1, n_values, 32 * n_words)
    streams = _streams(oracle, _fetch.one_hot(keys, n_values, n_words))
    want = [int(k) if k >= 0 else vl.U64_MAX for k in keys[100:400]]
    assert vl.ref_values(streams, 100, 300, FIRST) == want and vl.values_of(streams, 100, 300, FIRST).tolist() == want
    assert vl.model(streams, 100, 300, FIRST)[0].tolist() == want
    assert vl.values_of(streams + streams, 100, 300, FIRST).tolist() == want  # two columns set: the lower one


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
def test_halves_are_cut_from_the_least_significant_end():
    assert [vl.halves(BITS, k) for k in (1, 32, 33, 64)] == [1, 1, 2, 2] and vl.halves(FIRST, 4096) == 1
    assert list(vl.half_rows(BITS, 5, 0)) == [0, 1, 2, 3, 4] and list(vl.half_rows(BITS, 32, 0)) == list(range(32))
    assert list(vl.half_rows(BITS, 33, 0)) == list(range(1, 33)) and list(vl.half_rows(BITS, 33, 1)) == [0]
    assert list(vl.half_rows(BITS, 64, 0)) == list(range(32, 64)) and list(vl.half_rows(BITS, 64, 1)) == list(range(32))
    for k in vl.BITS_WIDTHS:
        rows = [j for h in range(vl.halves(BITS, k)) for j in vl.half_rows(BITS, k, h)]
        assert sorted(rows) == list(range(k))  # every table row is walked, by exactly one half
        for h in range(vl.halves(BITS, k)):
            assert all((k - 1 - j) // 32 == h for j in vl.half_rows(BITS, k, h))
    assert list(vl.half_rows(FIRST, 129, 0)) == list(range(129))


def test_segments_and_rows_of_a_window():
    assert list(vl.window_segments(0, 0)) == [] and list(vl.window_segments(SEG_BITS, 0)) == []
    assert list(vl.window_segments(0, SEG_BITS)) == [0] and list(vl.window_segments(0, SEG_BITS + 1)) == [0, 1]
    assert list(vl.window_segments(SEG_BITS - 1, 1)) == [0] and list(vl.window_segments(SEG_BITS - 1, 2)) == [0, 1]
    assert list(vl.window_segments(SEG_BITS, 1)) == [1] and list(vl.window_segments(SEG_BITS + 100, 5000)) == [1]
    assert list(vl.window_segments(5, 2 * SEG_BITS)) == [0, 1, 2]
    assert vl.item_rows(1, SEG_BITS - 5, 10) == range(SEG_BITS, SEG_BITS + 5) and vl.item_rows(0, SEG_BITS - 5, 10) == range(SEG_BITS - 5, SEG_BITS)
    assert vl.item_bytes(BITS, 32, 0, 0, 7, 2) == [(0, 8), (8, 8)]
    assert vl.item_bytes(BITS, 33, 0, 0, 7, 2) == [(0, 4), (8, 4)] and vl.item_bytes(BITS, 33, 0, 1, 7, 2) == [(4, 4), (12, 4)]
    assert vl.item_bytes(FIRST, 4096, 1, 0, SEG_BITS - 1, 3) == [(8, 8), (16, 8)]
    assert vl.items(BITS, 33, SEG_BITS - 1, 2) == [(0, 0), (0, 1), (1, 0), (1, 1)] and vl.items(FIRST, 33, SEG_BITS - 1, 2) == [(0, 0), (1, 0)]


@pytest.mark.parametrize("n_words", vl.SIZES)
def test_the_items_tile_the_output_exactly_once(n_words):
    """Every shape of the GPU tests: every window of every size, one item and two items a segment."""
    wins = vl.windows(n_words)
    assert (0, 32 * n_words) in wins and (0, 0) in wins and (32 * n_words - 1, 1) in wins
    for first, n in wins:
        for mode, k in ((BITS, 1), (BITS, 32), (BITS, 33), (BITS, 64), (FIRST, 129)):
            writes = vl.writes_of(mode, k, first, n)
            assert writes.size == 8 * n and np.all(writes == 1), (first, n, mode, k)
            assert len(vl.items(mode, k, first, n)) == len(vl.window_segments(first, n)) * vl.halves(mode, k)
    small = [(a, n) for a, n in wins if n <= 40][:60]
    for first, n in small:  # the vectorised count is item_bytes'
        for mode, k in ((BITS, 32), (BITS, 33)):
            writes = np.zeros(8 * n, np.uint8)
            for s, h in vl.items(mode, k, first, n):
                for at, width in vl.item_bytes(mode, k, s, h, first, n):
                    writes[at: at + width] += 1
            assert np.array_equal(writes, vl.writes_of(mode, k, first, n))


def test_the_shapes_are_what_they_are_for():
    from tests import _select

    assert [_select.segments_of(n) for n in vl.SIZES] == [1, 1, 1, 2, 2, 3]
    assert _select.groups_of(vl.SIZES[-1]) % 1024 not in (0, 1023) and _select.groups_of(SEG + 1) % 1024 == 2  # ragged: nvalid < 1024
    wins = vl.windows(3 * SEG - 5)
    for e in (31, 32, SEG_BITS):
        for d in (-1, 0, 1):
            assert any(a == e + d for a, _ in wins) and any(a + n == e + d and n for a, n in wins), (e, d)
    assert any(a > SEG_BITS and a + n < 2 * SEG_BITS for a, n in wins)
    assert {n for a, n in wins if a == 31} >= {0, 1, 30, 31, 32}


# ---- the wrong models ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attribute(oracle):
    """40 random slices of two segments and a bit (993 words)."""
    n_words = SEG + 1
    return n_words, _streams(oracle, [oracle.gen_uniform(n_words, 50 + j, 0.5) for j in range(40)])


def test_every_wrong_model_is_one_of_the_named():
    assert set(vl.WRONG) == {"half from the wrong end", "last segment dropped on a seam", "word 32 addressing", "first takes the last"}


def test_the_half_cut_from_the_wrong_end_changes_the_wide_widths_only(attribute):
    _, streams = attribute
    for k in (33, 40):
        right = vl.model(streams[:k], 10, 60, BITS)[0]
        assert np.array_equal(right, vl.values_of(streams[:k], 10, 60, BITS))
        assert not np.array_equal(vl.model(streams[:k], 10, 60, BITS, "half from the wrong end")[0], right), k
    for k in (1, 31, 32):  # one item a segment: there is no cut
        assert np.array_equal(vl.model(streams[:k], 10, 60, BITS, "half from the wrong end")[0], vl.model(streams[:k], 10, 60, BITS)[0])


def test_the_dropped_last_segment_shows_when_the_last_row_is_a_segments_first(attribute):
    _, streams = attribute
    wrong = "last segment dropped on a seam"
    for first, n in ((SEG_BITS - 20, 21), (SEG_BITS - 1, 2), (0, SEG_BITS + 1)):
        assert (first + n - 1) % SEG_BITS == 0
        writes = vl.writes_of(BITS, 3, first, n, wrong)
        assert not writes[-8:].any() and np.all(writes[:-8] == 1), (first, n)  # the last element keeps the poison
    assert any((a + n - 1) % SEG_BITS == 0 and a < SEG_BITS and n > 1 for a, n in vl.windows(SEG + 1))  # (the GPU tests have such windows)
    got = vl.model(streams[:3], SEG_BITS - 20, 21, BITS, wrong)[0]
    assert int(got[-1]) == int.from_bytes(bytes([vl.POISON] * 8), "little")
    for first, n in ((SEG_BITS - 20, 20), (SEG_BITS - 20, 22), (SEG_BITS + 1, 5)):  # one before, one behind: nothing to see
        assert np.all(vl.writes_of(BITS, 3, first, n, wrong) == 1)


def test_word_32_addressing_changes_rows_behind_the_first_group(attribute):
    _, streams = attribute
    for mode in (BITS, FIRST):
        right, wrong = vl.model(streams[:4], 0, 200, mode)[0], vl.model(streams[:4], 0, 200, mode, "word 32 addressing")[0]
        assert np.array_equal(right[:31], wrong[:31]) and not np.array_equal(right[31:], wrong[31:])
        assert not np.array_equal(vl.model(streams[:4], SEG_BITS - 10, 30, mode)[0], vl.model(streams[:4], SEG_BITS - 10, 30, mode, "word 32 addressing")[0])


def test_first_taking_the_last_column_changes_rows_that_two_columns_set(oracle, attribute):
    _, streams = attribute
    right, wrong = vl.model(streams[:5], 40, 100, FIRST)[0], vl.model(streams[:5], 40, 100, FIRST, "first takes the last")[0]
    assert not np.array_equal(right, wrong)
    keys = np.random.default_rng(1).integers(0, 7, 32 * 10)  # one column a row: nothing to choose between
    one_hot = _streams(oracle, _fetch.one_hot(keys, 7, 10))
    assert np.array_equal(vl.model(one_hot, 0, 320, FIRST)[0], vl.model(one_hot, 0, 320, FIRST, "first takes the last")[0])
    assert np.array_equal(vl.model(one_hot, 0, 320, FIRST)[0], keys.astype(np.uint64))
