"""CPU proof of the fetch call's reference (tests/_fetch.py): ref_fetch, which looks a row up in the STREAM as group p // 31,
bit p % 31, agrees with plain indexing of the decoded bits (word p // 32, bit p % 32), with values[rows] for a bit-sliced
attribute and with keys[rows] for one-hot columns; and items_of cuts a list into what the interface promises."""
import numpy as np
import pytest

from tests import _bsi, _fetch, _select

SEG = _fetch.SEG_WORDS


def _rows(rng, n_words, count):
    return np.sort(rng.integers(0, 32 * n_words, count))


@pytest.mark.parametrize("n", [1, 31, SEG, SEG + 1, 2 * SEG + 17])
def test_bits_at_is_plain_indexing_of_the_decoded_bits(oracle, n):
    rng = np.random.default_rng(n)
    edges = [p for p in (0, 30, 31, 32, 61, 62, 31743, 31744, 32 * n - 1) if p < 32 * n]
    for name, words in _select.bitmaps(oracle, n).items():
        stream = oracle.compress(words)
        rows = np.sort(np.concatenate([_rows(rng, n, 300), edges]).astype(np.int64))
        want = _bsi.unpack_bits(words)[rows]
        assert np.array_equal(_fetch.bits_at(stream, rows).astype(bool), want), name
        assert _fetch.ref_fetch([stream], rows, _fetch.BITS) == want.astype(int).tolist(), name
        assert _fetch.ref_fetch([stream], rows, _fetch.FIRST) == [0 if b else _fetch.U64_MAX for b in want], name


@pytest.mark.parametrize("n_bits", [1, 4, 20, 63, 64])
def test_bits_mode_is_values_of_rows(oracle, n_bits):
    n = SEG + 40
    rng = np.random.default_rng(n_bits)
    for kind in ("uniform", "low", "clustered"):
        values = _bsi.make_values(kind, rng, 32 * n, n_bits)
        streams = [oracle.compress(row) for row in _bsi.build_slices(values, n_bits)]
        rows = _rows(rng, n, 200)
        assert _fetch.ref_fetch(streams, rows, _fetch.BITS) == [int(v) for v in values[rows]], kind
    if n_bits == 64:
        assert max(_fetch.ref_fetch(streams, rows, _fetch.BITS)) >> 63 == 1  # bit 63 is reached


def test_an_existence_row_in_front_is_the_top_bit(oracle):
    n, n_bits = SEG, 12
    rng = np.random.default_rng(3)
    values = _bsi.uniform_values(rng, 32 * n, n_bits)
    exists = rng.random(32 * n) < 0.8
    slices = _bsi.build_slices(values, n_bits, exists, zero_missing=True)
    streams = [oracle.compress(slices[n_bits])] + [oracle.compress(row) for row in slices[:n_bits]]
    rows = _rows(rng, n, 300)
    got = _fetch.ref_fetch(streams, rows, _fetch.BITS)
    assert [g >> n_bits for g in got] == exists[rows].astype(int).tolist()
    assert [g & ((1 << n_bits) - 1) for g in got] == [int(v) if e else 0 for v, e in zip(values[rows], exists[rows])]


@pytest.mark.parametrize("n_values", [1, 63, 64, 65, 129])
def test_first_mode_is_keys_of_rows(oracle, n_values):
    n = SEG
    rng = np.random.default_rng(n_values)
    keys = rng.integers(-1, n_values, 32 * n)  # -1: a row no column has
    streams = [oracle.compress(b) for b in _fetch.one_hot(keys, n_values, n)]
    rows = _rows(rng, n, 400)
    want = [int(k) if k >= 0 else _fetch.U64_MAX for k in keys[rows]]
    assert _fetch.ref_fetch(streams, rows, _fetch.FIRST) == want
    assert _fetch.U64_MAX in want or n_values == 1
    # two set columns: the lower one wins
    both = streams + [streams[0]]
    assert _fetch.ref_fetch(list(reversed(both)), rows, _fetch.FIRST)[:5] == [0 if k == 0 else (n_values - k if k > 0 else _fetch.U64_MAX) for k in keys[rows][:5]]


def _lists(rng, n_words):
    bits = 32 * n_words
    yield "one row", np.array([bits // 3])
    for count in (1, 63, 64, 65, 128, 129, 1000):
        yield f"{count} rows in one segment", np.sort(rng.integers(0, min(bits, _fetch.SEG_BITS), count))
    yield "every row of a segment", np.arange(min(bits, _fetch.SEG_BITS))
    if bits > 2 * _fetch.SEG_BITS:
        for at in (63, 64, 65):
            yield f"a segment change at index {at}", np.concatenate([np.arange(at), _fetch.SEG_BITS + np.arange(70)])
        yield "a change at every row", np.arange(bits // _fetch.SEG_BITS) * _fetch.SEG_BITS + 5
        yield "duplicates", np.sort(np.concatenate([np.full(70, 17), np.full(3, _fetch.SEG_BITS + 1)]))
    yield "uniform", np.sort(rng.integers(0, bits, 5000))
    yield "empty", np.zeros(0, np.int64)


@pytest.mark.parametrize("n", [1, SEG, 3 * SEG + 5, 200 * SEG])
def test_items_partition_the_list(n):
    rng = np.random.default_rng(n)
    for name, rows in _lists(rng, n):
        items = _fetch.items_of(rows, n)
        assert len(items) <= _fetch.item_bound(rows.size, n), name
        at = 0
        for head, count in items:
            assert head == at and 1 <= count <= _fetch.ITEM_ROWS, name
            seg = rows[head: head + count] // _fetch.SEG_BITS
            assert np.all(seg == seg[0]), name
            assert head // 64 == (head + count - 1) // 64, name  # an item never crosses a multiple of 64 of the list
            at += count
        assert at == rows.size, name
        # consecutive items are not mergeable: another segment, or a multiple of 64
        for (h0, _), (h1, _) in zip(items, items[1:]):
            assert h1 % 64 == 0 or rows[h1] // _fetch.SEG_BITS != rows[h1 - 1] // _fetch.SEG_BITS, name


def test_the_item_bound_is_reached():
    """200 rows in 200 segments: every row is a head; with 64 rows a segment only the multiples of 64 are."""
    n = 200 * SEG
    assert len(_fetch.items_of(np.arange(200) * _fetch.SEG_BITS, n)) == 200 <= _fetch.item_bound(200, n) == 4 + 200
    assert len(_fetch.items_of(np.arange(640), n)) == 10


def test_grid_constant_is_found():
    g = _fetch.grid_waves()
    assert g >= 4 and g % 4 == 0
