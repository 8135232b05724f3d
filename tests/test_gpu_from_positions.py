"""GPU tests of wah_from_positions_device (include/wah.h) and its front ends: compressed bitmaps straight from sorted lists of
row numbers.  Everything is exact: the words, their count and every index entry against the reference of tests/_rows.py -- the
CPU oracle's compress() of every list's decoded bitmap (the builders and their routes are proven in
tests/test_rows_reference.py).  The largest bitmap is five segments.
Sizes beyond one grid, where a wavefront takes a second (list, segment) item or a check loop a second trip: tests/test_gpu_full_grid.py."""
import importlib

import numpy as np
import pytest

from tests import _rows, _select

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6
CASES = _rows.switch_cases()


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


def _dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _build(wah, lists, n, **kw):
    rows, ends = _rows.flatten(lists)
    return wah.from_positions_device(_dev64(rows), _dev64(ends), n, **kw)


def _same(wah, oracle, lists, n, what):
    """The call's stream, word count and index are the reference's."""
    want, want_index = _rows.reference(oracle, lists, n)
    got, index = _build(wah, lists, n)
    assert got.numel() == want.size, (what, got.numel(), want.size)
    assert np.array_equal(index.cpu().numpy(), want_index), what
    assert np.array_equal(_host(got), want), what
    return got, index


@pytest.mark.parametrize("n", (1, 30, 31, 992, 993, 2976, 2981))
def test_parity_ten_bitmaps_in_one_call(wah, oracle, n):
    lists = _rows.parity_lists(oracle, n)
    assert len(lists) == 10
    _, index = _same(wah, oracle, lists, n, n)
    assert index.numel() == 10 * _select.segments_of(n) + 1


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_switch_point_alone(wah, oracle, case):
    name, n, rows, words = case
    _, index = _same(wah, oracle, [rows], n, name)
    assert list(np.diff(index.cpu().numpy())) == words


def test_switch_points_as_lists_of_one_call(wah, oracle):
    for n, lists in _rows.switch_cases_by_length().items():
        _same(wah, oracle, lists, n, n)


def test_empty_lists(wah, oracle):
    import torch

    n = 2981
    full = [np.arange(7, 32 * n, 311, dtype=np.int64), np.array([0, 31743, 31744, 32 * n - 1], np.int64)]
    none = np.empty(0, np.int64)
    _same(wah, oracle, [none] + full, n, "first")
    _same(wah, oracle, [full[0], none, none, full[1]], n, "in the middle")
    _same(wah, oracle, full + [none], n, "last")
    # all lists empty and no rows at all: a null d_rows
    want, want_index = _rows.reference(oracle, [none] * 3, n)
    ends = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    got, index = wah.from_positions_device(torch.empty(0, dtype=torch.int64, device="cuda:0"), ends, n)
    assert np.array_equal(_host(got), want) and np.array_equal(index.cpu().numpy(), want_index)
    assert got.numel() == 3 * _select.segments_of(n)


def test_round_trip_through_count_and_positions(wah, oracle):
    n = 2981
    segments = _select.segments_of(n)
    lists = _rows.parity_lists(oracle, n)
    stream, index = _build(wah, lists, n)
    operands = [(stream, index[c * segments:]) for c in range(len(lists))]
    counts = wah.count_device(operands, n)
    assert counts.tolist() == [len(r) for r in lists]
    for c, rows in enumerate(lists):
        back, total = wah.positions_device(stream, index[c * segments:], n)
        assert total == len(rows) and np.array_equal(back.cpu().numpy(), rows), c


@pytest.mark.parametrize("n_lists,n", _rows.MANY_LISTS)
def test_many_lists(wah, oracle, n_lists, n):
    """Around the 4096 entries of one chunk of the index's prefix sum; list c holds the one row c mod 31744."""
    segments = _select.segments_of(n)
    lists = _rows.many_lists(n_lists)
    assert n_lists * segments + 1 in (4096, 4097, 4098, 4099)
    words = [oracle.compress(_select.bitmap_of(r, n)) for r in lists]
    got, index = _build(wah, lists, n)
    want = np.concatenate(words)
    want_index = np.concatenate([_select.index_of(w)[:-1] + at for w, at in zip(words, np.cumsum([0] + [w.size for w in words[:-1]]))] + [[want.size]])
    assert got.numel() == want.size == sum(_rows.one_row_words(int(r[0]), n) for r in lists)
    assert np.array_equal(index.cpu().numpy(), want_index)
    assert np.array_equal(_host(got), want)


def _one_hot(keys, n_values, n):
    m = np.zeros((n_values, n), np.uint32)
    for v in range(n_values):
        m[v] = _select.bitmap_of(np.flatnonzero(keys == v), n)
    return m


def _attribute(wah, seed, n_rows, n_values, unused):
    import torch

    rng = np.random.default_rng(seed)
    values = np.array([v for v in range(n_values) if v != unused])
    keys = values[np.arange(n_rows) % values.size]
    rng.shuffle(keys)
    built = wah.columns.index_from_keys(wah, torch.from_numpy(keys.astype(np.int64)).cuda(), n_values)
    return keys, built


def test_index_from_keys(wah, oracle):
    import torch

    n_rows, n_values = 3 * 31744 + 17, 7
    keys, (stream, seg_offsets, n) = _attribute(wah, 5, n_rows, n_values, unused=5)
    assert n == 4 * 992 and not np.any(keys == 5)
    matrix = _one_hot(keys, n_values, n)
    comp = wah.DeviceCompressor(matrix.size, indexed=True)
    want, _ = wah.columns.compress_column_matrix(comp, torch.from_numpy(matrix.view(np.int32)).cuda())
    assert stream.numel() == want.numel() and bool((stream == want).all())
    assert bool((seg_offsets == comp.seg_offsets).all())
    assert np.array_equal(_host(stream), np.concatenate([oracle.compress(row) for row in matrix]))
    ids = list(range(n_values))
    counts = wah.columns.count_columns(wah, stream, seg_offsets, n, ids)
    assert counts.tolist() == np.bincount(keys, minlength=n_values).tolist() and counts[5].item() == 0
    other_keys, (other, other_offsets, _) = _attribute(wah, 6, n_rows, n_values, unused=2)
    table = wah.columns.crosstab_columns(wah, (stream, seg_offsets, ids), (other, other_offsets, ids), n)
    want_table, _, _ = np.histogram2d(keys, other_keys, bins=[np.arange(n_values + 1)] * 2)
    assert np.array_equal(table.cpu().numpy(), want_table.astype(np.int64))
    with pytest.raises(ValueError):
        wah.columns.index_from_keys(wah, torch.from_numpy(keys.astype(np.int64)).cuda(), 6)


def test_bitmaps_from_rows(wah, oracle):
    n = 992
    lists = [np.array([3, 77, 31000], np.int64), np.empty(0, np.int64), np.arange(0, 31744, 2, dtype=np.int64)]
    got, index = wah.columns.bitmaps_from_rows(wah, [_dev64(r) for r in lists], n)
    want, want_index = _rows.reference(oracle, lists, n)
    assert np.array_equal(_host(got), want) and np.array_equal(index.cpu().numpy(), want_index)
    both, _ = wah.columns.combine_columns(wah, "or", got, index, n, [0, 2])
    assert np.array_equal(_host(both), oracle.compress(_select.bitmap_of(np.union1d(lists[0], lists[2]), n)))


def _status(wah, rows, ends, n, out=None):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    sc = torch.empty(int(wah.lib().wah_from_positions_scratch_bytes(n, len(ends))), dtype=torch.uint8, device="cuda:0")
    wah.from_positions_device(_dev64(rows), _dev64(ends), n, scratch=sc, out=out, check=False)
    return int(wah.lib().wah_from_positions_status(sc.data_ptr(), None))


def _valid_input():
    """Three lists of 200, 200 and 100 rows over a bitmap of 2981 words; the second one starts below the first one's end."""
    n = 2981
    lists = [np.arange(200, dtype=np.int64) * 470 + 11, np.arange(200, dtype=np.int64) * 31 + 5, np.arange(100, dtype=np.int64) * 900 + 1]
    rows, ends = _rows.flatten(lists)
    assert rows[199] > rows[200] and rows[399] > rows[400]  # descents exactly on the list boundaries
    return n, rows, ends


@pytest.mark.parametrize("at", (0, 100, 199), ids=("first", "middle", "last"))
def test_refused_rows(wah, at):
    """Each defect alone in otherwise valid input, in a list of 200 rows (the call's second list)."""
    n, rows, ends = _valid_input()
    assert _status(wah, rows, ends, n) == 0  # (descents on the two list boundaries are legal)
    i = 200 + at
    if at < 199:
        bad = rows.copy()
        bad[i + 1] = bad[i]  # a duplicate
        assert _status(wah, bad, ends, n) == WAH_ERR_STREAM
        bad = rows.copy()
        bad[i], bad[i + 1] = rows[i + 1], rows[i]  # a descending pair
        assert _status(wah, bad, ends, n) == WAH_ERR_STREAM
    if at > 0:
        bad = rows.copy()
        bad[i] = bad[i - 1]  # a duplicate of the row in front
        assert _status(wah, bad, ends, n) == WAH_ERR_STREAM
        bad = rows.copy()
        bad[i - 1], bad[i] = rows[i], rows[i - 1]
        assert _status(wah, bad, ends, n) == WAH_ERR_STREAM
    bad = rows.copy()
    bad[i] = 32 * n  # the first position behind the bitmap
    assert _status(wah, bad, ends, n) == WAH_ERR_STREAM
    if at == 199:
        ok = rows.copy()
        ok[i] = 32 * n - 1  # the last position inside it
        assert _status(wah, ok, ends, n) == 0


def test_refused_ends(wah):
    n, rows, ends = _valid_input()
    for bad in ([200, 199, 500], [400, 200, 500], [200, 400, 499], [200, 400, 501], [200, 600, 500]):
        assert _status(wah, rows, np.array(bad, np.int64), n) == WAH_ERR_STREAM, bad
    # a boundary that is moved off the descent leaves a descent inside a list
    assert _status(wah, rows, np.array([201, 400, 500], np.int64), n) == WAH_ERR_STREAM
    # an empty list on the descent: the same boundary twice
    assert _status(wah, rows, np.array([200, 200, 400, 500], np.int64), n) == 0
    with pytest.raises(wah.WahError):
        wah.from_positions_device(_dev64(rows), _dev64([200, 400, 499]), n)


def test_capacity(wah, oracle):
    import torch

    n, rows, ends = _valid_input()
    lists = [rows[:200], rows[200:400], rows[400:]]
    want, _ = _rows.reference(oracle, lists, n)
    total = want.size
    buf = torch.full((total + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    assert _status(wah, rows, ends, n, out=buf[: total - 1]) == WAH_ERR_CAPACITY
    assert bool((buf[total - 1:] == 0x5A5A5A5A).all())
    assert _status(wah, rows, ends, n, out=buf[:total]) == 0
    assert np.array_equal(_host(buf[:total]), want) and bool((buf[total:] == 0x5A5A5A5A).all())


def test_placement(wah, oracle):
    """d_out one word past a 16-byte boundary, d_rows and d_list_ends one entry past a 256-byte boundary."""
    import torch

    n, rows, ends = _valid_input()
    want, want_index = _rows.reference(oracle, [rows[:200], rows[200:400], rows[400:]], n)
    d_rows = torch.empty(rows.size + 33, dtype=torch.int64, device="cuda:0")
    d_ends = torch.empty(ends.size + 33, dtype=torch.int64, device="cuda:0")
    out = torch.empty(want.size + 5, dtype=torch.int32, device="cuda:0")
    r0 = (-d_rows.data_ptr() // 8) % 32 + 1
    e0 = (-d_ends.data_ptr() // 8) % 32 + 1
    o0 = (-out.data_ptr() // 4) % 4 + 1
    d_rows, d_ends, out = d_rows[r0: r0 + rows.size], d_ends[e0: e0 + ends.size], out[o0: o0 + want.size]
    assert d_rows.data_ptr() % 256 == 8 and d_ends.data_ptr() % 256 == 8 and out.data_ptr() % 16 == 4
    d_rows.copy_(_dev64(rows))
    d_ends.copy_(_dev64(ends))
    got, index = wah.from_positions_device(d_rows, d_ends, n, out=out)
    assert got.data_ptr() == out.data_ptr() and got.numel() == want.size
    assert np.array_equal(_host(got), want) and np.array_equal(index.cpu().numpy(), want_index)


def test_graph_replay_with_other_lists(wah, oracle):
    """The lists are only ever read by the device: ONE captured call, replayed after rows and ends were overwritten in place
    (same counts), builds the new lists (capture as the replay test of tests/test_gpu_bitop_list.py: side stream, warm-up
    outside, check=False; one chain of launches, no parallel branches)."""
    import torch

    n = 2981
    segments = _select.segments_of(n)
    rng = np.random.default_rng(9)

    def lists_of(sizes):
        return [np.sort(rng.choice(32 * n, size=k, replace=False)).astype(np.int64) for k in sizes]

    variants = [lists_of(s) for s in ((100, 300, 0, 200), (0, 1, 598, 1), (150, 150, 150, 150), (600, 0, 0, 0))]
    rows, ends = _rows.flatten(variants[0])
    d_rows, d_ends = _dev64(rows), _dev64(ends)
    sc = torch.empty(int(wah.lib().wah_from_positions_scratch_bytes(n, 4)), dtype=torch.uint8, device="cuda:0")
    res = torch.empty(wah.from_positions_max_words(n, 4, 600), dtype=torch.int32, device="cuda:0")
    res_offs = torch.zeros(4 * segments + 1, dtype=torch.int64, device="cuda:0")
    wah.from_positions_device(d_rows, d_ends, n, scratch=sc, out=res, out_offsets=res_offs, check=False)  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _, count, _ = wah.from_positions_device(d_rows, d_ends, n, scratch=sc, out=res, out_offsets=res_offs, check=False)
    for lists in (variants[1], variants[2], variants[3], variants[0]):
        rows, ends = _rows.flatten(lists)
        assert rows.size == 600
        d_rows.copy_(_dev64(rows))
        d_ends.copy_(_dev64(ends))
        res.fill_(0x5A5A5A5A)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_from_positions_status(sc.data_ptr(), None) == 0
        want, want_index = _rows.reference(oracle, lists, n)
        c = int(count.item())
        assert c == want.size and np.array_equal(_host(res[:c]), want)
        assert np.array_equal(res_offs.cpu().numpy(), want_index)
