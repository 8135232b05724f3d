"""GPU tests of wah_bsi_build_device (include/wah.h) and its front ends: the bit-sliced index of a value column in one call.
Everything is exact: the words, their count and every index entry against the CPU oracle's compress() of the slice matrix that
numpy builds FROM THE VALUES (tests/_slices.py, tests/_bsi.build_slices with zero_missing=True) and an indexed compress of it.
tests/test_slices_reference.py proves that every case can fail.  The largest column is three segments.
Sizes beyond one grid, where a wavefront takes a second block of 2048 rows: tests/test_gpu_full_grid.py."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _slices

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6
SEG = _slices.SEG


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


def _dev_words(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _dev_values(values):
    import torch

    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64)).cuda()


def _dev_exists(exists):
    import torch

    return None if exists is None else torch.from_numpy(np.ascontiguousarray(exists, dtype=bool)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


class Indexed:
    """One indexed compressor of a whole slice matrix, reused for the expected segment indexes."""

    def __init__(self, wah, n_words):
        self.comp = wah.DeviceCompressor(n_words, indexed=True)

    def of(self, matrix):
        self.comp.run(_dev_words(matrix.reshape(-1)))
        return self.comp.result().clone(), self.comp.seg_offsets.clone()


def _same(indexed, oracle, got, offs, matrix, what):
    """(got, offs) is exactly compress(matrix as one bitmap) and its segment index."""
    want = _slices.expected_stream(oracle, matrix)
    assert got.numel() == want.size, (what, got.numel(), want.size)
    assert np.array_equal(_host(got), want), what
    ref, ref_offs = indexed.of(matrix)
    assert offs.numel() == matrix.shape[0] * (matrix.shape[1] // SEG) + 1 == ref_offs.numel(), what
    assert np.array_equal(offs.cpu().numpy(), ref_offs.cpu().numpy()), what
    assert int(offs[-1].item()) == want.size and np.array_equal(_host(ref), want), what


# ---- 1: parity at the switch points ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_words", _slices.N_WORDS)
@pytest.mark.parametrize("n_bits", _slices.N_BITS)
@pytest.mark.parametrize("with_exists", (False, True), ids=("plain", "exists"))
def test_parity_at_the_switch_points(wah, oracle, n_words, n_bits, with_exists):
    indexed = Indexed(wah, (n_bits + with_exists) * n_words)
    for n_rows in _slices.row_counts(n_words):
        what = (n_words, n_rows, n_bits, with_exists)
        values, exists = _slices.case(n_words, n_rows, n_bits, with_exists)
        matrix = _slices.expected_matrix(values, exists, n_bits, n_words)
        got, offs = wah.bsi_build_device(_dev_values(values), n_bits, n_words, exists=_dev_exists(exists))
        _same(indexed, oracle, got, offs, matrix, what)


def test_every_slice_is_a_window_of_the_index(wah, oracle):
    n, n_bits = SEG * 3, 33
    values, exists = _slices.case(n, 32 * n - 1, n_bits, True)
    matrix = _slices.assert_case_matters(values, exists, n_bits, n, "windows")
    stream, offs = wah.bsi_build_device(_dev_values(values), n_bits, n, exists=_dev_exists(exists))
    segs = n // SEG
    for i in (0, 16, n_bits):  # the most significant slice, one in the middle, the existence bitmap
        first, last = int(offs[i * segs].item()), int(offs[(i + 1) * segs].item())
        assert np.array_equal(_host(stream[first:last]), oracle.compress(matrix[i])), i


@pytest.mark.parametrize("at", (1, 2, 3))
def test_placement(wah, oracle, at):
    """The values start on an 8-byte boundary that is no 16-byte one, the existence bytes `at` bytes behind a 4-byte boundary."""
    import torch

    n, n_bits, n_rows = SEG, 33, 2049 + 64 * at
    values, exists = _slices.case(n, n_rows, n_bits, True)
    matrix = _slices.assert_case_matters(values, exists, n_bits, n, at)
    v = torch.zeros(n_rows + 3, dtype=torch.int64, device="cuda:0")
    v0 = 1 if v.data_ptr() % 16 == 0 else 2
    e = torch.zeros(n_rows + 8, dtype=torch.bool, device="cuda:0")
    e0 = (-e.data_ptr()) % 4 + at
    d_values, d_exists = v[v0: v0 + n_rows], e[e0: e0 + n_rows]
    assert d_values.data_ptr() % 16 == 8 and d_exists.data_ptr() % 4 == at
    d_values.copy_(_dev_values(values))
    d_exists.copy_(_dev_exists(exists))
    got, offs = wah.bsi_build_device(d_values, n_bits, n, exists=d_exists)
    _same(Indexed(wah, matrix.size), oracle, got, offs, matrix, at)


# ---- 2: what the call refuses -----------------------------------------------------------------------------------------------
def _status(wah, d_values, n_bits, n, d_exists=None, out=None):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    k = n_bits + (d_exists is not None)
    sc = torch.empty(int(wah.lib().wah_bsi_build_scratch_bytes(n, k)), dtype=torch.uint8, device="cuda:0")
    wah.bsi_build_device(d_values, n_bits, n, exists=d_exists, scratch=sc, out=out, check=False)
    return int(wah.lib().wah_bsi_build_status(sc.data_ptr(), n, k, None))


@pytest.mark.parametrize("n_bits", (1, 20, 31, 32, 33, 63))
def test_a_value_of_two_to_the_width_is_refused(wah, n_bits):
    """One value of exactly 2^n_bits in otherwise valid input: in row 0, in the last row, and in a row that does not exist --
    every row is checked, whatever its existence byte says."""
    n, n_rows = SEG, 5000
    values, exists = _slices.case(n, n_rows, n_bits, True)
    missing = int(np.flatnonzero(~exists)[7])
    d_exists = _dev_exists(exists)
    assert _status(wah, _dev_values(values), n_bits, n) == 0
    assert _status(wah, _dev_values(values), n_bits, n, d_exists) == 0
    for row in (0, n_rows - 1, missing):
        bad = values.copy()
        bad[row] = np.uint64(1 << n_bits)
        assert _status(wah, _dev_values(bad), n_bits, n) == WAH_ERR_STREAM, row
        assert _status(wah, _dev_values(bad), n_bits, n, d_exists) == WAH_ERR_STREAM, row
        ok = values.copy()
        ok[row] = np.uint64((1 << n_bits) - 1)
        assert _status(wah, _dev_values(ok), n_bits, n, d_exists) == 0, row


def test_negative_values_are_refused_at_63_bits_and_are_values_at_64(wah, oracle):
    n, n_rows = SEG, 5000
    values, _ = _slices.case(n, n_rows, 63, False)
    for row, v in ((0, -1), (n_rows - 1, -(1 << 63)), (2500, -12345)):
        bad = values.view(np.int64).copy()
        bad[row] = v
        assert bad[row] < 0
        assert _status(wah, _dev_values(bad.view(np.uint64)), 63, n) == WAH_ERR_STREAM, row
        got, offs = wah.bsi_build_device(_dev_values(bad.view(np.uint64)), 64, n)
        matrix = _slices.expected_matrix(bad.view(np.uint64), None, 64, n)
        assert matrix[0].any()  # (the top slice holds the sign bit)
        _same(Indexed(wah, matrix.size), oracle, got, offs, matrix, row)
    with pytest.raises(wah.WahError):
        wah.bsi_build_device(_dev_values(bad.view(np.uint64)), 63, n)


@pytest.mark.parametrize("n_rows", (4992, 5000))
def test_a_value_behind_the_rows_is_never_looked_at(wah, oracle, n_rows):
    """The tensor's storage goes on behind n_rows with values that no width below 64 holds, and existence bytes that are set."""
    import torch

    n, n_bits = SEG, 20
    values, exists = _slices.case(n, n_rows, n_bits, True)
    storage = torch.full((n_rows + 4096,), -1, dtype=torch.int64, device="cuda:0")
    storage[:n_rows] = _dev_values(values)
    e_storage = torch.ones(n_rows + 4096, dtype=torch.bool, device="cuda:0")
    e_storage[:n_rows] = _dev_exists(exists)
    assert _status(wah, storage[:n_rows], n_bits, n, e_storage[:n_rows]) == 0
    assert _status(wah, storage[: n_rows + 1], n_bits, n, e_storage[: n_rows + 1]) == WAH_ERR_STREAM
    got, offs = wah.bsi_build_device(storage[:n_rows], n_bits, n, exists=e_storage[:n_rows])
    matrix = _slices.expected_matrix(values, exists, n_bits, n)
    _same(Indexed(wah, matrix.size), oracle, got, offs, matrix, n_rows)


def test_capacity(wah, oracle):
    import torch

    n, n_bits, n_rows = SEG, 20, 5000
    values, exists = _slices.case(n, n_rows, n_bits, True)
    want = _slices.expected_stream(oracle, _slices.expected_matrix(values, exists, n_bits, n))
    total = want.size
    d_values, d_exists = _dev_values(values), _dev_exists(exists)
    buf = torch.full((total + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    assert _status(wah, d_values, n_bits, n, d_exists, out=buf[: total - 1]) == WAH_ERR_CAPACITY
    assert bool((buf[total - 1:] == 0x5A5A5A5A).all())
    assert _status(wah, d_values, n_bits, n, d_exists, out=buf[:total]) == 0
    assert np.array_equal(_host(buf[:total]), want) and bool((buf[total:] == 0x5A5A5A5A).all())


# ---- 3: graph capture ---------------------------------------------------------------------------------------------------------
def test_graph_replay_with_other_values(wah, oracle):
    """The column is only ever read by the device: ONE captured call, replayed after values and existence bytes were overwritten in
    place, builds the new index (capture as the replay test of tests/test_gpu_from_positions.py: side stream, warm-up outside,
    check=False; one chain of launches, no parallel branches)."""
    import torch

    n, n_bits, n_rows = SEG * 3, 33, 70000
    k = n_bits + 1
    variants = [_slices.case(n, n_rows, n_bits, True)]
    rng = np.random.default_rng(11)
    for _ in range(3):
        variants.append((_bsi.uniform_values(rng, n_rows, n_bits), rng.random(n_rows) < 0.5))
    d_values, d_exists = _dev_values(variants[0][0]), _dev_exists(variants[0][1])
    sc = torch.empty(int(wah.lib().wah_bsi_build_scratch_bytes(n, k)), dtype=torch.uint8, device="cuda:0")
    res = torch.empty(wah.max_compressed_words(k * n), dtype=torch.int32, device="cuda:0")
    res_offs = torch.zeros(k * (n // SEG) + 1, dtype=torch.int64, device="cuda:0")
    wah.bsi_build_device(d_values, n_bits, n, exists=d_exists, scratch=sc, out=res, out_offsets=res_offs, check=False)  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _, count, _ = wah.bsi_build_device(d_values, n_bits, n, exists=d_exists, scratch=sc, out=res, out_offsets=res_offs, check=False)
    indexed = Indexed(wah, k * n)
    for values, exists in (variants[1], variants[2], variants[3], variants[0]):
        d_values.copy_(_dev_values(values))
        d_exists.copy_(_dev_exists(exists))
        res.fill_(0x5A5A5A5A)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bsi_build_status(sc.data_ptr(), n, k, None) == 0
        matrix = _slices.assert_case_matters(values, exists, n_bits, n, "replay")
        _same(indexed, oracle, res[: int(count.item())], res_offs, matrix, "replay")


# ---- 4: the column front end and the calls that read the index ------------------------------------------------------------------
@pytest.mark.parametrize("n,n_rows", ((SEG * 2, 32 * SEG * 2), (SEG, 5000)))
def test_bsi_from_values_is_the_torch_route(wah, oracle, n, n_rows):
    n_bits = 20
    values, exists = _slices.case(n, n_rows, n_bits, True)
    d_values, d_exists = _dev_values(values), _dev_exists(exists)
    old = wah.columns._bsi_from_values_torch(wah, d_values, n_bits, n_words_per_column=n, exists=d_exists)
    new = wah.columns.bsi_from_values(wah, d_values, n_bits, n_words_per_column=n, exists=d_exists)
    assert new[2:] == old[2:] == (n, n_bits, True)
    assert new[0].numel() == old[0].numel() and bool((new[0] == old[0]).all())
    assert new[1].numel() == old[1].numel() and bool((new[1] == old[1]).all())
    assert np.array_equal(_host(new[0]), _slices.expected_stream(oracle, _slices.assert_case_matters(values, exists, n_bits, n, "front end")))
    out, out_offsets, *rest = wah.columns.bsi_from_values(wah, d_values, n_bits, n_words_per_column=n, exists=d_exists, check=False)
    count = int(out_offsets[-1].item())
    assert tuple(rest) == (n, n_bits, True) and out.numel() >= count == old[0].numel()
    assert bool((out[:count] == old[0]).all()) and bool((out_offsets == old[1]).all())
    bad = values.copy()
    bad[n_rows // 2] = np.uint64(1 << n_bits)
    for route in (wah.columns.bsi_from_values, wah.columns._bsi_from_values_torch):
        with pytest.raises(ValueError):
            route(wah, _dev_values(bad), n_bits, n_words_per_column=n, exists=d_exists)


def test_a_64_bit_attribute_answers_range_and_fetch(wah, oracle):
    n, n_bits = SEG * 2, 64
    n_rows = 32 * n - 5
    values, _ = _slices.case(n, n_rows, n_bits, False)
    stream, offs = wah.bsi_build_device(_dev_values(values), n_bits, n)
    table = wah.columns.column_operand_table(stream, offs, n, list(range(n_bits)))
    column, _ = _slices.padded(values, None, n)
    ordered = np.sort(values)
    lo, hi = int(ordered[n_rows // 3]), int(ordered[2 * n_rows // 3])
    assert lo < (1 << 63) < hi
    want = _bsi.expected_range(column, lo, hi)
    assert want.any() and not (want == _bsi.ONES).all()
    got, _ = wah.bsi_range_device(table, (lo, hi), n)
    assert np.array_equal(_host(got), oracle.compress(want))
    rows = np.sort(np.random.default_rng(5).choice(n_rows, size=100, replace=False)).astype(np.int64)
    rows[-1] = 32 * n - 1  # a row behind the caller's: value 0
    fetched = wah.fetch_device(table, _dev_values(rows.view(np.uint64)), n, wah.FETCH_BITS)
    assert np.array_equal(fetched.cpu().numpy().view(np.uint64), column[rows])
    assert column[rows[:-1]].all() and column[rows[-1]] == 0
