"""GPU tests of wah_bitop_list_indexed_device: one bit operation over an operand list of any length that lives in device
memory (include/wah.h), and its front ends in columns.py.  Everything is exact: the result's words, their count and its segment
index against compress() of the bitmaps combined with numpy -- the CPU oracle and an indexed compress of the combined bitmap.

These tests use the call from outside: random and clustered bitmaps, 1 to 300 operands, refusals, graph replay -- which way a
segment takes inside the kernel is left to the data.  The cases that sit ON its switch points (128 words a batch, four batches
in flight, 64 operands a chunk, fills of 8 / 9 / 64 groups, the settled one-word segment, the refusals at 1023 / 1025 groups and
at the count clamp) are built in tests/_switch.py and run by the test_list_* tests of tests/test_gpu_switch_points.py."""
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6

FOLD = {"and": lambda xs: np.bitwise_and.reduce(xs), "or": lambda xs: np.bitwise_or.reduce(xs),
        "xor": lambda xs: np.bitwise_xor.reduce(xs), "andnot": lambda xs: xs[0] & ~np.bitwise_or.reduce(xs[1:]) if len(xs) > 1 else xs[0]}


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _indexed_stream(wah, d_in):
    comp = wah.DeviceCompressor(d_in.numel(), indexed=True)
    comp.run(d_in)
    return comp.result().clone(), comp.seg_offsets.clone()


def _same(wah, oracle, got, offs, combined, what):
    """(got, offs) is exactly compress(combined) and its segment index."""
    combined = np.ascontiguousarray(combined, dtype=np.uint32)
    want = oracle.compress(combined)
    assert got.numel() == want.size, (what, got.numel(), want.size)
    assert np.array_equal(_host(got), want), what
    _, ref_offs = _indexed_stream(wah, _dev(combined))
    assert np.array_equal(offs.cpu().numpy(), ref_offs.cpu().numpy()), what


def _pool(oracle, n, size=300):
    """Bitmaps of every kind a bitmap index holds, in turn: uniform p in {0.3, 0.9, 2^-10, 2^-13}, clustered with mean runs from
    200 to 12 000 bits, all zeros, all ones."""
    maps = []
    for j in range(size):
        kind = j % 8
        if kind in (0, 2, 3, 5):
            maps.append(oracle.gen_uniform(n, 100 + j, {0: 0.3, 2: 0.9, 3: 2.0 ** -10, 5: 2.0 ** -13}[kind]))
        elif kind in (1, 4):
            maps.append(oracle.gen_clustered(n, 100 + j, 200 + (11800 * ((j * 7) % size)) // (size - 1)))
        elif kind == 6:
            maps.append(np.zeros(n, np.uint32))
        else:
            maps.append(np.full(n, 0xFFFFFFFF, np.uint32))
    return maps


@pytest.mark.parametrize("n", [992 * 40 + 9, 7, 1, 992 * 257, 992 * 64 + 991])
def test_any_number_of_operands_vs_oracle(wah, oracle, n):
    """1 to 300 operands of every kind, all four operations, ragged lengths (a last segment of few groups, a last group of few
    bits): the words, their count and the index of compress(fold(bitmaps)); and for up to 8 operands the very output of
    wah_bitop_many_indexed_device."""
    maps = _pool(oracle, n)
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    table = wah.bitop_operand_table(ops)
    assert tuple(table.shape) == (300, 3) and table.is_cuda
    for k in (1, 2, 8, 9, 17, 64, 300):
        stack = np.stack(maps[:k])
        for name, fn in FOLD.items():
            combined = fn(stack).astype(np.uint32)
            got, offs = wah.bitop_list_indexed_device(name, ops[:k], n)
            _same(wah, oracle, got, offs, combined, (n, k, name))
            # ... the same through a ready table (a slice of the big one is a table too)
            got2, offs2 = wah.bitop_list_indexed_device(name, table[:k], n)
            assert got2.numel() == got.numel() and bool((got2 == got).all()) and bool((offs2 == offs).all()), (n, k, name)
            if k <= 8:
                ref, ref_offs = wah.bitop_many_indexed_device(name, ops[:k], n)
                assert ref.numel() == got.numel() and bool((ref == got).all()) and bool((ref_offs == offs).all()), (n, k, name)


def test_empty_bitmap(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    got, out_offs = wah.bitop_list_indexed_device("or", [(stream, offs)] * 5, 0)
    assert got.numel() == 0 and int(out_offs[0].item()) == 0


def _equality_index(wah, n_rows, n_bins, seed):
    """keys, and the compressed equality-encoded index over them: one bitmap per bin, all through compress_column_matrix."""
    import torch

    rng = np.random.default_rng(seed)
    keys = rng.integers(0, n_bins, n_rows)
    cols = np.stack([np.packbits(keys == v, bitorder="little").view(np.uint32) for v in range(n_bins)])
    matrix = torch.from_numpy(cols.view(np.int32)).cuda()
    comp = wah.DeviceCompressor(matrix.numel(), indexed=True)
    stream, _ = wah.columns.compress_column_matrix(comp, matrix)
    return keys, cols, comp, stream


def _bitmap(mask):
    return np.packbits(mask, bitorder="little").view(np.uint32)


def test_in_lists_and_ranges_on_an_equality_index(wah, oracle):
    """What the call is for: `lo <= key <= hi` and `key IN (...)` over a 64-bin index of random keys, as ONE call each."""
    import torch

    n_rows = 32 * 992 * 37
    n = n_rows // 32
    keys, cols, comp, stream = _equality_index(wah, n_rows, 64, 7)
    index = comp.seg_offsets
    combine = wah.columns.combine_columns
    for lo, hi in ((5, 5), (0, 63), (10, 29), (0, 8), (40, 63), (31, 32)):
        ids = torch.arange(lo, hi + 1, dtype=torch.int64, device="cuda")
        got, offs = combine(wah, "or", stream, index, n, ids)
        _same(wah, oracle, got, offs, _bitmap((keys >= lo) & (keys <= hi)), ("range", lo, hi))
    rng = np.random.default_rng(11)
    for size in (1, 3, 17, 40):
        ids = [int(v) for v in rng.permutation(64)[:size]]
        got, offs = combine(wah, "or", stream, index, n, ids)  # a Python list
        _same(wah, oracle, got, offs, _bitmap(np.isin(keys, ids)), ("in", ids))
    ids = [int(v) for v in rng.permutation(64)[:23]]
    once, once_offs = combine(wah, "or", stream, index, n, ids)
    twice, twice_offs = combine(wah, "or", stream, index, n, ids + ids)        # OR is idempotent
    assert once.numel() == twice.numel() and bool((once == twice).all()) and bool((once_offs == twice_offs).all())
    shuffled = [ids[i] for i in rng.permutation(len(ids))]
    got, offs = combine(wah, "xor", stream, index, n, ids + shuffled)           # XOR cancels: one zero fill per segment
    assert got.numel() == n // 992
    _same(wah, oracle, got, offs, np.zeros(n, np.uint32), "xor twice")
    got, offs = combine(wah, "and", stream, index, n, [12, 50])                 # a key is in one bin
    _same(wah, oracle, got, offs, np.zeros(n, np.uint32), "and of two bins")
    got, offs = combine(wah, "andnot", stream, index, n, list(range(64)))       # bin 0 and not any other: bin 0
    _same(wah, oracle, got, offs, cols[0], "andnot")
    with pytest.raises(ValueError):
        wah.columns.column_operand_table(stream, index, n, [3, 64])
    with pytest.raises(ValueError):
        wah.columns.column_operand_table(stream, index, n - 1, [3])


def test_overlapping_columns_and_chaining(wah, oracle):
    """Columns that overlap (column_spec(): sparse, clustered, dense in turn): AND and ANDNOT over 9 and more of them; and a
    result chains, through its own index, into wah_bitop_indexed_device."""
    n = 992 * 120
    specs = [wah.columns.column_spec(c, n, seed=900) for c in range(14)]
    matrix = wah.columns.make_column_matrix(wah, specs, "cuda:0")
    comp = wah.DeviceCompressor(matrix.numel(), indexed=True)
    stream, _ = wah.columns.compress_column_matrix(comp, matrix)
    cols = _host(matrix)
    for name, ids in (("and", [2, 5, 8, 11, 2, 0, 3, 6, 9, 12]), ("and", [2, 5, 8, 11, 5, 8, 11, 2, 5, 8]), ("andnot", [5, 0, 1, 3, 4, 6, 7, 9, 10, 12]),
                      ("andnot", [2] + list(range(3, 14))), ("xor", list(range(14))), ("or", [0, 1, 3, 4, 6, 7, 9, 10, 12, 13, 0])):
        got, offs = wah.columns.combine_columns(wah, name, stream, comp.seg_offsets, n, ids)
        _same(wah, oracle, got, offs, FOLD[name](cols[ids]), (name, ids))
    # (sparse or clustered ...) and dense, through the first result's index
    ids = [0, 1, 3, 4, 6, 7, 9, 10, 12]
    first, first_offs = wah.columns.combine_columns(wah, "or", stream, comp.seg_offsets, n, ids)
    other = _indexed_stream(wah, matrix[2].contiguous())
    got, offs = wah.bitop_indexed_device("and", first.clone(), first_offs.clone(), *other, n)
    _same(wah, oracle, got, offs, np.bitwise_or.reduce(cols[ids]) & cols[2], "chained")
    # ... and into another list call, beside columns of the matrix
    table = wah.columns.column_operand_table(stream, comp.seg_offsets, n, [5, 8])
    import torch

    mixed = torch.cat([wah.bitop_operand_table([(first, first_offs)]), table])
    got, offs = wah.bitop_list_indexed_device("andnot", mixed, n)
    _same(wah, oracle, got, offs, np.bitwise_or.reduce(cols[ids]) & ~(cols[5] | cols[8]), "chained list")


def test_graph_replay_with_another_selection(wah, oracle):
    """The operand table is only ever read by the device: ONE captured list call, replayed after the table was overwritten in place,
    combines the new selection (capture as test_indexed_path_is_graph_capturable: side stream, warm-up outside, check=False; one
    chain of launches, no parallel branches)."""
    import torch

    n_rows = 32 * 992 * 50
    n = n_rows // 32
    keys, cols, comp, stream = _equality_index(wah, n_rows, 32, 23)
    selections = ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [31, 3, 17, 5, 22, 9, 30, 1, 12, 14, 28, 2], [20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31])
    table = wah.columns.column_operand_table(stream, comp.seg_offsets, n, selections[0])
    sc = torch.empty(int(wah.lib().wah_bitop_list_scratch_bytes(n, table.shape[0])), dtype=torch.uint8, device="cuda:0")
    res = torch.empty(wah.max_compressed_words(n), dtype=torch.int32, device="cuda:0")
    res_offs = torch.zeros(n // 992 + 2, dtype=torch.int64, device="cuda:0")
    wah.bitop_list_indexed_device("or", table, n, scratch=sc, out=res, out_offsets=res_offs, check=False)  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _, count, _ = wah.bitop_list_indexed_device("or", table, n, scratch=sc, out=res, out_offsets=res_offs, check=False)
    for sel in (selections[1], selections[2], selections[0], selections[1]):
        ids = torch.tensor(sel, dtype=torch.int64, device="cuda:0")
        same = wah.columns.column_operand_table(stream, comp.seg_offsets, n, ids, out=table)  # in place, on the device
        assert same.data_ptr() == table.data_ptr()
        res.fill_(0x5A5A5A5A)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bitop_list_status(sc.data_ptr(), n, table.shape[0], None) == 0
        c = int(count.item())
        _same(wah, oracle, res[:c], res_offs[: n // 992 + 1], _bitmap(np.isin(keys, sel)), sel)


def _status(wah, name, operands, n, **kw):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    table = operands if isinstance(operands, torch.Tensor) else wah.bitop_operand_table(operands)
    sc = torch.empty(int(wah.lib().wah_bitop_list_scratch_bytes(n, table.shape[0])), dtype=torch.uint8, device="cuda:0")
    wah.bitop_list_indexed_device(name, table, n, scratch=sc, check=False, **kw)
    return int(wah.lib().wah_bitop_list_status(sc.data_ptr(), n, table.shape[0], None))


def test_refusals_come_from_the_status_call(wah, oracle):
    """What only the device sees: an index that is not the stream's, a fill that runs past its segment, an empty fill, a table entry
    without an index, too small an output -- each reported, none followed outside the tensors."""
    import torch

    n = 992 * 64
    maps = [oracle.gen_uniform(n, 1, 0.1), oracle.gen_clustered(n, 2, 4000), oracle.gen_uniform(n, 3, 2.0 ** -9), np.zeros(n, np.uint32)]
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    many = ops[:3] * 4
    assert _status(wah, "or", many, n) == 0
    bad = ops[0][1].clone()
    bad[3] += 1
    for at in (0, 5, 11):
        broken = list(many)
        broken[at] = (ops[0][0], bad)
        assert _status(wah, "or", broken, n) == WAH_ERR_STREAM, at
        with pytest.raises(wah.WahError):
            wah.bitop_list_indexed_device("or", broken, n)
    sz, oz = ops[3]  # 64 words: one zero fill of 1024 groups per segment
    for word in (0x80000000 | 1025, 0x80000000, 0x80000000 | 1023, 0xC0000000 | 1025):
        fill = sz.clone()
        fill[5] = word - (1 << 32)
        for name in ("or", "and", "xor", "andnot"):
            assert _status(wah, name, [ops[1], (fill, oz), ops[2]], n) == WAH_ERR_STREAM, (hex(word), name)
    # an index that points behind the stream's stated length
    short = ops[0][0][: ops[0][0].numel() - 5]
    assert _status(wah, "or", [ops[1], (short, ops[0][1])], n) == WAH_ERR_STREAM
    # a table entry whose index pointer is 0, or misaligned; whose stream pointer is 0
    for col, value in ((2, 0), (0, 0)):
        table = wah.bitop_operand_table(many)
        table[7, col] = value
        assert _status(wah, "xor", table, n) == WAH_ERR_STREAM, (col, value)
    table = wah.bitop_operand_table(many)
    table[7, 2] += 4  # (inside the index tensor: nothing outside it would be read even if it were followed)
    assert _status(wah, "xor", table, n) == WAH_ERR_STREAM
    # an output of 3 words
    small = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert _status(wah, "or", many, n, out=small[:3]) == WAH_ERR_CAPACITY
    assert bool((small[3:] == 0x5A5A5A5A).all())
    with pytest.raises(wah.WahError):
        wah.bitop_list_indexed_device("or", many, n, out=small[:3])


def test_stream_that_is_only_four_byte_aligned(wah, oracle):
    import torch

    n = 992 * 90 + 77
    maps = [oracle.gen_uniform(n, 40 + j, 0.2) if j % 2 else oracle.gen_clustered(n, 40 + j, 900) for j in range(10)]
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    want, want_offs = wah.bitop_list_indexed_device("xor", ops, n)
    for at in (0, 4, 9):
        st = ops[at][0]
        shifted = torch.empty(st.numel() + 3, dtype=torch.int32, device="cuda:0")[3:]
        shifted.copy_(st)
        assert shifted.data_ptr() % 16 == 12
        moved = list(ops)
        moved[at] = (shifted, ops[at][1])
        got, offs = wah.bitop_list_indexed_device("xor", moved, n)
        assert got.numel() == want.numel() and bool((got == want).all()) and bool((offs == want_offs).all()), at
    _same(wah, oracle, want, want_offs, FOLD["xor"](np.stack(maps)), "xor of ten")
