"""GPU tests of wah_count_list_indexed_device and wah_positions_indexed_device (include/wah.h) and their front ends in api.py
and columns.py.  Everything is exact: counts against the popcount, positions against np.flatnonzero of the bitmap's bits
(tests/_select.py; its stream-level references are proven on the CPU by tests/test_select_reference.py), every window of
ranks, both output alignments, sentinels around every output.  Shapes are small -- the largest bitmap is 992 * 257 words --
except the two hand-built streams of more segments than one and two levels of the rank scan hold, which exist only
compressed."""
import importlib

import numpy as np
import pytest

from tests import _select as sel

pytestmark = pytest.mark.gpu

WAH_ERR_STREAM = -6
SENTINEL = 0x5A5A5A5A5A5A5A5A
LENGTHS = [1, 7, 31, 992, 993, 992 * 3 + 5, 992 * 64 + 991, 992 * 257]


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


def _dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _indexed_stream(wah, words):
    d_in = _dev(words)
    comp = wah.DeviceCompressor(d_in.numel(), indexed=True)
    comp.run(d_in)
    return comp.result().clone(), comp.seg_offsets.clone()


def _hand_stream(stream, index=None):
    return _dev(stream), _dev64(sel.index_of(stream) if index is None else index)


@pytest.fixture(scope="module")
def cases(wah, oracle):
    """n -> name -> (bitmap, (stream, index) on the device, expected positions): made once per length, shared, never changed."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = {name: (words, _indexed_stream(wah, words), sel.ref_positions(words, n)) for name, words in sel.bitmaps(oracle, n).items()}
        return made[n]

    return get


def _scratch(wah, n, k=1):
    import torch

    return torch.empty(int(wah.lib().wah_select_scratch_bytes(n, k)), dtype=torch.uint8, device="cuda:0")


# ---- 1: counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_counts_vs_popcount(wah, cases, n):
    case = cases(n)
    want = [sel.ref_count(words, n) for words, _, _ in case.values()]
    assert len(set(want)) > 3 and any(want) and want == [pos.size for _, _, pos in case.values()]  # neither all equal nor all zero
    ops = [op for _, op, _ in case.values()]
    got = wah.count_device(ops, n)
    assert str(got.dtype) == "torch.int64" and got.cpu().tolist() == want
    for op, w in zip(ops, want):  # one operand at a time
        assert wah.count_device([op], n).cpu().tolist() == [w]


def test_count_of_an_empty_bitmap(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    counts = torch.full((3,), 77, dtype=torch.int64, device="cuda")
    assert wah.count_device([(stream, offs)] * 3, 0, counts=counts).cpu().tolist() == [0, 0, 0]
    pos, total = wah.positions_device(stream, offs, 0)
    assert pos.numel() == 0 and total == 0


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 130, 4097])
def test_table_shapes(wah, oracle, cases, k):
    """k operands drawn with repeats from the pool, as a list and as a ready table; and k windows into a column matrix."""
    import torch

    n = 992 * 3 + 5
    case = list(cases(n).values())
    rng = np.random.default_rng(k)
    ids = rng.integers(0, len(case), k)
    ids[-1] = ids[0]  # (a repeat even at k = 2)
    want = [case[i][2].size for i in ids]
    assert k <= 2 or len(set(want)) > 1
    ops = [case[i][1] for i in ids]
    assert wah.count_device(ops, n).cpu().tolist() == want
    table = wah.bitop_operand_table(ops)
    sc, counts = _scratch(wah, n, k), torch.full((k,), -1, dtype=torch.int64, device="cuda")
    assert wah.count_device(table, n, scratch=sc, counts=counts) is counts and counts.cpu().tolist() == want
    # windows into a column matrix: the columns' own counts, row by row
    m = 992 * 3
    cols = np.stack([w[:m] for w, _, _ in case])
    comp = wah.DeviceCompressor(cols.size, indexed=True)
    stream, _ = wah.columns.compress_column_matrix(comp, torch.from_numpy(cols.view(np.int32)).cuda())
    per_column = [sel.ref_count(c, m) for c in cols]
    assert len(set(per_column)) > 3
    got = wah.columns.count_columns(wah, stream, comp.seg_offsets, m, torch.from_numpy(ids).cuda())  # device-resident numbers
    assert got.cpu().tolist() == [per_column[i] for i in ids]
    assert wah.columns.count_columns(wah, stream, comp.seg_offsets, m, [int(i) for i in ids[:5]]).cpu().tolist() == [per_column[i] for i in ids[:5]]


def _equality_index(wah, keys, n_bins):
    import torch

    cols = np.stack([np.packbits(keys == v, bitorder="little").view(np.uint32) for v in range(n_bins)])
    matrix = torch.from_numpy(cols.view(np.int32)).cuda()
    comp = wah.DeviceCompressor(matrix.numel(), indexed=True)
    stream, _ = wah.columns.compress_column_matrix(comp, matrix)
    return cols, comp, stream


def test_histogram_of_an_equality_encoded_attribute(wah):
    """One column per value: the per-column counts are GROUP BY value."""
    n_rows = 992 * 8 * 32
    keys = np.random.default_rng(3).integers(0, 37, (2, n_rows)).min(axis=0)  # (a skewed attribute: 37 values of unequal frequency)
    want = np.bincount(keys, minlength=37)
    assert want.sum() == n_rows and want.min() > 0 and len(set(want.tolist())) > 30
    _, comp, stream = _equality_index(wah, keys, 37)
    got = wah.columns.count_columns(wah, stream, comp.seg_offsets, n_rows // 32, list(range(37)))
    assert got.cpu().tolist() == want.tolist() and int(got.sum().item()) == n_rows


# ---- 2: positions ---------------------------------------------------------------------------------------------------------------
def _raw_positions(wah, op, n, first, cap, buf, at, info, sc):
    """The C call itself: cap entries at buf[at ..]; returns the status."""
    lib = wah.lib()
    stream, offs = op
    rc = lib.wah_positions_indexed_device(n, stream.data_ptr(), stream.numel(), offs.data_ptr(), first, buf.data_ptr() + 8 * at if cap else None,
                                          cap, info.data_ptr(), sc.data_ptr(), sc.numel(), None)
    assert rc == 0, lib.wah_last_error()
    return int(lib.wah_select_status(sc.data_ptr(), None))


def _windows(want):
    """(first_rank, out_capacity) pairs: first ranks at both ends, inside and at the start of a segment, and behind the end, each
    with capacities around the wavefront width and around what is left."""
    total = want.size
    seg_first = int(np.searchsorted(want, sel.SEG_BITS))  # the first rank of segment 1 (total: no bit behind segment 0)
    firsts = sorted({0, 1, seg_first + 3, seg_first, max(total - 1, 0), total, total + 5})
    out = []
    for first in firsts:
        rest = max(total - first, 0)
        out += [(first, cap) for cap in sorted({0, 1, 63, 64, 65, rest, rest + 7})]
    return out


@pytest.mark.parametrize("n", LENGTHS)
def test_positions_vs_flatnonzero(wah, cases, n):
    import torch

    sc = _scratch(wah, n)
    info = torch.empty(2, dtype=torch.int64, device="cuda")
    for name, (words, op, want) in cases(n).items():
        total = want.size
        got, got_total = wah.positions_device(op[0], op[1], n)  # two calls: the total, then an exactly sized output
        assert got_total == total and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (n, name)
        want_d = torch.from_numpy(want).cuda()
        buf = torch.empty(total + 7 + 8, dtype=torch.int64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        for w, (first, cap) in enumerate(_windows(want)):
            at = 2 + w % 2  # the output 0 and 8 bytes behind a 16-byte boundary
            buf.fill_(SENTINEL)
            info.fill_(-1)
            assert _raw_positions(wah, op, n, first, cap, buf, at, info, sc) == 0
            written = min(max(total - first, 0), cap)
            assert info.cpu().tolist() == [total, written], (n, name, first, cap)
            assert torch.equal(buf[at: at + written], want_d[first: first + written]), (n, name, first, cap)
            assert bool((buf[:at] == SENTINEL).all()) and bool((buf[at + written:] == SENTINEL).all()), (n, name, first, cap)


def test_positions_front_end(wah, cases):
    import torch

    n = 992 * 3 + 5
    words, op, want = cases(n)["uniform 0.3"]
    got, total = wah.positions_device(op[0], op[1], n, first=100, limit=1000)
    assert total == want.size and np.array_equal(got.cpu().numpy(), want[100:1100])
    got, total = wah.positions_device(op[0], op[1], n, first=want.size - 10, limit=1000)
    assert np.array_equal(got.cpu().numpy(), want[-10:])
    out = torch.full((50,), -1, dtype=torch.int64, device="cuda")
    got, total = wah.positions_device(op[0], op[1], n, first=7, out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want[7:57])
    got, info = wah.positions_device(op[0], op[1], n, limit=20, check=False)
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [want.size, 20] and np.array_equal(got.cpu().numpy(), want[:20])
    with pytest.raises(wah.WahError):
        wah.positions_device(op[0], op[1], n, check=False)


def test_segments_on_the_staging_and_batch_edges(wah, oracle):
    """Segments of exactly 0, 1, 64 x 31 - 1, 64 x 31, 64 x 31 + 1, 31743 and 31744 set bits, and segments of 1 .. 1024 stream
    words around the load batches, in one bitmap; every window of one segment's ranks."""
    rng = np.random.default_rng(9)
    parts = [sel.segment_of_bits(k) for k in sel.SEGMENT_BIT_EDGES]
    parts += [sel.segment_of_words(w, rng, bit) for w in sel.SEGMENT_WORD_EDGES for bit in (0, 1)]
    words = np.concatenate(parts)
    n = words.size
    want = sel.ref_positions(words, n)
    per_segment = [sel.ref_count(p, sel.SEG_WORDS) for p in parts]
    assert per_segment[: len(sel.SEGMENT_BIT_EDGES)] == list(sel.SEGMENT_BIT_EDGES)
    op = _indexed_stream(wah, words)
    assert np.array_equal(np.diff(op[1].cpu().numpy())[len(sel.SEGMENT_BIT_EDGES):], np.repeat(sel.SEGMENT_WORD_EDGES, 2))
    assert wah.count_device([op], n).cpu().tolist() == [want.size]
    got, total = wah.positions_device(op[0], op[1], n)
    assert total == want.size and np.array_equal(got.cpu().numpy(), want)
    # each segment alone as a bitmap of its own: its count
    singles = [_indexed_stream(wah, p) for p in parts]
    assert wah.count_device(singles, sel.SEG_WORDS).cpu().tolist() == per_segment
    # windows that begin and end on the segments' first ranks
    starts = np.concatenate([[0], np.cumsum(per_segment)])
    for s in range(len(parts)):
        got, _ = wah.positions_device(op[0], op[1], n, first=int(starts[s]), limit=per_segment[s])
        assert np.array_equal(got.cpu().numpy(), want[starts[s]: starts[s + 1]]), s


def test_pad_rule_on_the_device(wah):
    """Hand-built streams that set pad bits (tests/test_select_reference.py holds the same streams against the walk)."""
    for what, n, stream, bits in sel.pad_streams():
        op = _hand_stream(stream)
        want = sel.stream_positions(stream, n)
        assert want.size == bits
        assert wah.count_device([op], n).cpu().tolist() == [bits], what
        got, total = wah.positions_device(op[0], op[1], n)
        assert total == bits and np.array_equal(got.cpu().numpy(), want), what


@pytest.mark.parametrize("n_segments", [sel.RANK_CHUNK - 1, sel.RANK_CHUNK, 2 * sel.RANK_CHUNK + 5, sel.RANK_CHUNK ** 2 + 1])
def test_more_segments_than_a_scan_level_holds(wah, n_segments):
    """The rank table has n_segments + 1 entries: one chunk, one more, a second level, a third (positions beyond 2^32)."""
    c = sel.RANK_CHUNK
    marked = {s: (7 * s) % 31 for s in (0, 1, c - 2, c - 1, c, c + 1, 2 * c - 1, 2 * c, c * c - 1, c * c, n_segments - 1) if s < n_segments}
    n, stream, index, want = sel.long_stream(n_segments, marked)
    op = _hand_stream(stream, index)
    assert wah.count_device([op, op], n).cpu().tolist() == [want.size] * 2
    got, total = wah.positions_device(op[0], op[1], n)
    assert total == want.size and np.array_equal(got.cpu().numpy(), want)
    got, total = wah.positions_device(op[0], op[1], n, first=want.size - 2, limit=5)
    assert np.array_equal(got.cpu().numpy(), want[-2:])
    assert n_segments <= c * c or want[-1] > 1 << 32


# ---- 3: the chain ---------------------------------------------------------------------------------------------------------------
ONES = np.uint32(0xFFFFFFFF)


def evaluate(maps, query):
    """query: list of (indices into maps, negate).  NOT is over the 32 * n_words bits of the bitmap."""
    result = np.full(maps[0].shape, ONES, np.uint32)
    for ids, negate in query:
        clause = np.zeros(maps[0].shape, np.uint32)
        for i in sorted(set(ids)):
            clause |= maps[i]
        result &= ~clause if negate else clause
    return result


def test_select_rows_over_three_attributes(wah):
    """SELECT rowid WHERE 10 <= a <= 29 AND b IN (3, 7, 11, 12) AND c NOT IN (0, 5), whole and with LIMIT / OFFSET."""
    import torch

    n_rows = 32 * 992 * 9
    n = n_rows // 32
    rng = np.random.default_rng(5)
    keys = [rng.integers(0, bins, n_rows) for bins in (64, 16, 8)]
    index = [_equality_index(wah, k, bins) for k, bins in zip(keys, (64, 16, 8))]
    (cols_a, comp_a, st_a), (cols_b, comp_b, st_b), (cols_c, comp_c, st_c) = index
    maps = list(cols_a) + list(cols_b) + list(cols_c)
    query = [(list(range(10, 30)), False), ([64 + v for v in (3, 7, 11, 12)], False), ([80 + 0, 80 + 5], True)]
    want_map = evaluate(maps, query)
    assert want_map.any() and not (want_map == ONES).all()
    want = sel.ref_positions(want_map, n)
    mask = (keys[0] >= 10) & (keys[0] <= 29) & np.isin(keys[1], (3, 7, 11, 12)) & ~np.isin(keys[2], (0, 5))
    assert np.array_equal(want, np.flatnonzero(mask)) and 1000 < want.size < n_rows // 4
    predicates = [(st_a, comp_a.seg_offsets, torch.arange(10, 30, dtype=torch.int64, device="cuda"), False),
                  (st_b, comp_b.seg_offsets, [3, 7, 11, 12], False), (st_c, comp_c.seg_offsets, [0, 5], True)]
    rows, total = wah.columns.select_rows(wah, predicates, n)
    assert total == want.size and np.array_equal(rows.cpu().numpy(), want)
    rows, total = wah.columns.select_rows(wah, predicates, n, first=500, limit=100)
    assert total == want.size and np.array_equal(rows.cpu().numpy(), want[500:600])


# ---- 4: refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_status_call(wah, cases):
    """Streams and tables the kernels are written to refuse before touching anything: a null index in a table row, an index range
    outside stream_words, a segment one group short, an empty fill.  The status is WAH_ERR_STREAM, and the positions call leaves
    its output alone."""
    import torch

    lib = wah.lib()
    n = 992 * 3 + 5
    _, good, want = cases(n)["uniform 0.3"]
    _, other, _ = cases(n)["clustered"]
    beyond = good[1].clone()
    beyond[-1] = good[0].numel() + 1
    short = _hand_stream([0x80000400, 0x800003FF], [0, 1, 2])          # n = 992 * 2: the second segment has 1023 groups
    empty = _hand_stream([0x80000400, 0x80000000, 0x80000400], [0, 1, 3])  # ... an empty fill in front of its 1024 groups
    for op, m in ((short, 992 * 2), (empty, 992 * 2)):
        assert int(op[0].numel()) == int(op[1][-1].item()) and sel.segments_of(m) + 1 == op[1].numel()
    refused = [("index range outside the stream", (good[0], beyond), n), ("a segment one group short", short, 992 * 2), ("an empty fill", empty, 992 * 2)]

    def count_status(table, m):
        sc = _scratch(wah, m, table.shape[0])
        counts = torch.empty(table.shape[0], dtype=torch.int64, device="cuda")
        wah.count_device(table, m, scratch=sc, counts=counts, check=False)
        return int(lib.wah_select_status(sc.data_ptr(), None)), counts

    # the table call: a good table first, then each refusal in the middle of good rows
    table = wah.bitop_operand_table([good, other, good])
    status, counts = count_status(table, n)
    assert status == 0 and counts.cpu().tolist() == [want.size, cases(n)["clustered"][2].size, want.size]
    null_index = table.clone()
    null_index[1, 2] = 0
    assert count_status(null_index, n)[0] == WAH_ERR_STREAM
    for what, op, m in refused:
        fine, fine_bits = (good, want.size) if m == n else (_hand_stream([0x80000400, 0xC0000400], [0, 1, 2]), sel.SEG_BITS)
        status, counts = count_status(wah.bitop_operand_table([fine, fine]), m)
        assert status == 0 and counts.cpu().tolist() == [fine_bits] * 2, what
        status, counts = count_status(wah.bitop_operand_table([fine, op, fine]), m)
        assert status == WAH_ERR_STREAM, what
        assert counts[0].item() == counts[2].item() == fine_bits, what  # the rows beside the refused one are counted all the same
        with pytest.raises(wah.WahError):
            wah.count_device([fine, op], m)

    # the positions call: status, output untouched, totals zero
    buf = torch.empty(64, dtype=torch.int64, device="cuda")
    info = torch.empty(2, dtype=torch.int64, device="cuda")
    for what, op, m in refused + [("a null index", (good[0], None), n)]:
        buf.fill_(SENTINEL)
        info.fill_(-1)
        sc = _scratch(wah, m)
        rc = lib.wah_positions_indexed_device(m, op[0].data_ptr(), op[0].numel(), op[1].data_ptr() if op[1] is not None else None, 0,
                                              buf.data_ptr() + 16, 40, info.data_ptr(), sc.data_ptr(), sc.numel(), None)
        assert rc == 0, what
        assert lib.wah_select_status(sc.data_ptr(), None) == WAH_ERR_STREAM, what
        assert bool((buf == SENTINEL).all()) and info.cpu().tolist() == [0, 0], what
    with pytest.raises(wah.WahError):
        wah.positions_device(good[0], beyond, n)


# ---- 5: graph replay ------------------------------------------------------------------------------------------------------------
def test_graph_replay_counts_the_new_selection(wah):
    """The table is only ever read by the device: ONE captured call, replayed after the table was overwritten in place, counts the
    new columns (capture as the list call's test: side stream, warm-up outside, check=False)."""
    import torch

    n_rows = 32 * 992 * 6
    n = n_rows // 32
    keys = np.random.default_rng(23).integers(0, 32, (2, n_rows)).min(axis=0)
    want = np.bincount(keys, minlength=32)
    assert len(set(want.tolist())) > 8
    _, comp, stream = _equality_index(wah, keys, 32)
    selections = [[0, 1, 2, 3, 4], [31, 30, 7, 7, 0], [9, 8, 3, 20, 25], [0, 1, 2, 3, 4]]
    table = torch.empty((5, 3), dtype=torch.int64, device="cuda:0")

    def write(ids):
        wah.columns.column_operand_table(stream, comp.seg_offsets, n, torch.tensor(ids, dtype=torch.int64, device="cuda:0"), out=table)

    write(selections[0])
    sc = _scratch(wah, n, 5)
    counts = torch.empty(5, dtype=torch.int64, device="cuda:0")
    wah.count_device(table, n, scratch=sc, counts=counts, check=False)  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            wah.count_device(table, n, scratch=sc, counts=counts, check=False)
    for ids in selections[1:]:
        write(ids)
        torch.cuda.synchronize()
        counts.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_select_status(sc.data_ptr(), None) == 0
        assert counts.cpu().tolist() == [int(want[i]) for i in ids], ids
