"""GPU tests of wah_count_masked_indexed_device (include/wah.h) and its front ends in api.py and columns.py.  Every comparison is
exact: counts against the popcount of the AND of the two bitmaps, or, for hand-built streams, of their groups (tests/_masked.py;
proven on the CPU by tests/test_masked_reference.py).  Shapes are the smallest that reach each switch of count_masked_kernel:
the load batches of both sides, the steps and the end of the mask image, mask segments of one fill, runs of triples that cross
operands and masks, bitmaps of one segment (the image is kept) and of several."""
import importlib

import numpy as np
import pytest

from tests import _masked as msk
from tests import _select as sel

pytestmark = pytest.mark.gpu

WAH_ERR_STREAM = -6
LENGTHS = [1, 30, 31, 32, 991, 992, 993, 2 * 992 + 5, 37 * 992 + 5]


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


def _bits(words, n):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32)[:n].view(np.uint8)).astype(np.int64)


def _ref_matrix(mask_words, op_words, n):
    """ref_counts for every pair, as one integer matrix product of the bitmaps' bits."""
    a = np.stack([_bits(w, n) for w in mask_words])
    b = np.stack([_bits(w, n) for w in op_words])
    return (a @ b.T).tolist()


@pytest.fixture(scope="module")
def cases(wah, oracle):
    """n -> (names, bitmaps, (stream, index) on the device, the matrix of all pairs): made once per length, shared, never changed."""
    made = {}

    def get(n):
        if n not in made:
            maps = sel.bitmaps(oracle, n)
            words = list(maps.values())
            made[n] = (list(maps), words, [_indexed_stream(wah, w) for w in words], _ref_matrix(words, words, n))
        return made[n]

    return get


def _scratch(wah, n, k=1):
    import torch

    return torch.empty(int(wah.lib().wah_select_scratch_bytes(n, k)), dtype=torch.uint8, device="cuda:0")


# ---- 1: lengths and kinds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_every_kind_as_mask_and_as_operand(wah, cases, n):
    names, words, ops, want = cases(n)
    assert len(ops) == 10 and want[1][1] == 32 * n and want[0] == [0] * 10
    for a in (2, 6, 9):  # the helper itself, pair by pair, on a few rows
        assert want[a] == [msk.ref_counts(words[a], w, n) for w in words]
    got = wah.count_masked_device(ops, ops, n)
    assert str(got.dtype) == "torch.int64" and tuple(got.shape) == (10, 10)
    assert got.cpu().tolist() == want
    # the diagonal is each bitmap's own count, the row of the all-ones mask the operands' counts
    assert [want[i][i] for i in range(10)] == want[1] == wah.count_device(ops, n).cpu().tolist()
    # one pair at a time, and a ragged table
    assert wah.count_masked_device([ops[6]], [ops[2]], n).cpu().tolist() == [[want[6][2]]]
    assert wah.count_masked_device(ops[2:5], ops[1:8], n).cpu().tolist() == [row[1:8] for row in want[2:5]]


def test_an_empty_bitmap_counts_nothing(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    counts = torch.full((2, 3), 77, dtype=torch.int64, device="cuda")
    got = wah.count_masked_device([(stream, offs)] * 2, [(stream, offs)] * 3, 0, counts=counts)
    assert got is counts and counts.cpu().tolist() == [[0, 0, 0], [0, 0, 0]]


def test_front_end_arguments(wah, cases):
    import torch

    n = 993
    _, _, ops, want = cases(n)
    masks, operands = wah.bitop_operand_table(ops[:3]), wah.bitop_operand_table(ops[3:8])
    sc, counts = _scratch(wah, n, 5), torch.full((3, 5), -1, dtype=torch.int64, device="cuda")
    got = wah.count_masked_device(masks, operands, n, scratch=sc, counts=counts, check=False)
    assert got is counts and wah.lib().wah_select_status(sc.data_ptr(), None) == 0
    assert counts.cpu().tolist() == [row[3:8] for row in want[:3]]
    with pytest.raises(wah.WahError):
        wah.count_masked_device(masks, operands, n, counts=torch.empty((5, 3), dtype=torch.int64, device="cuda"))
    with pytest.raises(wah.WahError):
        wah.count_masked_device(masks[:, :2], operands, n)
    with pytest.raises(wah.WahError):
        wah.count_masked_device([], operands, n)


# ---- 2: the load batches of both sides ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second_of_two", [False, True])
@pytest.mark.parametrize("fill_bit", [0, 1])
def test_segments_on_the_batch_edges(wah, oracle, fill_bit, second_of_two):
    """Mask segments of w and operand segments of v stream words, w and v around a load batch and around the tests of
    seg_load_words, every pair in one call; alone, and behind another segment."""
    rng = np.random.default_rng(40 + fill_bit)
    front = [oracle.gen_uniform(sel.SEG_WORDS, 77, 0.4)] if second_of_two else []
    n = sel.SEG_WORDS * (1 + len(front))
    mask_words = [np.concatenate(front + [sel.segment_of_words(w, rng, fill_bit)]) for w in sel.SEGMENT_WORD_EDGES]
    op_words = [np.concatenate(front + [sel.segment_of_words(v, rng, fill_bit)]) for v in sel.SEGMENT_WORD_EDGES]
    masks = [_indexed_stream(wah, w) for w in mask_words]
    ops = [_indexed_stream(wah, w) for w in op_words]
    for side in (masks, ops):
        assert [int(o[-1] - o[-2]) for _, o in side] == list(sel.SEGMENT_WORD_EDGES)
    want = _ref_matrix(mask_words, op_words, n)
    assert len({c for row in want for c in row}) > 40
    assert wah.count_masked_device(masks, ops, n).cpu().tolist() == want
    assert wah.count_masked_device(ops, masks, n).cpu().tolist() == [list(col) for col in zip(*want)]


# ---- 3: the steps and the end of the mask image ---------------------------------------------------------------------------------
def test_runs_on_the_image_edges(wah):
    """Hand-built operands: a zero-fill of a groups, a one-fill up to group a + b, zeros behind; a and a + b around a step of the
    image (64) and at its end (1024).  Under a mask of random literals and one of one-group one-fills and literals in turn."""
    rng = np.random.default_rng(31)
    n = sel.SEG_WORDS
    literal_mask = rng.integers(1, sel.M31, sel.SEG_GROUPS, dtype=np.uint64).astype(np.uint32)
    mask_streams = [literal_mask, msk.alternating_mask(rng)]
    op_streams = [msk.run_operand(a, ab - a) for a in msk.RUN_EDGES for ab in msk.RUN_EDGES if ab >= a]
    assert len(op_streams) == 15
    want = [[msk.stream_counts(m, o, n) for o in op_streams] for m in mask_streams]
    assert want[0][0] == 0 and len({c for row in want for c in row}) > 15
    masks, ops = [_hand_stream(m) for m in mask_streams], [_hand_stream(o) for o in op_streams]
    assert wah.count_masked_device(masks, ops, n).cpu().tolist() == want
    # the other way round: the runs are the masks (images of three words), the long streams the operands
    assert wah.count_masked_device(ops, masks, n).cpu().tolist() == [list(col) for col in zip(*want)]


# ---- 4: mask segments of one fill -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [992, 992 * 3, 992 * 3 + 5])
def test_masks_of_one_fill_per_segment(wah, cases, n):
    segs = sel.segments_of(n)
    rest = sel.groups_of(n) - sel.SEG_GROUPS * (segs - 1)
    zeros = np.array([sel.FILL | sel.SEG_GROUPS] * (segs - 1) + [sel.FILL | rest], np.uint32)
    ones = zeros | np.uint32(sel.ONE)  # (over the pad bits as well, where there are any)
    masks = [_hand_stream(zeros), _hand_stream(ones)]
    assert all(int(o.numel()) == segs + 1 and int(s.numel()) == segs for s, o in masks)
    if n not in (992, 992 * 3):
        names, words, ops, _ = cases(n)
    else:
        _, words5, _, _ = cases(992 * 3 + 5)
        words = [w[:n] for w in words5]
        ops = [_indexed_stream(wah, w) for w in words]
    own = [sel.ref_count(w, n) for w in words]
    assert wah.count_masked_device(masks, ops, n).cpu().tolist() == [[0] * len(ops), own]
    assert wah.count_device(ops, n).cpu().tolist() == own
    # a mask as its own operand: its count; the two trivial masks against each other
    assert wah.count_masked_device(masks, masks, n).cpu().tolist() == [[0, 0], [0, 32 * n]]
    for op, c in zip(ops, own):
        assert wah.count_masked_device([op], [op], n).cpu().tolist() == [[c]]


# ---- 5: the pad rule ------------------------------------------------------------------------------------------------------------
def test_pad_rule_on_the_device(wah):
    """Hand-built streams that set pad bits, as masks and as operands against the others of their length."""
    pads = sel.pad_streams()
    for n in sorted({n for _, n, _, _ in pads}):
        streams = [st for _, m, st, _ in pads if m == n]
        want = [[msk.stream_counts(a, b, n) for b in streams] for a in streams]
        assert [want[i][i] for i in range(len(streams))] == [bits for _, m, _, bits in pads if m == n]
        ops = [_hand_stream(st) for st in streams]
        assert wah.count_masked_device(ops, ops, n).cpu().tolist() == want, n


# ---- 6: runs that cross pairs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,n", [(3, 130, 36 * 992 + 5), (3, 4097, 992)])
def test_runs_that_cross_operands_and_masks(wah, oracle, m, k, n):
    """More triples than a full grid has wavefronts: a wavefront's run crosses operand and mask boundaries -- with 37 segments
    per bitmap inside operands, with one segment per bitmap over whole operands (and the mask image is kept from one triple to the
    next).  Rows repeat, and repeated rows give equal counts."""
    import torch

    assert m * k * sel.segments_of(n) > msk.GRID_WAVES
    maps = sel.bitmaps(oracle, n)
    words = list(maps.values())
    pool = [_indexed_stream(wah, w) for w in words]
    full = np.array(_ref_matrix(words, words, n))
    rng = np.random.default_rng(k)
    mask_ids = np.array([2, 6, 2])  # uniform 0.3, clustered, and the first again
    op_ids = rng.integers(0, len(pool), k)
    op_ids[-1] = op_ids[0]
    want = full[np.ix_(mask_ids, op_ids)]
    assert len(set(want.reshape(-1).tolist())) > 10
    got = wah.count_masked_device([pool[i] for i in mask_ids], [pool[j] for j in op_ids], n)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got[0], got[2]) and torch.equal(got[:, 0], got[:, -1])


@pytest.mark.parametrize("m,k,n_segments,chunk", [(16, 4097, 1, 2), (1, 70, 8200, 16), (2, 70, 33000, 64)])
def test_chunks_of_operands_under_one_image(wah, m, k, n_segments, chunk):
    """With eight items or more per wavefront of a full grid the launcher lets 2 .. 64 consecutive operands share a mask image,
    lane l of the wavefront keeping the l-th operand's count: chunks of 2 in bitmaps of one segment, of 16 and of 64 in hand-built
    bitmaps of thousands of one-word segments (they exist only compressed), each with a ragged last chunk.  The masks: marked
    segments (an image) among zero-fills, and one-fills throughout."""
    assert msk.chunk_of(m, k, n_segments) == chunk and k % chunk
    marks = [s for s in (0, 1, 5, n_segments // 2, n_segments - 2, n_segments - 1) if 0 <= s < n_segments]
    rng = np.random.default_rng(k)
    made = [sel.long_stream(n_segments, {s: (3 * s) % 31 for s in marks}),
            sel.long_stream(n_segments, {s: (3 * s) % 31 for s in marks[::2]}),
            sel.long_stream(n_segments, {s: (5 * s + 1) % 31 for s in marks[-3:]}),
            sel.long_stream(n_segments, {s: (3 * s) % 31 for s in marks[1:]})]
    n = made[0][0]
    ones = np.full(n_segments, sel.FILL | sel.ONE | sel.SEG_GROUPS, np.uint32)
    pool = [_hand_stream(st, index) for _, st, index, _ in made] + [_hand_stream(ones)]
    positions = [pos for _, _, _, pos in made] + [None]

    def shared(a, b):
        if positions[a] is None or positions[b] is None:
            return 32 * n if a == b else (positions[a] if positions[b] is None else positions[b]).size
        return int(np.intersect1d(positions[a], positions[b]).size)

    mask_ids = ([3, 4] * m)[:m]
    op_ids = rng.integers(0, 4, k)
    op_ids[:5] = [0, 1, 2, 3, 4]
    want = [[shared(a, b) for b in op_ids] for a in mask_ids]
    assert len({c for row in want for c in row}) >= 3
    got = wah.count_masked_device([pool[a] for a in mask_ids], [pool[b] for b in op_ids], n)
    assert got.cpu().tolist() == want


# ---- 7: end to end --------------------------------------------------------------------------------------------------------------
def _equality_index(wah, keys, n_bins):
    import torch

    cols = np.stack([np.packbits(keys == v, bitorder="little").view(np.uint32) for v in range(n_bins)])
    matrix = torch.from_numpy(cols.view(np.int32)).cuda()
    comp = wah.DeviceCompressor(matrix.numel(), indexed=True)
    stream, _ = wah.columns.compress_column_matrix(comp, matrix)
    return cols, comp, stream


def test_group_by_under_a_filter_and_cross_tab(wah):
    """SELECT b, COUNT(*) WHERE 3 <= a <= 9 AND c NOT IN (0, 5) GROUP BY b, and SELECT a, b, COUNT(*) GROUP BY a, b."""
    import torch

    n_rows = 32 * 992 * 5
    n = n_rows // 32
    rng = np.random.default_rng(17)
    a = rng.integers(0, 16, (2, n_rows)).min(axis=0)
    b = rng.integers(0, 24, (2, n_rows)).max(axis=0)
    c = rng.integers(0, 8, n_rows)
    (_, comp_a, st_a), (_, comp_b, st_b), (_, comp_c, st_c) = (_equality_index(wah, keys, bins) for keys, bins in ((a, 16), (b, 24), (c, 8)))
    chosen = (a >= 3) & (a <= 9) & ~np.isin(c, (0, 5))
    want = np.bincount(b[chosen], minlength=24)
    assert 1000 < chosen.sum() < n_rows // 2 and len(set(want.tolist())) > 15
    predicates = [(st_a, comp_a.seg_offsets, torch.arange(3, 10, dtype=torch.int64, device="cuda"), False), (st_c, comp_c.seg_offsets, [0, 5], True)]
    ids = torch.arange(24, dtype=torch.int64, device="cuda")  # device-resident: no host round trip between filter and count
    got = wah.columns.count_columns_where(wah, predicates, st_b, comp_b.seg_offsets, n, ids)
    assert str(got.dtype) == "torch.int64" and got.cpu().tolist() == want.tolist()
    result, result_offsets = wah.columns.filter_columns(wah, predicates, n)
    assert int(got.sum().item()) == int(chosen.sum()) == wah.count_device([(result, result_offsets)], n).cpu().tolist()[0]
    some = [23, 0, 7, 7]
    assert wah.columns.count_columns_where(wah, predicates, st_b, comp_b.seg_offsets, n, some).cpu().tolist() == [int(want[v]) for v in some]
    # the cross-tab
    table = np.zeros((16, 24), np.int64)
    np.add.at(table, (a, b), 1)
    got = wah.columns.crosstab_columns(wah, (st_a, comp_a.seg_offsets, list(range(16))), (st_b, comp_b.seg_offsets, ids), n)
    assert tuple(got.shape) == (16, 24) and np.array_equal(got.cpu().numpy(), table) and int(got.sum().item()) == n_rows
    got = wah.columns.crosstab_columns(wah, (st_b, comp_b.seg_offsets, [5, 5, 20]), (st_a, comp_a.seg_offsets, [15, 1]), n)
    assert np.array_equal(got.cpu().numpy(), table.T[np.ix_([5, 5, 20], [15, 1])])


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_status_call(wah, cases):
    """Rows and streams the kernel is written to refuse before it touches anything, each once in a mask row and once in an
    operand row: the status is WAH_ERR_STREAM, and a clean call behind it is accepted and right."""
    import torch

    lib = wah.lib()
    n = 992 * 2 + 5
    _, _, pool, full = cases(n)
    good, other = pool[2], pool[6]
    clean = wah.bitop_operand_table([good, other, good])
    want = [[full[a][b] for b in (2, 6, 2)] for a in (2, 6, 2)]
    beyond = good[1].clone()
    beyond[-1] = good[0].numel() + 1
    m2 = 992 * 2
    fine2 = _hand_stream([0x80000400, 0xC0000400], [0, 1, 2])
    short = _hand_stream([0x80000400, 0x800003FF], [0, 1, 2])              # the second segment has 1023 groups
    empty = _hand_stream([0x80000400, 0x80000000, 0x80000400], [0, 1, 3])  # ... an empty fill in front of its 1024 groups
    long_short = _hand_stream([0x80000400, 0x12345, 0x800003FE], [0, 1, 3])  # ... a literal and a fill: an image, one group short

    def status(masks, operands, m):
        sc = _scratch(wah, m, operands.shape[0])
        counts = wah.count_masked_device(masks, operands, m, scratch=sc, check=False)
        return int(lib.wah_select_status(sc.data_ptr(), None)), counts.cpu().tolist()

    def edited(row, column, value=None, add=0):
        t = clean.clone()
        t[row, column] = (int(t[row, column].item()) if value is None else value) + add
        return t

    rows = [("a null stream", edited(1, 0, 0)), ("a misaligned stream", edited(1, 0, add=2)), ("a null index", edited(1, 2, 0)),
            ("a misaligned index", edited(1, 2, add=4)), ("a length of 2^40", edited(1, 1, 1 << 40)),
            ("an index range outside the stream", wah.bitop_operand_table([good, (good[0], beyond), good]))]
    assert status(clean, clean, n) == (0, want)
    for what, table in rows:
        assert status(table, clean, n)[0] == WAH_ERR_STREAM, ("mask", what)
        assert status(clean, table, n)[0] == WAH_ERR_STREAM, ("operand", what)
        assert status(clean, clean, n) == (0, want), what
    clean2 = wah.bitop_operand_table([fine2, fine2])
    for what, op in (("a segment one group short", short), ("an empty fill", empty), ("an image one group short", long_short)):
        table = wah.bitop_operand_table([fine2, op])
        assert status(table, clean2, m2)[0] == WAH_ERR_STREAM, ("mask", what)
        assert status(clean2, table, m2)[0] == WAH_ERR_STREAM, ("operand", what)
        assert status(clean2, clean2, m2) == (0, [[sel.SEG_BITS] * 2] * 2), what
        with pytest.raises(wah.WahError):
            wah.count_masked_device([fine2, op], [fine2], m2)
    # under a mask of zeros the operand is still checked: the verdict does not depend on the data
    zeros2 = _hand_stream([0x80000400, 0x80000400], [0, 1, 2])
    assert status(wah.bitop_operand_table([zeros2]), wah.bitop_operand_table([fine2, short]), m2)[0] == WAH_ERR_STREAM
    assert status(wah.bitop_operand_table([zeros2]), clean2, m2) == (0, [[0, 0]])


# ---- 9: graph replay ------------------------------------------------------------------------------------------------------------
def test_graph_replay_counts_the_new_selection(wah):
    """Both tables are only ever read by the device: ONE captured call, replayed after the mask row and the operand table were
    overwritten in place, counts the new selection (a linear capture on a side stream, warm-up outside, check=False)."""
    import torch

    n_rows = 32 * 992 * 4
    n = n_rows // 32
    rng = np.random.default_rng(29)
    a = rng.integers(0, 8, n_rows)
    b = rng.integers(0, 32, (2, n_rows)).min(axis=0)
    (_, comp_a, st_a), (_, comp_b, st_b) = _equality_index(wah, a, 8), _equality_index(wah, b, 32)
    table = np.zeros((8, 32), np.int64)
    np.add.at(table, (a, b), 1)
    selections = [(0, [0, 1, 2, 3, 4]), (7, [31, 30, 7, 7, 0]), (3, [9, 8, 3, 20, 25]), (0, [0, 1, 2, 3, 4])]
    mask, operands = (torch.empty((k, 3), dtype=torch.int64, device="cuda:0") for k in (1, 5))

    def write(which, ids):
        wah.columns.column_operand_table(st_a, comp_a.seg_offsets, n, torch.tensor([which], dtype=torch.int64, device="cuda:0"), out=mask)
        wah.columns.column_operand_table(st_b, comp_b.seg_offsets, n, torch.tensor(ids, dtype=torch.int64, device="cuda:0"), out=operands)

    write(*selections[0])
    sc = _scratch(wah, n, 5)
    counts = torch.empty((1, 5), dtype=torch.int64, device="cuda:0")
    wah.count_masked_device(mask, operands, n, scratch=sc, counts=counts, check=False)  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            wah.count_masked_device(mask, operands, n, scratch=sc, counts=counts, check=False)
    for which, ids in selections[1:]:
        write(which, ids)
        torch.cuda.synchronize()
        counts.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_select_status(sc.data_ptr(), None) == 0
        assert counts.cpu().tolist() == [[int(table[which, j]) for j in ids]], (which, ids)
