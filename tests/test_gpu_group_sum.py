"""GPU tests of wah_group_sum_indexed_device (include/wah.h) and its front ends in api.py and columns.py.  Every comparison is
exact: the groups' row counts, the counts and the sums against the popcounts of the ANDed bitmaps, or, for hand-built streams, of
their groups (tests/_group.py; proven on the CPU by tests/test_group_reference.py).  Shapes are the smallest that reach each
switch of group_count_kernel: every kind of segment as filter, as group row and as operand, the three short cuts, the limits of
the conjunction, chunks of 2, 16 and 64 operands, runs that change group and chunk inside a wavefront and inside a workgroup,
and sums beyond 64 bits."""
import importlib

import numpy as np
import pytest

from tests import _group as grp
from tests import _masked as msk
from tests import _select as sel

pytestmark = pytest.mark.gpu

WAH_ERR_STREAM = -6
U64 = (1 << 64) - 1


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


def _scratch(wah, n, k=1):
    import torch

    return torch.empty(int(wah.lib().wah_select_scratch_bytes(n, k)), dtype=torch.uint8, device="cuda:0")


def _ints(result):
    """(group_rows, counts, sums) of a call as the references give them: nested lists of Python ints, a sum low + (high << 64)."""
    rows, counts, sums = result
    words = [[[int(v) & U64 for v in pair] for pair in group] for group in sums.cpu().tolist()]
    return rows.cpu().tolist(), counts.cpu().tolist(), [[low + (high << 64) for low, high in group] for group in words]


def _flat(groups):
    return [row for own in groups for row in own]


@pytest.fixture(scope="module")
def kinds(wah):
    """n -> (names, streams, their bitmaps, (stream, index) on the device) of tests/_group.kind_streams: made once per length."""
    made = {}

    def get(n):
        if n not in made:
            names, streams, indexes = grp.kind_streams(np.random.default_rng(100 + n), n)
            maps = [grp.bitmap_of_stream(st, n) for st in streams]
            made[n] = (names, streams, maps, [_hand_stream(st, ix) for st, ix in zip(streams, indexes)])
        return made[n]

    return get


# ---- 1: every kind in every role --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 992, 992 * 3 + 5])
def test_every_kind_as_filter_as_group_row_and_as_operand(wah, kinds, n):
    """Zero fill, one fill, literals, mixed and runs on the image's edges: each as the filter (F = 1), as one of two filters, as a
    group's only row and as one of its two, and as operand; with F = 0 as well.  In the longer bitmaps stream k holds kind k + s
    in segment s, so every segment of a conjunction meets another mix."""
    names, streams, maps, ops = kinds(n)
    k = len(ops)
    assert k == 14
    attr_bits = [7, 1, 6]
    seen = set()
    for r in (1, 2):
        own = [[g, (g + 3) % k][:r] for g in range(k)]
        for filters in [[]] + [[f] for f in range(k)] + [[f, (f + 5) % k] for f in range(k)]:
            want = grp.ref_group([maps[f] for f in filters], [[maps[x] for x in rows] for rows in own], maps, attr_bits, n)
            got = wah.group_sum_device([ops[f] for f in filters], _flat([[ops[x] for x in rows] for rows in own]), ops, attr_bits, n, rows_per_group=r)
            assert _ints(got) == want, (n, r, [names[f] for f in filters])
            seen.update(want[0])
    # (in the longer bitmaps no stream is one kind throughout: none is all ones)
    assert 0 in seen and (32 * n in seen or n > 992) and len(seen) > (4 if n == 5 else 20)
    # the stream level gives the same: the pad bits some of these streams set are not counted
    assert grp.stream_group([streams[2]], [[s] for s in streams], streams, attr_bits, n) == grp.ref_group([maps[2]], [[m] for m in maps], maps, attr_bits, n)
    rows, counts, sums = wah.group_sum_device(None, ops, ops, attr_bits, n)
    assert str(rows.dtype) == str(counts.dtype) == str(sums.dtype) == "torch.int64"
    assert tuple(rows.shape) == (k,) and tuple(counts.shape) == (k, k) and tuple(sums.shape) == (k, 3, 2)
    # with no filter and one row per group the counts are the masked count's, the rows the count call's
    assert counts.cpu().tolist() == wah.count_masked_device(ops, ops, n).cpu().tolist()
    assert rows.cpu().tolist() == wah.count_device(ops, n).cpu().tolist()


def test_an_empty_bitmap_sums_nothing(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    sums = torch.full((2, 2, 2), 77, dtype=torch.int64, device="cuda")
    rows, counts, got = wah.group_sum_device(None, [(stream, offs)] * 2, [(stream, offs)] * 3, [2, 1], 0, sums=sums)
    assert got is sums and _ints((rows, counts, sums)) == ([0, 0], [[0] * 3] * 2, [[0, 0]] * 2)


def test_front_end_arguments(wah, kinds):
    import torch

    n = 992
    _, _, maps, ops = kinds(n)
    filters, groups, operands = wah.bitop_operand_table(ops[2:4]), wah.bitop_operand_table(ops[4:10]), wah.bitop_operand_table(ops[1:6])
    want = grp.ref_group(maps[2:4], [maps[4:6], maps[6:8], maps[8:10]], maps[1:6], [4, 1], n)
    sc = _scratch(wah, n, 5)
    outs = [torch.full(shape, -1, dtype=torch.int64, device="cuda") for shape in ((3,), (3, 5), (3, 2, 2))]
    got = wah.group_sum_device(filters, groups, operands, [4, 1], n, rows_per_group=2, scratch=sc, group_rows=outs[0], counts=outs[1], sums=outs[2], check=False)
    assert all(a is b for a, b in zip(got, outs)) and wah.lib().wah_select_status(sc.data_ptr(), None) == 0
    assert _ints(got) == want
    for bad in (dict(rows_per_group=4), dict(rows_per_group=0), dict(counts=torch.empty((5, 3), dtype=torch.int64, device="cuda")),
                dict(sums=torch.empty((3, 2), dtype=torch.int64, device="cuda")), dict(group_rows=torch.empty(3, dtype=torch.int32, device="cuda"))):
        with pytest.raises(wah.WahError):
            wah.group_sum_device(filters, groups, operands, [4, 1], n, **{"rows_per_group": 2, **bad})
    for bits in ([4, 2], [6], [], [0, 5], [65]):
        with pytest.raises(wah.WahError):
            wah.group_sum_device(filters, groups, operands, bits, n, rows_per_group=2)
    with pytest.raises(wah.WahError):
        wah.group_sum_device(filters[:, :2], groups, operands, [4, 1], n, rows_per_group=2)


# ---- 2: the limits of the conjunction ---------------------------------------------------------------------------------------------
def test_sixty_four_filters_and_eight_rows_per_group(wah):
    """F = 64 and R = 8 on one segment: 72 conjuncts ANDed into one image.  Each is 98 % ones, so a quarter of the bits survive;
    every eighth filter is a one-fill and is skipped, and the first conjunct of all is one as well."""
    rng = np.random.default_rng(64)
    n = sel.SEG_WORDS

    def dense():
        bits = rng.random((sel.SEG_GROUPS, 31)) < 0.98
        return (bits.astype(np.uint64) << np.arange(31, dtype=np.uint64)).sum(axis=1).astype(np.uint32)

    filters = [grp.fill_segment(True) if f % 8 == 0 else dense() for f in range(64)]
    groups = [[dense() for _ in range(8)], [dense() for _ in range(7)] + [grp.fill_segment(True)], [dense() for _ in range(7)] + [grp.fill_segment(False)]]
    operands = [grp.literal_segment(rng), grp.mixed_segment(rng), grp.fill_segment(True), msk.run_operand(63, 2)]
    want = grp.stream_group(filters, groups, operands, [3, 1], n)
    assert 0.15 * 32 * n < want[0][0] < 0.35 * 32 * n and want[0][1] > want[0][0] and want[0][2] == 0 and want[1][0][2] == want[0][0]
    got = wah.group_sum_device([_hand_stream(s) for s in filters], [_hand_stream(s) for s in _flat(groups)], [_hand_stream(s) for s in operands], [3, 1], n, rows_per_group=8)
    assert _ints(got) == want


# ---- 3: the short cuts, one test each ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def segment(wah):
    """One segment of each kind a short cut tells apart, on the device, with their bitmaps' reference."""
    rng = np.random.default_rng(33)
    streams = {"zeros": grp.fill_segment(False), "ones": grp.fill_segment(True), "a": grp.literal_segment(rng), "b": grp.literal_segment(rng),
               "mixed": grp.mixed_segment(rng), "run": msk.run_operand(64, 959)}
    return streams, {name: _hand_stream(st) for name, st in streams.items()}


def _short_cut(wah, segment, filters, groups, rows_per_group):
    streams, dev = segment
    operands = ["a", "mixed", "run", "ones", "zeros"]
    own = [groups[i: i + rows_per_group] for i in range(0, len(groups), rows_per_group)]
    want = grp.stream_group([streams[x] for x in filters], [[streams[x] for x in rows] for rows in own], [streams[x] for x in operands], [3, 2], sel.SEG_WORDS)
    got = wah.group_sum_device([dev[x] for x in filters], [dev[x] for x in groups], [dev[x] for x in operands], [3, 2], sel.SEG_WORDS, rows_per_group=rows_per_group)
    assert _ints(got) == want
    return want


def test_a_zero_fill_group_row_under_an_image_filter(wah, segment):
    rows, counts, sums = _short_cut(wah, segment, ["a"], ["zeros", "b"], 1)
    assert rows[0] == 0 and counts[0] == [0] * 5 and sums[0] == [0, 0] and rows[1] > 0


def test_a_zero_fill_filter_over_image_group_rows(wah, segment):
    rows, counts, _ = _short_cut(wah, segment, ["zeros"], ["a", "b", "mixed"], 1)
    assert rows == [0, 0, 0] and counts == [[0] * 5] * 3


def test_all_conjuncts_one_fills_take_the_ones_route_with_the_pad_rule(wah):
    """n = 993: a last segment of two groups, 30 pad bits, under one-fills that cover them -- as filter, as both rows of the
    group, and in the operands."""
    n = 993
    pads = {what: st for what, m, st, _ in sel.pad_streams() if m == n}
    ones, last = pads["n = 993: a last segment of two groups under a one-fill"], pads["n = 993: zeros, then a last literal of pad bits and one real bit"]
    rng = np.random.default_rng(9)
    lit = np.concatenate([grp.literal_segment(rng), [sel.M31, sel.M31]]).astype(np.uint32)  # literals that set every pad bit
    operands = [ones, last, lit]
    want = grp.stream_group([ones], [[ones, ones]], operands, [2, 1], n)
    assert want[0] == [32 * n] and want[1][0][0] == 32 * n and want[1][0][1] == 1
    assert want[1][0][2] == sel.stream_count(lit, n) < int(np.unpackbits(lit.view(np.uint8)).sum())
    got = wah.group_sum_device([_hand_stream(ones)], [_hand_stream(ones)] * 2, [_hand_stream(s) for s in operands], [2, 1], n, rows_per_group=2)
    assert _ints(got) == want


def test_a_one_fill_conjunct_between_two_image_conjuncts(wah, segment):
    rows, _, _ = _short_cut(wah, segment, ["a", "ones"], ["b", "mixed"], 1)
    streams = segment[0]
    assert rows[0] == msk.stream_counts(streams["a"], streams["b"], sel.SEG_WORDS) > 0


def test_a_first_conjunct_that_is_a_one_fill(wah, segment):
    """The first STORE into the image comes from a later conjunct: behind a one-fill filter, and behind a one-fill first row of
    the group when there is no filter."""
    streams = segment[0]
    rows, _, _ = _short_cut(wah, segment, ["ones", "a"], ["b", "run"], 1)
    assert rows[0] == msk.stream_counts(streams["a"], streams["b"], sel.SEG_WORDS)
    rows, _, _ = _short_cut(wah, segment, [], ["ones", "a", "ones", "ones", "ones", "mixed"], 2)
    assert rows == [sel.stream_count(streams["a"], sel.SEG_WORDS), sel.SEG_BITS, sel.stream_count(streams["mixed"], sel.SEG_WORDS)]


# ---- 4: the pad rule --------------------------------------------------------------------------------------------------------------
def test_pad_rule_in_every_role(wah):
    """Hand-built streams that set pad bits, each as the filter, as a group row and as an operand against the others of their
    length: neither group_rows nor any count sees those bits."""
    pads = sel.pad_streams()
    for n in sorted({n for _, n, _, _ in pads}):
        streams = [st for _, m, st, _ in pads if m == n]
        dev = [_hand_stream(st) for st in streams]
        bits = [1] * len(streams)
        for f, filt in enumerate(streams):
            want = grp.stream_group([filt], [[s] for s in streams], streams, bits, n)
            assert want[0][f] == sel.stream_count(filt, n) == want[1][f][f]
            assert _ints(wah.group_sum_device([dev[f]], dev, dev, bits, n)) == want, (n, f)
        want = grp.stream_group([], [[s, s] for s in streams], streams, bits, n)
        assert want[0] == [b for _, m, _, b in pads if m == n]
        assert _ints(wah.group_sum_device(None, _flat([[d, d] for d in dev]), dev, bits, n, rows_per_group=2)) == want, n


# ---- 5: chunks and attributes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,attr_bits", [(65, [55, 10]), (130, [55, 20, 55])])
def test_more_operands_than_a_wavefront_has_lanes(wah, kinds, k, attr_bits):
    """K = 65 and K = 130 on one segment: the second and third chunk of 64, whatever chunk the launcher takes."""
    n = 992
    _, _, maps, ops = kinds(n)
    op_ids = np.random.default_rng(k).integers(0, len(ops), k)
    own = [[2, 3], [3, 12], [1, 1]]
    want = grp.ref_group([maps[5]], [[maps[x] for x in rows] for rows in own], [maps[j] for j in op_ids], attr_bits, n)
    assert max(s for group in want[2] for s in group) >= 1 << 64
    got = wah.group_sum_device([ops[5]], _flat([[ops[x] for x in rows] for rows in own]), [ops[j] for j in op_ids], attr_bits, n, rows_per_group=2)
    assert _ints(got) == want


@pytest.mark.parametrize("g,k,n_segments,chunk,attr_bits", [(16, 4095, 1, 2, [64] * 63 + [63]), (1, 70, 8200, 16, [55, 15]), (2, 70, 33000, 64, [55, 15]),
                                                            (2, 130, 33000, 64, [55, 20, 55])])
def test_chunks_of_operands_under_one_image(wah, g, k, n_segments, chunk, attr_bits):
    """The launcher's chunks of 2, 16 and 64 consecutive operands under one image, each with a ragged last chunk, at the shapes of
    the masked count's test with the groups in the masks' place (4095 operands for its 4097: 64 attributes of 64 slices are 4096
    at the most) -- and 130 operands in chunks of 64, where a 20-bit attribute that starts at operand 55 crosses a chunk.  Hand-built
    bitmaps of thousands of one-word segments (they exist only compressed); the conjunctions: marked segments (an image) among
    zero-fills, one-fills throughout (the ones route), and the two ANDed."""
    assert grp.chunk_of(g, k, n_segments) == chunk and k % chunk and sum(attr_bits) == k
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

    def both(a, b):  # the rows two bitmaps share: None stands for all of them
        return b if a is None else a if b is None else np.intersect1d(a, b)

    def size(p):
        return 32 * n if p is None else int(p.size)

    own = ([[3, 4], [4, 4], [0, 3]] * g)[:g]  # an image under a one-fill, one-fills only, two images
    op_ids = rng.integers(0, 5, k)
    op_ids[:5] = [0, 1, 2, 3, 4]
    conj = [both(positions[4], both(positions[a], positions[b])) for a, b in own]
    counts = [[size(both(c, positions[j])) for j in op_ids] for c in conj]
    want = ([size(c) for c in conj], counts, [grp.fold(row, attr_bits) for row in counts])
    assert len({c for row in counts for c in row}) >= 3
    got = wah.group_sum_device([pool[4]], _flat([[pool[a], pool[b]] for a, b in own]), [pool[j] for j in op_ids], attr_bits, n, rows_per_group=2)
    assert _ints(got) == want


# ---- 6: runs that change group and chunk ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,k,n", [(3, 130, 36 * 992 + 5), (4097, 2, 992)])
def test_runs_that_change_group_and_chunk(wah, oracle, g, k, n):
    """More items than a full grid has wavefronts: a wavefront's run, and a workgroup's four, change (group, chunk) -- with 37
    segments per bitmap inside a group's chunks, with one segment per bitmap over whole groups (three per wavefront).  The groups'
    own row counts are exact there too: counted once, not once per chunk."""
    per, _ = grp.runs_of(g, k, sel.segments_of(n))
    assert g * k * sel.segments_of(n) > msk.GRID_WAVES and grp.chunk_of(g, k, sel.segments_of(n)) == 1 and per > 1
    maps = sel.bitmaps(oracle, n)
    words = list(maps.values())
    pool = [_indexed_stream(wah, w) for w in words]
    rng = np.random.default_rng(k)
    own = rng.integers(1, len(pool), (g, 2))
    own[0], own[-1] = [2, 6], [2, 6]  # uniform 0.3 AND clustered, first and last
    op_ids = rng.integers(0, len(pool), k)
    attr_bits = [55, 20, 55] if k == 130 else [2]
    filt = 3  # uniform 0.9
    made = {}
    for a, b in {(int(a), int(b)) for a, b in own}:
        conj = words[filt][:n] & words[a][:n] & words[b][:n]
        made[a, b] = (sel.ref_count(conj, n), [msk.ref_counts(conj, w, n) for w in words])
    want_rows = [made[int(a), int(b)][0] for a, b in own]
    want_counts = [[made[int(a), int(b)][1][j] for j in op_ids] for a, b in own]
    want = (want_rows, want_counts, [grp.fold(row, attr_bits) for row in want_counts])
    assert len(set(want_rows)) > (1 if g == 3 else 10)
    got = _ints(wah.group_sum_device([pool[filt]], [pool[x] for x in own.reshape(-1)], [pool[j] for j in op_ids], attr_bits, n, rows_per_group=2))
    assert got[0] == want[0]
    assert got == want and got[1][0] == got[1][-1]


# ---- 7: the 128-bit fold ----------------------------------------------------------------------------------------------------------
def test_a_sum_beyond_64_bits(wah):
    """One attribute of 64 slices, every one a one-fill over 992 words: 31 744 * (2^64 - 1), the high word not 0."""
    ones = _hand_stream(grp.fill_segment(True))
    rows, counts, sums = wah.group_sum_device(None, [ones], [ones] * 64, [64], sel.SEG_WORDS)
    assert rows.cpu().tolist() == [sel.SEG_BITS] and counts.cpu().tolist() == [[sel.SEG_BITS] * 64]
    low, high = (int(v) & U64 for v in sums.cpu().tolist()[0][0])
    assert (low, high) == grp.split128(sel.SEG_BITS * U64) and high == sel.SEG_BITS - 1
    assert _ints((rows, counts, sums))[2] == [[31744 * ((1 << 64) - 1)]]


def test_attributes_of_one_bit(wah, kinds):
    n = 992
    _, _, maps, ops = kinds(n)
    want = grp.ref_group([], [[maps[2]], [maps[3]]], [maps[3]], [1], n)
    assert _ints(wah.group_sum_device(None, [ops[2], ops[3]], [ops[3]], [1], n)) == want and want[2] == [[c] for (c,) in want[1]]
    ids = [j % len(ops) for j in range(64)]
    want = grp.ref_group([maps[2]], [[maps[3]], [maps[1]]], [maps[j] for j in ids], [1] * 64, n)
    got = _ints(wah.group_sum_device([ops[2]], [ops[3], ops[1]], [ops[j] for j in ids], [1] * 64, n))
    assert got == want and got[2] == got[1] and len(set(got[1][0])) > 8


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_status_call(wah):
    """A corrupt segment -- the second of two, one group short -- in a filter row, in a group row, in an operand row that lies
    under a zero conjunction and in a conjunct behind a zero-fill conjunct: WAH_ERR_STREAM each time, and a clean call behind it
    is accepted and right.  The verdict does not depend on the data."""
    lib = wah.lib()
    n = 992 * 2
    fine = _hand_stream([0x80000400, 0xC0000400], [0, 1, 2])
    zeros = _hand_stream([0x80000400, 0x80000400], [0, 1, 2])
    short = _hand_stream([0x80000400, 0x800003FF], [0, 1, 2])              # the second segment has 1023 groups
    long_short = _hand_stream([0x80000400, 0x12345, 0x800003FE], [0, 1, 3])  # ... a literal and a fill: an image, one group short

    def status(filters, groups, operands, rows_per_group=1):
        sc = _scratch(wah, n, len(operands))
        got = wah.group_sum_device(filters, groups, operands, [len(operands)], n, rows_per_group=rows_per_group, scratch=sc, check=False)
        return int(lib.wah_select_status(sc.data_ptr(), None)), _ints(got)

    clean = (0, ([sel.SEG_BITS], [[sel.SEG_BITS, 0]], [[2 * sel.SEG_BITS]]))
    assert status([fine], [fine], [fine, zeros]) == clean
    for bad in (short, long_short):
        assert status([bad], [fine], [fine, zeros])[0] == WAH_ERR_STREAM           # a filter row
        assert status([fine, bad], [fine], [fine, zeros])[0] == WAH_ERR_STREAM
        assert status([fine], [bad], [fine, zeros])[0] == WAH_ERR_STREAM           # a group row
        assert status([fine], [fine, bad], [fine, zeros], 2)[0] == WAH_ERR_STREAM
        assert status([zeros], [fine], [fine, bad])[0] == WAH_ERR_STREAM           # an operand under a zero conjunction
        assert status([fine], [zeros], [bad, fine])[0] == WAH_ERR_STREAM
        assert status([zeros], [bad], [fine, zeros])[0] == WAH_ERR_STREAM          # a conjunct behind a zero-fill conjunct
        assert status([zeros, bad], [fine], [fine, zeros])[0] == WAH_ERR_STREAM
        assert status(None, [zeros, bad], [fine, zeros], 2)[0] == WAH_ERR_STREAM
        assert status([fine], [fine], [fine, zeros]) == clean
        with pytest.raises(wah.WahError):
            wah.group_sum_device([fine], [bad], [fine], [1], n)
    assert status([zeros], [fine], [fine, zeros]) == (0, ([0], [[0, 0]], [[0]]))
    # rows the kernel refuses before it follows a pointer of them
    table = wah.bitop_operand_table([fine])
    for column, value in ((0, 0), (0, int(table[0, 0].item()) + 2), (2, 0), (2, int(table[0, 2].item()) + 4), (1, 1 << 40)):
        broken = table.clone()
        broken[0, column] = value
        for where in range(3):
            tables = [broken if where == role else table for role in range(3)]
            sc = _scratch(wah, n)
            wah.group_sum_device(tables[0], tables[1], tables[2], [1], n, scratch=sc, check=False)
            assert int(lib.wah_select_status(sc.data_ptr(), None)) == WAH_ERR_STREAM, (column, value, where)


# ---- 9: graph replay --------------------------------------------------------------------------------------------------------------
def test_graph_replay_sums_the_new_selection(wah, kinds):
    """The tables are only ever read by the device: ONE captured call, replayed after the filter row was overwritten in place,
    sums the new selection (a linear capture on a side stream, warm-up outside, check=False)."""
    import torch

    n = 992 * 3 + 5
    _, _, maps, ops = kinds(n)
    own = [[2, 3], [3, 12], [1, 1]]
    attr_bits = [7, 1, 6]
    groups, operands = wah.bitop_operand_table(_flat([[ops[x] for x in rows] for rows in own])), wah.bitop_operand_table(ops)
    filt = wah.bitop_operand_table([ops[5]])
    sc = _scratch(wah, n, len(ops))
    outs = dict(group_rows=torch.empty(3, dtype=torch.int64, device="cuda:0"), counts=torch.empty((3, len(ops)), dtype=torch.int64, device="cuda:0"),
                sums=torch.empty((3, 3, 2), dtype=torch.int64, device="cuda:0"))
    wah.group_sum_device(filt, groups, operands, attr_bits, n, rows_per_group=2, scratch=sc, check=False, **outs)  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            wah.group_sum_device(filt, groups, operands, attr_bits, n, rows_per_group=2, scratch=sc, check=False, **outs)
    seen = []
    for f in (7, 0, 1, 3, 5):
        filt.copy_(wah.bitop_operand_table([ops[f]]))
        torch.cuda.synchronize()
        for t in outs.values():
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_select_status(sc.data_ptr(), None) == 0
        want = grp.ref_group([maps[f]], [[maps[x] for x in rows] for rows in own], maps, attr_bits, n)
        assert _ints((outs["group_rows"], outs["counts"], outs["sums"])) == want, f
        seen.append(want[2])
    assert len({str(s) for s in seen}) == 5


# ---- 10: end to end ---------------------------------------------------------------------------------------------------------------
def test_aggregate_and_extremes_end_to_end(wah):
    """SELECT a, b, COUNT(*), SUM(x), SUM(y), COUNT(y), MIN(y), MAX(y) WHERE lo <= x <= hi GROUP BY a, b over 100 000 rows: the
    one call equals the value model and the road through one filter_columns per group and sum_column_where; the rows of a = 2 lie
    below the range, so the filter empties its groups."""
    import torch

    rows = 100_000
    rng = np.random.default_rng(21)
    a, b = rng.integers(0, 3, rows), rng.integers(0, 2, rows)
    x, y = rng.integers(0, 1 << 12, rows), rng.integers(0, 1 << 20, rows)
    lo, hi = 300, 3500
    x[a == 2] = rng.integers(0, lo, int((a == 2).sum()))
    y_exists = rng.random(rows) < 0.7
    chosen = (x >= lo) & (x <= hi)
    cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64)).cuda()  # noqa: E731
    st_a, offs_a, n = wah.columns.index_from_keys(wah, cuda(a), 3)
    st_b, offs_b, _ = wah.columns.index_from_keys(wah, cuda(b), 2)
    bsi_x = wah.columns.bsi_from_values(wah, cuda(x), 12)
    bsi_y = wah.columns.bsi_from_values(wah, cuda(y), 20, exists=torch.from_numpy(y_exists).cuda())
    assert n == 992 * 4 == bsi_x[2] == bsi_y[2]
    where = wah.columns.range_column(wah, bsi_x, lo, hi)
    keys = [(st_a, offs_a, [0, 1, 2]), (st_b, offs_b, torch.arange(2, dtype=torch.int64, device="cuda"))]
    got = wah.columns.aggregate_columns(wah, keys, [bsi_x, bsi_y], n, where=where)
    want_rows, want_sums, want_counts = grp.value_model([a, b], [3, 2], [(x, None), (y, y_exists)], chosen)
    assert want_rows[2] == [0, 0] and min(want_rows[0] + want_rows[1]) > 1000
    assert str(got["rows"].dtype) == "torch.int64" and tuple(got["rows"].shape) == (3, 2) and got["rows"].cpu().tolist() == want_rows
    assert [s.tolist() for s in got["sums"]] == want_sums and all(isinstance(v, int) for v in got["sums"][1].reshape(-1))
    assert [c.cpu().tolist() for c in got["counts"]] == want_counts and got["counts"][0] is got["rows"]
    # where as a list, no where at all, one key
    assert wah.columns.aggregate_columns(wah, keys, [bsi_y], n, where=[where, where])["sums"][0].tolist() == want_sums[1]
    every = grp.value_model([a], [3], [(x, None)], np.ones(rows, bool))
    alone = wah.columns.aggregate_columns(wah, keys[:1], [bsi_x], n)
    assert alone["rows"].cpu().tolist() == every[0] and alone["sums"][0].tolist() == every[1][0] and sum(every[0]) == rows
    # the road there was before: one filter_columns per group, then sum_column_where
    for i in range(3):
        for j in range(2):
            mask = wah.columns.filter_columns(wah, [(where[0], where[1], [0], False), (st_a, offs_a, [i], False), (st_b, offs_b, [j], False)], n)
            assert wah.columns.sum_column_where(wah, bsi_x, *mask) == got["sums"][0][i, j]
            assert wah.columns.sum_column_where(wah, bsi_y, *mask) == got["sums"][1][i, j]
            assert wah.count_device([mask], n).cpu().tolist() == [want_rows[i][j]]
    # grouped MIN / MAX
    low, high = wah.columns.extremes_by(wah, keys, bsi_y, n, where=where)
    assert low.shape == high.shape == (3, 2)
    for i in range(3):
        for j in range(2):
            mine = y[chosen & y_exists & (a == i) & (b == j)]
            assert (low[i, j], high[i, j]) == ((int(mine.min()), int(mine.max())) if mine.size else (None, None)), (i, j)
    assert low[2, 0] is None and high[2, 1] is None and low[0, 0] is not None
    low, high = wah.columns.extremes_by(wah, keys[1:], bsi_x, n)
    beyond = 32 * n - rows  # the column's rows behind the table's belong to no group
    assert beyond > 0 and [(low[j], high[j]) for j in range(2)] == [(int(x[b == j].min()), int(x[b == j].max())) for j in range(2)]
