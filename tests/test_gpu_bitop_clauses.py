"""GPU tests of wah_bitop_clauses_indexed_device: AND over clauses of (negated) ORs over operand lists that live in device
memory (include/wah.h), and its front ends in api.py and columns.py.  Everything is exact: the result's words, their count and
its segment index against compress() of the bitmap evaluated with numpy -- the CPU oracle and an indexed compress of it.

The queries come in three kinds: random ones over a pool of every kind of bitmap, the identities with the existing calls, and
the kernel's own switch points built deliberately (a clause end beside the 64-operand chunk, clauses whose operands are all
settled in the gather, batches of 128 words, ragged last groups under a negation).  For the headline queries the test first
asserts, with numpy alone, that every clause and every negate flag matters: a kernel that dropped a clause or ignored a flag
cannot pass."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6
M31 = 0x7FFFFFFF
NEG = -(1 << 63)
ONES = np.uint32(0xFFFFFFFF)


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


def _equal(a, b):
    """Two (stream, seg_offsets) results tensor for tensor."""
    return a[0].numel() == b[0].numel() and bool((a[0] == b[0]).all()) and bool((a[1] == b[1]).all())


# ---- the numpy model ----------------------------------------------------------------------------------------------------------
def evaluate(maps, query):
    """query: list of (indices into maps, negate).  NOT is over the 32 * n_words bits of the bitmap."""
    result = np.full(maps[0].shape, ONES, np.uint32)
    for ids, negate in query:
        clause = np.zeros(maps[0].shape, np.uint32)
        for i in sorted(set(ids)):
            clause |= maps[i]
        result &= ~clause if negate else clause
    return result


def assert_every_clause_and_flag_matters(maps, query, what):
    """The vacuity guard: the expected bitmap is neither all zeros nor all ones, and dropping any single clause or flipping any
    single negate flag changes it."""
    want = evaluate(maps, query)
    assert want.any() and not (want == ONES).all(), what
    for i in range(len(query)):
        if len(query) > 1:
            assert not np.array_equal(evaluate(maps, query[:i] + query[i + 1:]), want), (what, "clause", i, "does not matter")
        flipped = query[:i] + [(query[i][0], not query[i][1])] + query[i + 1:]
        assert not np.array_equal(evaluate(maps, flipped), want), (what, "flag", i, "does not matter")
    return want


KINDS = 8  # pool entry j is of kind j % 8: uniform 0.3, clustered, uniform 0.9, uniform 2^-10, clustered, uniform 2^-13, zeros, ones


def make_pool(oracle, n, size=48):
    maps = []
    for j in range(size):
        kind = j % KINDS
        if kind in (0, 2, 3, 5):
            maps.append(oracle.gen_uniform(n, 100 + j, {0: 0.3, 2: 0.9, 3: 2.0 ** -10, 5: 2.0 ** -13}[kind]))
        elif kind in (1, 4):
            maps.append(oracle.gen_clustered(n, 100 + j, 200 + (11800 * ((j * 7) % size)) // (size - 1)))
        elif kind == 6:
            maps.append(np.zeros(n, np.uint32))
        else:
            maps.append(np.full(n, 0xFFFFFFFF, np.uint32))
    return [np.ascontiguousarray(m, dtype=np.uint32) for m in maps]


def headline_query(n):
    """Five clauses in which every kind of bitmap has a part (pool indices: make_pool).  Bitmaps of a few words have no room for
    sparse or clustered operands to matter: there the clauses are dense ones."""
    if n < 992:
        return [([0, 8], False), ([16], True), ([34], False)]  # (density 0.3 | 0.3, NOT 0.3, 0.9)
    return [([3, 11, 5, 1, 9], False),        # sparse and clustered operands: a positive IN-list
            ([0, 8, 6], False),               # two of density 0.3 and an all-zeros operand
            ([19, 13, 27, 22], True),         # NOT IN: sparse operands and an all-zeros one
            ([2, 21], False),                 # density 0.9 | 2^-13
            ([4], True)]                      # a negated clustered operand


def random_query(rng, n_maps, flags):
    sizes = (1, 1, 2, 3, 5, 17, 63, 64, 65, 130)
    query = []
    for _ in range(int(rng.integers(1, 13))):
        kinds = rng.permutation(KINDS)[: int(rng.integers(1, 4))]  # a clause draws from one to three kinds of bitmap
        allowed = [j for j in range(n_maps) if j % KINDS in kinds]
        ids = [int(allowed[i]) for i in rng.integers(0, len(allowed), int(sizes[int(rng.integers(0, len(sizes)))]))]
        negate = {"random": bool(rng.integers(0, 2)), "none": False, "all": True}[flags]
        query.append((ids, negate))
    return query


def _run(wah, ops, query, n, **kw):
    return wah.bitop_clauses_indexed_device([([ops[i] for i in ids], negate) for ids, negate in query], n, **kw)


# ---- 1: random queries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [992 * 40 + 9, 7, 1, 992 * 257, 992 * 64 + 991])
def test_random_queries_vs_oracle(wah, oracle, n):
    """1 to 12 clauses of 1 to 130 operands of every kind, flags at random, none and all negated, at ragged lengths; first the
    headline query, whose every clause and flag is shown to matter before anything is launched."""
    maps = make_pool(oracle, n)
    head = headline_query(n)
    want = assert_every_clause_and_flag_matters(maps, head, ("headline", n))
    rng = np.random.default_rng(1000 + n)
    queries = [random_query(rng, len(maps), flags) for flags in ("random",) * 6 + ("none", "all")]
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    got, offs = _run(wah, ops, head, n)
    _same(wah, oracle, got, offs, want, ("headline", n))
    for q, query in enumerate(queries):
        got, offs = _run(wah, ops, query, n)
        _same(wah, oracle, got, offs, evaluate(maps, query), (n, q, [(len(ids), neg) for ids, neg in query]))
    # ... the same through a ready pair of tables
    table, ends = wah.bitop_clause_table([([ops[i] for i in ids], negate) for ids, negate in head])
    assert tuple(table.shape) == (sum(len(ids) for ids, _ in head), 3) and tuple(ends.shape) == (len(head),) and ends.is_cuda
    assert _equal(wah.bitop_clauses_indexed_device((table, ends), n), _run(wah, ops, head, n))


def test_empty_bitmap(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    got, out_offs = wah.bitop_clauses_indexed_device([([(stream, offs)] * 3, True), ([(stream, offs)], False)], 0)
    assert got.numel() == 0 and int(out_offs[0].item()) == 0


# ---- 2: the identities ----------------------------------------------------------------------------------------------------------
def test_identities_with_the_existing_calls(wah, oracle):
    n = 992 * 40 + 9
    maps = make_pool(oracle, n, 24)
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    for ids in ([3], [0, 1, 3, 4, 5, 6], list(range(24)) * 3, [11, 13, 19, 1, 9, 12] * 11):
        assert _equal(_run(wah, ops, [(ids, False)], n), wah.bitop_list_indexed_device("or", [ops[i] for i in ids], n)), ("or", ids)
    for ids in ([2], [2, 10, 7, 15], [2, 10, 18, 0, 7, 1, 15, 23, 2], [2, 7] * 40):
        assert _equal(_run(wah, ops, [([i], False) for i in ids], n), wah.bitop_list_indexed_device("and", [ops[i] for i in ids], n)), ("and", ids)
    for first, clauses in ((2, [[3]]), (0, [[3, 11, 1], [5]]), (10, [[4, 19], [13], [6, 21, 9] * 25]), (7, [[6], [12, 3]])):
        query = [([first], False)] + [(ids, True) for ids in clauses]
        flat = [first] + [i for ids in clauses for i in ids]
        assert _equal(_run(wah, ops, query, n), wah.bitop_list_indexed_device("andnot", [ops[i] for i in flat], n)), ("andnot", first, clauses)
    for i in (0, 1, 3, 6, 7):  # the complement of a compressed bitmap; twice: the bitmap's own stream and index
        once = _run(wah, ops, [([i], True)], n)
        _same(wah, oracle, once[0], once[1], ~maps[i], ("not", i))
        twice = wah.bitop_clauses_indexed_device([([(once[0].clone(), once[1].clone())], True)], n)
        assert _equal(twice, ops[i]), ("not not", i)


# ---- 3: several attributes ------------------------------------------------------------------------------------------------------
def _equality_index(wah, keys, n_bins):
    """The compressed equality-encoded index over keys: one bitmap per bin, all through compress_column_matrix."""
    import torch

    cols = np.stack([np.packbits(keys == v, bitorder="little").view(np.uint32) for v in range(n_bins)])
    matrix = torch.from_numpy(cols.view(np.int32)).cuda()
    comp = wah.DeviceCompressor(matrix.numel(), indexed=True)
    stream, _ = wah.columns.compress_column_matrix(comp, matrix)
    return cols, comp, stream


def _bitmap(mask):
    return np.packbits(mask, bitorder="little").view(np.uint32)


def test_filter_columns_over_three_attributes(wah, oracle):
    """`10 <= a <= 29 AND b IN (3, 7, 11, 12) AND c NOT IN (0, 5) AND a != 17` over three equality indexes of 64, 16 and 8 bins:
    one call; the expected bitmap from the keys."""
    import torch

    n_rows = 32 * 992 * 37
    n = n_rows // 32
    rng = np.random.default_rng(5)
    keys = [rng.integers(0, bins, n_rows) for bins in (64, 16, 8)]
    a_range, b_in, c_not, a_not = list(range(10, 30)), [3, 7, 11, 12], [0, 5], [17]
    # the guard, on the bins' bitmaps: one clause per predicate
    flat = [_bitmap(keys[0] == v) for v in a_range] + [_bitmap(keys[1] == v) for v in b_in] + [_bitmap(keys[2] == v) for v in c_not] + [_bitmap(keys[0] == 17)]
    query = [(list(range(0, 20)), False), (list(range(20, 24)), False), ([24, 25], True), ([26], True)]
    want = assert_every_clause_and_flag_matters(flat, query, "three attributes")
    mask = (keys[0] >= 10) & (keys[0] <= 29) & np.isin(keys[1], b_in) & ~np.isin(keys[2], c_not) & (keys[0] != 17)
    assert np.array_equal(want, _bitmap(mask))
    index = [_equality_index(wah, k, bins) for k, bins in zip(keys, (64, 16, 8))]
    (_, comp_a, st_a), (_, comp_b, st_b), (_, comp_c, st_c) = index
    predicates = [(st_a, comp_a.seg_offsets, torch.arange(10, 30, dtype=torch.int64, device="cuda"), False),  # device-resident numbers
                  (st_b, comp_b.seg_offsets, b_in, False), (st_c, comp_c.seg_offsets, c_not, True), (st_a, comp_a.seg_offsets, a_not, True)]
    got, offs = wah.columns.filter_columns(wah, predicates, n)
    _same(wah, oracle, got, offs, want, "three attributes")
    # a single positive bin AND a NOT IN, into tables that are reused
    tables = (torch.empty((4, 3), dtype=torch.int64, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda"))
    for b, c_out in ((5, [1, 2, 3]), (0, [7, 0, 4])):
        got, offs = wah.columns.filter_columns(wah, [(st_b, comp_b.seg_offsets, [b], False), (st_c, comp_c.seg_offsets, c_out, True)], n, tables=tables)
        _same(wah, oracle, got, offs, _bitmap((keys[1] == b) & ~np.isin(keys[2], c_out)), (b, c_out))
    assert tables[1].cpu().tolist() == [1, 4 + NEG]
    with pytest.raises(ValueError):
        wah.columns.filter_columns(wah, [], n)
    with pytest.raises(ValueError):
        wah.columns.filter_columns(wah, [(st_b, comp_b.seg_offsets, [16], False)], n)


# ---- 4: the kernel's switch points ----------------------------------------------------------------------------------------------
def pack(groups):
    """31-bit groups -> the bitmap's words: bit j of group g is bit 31 g + j of the bitmap, bit k of the bitmap is bit k % 32 of
    word k / 32.  The last word is zero padded."""
    g = np.ascontiguousarray(groups, dtype=np.uint32)
    assert not np.any(g >> 31)
    bits = ((g[:, None] >> np.arange(31, dtype=np.uint32)) & 1).astype(np.uint8).reshape(-1)
    pad = (-bits.size) % 32
    if pad:
        bits = np.concatenate([bits, np.zeros(pad, np.uint8)])
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def segment_of_words(words, rng, fill_bit=0):
    """992 bitmap words (1024 groups) that compress to exactly `words` words: words - 1 literals, then one fill (1024 words: a lone
    fill group behind 1023 literals)."""
    lit = rng.integers(1, M31, words - 1, dtype=np.uint64).astype(np.uint32)
    return pack(np.concatenate([lit, np.full(1024 - (words - 1), M31 if fill_bit else 0, np.uint32)]))


def test_clause_end_beside_the_chunk_of_64_operands(wah, oracle):
    """A clause end at operand 63, 64, 65 and 128 of the flattened table (the table is walked 64 operands at a time whatever the
    clauses are): the operands on both sides of the end are dense, so an end taken one operand early or late changes the result."""
    n = 992 * 5 + 100
    sparse = [oracle.gen_uniform(n, 300 + j, 2.0 ** -9) if j % 3 else oracle.gen_clustered(n, 300 + j, 700) for j in range(12)]
    dense = [oracle.gen_uniform(n, 400 + j, 0.3) for j in range(4)]
    maps = sparse + dense
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    for end in (63, 64, 65, 128):
        for flags in ((False, False), (False, True), (True, False)):
            first = [j % 12 for j in range(end - 1)] + [12]              # ... a dense operand last
            second = [13] + [(5 * j) % 12 for j in range(130 - end - 1)]  # a dense operand first ...
            query = [(first, flags[0]), (second, flags[1])]
            want = assert_every_clause_and_flag_matters(maps, query, (end, flags))
            for moved in (-1, 1):  # the same operands cut one place further on or back: another bitmap
                both = first + second
                assert not np.array_equal(evaluate(maps, [(both[: end + moved], flags[0]), (both[end + moved:], flags[1])]), want)
            got, offs = _run(wah, ops, query, n)
            _same(wah, oracle, got, offs, want, (end, flags))
    # a clause of exactly one chunk followed by a one-operand clause; and in front of it
    for query in ([([j % 12 for j in range(64)], False), ([13], False)], [([14], True), ([j % 12 for j in range(63)] + [15], False)],
                  [([j % 12 for j in range(64)], True), ([13], True)]):
        want = assert_every_clause_and_flag_matters(maps, query, "one chunk and one operand")
        got, offs = _run(wah, ops, query, n)
        _same(wah, oracle, got, offs, want, "one chunk and one operand")


def test_clauses_of_settled_operands(wah, oracle):
    """A clause all of whose operands are one-fill segments: zeros (settled while the chunk is gathered: never a batch) and ones
    (NOT settled under OR), positive and negated, first, in the middle, last, and alone; the fold happens all the same."""
    n = 992 * 6 + 50
    maps = [oracle.gen_uniform(n, 500, 0.4), oracle.gen_clustered(n, 501, 900), oracle.gen_uniform(n, 502, 2.0 ** -8),
            np.zeros(n, np.uint32), np.full(n, 0xFFFFFFFF, np.uint32)]
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    data = [([0, 1], False), ([2], True)]
    want_data = assert_every_clause_and_flag_matters(maps, data, "data clauses")
    zero, one = 3, 4
    for fill, negate, keeps in ((zero, True, True), (one, False, True), (zero, False, False), (one, True, False)):
        for size in (1, 3, 64, 70):
            extra = ([fill] * size, negate)
            for query in ([extra] + data, [data[0], extra, data[1]], data + [extra], [data[0], extra, extra, data[1], extra]):
                want = evaluate(maps, query)
                assert np.array_equal(want, want_data if keeps else np.zeros(n, np.uint32))
                got, offs = _run(wah, ops, query, n)
                _same(wah, oracle, got, offs, want, (fill, negate, size, len(query)))
        got, offs = _run(wah, ops, [([fill] * 2, negate)], n)  # alone: all ones or all zeros
        _same(wah, oracle, got, offs, np.full(n, 0xFFFFFFFF if keeps else 0, np.uint32), (fill, negate, "alone"))


def test_one_hundred_and_thirty_one_operand_clauses(wah, oracle):
    """130 clauses of one operand each -- three windows of the clause table, three chunks of the operand table, a fold per operand."""
    n = 992 * 4 + 17
    maps = [oracle.gen_uniform(n, 600 + j, 2.0 ** -7) for j in range(10)] + [oracle.gen_uniform(n, 620 + j, 0.9) for j in range(3)] + \
           [np.full(n, 0xFFFFFFFF, np.uint32), np.zeros(n, np.uint32)]
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    query = []
    for j in range(130):
        if j in (5, 64, 129):
            query.append(([10 + (j % 3)], False))      # density 0.9
        elif j % 7 == 0:
            query.append(([13], False))                # all ones, positive: no effect
        elif j % 11 == 0:
            query.append(([14], True))                 # all zeros, negated: no effect
        else:
            query.append(([j % 10], True))             # NOT sparse
    want = evaluate(maps, query)
    assert want.any() and not (want == ONES).all()
    for at in (5, 64, 129, 1, 63, 65, 127, 128):  # flags and clauses around the chunk and window ends matter
        flipped = query[:at] + [(query[at][0], not query[at][1])] + query[at + 1:]
        assert not np.array_equal(evaluate(maps, flipped), want), at
    got, offs = _run(wah, ops, query, n)
    _same(wah, oracle, got, offs, want, "130 clauses")


@pytest.mark.parametrize("words", [128, 129, 512, 513])
def test_operand_of_whole_batches(wah, oracle, words):
    """A clause whose operand has exactly 128 / 129 / 512 / 513 words in a segment (128 words a batch, four batches in flight),
    alone and negated, and beside other operands, with clause ends in front of and behind it."""
    rng = np.random.default_rng(words)
    n = 992 * 3
    probe = np.concatenate([segment_of_words(w, rng, bit) for w, bit in ((words, 0), (words, 1), (words, 0))])
    assert oracle.compress(probe).size == 3 * words
    maps = [probe, oracle.gen_uniform(n, 700, 0.5), oracle.gen_clustered(n, 701, 500), oracle.gen_uniform(n, 702, 0.2)]
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    for query in ([([0], True)], [([0], False)], [([1], False), ([0], True), ([2, 3], False)], [([3, 0], False), ([1], True)],
                  [([1, 2], False), ([0], False), ([0], True)], [([2], True), ([1, 0, 3], True)]):
        got, offs = _run(wah, ops, query, n)
        _same(wah, oracle, got, offs, evaluate(maps, query), (words, query))
    assert_every_clause_and_flag_matters(maps, [([1], False), ([0], True), ([2, 3], False)], words)


@pytest.mark.parametrize("n", [31, 30, 1, 992 * 3 + 30, 992 * 2 + 1, 992 + 31])
def test_ragged_lengths_under_negation(wah, oracle, n):
    """NOT is over the bitmap's 32 n bits: the last group's 31 G - 32 n spare bits (0 at n = 31, 1 at 30, 30 at 1; 992 k + 1: a
    last segment of two groups, the fewest a ragged length leaves) stay out of the result.  An all-negated query over operands
    without a set bit gives compress() of all ones, word for word; beside it, negations of operands with bits in the last word."""
    all_ones = np.full(n, 0xFFFFFFFF, np.uint32)
    rng = np.random.default_rng(n)
    last = np.zeros(n, np.uint32)
    last[-1] = 0x80000001
    maps = [np.zeros(n, np.uint32), last, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), all_ones]
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    for query in ([([0], True)], [([0, 0, 0], True), ([0], True)], [([0], True)] * 5):
        got, offs = _run(wah, ops, query, n)
        assert np.array_equal(_host(got), oracle.compress(all_ones)), (n, query)
        _same(wah, oracle, got, offs, all_ones, (n, query))
    for query in ([([1], True)], [([2], True)], [([2], True), ([1], True)], [([3], True)], [([3], False), ([0, 1], True)], [([0], True), ([2], False)]):
        got, offs = _run(wah, ops, query, n)
        _same(wah, oracle, got, offs, evaluate(maps, query), (n, query))


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------
def _status(wah, table, ends, n, **kw):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    sc = torch.empty(int(wah.lib().wah_bitop_clauses_scratch_bytes(n, table.shape[0], ends.shape[0])), dtype=torch.uint8, device="cuda:0")
    wah.bitop_clauses_indexed_device((table, ends), n, scratch=sc, check=False, **kw)
    return int(wah.lib().wah_bitop_clauses_status(sc.data_ptr(), n, table.shape[0], ends.shape[0], None))


def _ends(values):
    import torch

    return torch.tensor(values, dtype=torch.int64, device="cuda:0")


def test_refusals_come_from_the_status_call(wah, oracle):
    """What only the device sees -- a clause table that is not strictly increasing, has an empty clause, does not end at
    n_operands, points beyond it or carries a stray bit; a bad operand in any clause, also behind a clause that has already
    made the result all zeros; too small an output -- is reported, and nothing is followed before it was checked."""
    import torch

    n = 992 * 64
    maps = [oracle.gen_uniform(n, 1, 0.1), oracle.gen_clustered(n, 2, 4000), oracle.gen_uniform(n, 3, 2.0 ** -9), np.zeros(n, np.uint32),
            np.full(n, 0xFFFFFFFF, np.uint32)]
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    many = ops[:3] * 4
    table = wah.bitop_operand_table(many)
    assert _status(wah, table, _ends([4, 8, 12]), n) == 0
    assert _status(wah, table, _ends([4, 8 + NEG, 12 + NEG]), n) == 0
    for ends in ([8, 4, 12], [4, 4, 12], [4, 8, 11], [4, 8, 13], [4, 13, 12], [13, 14, 12], [0, 8, 12], [4, 8 + (1 << 62), 12], [4 + (1 << 40), 8, 12],
                 [4, 8, 12 + (1 << 24)], [4 + NEG, 8 + NEG + (1 << 33), 12], [12 + NEG + (1 << 31)], [11], [13], [0]):
        assert _status(wah, table, _ends(ends), n) == WAH_ERR_STREAM, [hex(e & ((1 << 64) - 1)) for e in ends]
    with pytest.raises(wah.WahError):
        wah.bitop_clauses_indexed_device((table, _ends([4, 4, 12])), n)
    # beyond the first 64 clauses: 130 one-operand clauses, one end wrong
    big = wah.bitop_operand_table((ops[:3] * 44)[:130])
    good = list(range(1, 131))
    assert _status(wah, big, _ends(good), n) == 0
    for at, value in ((100, 100), (129, 129), (129, 131), (64, 66), (70, 71 + (1 << 50))):
        ends = list(good)
        ends[at] = value
        assert _status(wah, big, _ends(ends), n) == WAH_ERR_STREAM, (at, value)
    # a bad operand in the first, a middle and the last clause
    bad = ops[0][1].clone()
    bad[3] += 1
    for at in (0, 5, 11):
        broken = list(many)
        broken[at] = (ops[0][0], bad)
        assert _status(wah, wah.bitop_operand_table(broken), _ends([4, 8 + NEG, 12]), n) == WAH_ERR_STREAM, at
        with pytest.raises(wah.WahError):
            wah.bitop_clauses_indexed_device([(broken[:4], False), (broken[4:8], True), (broken[8:], False)], n)
    # ... and BEHIND a clause that has already made the result all zeros: the verdict does not depend on the data
    for zeroing, flag in ((ops[3], 0), (ops[4], NEG)):
        for at in (1, 2, 70):
            broken = [zeroing] + (ops[:3] * 24)[:71]
            assert _status(wah, wah.bitop_operand_table(broken), _ends([1 + flag, 72]), n) == 0
            broken[at] = (ops[0][0], bad)
            assert _status(wah, wah.bitop_operand_table(broken), _ends([1 + flag, 72]), n) == WAH_ERR_STREAM, (flag, at)
    # a table entry without an index
    t = table.clone()
    t[7, 2] = 0
    assert _status(wah, t, _ends([4, 8, 12]), n) == WAH_ERR_STREAM
    # an output one word too small, for a result of many words: (0.1 | clustered) AND NOT sparse
    cap_table, cap_ends = wah.bitop_operand_table(ops[:3]), _ends([2, 3 + NEG])
    need = int(oracle.compress((maps[0] | maps[1]) & ~maps[2]).size)
    assert need > 64 * 100
    out, count, _ = wah.bitop_clauses_indexed_device((cap_table, cap_ends), n, check=False)
    torch.cuda.synchronize()
    assert int(count.item()) == need
    small = torch.full((need + 63,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert _status(wah, cap_table, cap_ends, n, out=small[:need]) == 0
    assert bool((small[:need] == out[:need]).all()) and bool((small[need:] == 0x5A5A5A5A).all())
    small.fill_(0x5A5A5A5A)
    assert _status(wah, cap_table, cap_ends, n, out=small[: need - 1]) == WAH_ERR_CAPACITY
    assert bool((small[need - 1:] == 0x5A5A5A5A).all())


# ---- 6: graph replay ------------------------------------------------------------------------------------------------------------
def test_graph_replay_with_another_query(wah, oracle):
    """Both tables are only ever read by the device: ONE captured call, replayed after both were overwritten in place with a query of
    the same counts -- other boundaries, other flags, other columns -- answers the new query (capture as the list call's test:
    side stream, warm-up outside, check=False; one chain of launches)."""
    import torch

    n_rows = 32 * 992 * 50
    n = n_rows // 32
    rng = np.random.default_rng(23)
    keys = rng.integers(0, 32, n_rows)
    cols, comp, stream = _equality_index(wah, keys, 32)
    # 12 operands in 3 clauses
    queries = [[(list(range(0, 9)), False), ([3, 17], True), ([5], True)],                        # key < 9 and not 5
               [([31], True), ([3, 17, 5, 22, 9, 30, 1, 12, 14, 28], False), ([9], True)],
               [([20, 21], True), ([22, 23, 24, 25, 26], True), ([27, 28, 29, 30, 31], True)],    # all negated
               [(list(range(4, 12)), False), ([8, 9, 10], False), ([9], True)]]
    table = torch.empty((12, 3), dtype=torch.int64, device="cuda:0")
    ends = torch.empty(3, dtype=torch.int64, device="cuda:0")

    def write(query):
        flat = [i for ids, _ in query for i in ids]
        assert len(flat) == 12 and len(query) == 3
        wah.columns.column_operand_table(stream, comp.seg_offsets, n, torch.tensor(flat, dtype=torch.int64, device="cuda:0"), out=table)
        ends.copy_(torch.tensor(list(np.cumsum([len(ids) for ids, _ in query]) + np.array([NEG if neg else 0 for _, neg in query])), dtype=torch.int64))

    write(queries[0])
    sc = torch.empty(int(wah.lib().wah_bitop_clauses_scratch_bytes(n, 12, 3)), dtype=torch.uint8, device="cuda:0")
    res = torch.empty(wah.max_compressed_words(n), dtype=torch.int32, device="cuda:0")
    res_offs = torch.zeros(n // 992 + 2, dtype=torch.int64, device="cuda:0")
    wah.bitop_clauses_indexed_device((table, ends), n, scratch=sc, out=res, out_offsets=res_offs, check=False)  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _, count, _ = wah.bitop_clauses_indexed_device((table, ends), n, scratch=sc, out=res, out_offsets=res_offs, check=False)
    for query in queries[1:] + queries[:2]:
        want = evaluate(list(cols), query)
        write(query)
        torch.cuda.synchronize()
        res.fill_(0x5A5A5A5A)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bitop_clauses_status(sc.data_ptr(), n, 12, 3, None) == 0
        c = int(count.item())
        _same(wah, oracle, res[:c], res_offs[: n // 992 + 1], want, query)


# ---- 7: the route on which nobody waits ---------------------------------------------------------------------------------------
def test_same_words_on_the_no_wait_route(wah, oracle, monkeypatch):
    """WAH_FORCE_FALLBACK=1 (read per call) sends the compress passes behind the combining kernel the no-wait way: same words, same index."""
    n = 992 * 70 + 333
    maps = make_pool(oracle, n)
    query = headline_query(n)
    want = assert_every_clause_and_flag_matters(maps, query, "no-wait route")
    ops = [_indexed_stream(wah, _dev(m)) for m in maps]
    normal = _run(wah, ops, query, n)
    normal = (normal[0].clone(), normal[1].clone())
    monkeypatch.setenv("WAH_FORCE_FALLBACK", "1")
    forced = _run(wah, ops, query, n)
    assert _equal(forced, normal)
    assert np.array_equal(_host(forced[0]), oracle.compress(want))
    monkeypatch.delenv("WAH_FORCE_FALLBACK")
    _same(wah, oracle, normal[0], normal[1], want, "no-wait route")
