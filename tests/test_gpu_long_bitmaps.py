"""GPU tests of the indexed calls (include/wah.h) on bitmaps of more than 2^32 rows, which exist only compressed: a constant
segment is one fill word, so a bitmap of 4.3e9 rows is 135 400 words and an index of 1 MB.  Everything is exact, against the
segment-sparse model of tests/_long.py, which tests/test_long_reference.py proves on the CPU against the dense models of the
other helper modules and whose named rows, counts, sums and ranks it shows to lie beyond 2^31 / 2^32 / 2^36 where a name here
says so.  No bitmap of these sizes is ever decoded or allocated, on the host or on the device; results that are streams are
compared on the device (torch.equal with the uploaded expectation), guard word behind every output.

Two sizes (tests/_long.py):
  A = 135 400 segments, 4 298 137 600 rows: row 2^31 is bit 2048 of segment 67 650, row 2^32 bit 4096 of segment 135 300;
  B = 4 330 000 segments, 1.37e11 rows: 4.30e9 words and 4.43e9 groups (both > 2^32), rows > 2^36.

Every output and scratch buffer is passed in, sized from the model or from the call's own *_max_words / *_scratch_bytes; a test
holds at most 2 GiB of device memory.  What that cap decides (bytes the scratch functions ask for):
  at B  wah_bitop_indexed / _list / _clauses / wah_bsi_range / wah_bsi_compare_scratch_bytes = 17 190 494 464 (537 801 984 at A):
        the bit operations, the clause call and the 2-slice range predicate run at A only.
        Run at B: fetch (3 584 bytes), from-positions (35 328), splice (18 688); count and positions are in test_gpu_select.py.
  at A  wah_bsi_arith_scratch_bytes for 12-bit operands with existence (13 output rows) = 7 525 736 448, wah_bsi_mul_scratch_bytes
        for 12 x 12 -> 24 bits = 33 404 146 688: both beyond the cap already at A.  The widest shapes that fit run instead:
        2 + 2 -> 3 bits and 2 - 2 -> 3 bits without existence, 1 + 1 -> 2 bits with both existence bitmaps (1 612 868 608 each),
        1 x 1 -> 1 bit (1 646 998 528).  sum_product_where multiplies into ka + kb >= 2 slices (2 739 130 368) and does not run.

Narrowed expressions that these tests catch, each tried alone on a scratch copy of the source (never committed):
  gpu-wah_amd/csrc/wah_bitop_list.hip, fetch_items_kernel: the group of a listed row from its low 32 bits,
    `const u64 group = p / 31u;` -> `const u64 group = (u32)p / 31u;`
        test_fetch (all four cases), test_values_and_keys_at_rows
  gpu-wah_amd/csrc/wah_from_positions.hip, from_positions_kernel: the segment's first row in 32 bits,
    `const u64 base = seg * (u64)kSegBits;` -> `const u64 base = (u32)(seg * (u64)kSegBits);`
        test_bitmaps_from_rows[A], test_bitmaps_from_rows[B]
  gpu-wah_amd/csrc/wah_bitop_list.hip, the pick of wah_bsi_kth_indexed_device: the rank compared in 32 bits,
    `if (rank < below + h) {` -> `if ((u32)rank < (u32)(below + h)) {` (the first of the two: the ungrouped call's)
        test_kth_ranks_around_2_32
  the masked count's per-operand accumulator: see test_count_masked_under_masks_of_more_than_2_32_rows.
"""
import importlib

import numpy as np
import pytest

from tests import _long as lg
from tests import _switch as sw

pytestmark = pytest.mark.gpu

WAH_OK, WAH_ERR_STREAM = 0, -6
ROUTE_RUNS, ROUTE_GROUPS = 1, 2
GUARD = 0x5A5A5A5A
A, B = lg.A_SEGMENTS, lg.B_SEGMENTS
SEG_WORDS, SEG_BITS = lg.SEG_WORDS, lg.SEG_BITS
U64 = (1 << 64) - 1
SIZES = {"A": A, "B": B}


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


def _dev(words):
    import torch

    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).cuda()


def _dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


class Uploads:
    """LongBitmaps on the device, each uploaded once: (stream, index) pairs and, for several bitmaps back to back, the
    (stream, index, n_words, n_bits, has_exists) five-tuple the front ends of columns.py take."""

    def __init__(self, oracle):
        self.oracle, self.pairs = oracle, {}

    def pair(self, bitmap, split=1):
        key = (id(bitmap), split)
        if key not in self.pairs:
            stream, index = bitmap.stream_index(self.oracle, split)
            self.pairs[key] = (bitmap, _dev(stream), _dev64(index))   # (the bitmap is kept so that its id stays its own)
        return self.pairs[key][1:]

    def matrix(self, bitmaps):
        stream, index = lg.expected_streams(self.oracle, bitmaps)
        return _dev(stream), _dev64(index)

    def bsi(self, slices, exists=None):
        stream, index = self.matrix(list(slices) + ([exists] if exists is not None else []))
        return (stream, index, slices[0].n_words, len(slices), exists is not None)


@pytest.fixture(autouse=True)
def two_gib(wah):
    """No test holds more than 2 GiB of device memory at any time: the peak of what it allocated, uploads, scratch and outputs."""
    import gc

    import torch

    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    yield
    assert torch.cuda.max_memory_allocated() - before <= 2**31


@pytest.fixture
def up(oracle):
    """(Per test: what one test uploaded is freed before the next one.)"""
    return Uploads(oracle)


@pytest.fixture
def scratch_a(wah):
    """The scratch of the calls that write one bitmap of size A (537 801 984 bytes)."""
    import torch

    n = A * SEG_WORDS
    size = int(wah.lib().wah_bitop_indexed_scratch_bytes(n))
    assert size == wah.lib().wah_bitop_list_scratch_bytes(n, 9) == wah.lib().wah_bsi_range_scratch_bytes(n, 40) == wah.lib().wah_bsi_compare_scratch_bytes(n, 12, 12)
    return torch.empty(size, dtype=torch.uint8, device="cuda")


class Out:
    """Output buffers of exactly the expected size: the words with a guard word behind them, and the index entries."""

    def __init__(self, oracle, bitmaps, spare=0):
        import torch

        self.want_stream, self.want_index = lg.expected_streams(oracle, bitmaps)
        self.cap = self.want_stream.size + spare
        self.buf = torch.full((self.cap + 1,), GUARD, dtype=torch.int32, device="cuda")
        self.offsets = torch.full((self.want_index.size,), -1, dtype=torch.int64, device="cuda")

    @property
    def kw(self):
        return {"out": self.buf[: self.cap], "out_offsets": self.offsets}

    def check(self, got, what):
        import torch

        stream, offs = got[0], got[1]
        assert int(self.buf[self.cap].item()) == GUARD, (what, "guard")
        assert stream.numel() == self.want_stream.size, (what, stream.numel(), self.want_stream.size)
        assert torch.equal(offs[: self.want_index.size], _dev64(self.want_index)), (what, "index")
        same = torch.equal(stream, _dev(self.want_stream))
        assert same, (what, "first differing word", int(torch.nonzero(stream != _dev(self.want_stream))[0].item()))


def _as_u64(values):
    return [int(v) & U64 for v in values]


# ---- fetch ------------------------------------------------------------------------------------------------------------------------
def _fetch_table(size):
    return [lg.operand(SIZES[size], j) for j in range(5)]


def _fetch_want(table, rows, mode):
    bits = np.stack([b.bits_at(rows) for b in table]).astype(np.int64)   # [k, rows]
    if mode == "bits":
        return [sum(int(bits[j, i]) << (len(table) - 1 - j) for j in range(len(table))) for i in range(rows.size)]
    return [int(np.argmax(bits[:, i])) if bits[:, i].any() else U64 for i in range(rows.size)]


@pytest.mark.parametrize("mode", ("bits", "first"))
@pytest.mark.parametrize("size", ("A", "B"))
def test_fetch(wah, up, size, mode):
    """About 300 (A) / 100 (B) ascending rows: runs on both sides of rows 2^31 and 2^32 (A), of group 2^32 and decoded word 2^32
    (B), the last row, duplicates; five table rows of differing defaults and live segments."""
    import torch

    n_segments = SIZES[size]
    table, rows = _fetch_table(size), lg.fetch_rows(n_segments, 20 if size == "A" else 5)
    assert rows.max() == n_segments * SEG_BITS - 1 > 2**32
    want = _fetch_want(table, rows, mode)
    assert len(set(want)) > 3
    d_table = wah.bitop_operand_table([up.pair(b) for b in table])
    n = n_segments * SEG_WORDS
    scratch = torch.empty(int(wah.lib().wah_fetch_scratch_bytes(n, rows.size)), dtype=torch.uint8, device="cuda")
    out = torch.full((rows.size + 1,), GUARD, dtype=torch.int64, device="cuda")
    got = wah.fetch_device(d_table, _dev64(rows), n, wah.FETCH_BITS if mode == "bits" else wah.FETCH_FIRST, scratch=scratch, out=out[: rows.size])
    assert _as_u64(got.tolist()) == want and int(out[rows.size].item()) == GUARD


def test_values_and_keys_at_rows(wah, up):
    """The front ends over a 12-bit column with an existence bitmap and over five value columns, rows in any order."""
    import torch

    a, _, xa, _ = lg.columns_12()
    rows = lg.fetch_rows(A, 20)
    shuffled = np.random.default_rng(1).permutation(rows)
    values, have = wah.columns.values_at_rows(wah, up.bsi(a, xa), _dev64(shuffled))
    want = [lg.value_at(a, xa, r) for r in shuffled.tolist()]
    assert have.tolist() == [w is not None for w in want] and 10 < sum(have.tolist()) < rows.size
    # the index stores what the slices hold, also where the row does not exist
    assert values.tolist() == [lg.value_at(a, None, r) for r in shuffled.tolist()]
    table = _fetch_table("A")
    stream, index = up.matrix(table)
    keys = wah.columns.keys_at_rows(wah, (stream, index, A * SEG_WORDS), _dev64(shuffled))
    assert _as_u64(keys.tolist()) == _fetch_want(table, shuffled, "first")
    assert torch.is_tensor(keys)


def _fetch_status(wah, d_table, rows, n):
    import torch

    scratch = torch.empty(int(wah.lib().wah_fetch_scratch_bytes(n, len(rows))), dtype=torch.uint8, device="cuda")
    wah.fetch_device(d_table, _dev64(rows), n, wah.FETCH_BITS, scratch=scratch, check=False)
    return int(wah.lib().wah_fetch_status(scratch.data_ptr(), None))


def test_fetch_refuses_what_only_the_bits_above_32_show(wah, up):
    n = A * SEG_WORDS
    d_table = wah.bitop_operand_table([up.pair(b) for b in _fetch_table("A")])
    assert _fetch_status(wah, d_table, [5, 2**32 + 5], n) == WAH_OK
    assert _fetch_status(wah, d_table, [32 * n - 1], n) == WAH_OK
    assert _fetch_status(wah, d_table, [32 * n], n) == WAH_ERR_STREAM            # (32 n mod 2^32 is a row of the bitmap)
    assert _fetch_status(wah, d_table, [2**32 + 5, 5], n) == WAH_ERR_STREAM      # descending, the low words ascending: 5, 5
    assert _fetch_status(wah, d_table, [2**32 + 5, 6], n) == WAH_ERR_STREAM


# ---- from-positions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ("A", "B"))
def test_bitmaps_from_rows(wah, oracle, size):
    """A: three lists with rows across 2^31 and 2^32 and in the last segment, and an empty one; B: one list.  Words and index."""
    import torch

    n_segments = SIZES[size]
    lists = lg.row_lists(n_segments, 4 if size == "A" else 1)
    n, total = n_segments * SEG_WORDS, sum(x.size for x in lists)
    assert max(x.max() for x in lists if x.size) >= n_segments * SEG_BITS - SEG_BITS and (size == "B" or lists[-1].size == 0)
    out = Out(oracle, [lg.from_rows(n_segments, x) for x in lists])
    cap = wah.from_positions_max_words(n, len(lists), total)
    assert out.cap <= cap
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    out.buf, out.cap = buf, cap
    scratch = torch.empty(int(wah.lib().wah_from_positions_scratch_bytes(n, len(lists))), dtype=torch.uint8, device="cuda")
    got = wah.columns.bitmaps_from_rows(wah, [_dev64(x) for x in lists], n, scratch=scratch, **out.kw)
    out.check(got, size)


def test_from_positions_refuses_a_row_that_is_in_range_modulo_2_32(wah):
    import torch

    n = A * SEG_WORDS
    scratch = torch.empty(int(wah.lib().wah_from_positions_scratch_bytes(n, 1)), dtype=torch.uint8, device="cuda")
    buf = torch.empty(wah.from_positions_max_words(n, 1, 3), dtype=torch.int32, device="cuda")
    offs = torch.empty(A + 1, dtype=torch.int64, device="cuda")
    for rows, code in (([5, 2**32 + 5, 32 * n - 1], WAH_OK), ([5, 6, 32 * n], WAH_ERR_STREAM), ([5, 6, 2**33 + 7], WAH_ERR_STREAM),
                       ([5, 2**32 + 5, 2**32 + 5], WAH_ERR_STREAM), ([2**32 + 5, 6, 7], WAH_ERR_STREAM)):
        wah.from_positions_device(_dev64(rows), _dev64([3]), n, scratch=scratch, out=buf, out_offsets=offs, check=False)
        assert int(wah.lib().wah_from_positions_status(scratch.data_ptr(), None)) == code, rows


def test_expected_stream_index_is_what_the_call_emits_for_a_short_bitmap(wah, oracle):
    """The model's expected_stream_index against the device on 40 segments, where tests/test_long_reference.py holds it against
    compress() of the decoded bitmap: rows in every third segment, a segment of ones, the last row."""
    n_segments = 40
    rows = np.unique(np.concatenate([np.random.default_rng(4).integers(0, SEG_BITS, 300) + s * SEG_BITS for s in range(0, n_segments, 3)]
                                    + [np.arange(7 * SEG_BITS, 8 * SEG_BITS), [n_segments * SEG_BITS - 1]]))
    model = lg.from_rows(n_segments, rows)
    assert len(model.live) == 15 and model.count() == rows.size
    out = Out(oracle, [model])
    out.check(wah.from_positions_device(_dev64(rows), _dev64([rows.size]), n_segments * SEG_WORDS, **out.kw), "short")
    assert np.array_equal(out.want_stream, oracle.compress(model.decoded()))


# ---- splice -----------------------------------------------------------------------------------------------------------------------
def _splice_arguments(wah, up, pieces):
    table = wah.bitop_operand_table([up.pair(src) for srcs, _, _ in pieces for src in srcs])
    words = sum(int(up.pair(src)[0].numel()) for srcs, _, _ in pieces for src in srcs)
    return table, [(srcs[0].n_words, first, n) for srcs, first, n in pieces], words


@pytest.mark.parametrize("name", list(lg.splice_cases()))
def test_splice(wah, oracle, up, name):
    """At A, two columns: a piece taken from row 2^32 - 100 of its source, running starts that cross 2^32, a piece that lands at
    output row 2^32 - 7; a piece of 2^32 + 1000 rows of a constant source (both images fills for 135 000 segments).  At B, one
    column: a piece of more than 2^36 rows, then one whose first source row lies above 2^36."""
    import torch

    n_segments, pieces = lg.splice_cases()[name]
    k, n = len(pieces[0][0]), n_segments * SEG_WORDS
    out = Out(oracle, [lg.splice([(srcs[c], first, rows) for srcs, first, rows in pieces], n_segments) for c in range(k)])
    table, triples, source_words = _splice_arguments(wah, up, pieces)
    cap = wah.splice_max_words(n, k, len(pieces), source_words)
    assert out.cap <= cap
    out.buf, out.cap = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda"), cap
    scratch = torch.empty(int(wah.lib().wah_splice_scratch_bytes(n, k, len(pieces))), dtype=torch.uint8, device="cuda")
    got = wah.splice_device(triples, table, k, n, scratch=scratch, **out.kw)
    out.check(got, name)


def test_splice_refuses_rows_behind_the_operand_that_only_the_bits_above_32_show(wah, up):
    import torch

    n_segments, pieces = lg.splice_cases()["a piece lands at 2^32 - 7"]
    n = n_segments * SEG_WORDS
    table, triples, source_words = _splice_arguments(wah, up, pieces[:1])
    scratch = torch.empty(int(wah.lib().wah_splice_scratch_bytes(n, 2, 1)), dtype=torch.uint8, device="cuda")
    buf = torch.empty(wah.splice_max_words(n, 2, 1, source_words), dtype=torch.int32, device="cuda")
    offs = torch.empty(2 * n_segments + 1, dtype=torch.int64, device="cuda")
    n_src = triples[0][0]
    for piece, code in (((n_src, 5, 10), WAH_OK), ((n_src, 32 * n_src - 10, 10), WAH_OK), ((n_src, 32 * n_src - 10, 11), WAH_ERR_STREAM),
                        ((SEG_WORDS, 2**32 + 5, 10), WAH_ERR_STREAM), ((SEG_WORDS, 5, 2**32 + 10), WAH_ERR_STREAM), ((n_src, 2**33 + 5, 10), WAH_ERR_STREAM)):
        wah.splice_device([piece], table, 2, n, scratch=scratch, out=buf, out_offsets=offs, check=False)
        assert int(wah.lib().wah_splice_status(scratch.data_ptr(), None)) == code, piece


# ---- bit operations ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 3))
def test_two_and_three_operands_on_both_routes(wah, oracle, up, scratch_a, k):
    """Every operation; the run-merge route for operands of a word a segment, the decode route where one operand's constant
    segments are written as 128 fills each (17 million words: more than 112 a segment over all operands)."""
    n = A * SEG_WORDS
    bitmaps = [lg.operand(A, j) for j in range(k)]
    for split, route in ((1, ROUTE_RUNS), (128, ROUTE_GROUPS)):
        pairs = [up.pair(bitmaps[0], split)] + [up.pair(b) for b in bitmaps[1:]]
        total = sum(int(st.numel()) for st, _ in pairs)
        assert (total <= sw.RUNS_MAX_WORDS_PER_SEG * A) == (route == ROUTE_RUNS)
        for name in sw.LIST_OPS:
            out = Out(oracle, [lg.bitop(name, bitmaps)])
            if k == 2:
                got = wah.bitop_indexed_device(name, *pairs[0], *pairs[1], n, scratch=scratch_a, **out.kw)
            else:
                got = wah.bitop_many_indexed_device(name, pairs, n, scratch=scratch_a, **out.kw)
            assert wah.lib().wah_last_bitop_route() == route, (k, name, split)
            out.check(got, (k, name, split))


@pytest.mark.parametrize("k", (2, 3, 9))
def test_list_call(wah, oracle, up, scratch_a, k):
    n = A * SEG_WORDS
    bitmaps = [lg.operand(A, j) for j in range(k)]
    table = wah.bitop_operand_table([up.pair(b) for b in bitmaps])
    for name in sw.LIST_OPS:
        out = Out(oracle, [lg.bitop(name, bitmaps)])
        out.check(wah.bitop_list_indexed_device(name, table, n, scratch=scratch_a, **out.kw), (k, name))


def test_clauses_and_not(wah, oracle, up, scratch_a):
    """NOT of one operand (a negated clause alone: more than 2^32 rows set), and a conjunction of three clauses over nine."""
    n = A * SEG_WORDS
    bitmaps = [lg.operand(A, j) for j in range(9)]
    pairs = [up.pair(b) for b in bitmaps]
    for j in (0, 1):
        want = lg.invert(bitmaps[j])
        assert want.count() == bitmaps[j].n_bits - bitmaps[j].count()
        out = Out(oracle, [want])
        out.check(wah.bitop_clauses_indexed_device([([pairs[j]], True)], n, scratch=scratch_a, **out.kw), ("not", j))
    assert lg.invert(bitmaps[0]).count() > 2**32
    shape = [(slice(0, 3), False), (slice(3, 4), True), (slice(4, 9), False)]
    out = Out(oracle, [lg.clauses([(bitmaps[s], negate) for s, negate in shape])])
    out.check(wah.bitop_clauses_indexed_device([(pairs[s], negate) for s, negate in shape], n, scratch=scratch_a, **out.kw), "three clauses")


def test_or_andnot_and_clauses_are_not_run_at_size_b(wah):
    """The scratch the bit operations ask for at B is 17 190 494 464 bytes: beyond what a test may hold."""
    n = B * SEG_WORDS
    assert wah.lib().wah_bitop_indexed_scratch_bytes(n) == wah.lib().wah_bitop_clauses_scratch_bytes(n, 2, 1) == wah.lib().wah_bsi_range_scratch_bytes(n, 2) > 2**31


# ---- masked counts, grouped sums ----------------------------------------------------------------------------------------------------
def test_count_masked_under_masks_of_more_than_2_32_rows(wah, up):
    """Two masks of ones throughout (4 297 857 546 and 2^32 rows) against the 40 slices of a column whose constant segments hold
    0xABCDE12345: every count of a set slice passes 2^31, those under the first mask 2^32.  The per-operand accumulator of a
    wavefront (`acc` of count_masked_kernel): a wavefront adds up the rows of its own run of (mask, chunk, segment) items only,
    and launch_count_masked always starts a full grid for this many items -- the launcher takes no parameter that makes the grid
    small.  The 2 x 135 400 items of this call over 4096 wavefronts are 67 segments, 2.1 million rows, a wavefront, so no public
    input brings a 32-bit `acc` near 2^32 (that needs 135 300 segments in ONE wavefront's run); narrowing it is not a mutant
    these tests can catch.  What the counts do catch is a 32-bit atomic, a 32-bit merge of the workgroup's run ends or a 32-bit
    total."""
    import torch

    n = A * SEG_WORDS
    masks, column = [lg.operand(A, 1), lg.groups_at_2_32()[0]], lg.column_40()
    want = [[lg.bitop("and", [m, s]).count() for s in column] for m in masks]
    assert max(want[0]) > 2**32 and max(want[1]) > 2**31
    scratch = torch.empty(int(wah.lib().wah_select_scratch_bytes(n, len(column))), dtype=torch.uint8, device="cuda")
    counts = torch.full((2, len(column)), -1, dtype=torch.int64, device="cuda")
    got = wah.count_masked_device([up.pair(m) for m in masks], [up.pair(s) for s in column], n, scratch=scratch, counts=counts)
    assert got.tolist() == want
    counts = torch.full((len(masks) + 1,), -1, dtype=torch.int64, device="cuda")
    every = torch.empty(int(wah.lib().wah_select_scratch_bytes(n, 3)), dtype=torch.uint8, device="cuda")
    got = wah.count_device([up.pair(m) for m in masks] + [up.pair(lg.invert(masks[1]))], n, scratch=every, counts=counts)
    assert got.tolist() == [masks[0].count(), 2**32, masks[0].n_bits - 2**32]


def test_positions_of_ranks_around_2_32(wah, up):
    """The existing long streams of test_gpu_select.py hold a handful of set bits: here the RANKS pass 2^32 too.  Windows at
    the front, across rank 2^32 and at the end of a bitmap of 4 297 857 546 set bits, one that starts behind the last rank."""
    import torch

    bitmap = lg.operand(A, 1)
    n, total = A * SEG_WORDS, bitmap.count()
    assert total > 2**32 + 100
    stream, index = up.pair(bitmap)
    scratch = torch.empty(int(wah.lib().wah_select_scratch_bytes(n, 1)), dtype=torch.uint8, device="cuda")
    for first, limit in ((0, 70), (2**31 - 35, 70), (2**32 - 35, 70), (total - 40, 70), (total, 5)):
        out = torch.full((limit + 1,), GUARD, dtype=torch.int64, device="cuda")
        got, count = wah.positions_device(stream, index, n, first=first, out=out[:limit], scratch=scratch)
        want = bitmap.positions(first, limit)
        assert count == total and got.tolist() == want.tolist() and int(out[limit].item()) == GUARD, first
        assert first != 2**32 - 35 or want[-1] > 2**32


def test_group_sum_and_its_front_ends(wah, up):
    """SUM of the 40-bit column under a filter of ones, in two groups that split at row 2^32: the sums as Python ints in full
    width (the whole is above 2^64), COUNT(*) of the first group just below 2^32."""
    import torch

    n = A * SEG_WORDS
    mask, groups, column = lg.operand(A, 1), lg.groups_at_2_32(), lg.column_40()
    want = [lg.sum_count(column, lg.bitop("and", [mask, g])) for g in groups]
    per_slice = [[lg.bitop("and", [mask, g, s]).count() for s in column] for g in groups]
    assert sum(w[0] for w in want) > 2**64 and want[0][0] > 2**64 >> 10
    scratch = torch.empty(int(wah.lib().wah_select_scratch_bytes(n, len(column))), dtype=torch.uint8, device="cuda")
    rows, counts, sums = wah.group_sum_device([up.pair(mask)], [up.pair(g) for g in groups], [up.pair(s) for s in column], [40], n, scratch=scratch)
    assert rows.tolist() == [w[2] for w in want] and counts.tolist() == per_slice
    assert [(_as_u64(s)[0] + (_as_u64(s)[1] << 64)) for s in sums[:, 0].tolist()] == [w[0] for w in want]
    # the front ends: the groups as two columns of one key, the column as a bit-sliced attribute
    key_stream, key_index = up.matrix(list(groups))
    bsi = up.bsi(column)
    got = wah.columns.aggregate_columns(wah, [(key_stream, key_index, [0, 1])], [bsi], n, where=up.pair(mask), scratch=scratch)
    assert got["rows"].tolist() == [w[2] for w in want] and got["sums"][0].tolist() == [w[0] for w in want]
    assert wah.columns.sum_column_where(wah, bsi, *up.pair(mask)) == lg.sum_count(column, mask)[0] == sum(w[0] for w in want)


# ---- range and compare --------------------------------------------------------------------------------------------------------------
def test_range_predicates(wah, oracle, up, scratch_a):
    """Over the 40-bit column, with and without an existence bitmap: ranges that hold the constant segments' value (more than
    2^32 rows selected) and ranges that do not (a sparse result)."""
    column, exists = lg.column_40(), lg.operand(A, 4)
    v = lg.COLUMN_40
    for x in (None, exists):
        bsi = up.bsi(column, x)
        for lo, hi, many in ((v - 5, v + 5, True), (0, v, True), (v + 1, (1 << 40) - 1, False), (v, v, True), (0, v - 1, False), (5, 4, False)):
            want = lg.range_predicate(column, lo, hi, x)
            assert (want.count() > 2**32) == many, (lo, hi)
            out = Out(oracle, [want])
            out.check(wah.columns.range_column(wah, bsi, lo, hi, scratch=scratch_a, **out.kw), (lo, hi, x is not None))
    out = Out(oracle, [lg.range_predicate(column, v + 1, (1 << 40) - 1)])
    out.check(wah.columns.compare_column(wah, up.bsi(column), ">", v, scratch=scratch_a, **out.kw), "> constant")


def test_compare_two_columns(wah, oracle, up, scratch_a):
    """Two 12-bit columns with existence bitmaps, equal up to segment 60 000 and A < B behind it in the constant segments:
    `<=` selects more than 2^32 rows, `<` more than 2^31, `>` is sparse."""
    a, b, xa, xb = lg.columns_12()
    bsi_a, bsi_b = up.bsi(a, xa), up.bsi(b, xb)
    for op in ("<", "<=", ">", ">=", "==", "!="):
        out = Out(oracle, [lg.compare(a, b, op, xa, xb)])
        out.check(wah.columns.compare_columns(wah, bsi_a, op, bsi_b, scratch=scratch_a, **out.kw), op)
    out = Out(oracle, [lg.compare(a, b, "<=")])
    out.check(wah.columns.compare_columns(wah, up.bsi(a), "<=", up.bsi(b), scratch=scratch_a, **out.kw), "<= without existence")


# ---- add, subtract, multiply: the widths the 2 GiB cap admits (see the module docstring) ---------------------------------------------
def _narrow(bits, seed, constant):
    return lg.column(A, lg.A_NAMED, bits, seed, constant)


def _arith_case(wah, oracle, up, op, a, b, n_out, xa=None, xb=None):
    import torch

    n = A * SEG_WORDS
    flags = (1 if xa is not None else 0) | (2 if xb is not None else 0)
    if op == "*":
        size, call = int(wah.lib().wah_bsi_mul_scratch_bytes(n, len(a), n_out, flags)), wah.columns.multiply_columns
    else:
        size, call = int(wah.lib().wah_bsi_arith_scratch_bytes(n, n_out, flags)), wah.columns.add_columns if op == "+" else wah.columns.subtract_columns
    assert size < 2**31 - 2**27
    scratch = torch.empty(size, dtype=torch.uint8, device="cuda")
    out = Out(oracle, lg.arith(a, b, op, n_out, xa, xb))
    got = call(wah, up.bsi(a, xa), up.bsi(b, xb), n_bits=n_out, scratch=scratch, **out.kw)
    out.check(got, (op, len(a), len(b), n_out, flags))
    assert got[2:] == (n, n_out, flags != 0)


@pytest.mark.parametrize("op", ("+", "-"))
def test_add_and_subtract_two_bit_columns(wah, oracle, up, op):
    """2-bit operands, a 3-bit result, no existence: constant segments hold 2 in A and 3, then 1 in B: a carry / a borrow for
    more than 2^31 rows."""
    _arith_case(wah, oracle, up, op, _narrow(2, 21, 2), _narrow(2, 22, ([0, 70_000], [3, 1])), 3)


def test_add_one_bit_columns_with_existence(wah, oracle, up):
    _arith_case(wah, oracle, up, "+", _narrow(1, 23, 1), _narrow(1, 24, ([0, 70_000], [1, 0])), 2, lg.operand(A, 1), lg.operand(A, 4))


def test_multiply_one_bit_columns(wah, oracle, up):
    _arith_case(wah, oracle, up, "*", _narrow(1, 25, 1), _narrow(1, 26, ([0, 70_000], [1, 0])), 1)


# ---- order statistics ---------------------------------------------------------------------------------------------------------------
def _kth_queries(total):
    return [(lg.ASCENDING, 0, 1), (lg.ASCENDING, 2**32 - 1, 1), (lg.ASCENDING, 2**32, 1), (lg.ASCENDING, 2**32 + 1, 1), (lg.ASCENDING, total - 1, 1),
            (lg.QUANTILE, 1, 2), (lg.ASCENDING, total, 1), (lg.DESCENDING, total - 2**32, 1), (lg.DESCENDING, total - 2**32 - 1, 1),
            (lg.DESCENDING, 0, 1), (lg.DESCENDING, total, 1), (lg.QUANTILE, 0, 1), (lg.QUANTILE, 1, 1)]


def test_kth_ranks_around_2_32(wah, up):
    """Under a filter that selects 4 297 857 546 rows exactly 2^32 hold a value <= 7: rank 2^32 - 1 is 7, rank 2^32 the next
    value up.  Ranks 0, 2^32 - 1, 2^32, 2^32 + 1, selected - 1, the median, the same from the top, and rank == selected (no
    value); then the front ends."""
    import torch

    slices, mask = lg.kth_case()
    n, ranks = A * SEG_WORDS, lg.Ranks(slices, mask)
    table = wah.bitop_operand_table([up.pair(mask)] + [up.pair(s) for s in slices])
    scratch = torch.empty(int(wah.lib().wah_bsi_kth_scratch_bytes(n, len(slices))), dtype=torch.uint8, device="cuda")
    result = torch.empty(5, dtype=torch.int64, device="cuda")
    for query in _kth_queries(ranks.total):
        got = wah.bsi_kth_device(table, query, n, 1, scratch=scratch, result=result)
        assert tuple(_as_u64(got.tolist())) == ranks(*query), query
    assert ranks(lg.ASCENDING, 2**32 - 1)[1] != ranks(lg.ASCENDING, 2**32)[1] and ranks(lg.ASCENDING, ranks.total)[0] == 0
    bsi, m = up.bsi(slices), up.pair(mask)
    cols = wah.columns
    assert cols.kth_column_where(wah, bsi, 2**32 - 1, m) == (lg.KTH_LOW, ranks.total)
    assert cols.kth_column_where(wah, bsi, 2**32, m) == (ranks(lg.ASCENDING, 2**32)[1], ranks.total)
    assert cols.kth_column_where(wah, bsi, ranks.total, m) == (None, ranks.total)
    assert cols.kth_column_where(wah, bsi, ranks.total - 2**32, m, largest=True) == (lg.KTH_LOW, ranks.total)
    assert cols.quantile_column_where(wah, bsi, 1, 2, m) == (ranks(lg.QUANTILE, 1, 2)[1], ranks.total)
    assert cols.min_column_where(wah, bsi, m)[0] == ranks(lg.QUANTILE, 0, 1)[1] and cols.max_column_where(wah, bsi, m)[0] == 4095
    assert cols.median_column_where(wah, bsi, m)[0] == lg.KTH_LOW
    unmasked = lg.Ranks(slices)
    assert cols.kth_column_where(wah, bsi, 2**32 + 1) == (unmasked(lg.ASCENDING, 2**32 + 1)[1], slices[0].n_bits)


def test_grouped_kth_ranks_around_2_32(wah, up):
    """The same queries in two groups under the same filter: every row (more than 2^32 selected) and the rows from 2^32 on."""
    import torch

    slices, mask = lg.kth_case()
    n = A * SEG_WORDS
    groups = [lg.LongBitmap(A, 1), lg.groups_at_2_32()[1]]
    models = [lg.Ranks(slices, lg.bitop("and", [mask, g])) for g in groups]
    assert models[0].total > 2**32 > models[1].total > 0
    queries = _kth_queries(models[0].total)
    scratch = torch.empty(int(wah.lib().wah_bsi_kth_grouped_scratch_bytes(n, len(slices), 2, len(queries))), dtype=torch.uint8, device="cuda")
    results = torch.empty((2, len(queries), 5), dtype=torch.int64, device="cuda")
    got = wah.bsi_kth_grouped_device([up.pair(mask)], [up.pair(g) for g in groups], [up.pair(s) for s in slices], queries, n, scratch=scratch, results=results)
    for g, model in enumerate(models):
        for q, query in enumerate(queries):
            assert tuple(_as_u64(got[g, q].tolist())) == model(*query), (g, query)
    key_stream, key_index = up.matrix(groups)
    by = wah.columns.quantiles_by(wah, [(key_stream, key_index, [0, 1])], up.bsi(slices), n, ["min", "median", "max", (lg.ASCENDING, 2**32, 1)], where=up.pair(mask), scratch=scratch)
    assert by["values"].tolist() == [[m(lg.QUANTILE, 0, 1)[1], m(lg.QUANTILE, 1, 2)[1], 4095, m(lg.ASCENDING, 2**32, 1)[1] if m.total > 2**32 else None] for m in models]
    assert by["totals"][:, 0].tolist() == [m.total for m in models]


def test_top_rows_lie_above_2_32(wah, up):
    """The five largest values of a column that holds 5 everywhere but in two live segments behind row 2^32.  top_rows takes no
    buffers: its range_column and filter_columns results are allocated by wah_max_compressed_words (554 598 400 bytes each at A,
    with 537 801 984 of scratch): 1.65e9 bytes at the most at one time."""
    column, mask = lg.top_case()
    want = lg.top_rows(column, mask, 5)
    got = wah.columns.top_rows(wah, up.bsi(column), 5, mask=up.pair(mask))
    assert got.tolist() == want.tolist() and min(got.tolist()) > 2**32
