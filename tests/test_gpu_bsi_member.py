"""GPU tests of wah_bsi_member_indexed_device: `value IN (set)` / NOT IN over a bit-sliced attribute in one call (include/wah.h),
and its front ends in api.py and columns.py.  Everything is exact: the result's words, their count and its segment index against
compress() of the bitmap computed with numpy FROM THE VALUES (tests/_member.py: expected) -- the CPU oracle and an indexed
compress of it.  tests/test_member_reference.py proves that model against the restatement of the kernel's steps on the CPU, and
that the headline cases can fail.

Shapes are the smallest at which the kernel can still go wrong: 1, 31, 992 and 992 * 3 + 5 words (a ragged last segment, a
workgroup stride of more than one item above 32 slices), 1 .. 64 slices around the item-shape switch at 32 | 33 and the width
without a spare bit, one item more than the capped grid, and one bitmap of more than 2^32 rows."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _foreign as fg, _long as lg, _member as mb

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6
SEG = 992
GRID = 512  # kMemberGridItems of wah_member.hip: workgroups at the most
GUARD = 0x5A5A5A5A


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

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


class Streams:
    """One indexed compressor of n_words, reused for the operands and for the expected results' segment indexes."""

    def __init__(self, wah, n_words):
        self.comp = wah.DeviceCompressor(n_words, indexed=True)

    def of(self, words):
        self.comp.run(_dev(words))
        return self.comp.result().clone(), self.comp.seg_offsets.clone()


def _same(streams, oracle, got, offs, combined, what):
    """(got, offs) is exactly compress(combined) and its segment index."""
    combined = np.ascontiguousarray(combined, dtype=np.uint32)
    want = oracle.compress(combined)
    assert got.numel() == want.size, (what, got.numel(), want.size)
    assert np.array_equal(_host(got), want), what
    _, ref_offs = streams.of(combined)
    assert np.array_equal(offs.cpu().numpy(), ref_offs.cpu().numpy()), what


def _set_args(case):
    """The set of a case as bsi_member_device takes it (the tensors stay alive in the dict)."""
    if mb.is_bitset(case):
        return dict(members=_dev(case["words"]), bitset=True, set_bits=case["set_bits"])
    count = None if case["count"] is None else _dev64(np.array([case["count"]], dtype=np.uint64))
    return dict(members=_dev64(case["members"]), count=count)


def _call(wah, table, case, **kw):
    return wah.bsi_member_device(table, n_words=case["n"], exists=case["exists"] is not None, negate=case["negate"], **_set_args(case), **kw)


class Tables:
    """The slice tables of the attributes at hand, one upload per (values, exists): cases that share an attribute share it."""

    def __init__(self, wah):
        self.wah, self.streams, self.made = wah, {}, {}

    def streams_of(self, n):
        if n not in self.streams:
            self.streams[n] = Streams(self.wah, n)
        return self.streams[n]

    def of(self, case):
        key = (id(case["values"]), id(case["exists"]), case["k"])
        if key not in self.made:
            ops = [self.streams_of(case["n"]).of(row) for row in _bsi.build_slices(case["values"], case["k"], case["exists"])]
            self.made[key] = (ops, self.wah.bitop_operand_table(ops), case["values"], case["exists"])  # (raw pointers: everything stays alive)
        return self.made[key][1]


def _check(wah, oracle, tables, case, what):
    got, offs = _call(wah, tables.of(case), case)
    _same(tables.streams_of(case["n"]), oracle, got, offs, mb.expected(case), what)


# ---- 1: sizes and widths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, SEG, SEG * 3 + 5])
@pytest.mark.parametrize("k", [1, 2, 20, 32, 33, 63, 64])
def test_sizes_and_widths(wah, oracle, n, k):
    """Every width with and without an existence row, list and bit array, both NEGATE states; the attribute of a (width, existence)
    pair is uploaded once."""
    tables = Tables(wah)
    for with_exists in (False, True):
        for bitset in (False, True):
            case = mb.headline(n, k, with_exists, bitset=bitset)
            for negate in (False, True):
                _check(wah, oracle, tables, dict(case, negate=negate), (n, k, with_exists, bitset, negate))


def test_empty_bitmap(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    for exists in (False, True):
        for k in (3, 40):
            got, out_offs = wah.bsi_member_device([(stream, offs)] * (k + exists), wah.member_set([1, 2], "cuda"), 0, exists=exists)
            assert got.numel() == 0 and int(out_offs[0].item()) == 0


def test_rows_the_caller_does_not_have_hold_zero(wah, oracle):
    """Without an existence bitmap the rows behind the caller's own have the value 0: they match when 0 is in the set, and under
    NEGATE when it is not."""
    n = SEG + 7
    values = np.zeros(32 * n, np.uint64)
    values[:1000] = np.arange(1, 1001, dtype=np.uint64)
    tables = Tables(wah)
    for exists in (None, np.arange(32 * n) < 1000):
        for entries in ([0, 5], [5, 6]):
            for negate in (False, True):
                _check(wah, oracle, tables, mb.list_case(n, 12, values, exists, entries, negate), (exists is not None, entries, negate))
                rng = np.random.default_rng(3)
                case = mb.bitset_case(n, 12, values, exists, 700, rng, negate)
                case["words"][0] = (case["words"][0] & np.uint32(0xFFFFFFFE)) | np.uint32(entries[0] == 0)
                _check(wah, oracle, tables, case, (exists is not None, entries, negate, "bit array"))


# ---- 2, 3, 4: the edges of a list, of a bit array, of a half segment ------------------------------------------------------------------
@pytest.mark.parametrize("k,n,with_exists", [(20, SEG + 5, True), (64, 40, True), (33, 40, False)])
def test_list_edges(wah, oracle, k, n, with_exists):
    tables = Tables(wah)
    cases = mb.list_edges(k, n, with_exists)
    assert {"count 0", "count 65 poisoned", "duplicates", "smallest and largest present", "one above and one below"} <= set(cases)
    for name, case in cases.items():
        _check(wah, oracle, tables, case, (k, name))


def test_null_count_is_the_capacity(wah, oracle):
    tables = Tables(wah)
    case = mb.list_edges()["count 64"]
    assert case["count"] is None
    _check(wah, oracle, tables, case, "NULL count")
    _check(wah, oracle, tables, dict(case, count=case["members"].size), "count == capacity")


@pytest.mark.parametrize("k,n", [(24, SEG + 5), (40, 40)])
def test_bitset_edges(wah, oracle, k, n):
    tables = Tables(wah)
    cases = mb.bitset_edges(k, n)
    assert {"set_bits 0", "set_bits 1", "set_bits 31", "set_bits 32", "set_bits 33", f"set_bits {(1 << 20) + 5}"} <= set(cases)
    for name, case in cases.items():
        _check(wah, oracle, tables, case, (k, name))


@pytest.mark.parametrize("negate", [False, True])
def test_half_segment_seam(wah, oracle, negate):
    case = mb.seam_case(negate=negate)
    assert case["k"] > 32 and not case["exists"][mb.SEG_BITS: 2 * mb.SEG_BITS].any()
    _check(wah, oracle, Tables(wah), case, ("seam", negate))
    rng = np.random.default_rng(8)
    wide = mb.bitset_case(case["n"], case["k"], case["values"], case["exists"], 4097, rng, negate)
    _check(wah, oracle, Tables(wah), wide, ("seam, bit array", negate))


# ---- 5: one item more than the capped grid -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 33])
def test_one_item_more_than_the_grid(wah, oracle, k):
    """GRID workgroups stride over the items: at GRID * 992 + 1 words of 2 slices workgroup 0 takes a second item, the ragged last
    segment, and must clear the rows of its first; of 33 slices (two items a segment) every workgroup takes a second one and
    workgroups 0 and 1 a third."""
    n = GRID * SEG + 1
    rng = np.random.default_rng(k)
    values = rng.integers(0, 4, 32 * n, dtype=np.uint64)
    if k == 33:
        values |= rng.integers(0, 2, 32 * n, dtype=np.uint64) << np.uint64(32)
    values[-32:] = np.uint64(3)  # the ragged last segment: the last item, a workgroup's second (third above 32 slices)
    tables = Tables(wah)
    for negate in (False, True):
        case = mb.list_case(n, k, values, None, [3, (1 << 32) | 1] if k == 33 else [3], negate)
        want = _bsi.unpack_bits(mb.expected(case))
        assert want[-32:].all() != negate and want[:31744].any() and not want[:31744].all()
        _check(wah, oracle, tables, case, (k, negate))


# ---- 6: foreign re-encodings of the slices and the existence row -------------------------------------------------------------------------
def test_foreign_slices(wah, oracle):
    """Every way of tests/_foreign.py in every table row in turn, indexed with wah_build_index_device: non-canonical in, canonical out."""
    n, k = SEG * 2 + 30, 5
    rng = np.random.default_rng(61)
    values = _bsi.make_values("clustered", rng, 32 * n, k)
    exists = rng.random(32 * n) < 0.9
    exists[-4000:] = True  # (the one-fill pad ways need a bitmap that ends in ones)
    matrix = _bsi.build_slices(values, k, exists)
    ways = fg.ways_for(n)
    assert fg.pad_bits(n) and len(ways) == len(fg.WAYS) + len(fg.PAD_WAYS)
    streams = Streams(wah, n)
    cases = [mb.list_case(n, k, values, exists, [3, 7, 7, 19, 40], negate) for negate in (False, True)]
    cases.append(mb.bitset_case(n, k, values, exists, 29, rng))
    seen = set()
    for first in range(len(ways)):
        made = fg.rows_foreign(matrix, n, np.random.default_rng(first), ways, first)
        seen |= {way for way, _ in made}
        pairs = []
        for way, st in made:
            assert np.array_equal(oracle.decompress(st)[:n], matrix[len(pairs)]), way
            d = _dev(st)
            offs, groups = wah.build_index_device(d)
            assert groups == fg.n_groups(n)
            pairs.append((d, offs))
        table = wah.bitop_operand_table(pairs)
        for case in cases:
            got, offs = _call(wah, table, case)
            _same(streams, oracle, got, offs, mb.expected(case), (first, case["negate"]))
    assert seen >= set(fg.WAYS) | {"pad: literal"}


# ---- 7: windows into a column matrix, and the unchecked output of the builder ---------------------------------------------------------
def test_windows_and_unchecked_builder_output(wah, oracle):
    import torch

    n, k = SEG * 2, 20
    case = mb.headline(n, k, True)
    values, exists = case["values"], case["exists"]
    d_values, d_exists = _dev64(values), torch.from_numpy(exists).cuda()
    streams = Streams(wah, n)
    want = mb.expected(case)
    # windows into the builder's column matrix
    bsi = wah.columns.bsi_from_values(wah, d_values, k, exists=d_exists)
    table = wah.columns.column_operand_table(bsi[0], bsi[1], n, list(range(k + 1)))
    got, offs = _call(wah, table, case)
    _same(streams, oracle, got, offs, want, "windows")
    # the builder's output before anything of it was checked: the whole buffer, its capacity as the length
    out, index, *_ = wah.columns.bsi_from_values(wah, d_values, k, exists=d_exists, check=False)
    assert out.numel() >= wah.max_compressed_words((k + 1) * n)
    table = wah.columns.column_operand_table(out, index, n, list(range(k + 1)))
    got, offs = _call(wah, table, case)
    _same(streams, oracle, got, offs, want, "unchecked builder output")


# ---- 8: refusals only the device sees ---------------------------------------------------------------------------------------------
def _status(wah, table, case, **kw):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    n, k = case["n"], case["k"]
    sc = torch.empty(int(wah.lib().wah_bsi_member_scratch_bytes(n, k)), dtype=torch.uint8, device="cuda:0")
    _call(wah, table, case, scratch=sc, check=False, **kw)
    return int(wah.lib().wah_bsi_member_status(sc.data_ptr(), n, k, None))


@pytest.mark.parametrize("k", [12, 40])
def test_refusals_come_from_the_status_call(wah, oracle, k):
    import torch

    n = SEG * 4
    rng = np.random.default_rng(41 + k)
    values = _bsi.make_values("clustered", rng, 32 * n, k)  # fills in every slice ...
    half = 16 * n
    values[half:] = _bsi.uniform_values(rng, 32 * n - half, k)  # ... and a result of many words
    exists = rng.random(32 * n) < 0.9
    streams = Streams(wah, n)
    ops = [streams.of(row) for row in _bsi.build_slices(values, k, exists)]
    table = wah.bitop_operand_table(ops)
    present = sorted(set(int(v) for v in values[::977]) | set(int(v) for v in values[half::50]))
    good = mb.list_case(n, k, values, exists, present)
    empty = mb.list_case(n, k, values, exists, [])
    bits = mb.bitset_case(n, k, values, exists, 300, rng)
    every = (good, dict(good, negate=True), empty, bits)
    for case in every:
        assert _status(wah, table, case) == 0
    # a broken slice stream: a fill one group short, whatever the set is
    row = 3
    words = _host(ops[row][0]).copy()
    fills = np.flatnonzero((words >> 31 == 1) & ((words & 0x3FFFFFFF) >= 2))
    assert fills.size, "a clustered slice has fills"
    broken = words.copy()
    broken[int(fills[fills.size // 2])] -= 1
    for r in (row, 0, k - 1, k):  # any slice, the first, the last, and the existence row
        rows = list(ops)
        rows[r] = (_dev(broken), ops[row][1])
        bad_table = wah.bitop_operand_table(rows)
        for case in every:
            assert _status(wah, bad_table, case) == WAH_ERR_STREAM, (r, case["negate"])
    with pytest.raises(wah.WahError):
        _call(wah, bad_table, good)
    t = table.clone()
    t[5, 2] = 0  # a row without an index
    assert _status(wah, t, good) == WAH_ERR_STREAM
    # count > capacity; a descending pair inside the count; a descending pair behind the count
    assert _status(wah, table, dict(good, count=good["members"].size + 1)) == WAH_ERR_STREAM
    assert _status(wah, table, dict(good, count=(1 << 63) + 5)) == WAH_ERR_STREAM
    assert _status(wah, table, dict(good, count=good["members"].size)) == 0
    members = good["members"].copy()
    assert members.size >= 40 and members[20] < members[21]
    members[[20, 21]] = members[[21, 20]]
    swapped = dict(good, members=members)
    assert _status(wah, table, swapped) == WAH_ERR_STREAM
    assert _status(wah, table, dict(swapped, count=21)) == 0
    assert _status(wah, table, dict(swapped, count=22)) == WAH_ERR_STREAM
    last = good["members"].copy()
    last[-1] = last[-2] - np.uint64(1)
    assert _status(wah, table, dict(good, members=last)) == WAH_ERR_STREAM
    assert _status(wah, table, dict(good, members=last, count=last.size - 1)) == 0
    got, offs = _call(wah, table, dict(swapped, count=21))
    _same(streams, oracle, got, offs, mb.expected(dict(swapped, count=21)), "behind the count")
    # an output one word too small, with a guard behind the capacity
    need = int(oracle.compress(mb.expected(good)).size)
    assert need > 50
    small = torch.full((need + 63,), GUARD, dtype=torch.int32, device="cuda")
    assert _status(wah, table, good, out=small[:need]) == 0
    assert np.array_equal(_host(small[:need]), oracle.compress(mb.expected(good))) and bool((small[need:] == GUARD).all())
    small.fill_(GUARD)
    assert _status(wah, table, good, out=small[: need - 1]) == WAH_ERR_CAPACITY
    assert bool((small[need - 1:] == GUARD).all())


def test_front_end_refuses_bad_arguments(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    members = wah.member_set([1, 2], "cuda")
    words = torch.zeros(2, dtype=torch.int32, device="cuda")
    for bad in (lambda: wah.bsi_member_device([(stream, offs)] * 65, members, 0),
                lambda: wah.bsi_member_device([(stream, offs)], members, 0, exists=True),
                lambda: wah.bsi_member_device([(stream, offs)], words, 0),
                lambda: wah.bsi_member_device([(stream, offs)], members, 0, bitset=True),
                lambda: wah.bsi_member_device([(stream, offs)], words, 0, bitset=True, set_bits=65),
                lambda: wah.bsi_member_device([(stream, offs)], words, 0, bitset=True, count=torch.zeros(1, dtype=torch.int64, device="cuda")),
                lambda: wah.bsi_member_device([(stream, offs)], members, 0, count=torch.zeros(2, dtype=torch.int64, device="cuda"))):
        with pytest.raises(wah.WahError):
            bad()


# ---- 9: more than 2^32 rows ---------------------------------------------------------------------------------------------------------
def test_more_than_2_32_rows(wah, oracle):
    """A 2-slice column of 135 400 segments (rows 2^31 and 2^32 exist) whose constant segments hold 2 and whose few live segments hold
    random values, with an existence bitmap: IN (1, 3) selects rows of the live segments only, NOT IN (1, 3) more than 2^32 rows."""
    import torch

    segs = lg.A_SEGMENTS
    n = segs * lg.SEG_WORDS
    column, exists = lg.column(segs, lg.A_NAMED, 2, 77, 2), lg.operand(segs, 4)

    def member(negate):
        def fn(rows):
            v = (rows[0].astype(np.uint64) << np.uint64(1)) | rows[1].astype(np.uint64)
            return [(np.isin(v, [1, 3]) != negate).astype(np.uint8) & rows[2]]
        return lg.rowwise(fn, column + [exists])[0]

    stream, index = lg.expected_streams(oracle, column + [exists])
    d_stream, d_index = _dev(stream), _dev64(index)
    table = wah.columns.column_operand_table(d_stream, d_index, n, [0, 1, 2])
    scratch = torch.empty(int(wah.lib().wah_bsi_member_scratch_bytes(n, 2)), dtype=torch.uint8, device="cuda")
    members = wah.member_set([1, 3, 3, 4, 1 << 40], "cuda")
    for negate in (False, True):
        want = member(negate)
        assert (want.count() > 2**32) == negate and want.count() > 0
        want_stream, want_index = lg.expected_streams(oracle, [want])
        buf = torch.full((want_stream.size + 1,), GUARD, dtype=torch.int32, device="cuda")
        offs = torch.full((want_index.size,), -1, dtype=torch.int64, device="cuda")
        got, got_offs = wah.bsi_member_device(table, members, n, exists=True, negate=negate, scratch=scratch, out=buf[:-1], out_offsets=offs)
        assert int(buf[-1].item()) == GUARD and got.numel() == want_stream.size
        assert torch.equal(got_offs[: want_index.size], _dev64(want_index)) and torch.equal(got, _dev(want_stream)), negate


# ---- 10: the front ends ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star(wah):
    """A fact table of 2 * 31 744 rows with a 13-bit foreign key (NULLs: an existence bitmap) into a dimension table of 5000 rows
    (992 words: 31 744 row numbers, keys beyond 5000 dangle), an 8-bin key and a second attribute of 20 bits with NULLs."""
    import torch

    n, dim_n, dim_rows = SEG * 2, SEG, 5000
    rng = np.random.default_rng(10)
    fk = rng.integers(0, 8192, 32 * n).astype(np.uint64)
    fk_exists = rng.random(32 * n) < 0.9
    x = rng.integers(0, 3000, 32 * n).astype(np.uint64)
    x_exists = rng.random(32 * n) < 0.8
    y = rng.integers(1000, 5000, 32 * dim_n).astype(np.uint64)
    y[dim_rows:] = 0
    y_exists = (rng.random(32 * dim_n) < 0.7) & (np.arange(32 * dim_n) < dim_rows)
    region = rng.integers(0, 6, 32 * dim_n)
    region[dim_rows:] = 7
    keys = rng.integers(0, 8, 32 * n)
    cuda = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    c = wah.columns
    return dict(n=n, dim_n=dim_n, dim_rows=dim_rows, fk=fk, fk_exists=fk_exists, x=x, x_exists=x_exists, y=y, y_exists=y_exists, region=region,
                keys=keys,
                bsi_fk=c.bsi_from_values(wah, _dev64(fk), 13, exists=cuda(fk_exists)),
                bsi_x=c.bsi_from_values(wah, _dev64(x), 20, exists=cuda(x_exists)),
                bsi_x_plain=c.bsi_from_values(wah, _dev64(x), 20),
                bsi_y=c.bsi_from_values(wah, _dev64(y), 16, n_words_per_column=dim_n, exists=cuda(y_exists)),
                bsi_y_plain=c.bsi_from_values(wah, _dev64(y[:dim_rows]), 16, n_words_per_column=dim_n),
                dim_index=c.index_from_keys(wah, cuda(region), 8), index=c.index_from_keys(wah, cuda(keys), 8))


def test_isin_column(wah, oracle, star):
    import torch

    n, x, x_exists = star["n"], star["x"], star["x_exists"]
    streams = Streams(wah, n)
    wanted = [5, 17, 17, 2999, 1234, 4000, 1 << 50]
    for negate in (False, True):
        want = _bsi.pack_bits((np.isin(x, wanted) != negate) & x_exists)
        assert want.any()
        for values in (wanted, np.array(wanted, dtype=np.uint64), _dev64(np.array(wanted[::-1], dtype=np.uint64))):
            got, offs = wah.columns.isin_column(wah, star["bsi_x"], values, negate=negate)
            _same(streams, oracle, got, offs, want, ("isin", negate, type(values).__name__))
    got, offs = wah.columns.isin_column(wah, star["bsi_x_plain"], [])
    _same(streams, oracle, got, offs, np.zeros(n, np.uint32), "empty list")
    got, offs = wah.columns.isin_column(wah, star["bsi_x_plain"], torch.zeros(0, dtype=torch.int64, device="cuda"), negate=True)
    _same(streams, oracle, got, offs, np.full(n, 0xFFFFFFFF, np.uint32), "NOT IN ()")


def test_semi_join_rows_and_chaining(wah, oracle, star):
    """`WHERE fk IN (SELECT rowid FROM dim WHERE region IN (1, 4))`, the result as a predicate of filter_columns and count_columns_where."""
    n, dim_n, fk, fk_exists, region, keys = star["n"], star["dim_n"], star["fk"], star["fk_exists"], star["region"], star["keys"]
    streams = Streams(wah, n)
    dim_stream, dim_offsets, _ = star["dim_index"]
    dim_mask = wah.columns.filter_columns(wah, [(dim_stream, dim_offsets, [1, 4], False)], dim_n)
    selected = np.isin(region, [1, 4])
    assert selected.size == 32 * dim_n and fk.max() < selected.size and (fk >= star["dim_rows"]).any()
    for negate in (False, True):
        want = _bsi.pack_bits((selected[fk.astype(np.int64)] != negate) & fk_exists)
        got, offs = wah.columns.semi_join_rows(wah, star["bsi_fk"], dim_mask, dim_n, negate=negate)
        _same(streams, oracle, got, offs, want, ("semi_join_rows", negate))
    joined = _bsi.pack_bits(selected[fk.astype(np.int64)] & fk_exists)
    got, offs = wah.columns.semi_join_rows(wah, star["bsi_fk"], dim_mask, dim_n)
    key_stream, key_offsets, _ = star["index"]
    both, both_offs = wah.columns.filter_columns(wah, [(key_stream, key_offsets, [2, 5], False), (got, offs, [0], False)], n)
    _same(streams, oracle, both, both_offs, _bsi.pack_bits(np.isin(keys, [2, 5])) & joined, "join AND key IN")
    counts = wah.columns.count_columns_where(wah, [(got, offs, [0], False)], key_stream, key_offsets, n, list(range(8)))
    rows = _bsi.unpack_bits(joined)
    assert counts.tolist() == [int(((keys == b) & rows).sum()) for b in range(8)] and sum(counts.tolist()) > 0


def test_semi_join_values(wah, oracle, star):
    """`x IN (SELECT y FROM dim [WHERE region IN (0, 2)])` with NULLs on both sides: without a mask, under a mask, and under a mask
    with a list of a given capacity (no count is read back; a capacity below the selected rows is refused by the status)."""
    n, dim_n, dim_rows = star["n"], star["dim_n"], star["dim_rows"]
    x, x_exists, y, y_exists, region = star["x"], star["x_exists"], star["y"], star["y_exists"], star["region"]
    streams = Streams(wah, n)
    c = wah.columns
    for negate in (False, True):
        want = _bsi.pack_bits((np.isin(x, y[y_exists]) != negate) & x_exists)
        assert want.any() and not np.array_equal(want, _bsi.pack_bits((np.isin(x, y[:dim_rows]) != negate) & x_exists))
        got, offs = c.semi_join_values(wah, star["bsi_x"], star["bsi_y"], negate=negate)
        _same(streams, oracle, got, offs, want, ("no mask", negate))
    # no existence bitmap on the other side: every row of its bitmaps has a value, other_rows cuts them to the caller's
    got, offs = c.semi_join_values(wah, star["bsi_x"], star["bsi_y_plain"], other_rows=dim_rows)
    _same(streams, oracle, got, offs, _bsi.pack_bits(np.isin(x, y[:dim_rows]) & x_exists), "plain, cut")
    got, offs = c.semi_join_values(wah, star["bsi_x_plain"], star["bsi_y_plain"])
    _same(streams, oracle, got, offs, _bsi.pack_bits(np.isin(x, np.append(y[:dim_rows], 0))), "plain, whole")
    dim_stream, dim_offsets, _ = star["dim_index"]
    mask = c.filter_columns(wah, [(dim_stream, dim_offsets, [0, 2], False)], dim_n)
    selected = np.isin(region, [0, 2]) & y_exists
    for negate in (False, True):
        want = _bsi.pack_bits((np.isin(x, y[selected]) != negate) & x_exists)
        assert want.any()
        got, offs = c.semi_join_values(wah, star["bsi_x"], star["bsi_y"], other_mask=mask, negate=negate)
        _same(streams, oracle, got, offs, want, ("mask", negate))
        got, offs = c.semi_join_values(wah, star["bsi_x"], star["bsi_y"], other_mask=mask, negate=negate, capacity=int(selected.sum()) + 77)
        _same(streams, oracle, got, offs, want, ("mask, capacity", negate))
    got, offs = c.semi_join_values(wah, star["bsi_x"], star["bsi_y"], other_mask=mask, capacity=int(selected.sum()))
    _same(streams, oracle, got, offs, _bsi.pack_bits(np.isin(x, y[selected]) & x_exists), "mask, exact capacity")
    with pytest.raises(wah.WahError):
        c.semi_join_values(wah, star["bsi_x"], star["bsi_y"], other_mask=mask, capacity=int(selected.sum()) - 1)


# ---- 11: build -> member -> clause -> count, nothing read back; and as one captured graph ---------------------------------------------
def _swap_top_bits(values, k):
    a, b = np.uint64(1 << (k - 1)), np.uint64(1 << (k - 2))
    return (values & ~(a | b)) | np.where(values & a, b, np.uint64(0)) | np.where(values & b, a, np.uint64(0))


def test_chain_and_graph_replay(wah, oracle, star):
    """The chain with check=False throughout and one status read per call at the end; then the SAME four calls as one captured
    graph, replayed after the values, the set, its count and the slice table were overwritten in place: it answers the new query."""
    import torch

    n, k, keys = star["n"], 14, star["keys"]
    lib, c = wah.lib(), wah.columns
    rng = np.random.default_rng(11)
    key_stream, key_offsets, _ = star["index"]
    dev = key_stream.device
    d_values = torch.zeros(32 * n, dtype=torch.int64, device=dev)
    d_exists = torch.zeros(32 * n, dtype=torch.bool, device=dev)
    capacity = 600
    d_set = torch.zeros(capacity, dtype=torch.int64, device=dev)
    d_count = torch.zeros(1, dtype=torch.int64, device=dev)
    sc_build = torch.empty(int(lib.wah_bsi_build_scratch_bytes(n, k + 1)), dtype=torch.uint8, device=dev)
    sc_member = torch.empty(int(lib.wah_bsi_member_scratch_bytes(n, k)), dtype=torch.uint8, device=dev)
    sc_clause = torch.empty(int(lib.wah_bitop_clauses_scratch_bytes(n, 3, 2)), dtype=torch.uint8, device=dev)
    sc_count = torch.empty(int(lib.wah_select_scratch_bytes(n, 8)), dtype=torch.uint8, device=dev)
    built = torch.empty(wah.max_compressed_words((k + 1) * n), dtype=torch.int32, device=dev)
    built_offs = torch.zeros((k + 1) * (n // SEG) + 1, dtype=torch.int64, device=dev)
    res = torch.empty(wah.max_compressed_words(n), dtype=torch.int32, device=dev)
    res_offs = torch.zeros(n // SEG + 1, dtype=torch.int64, device=dev)
    both = torch.empty(wah.max_compressed_words(n), dtype=torch.int32, device=dev)
    both_offs = torch.zeros(n // SEG + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros((1, 8), dtype=torch.int64, device=dev)
    plain = c.column_operand_table(built, built_offs, n, list(range(k + 1)))
    swapped = c.column_operand_table(built, built_offs, n, [1, 0] + list(range(2, k + 1)))
    table = plain.clone()
    clause = wah.bitop_clause_table([([(key_stream[: key_stream.numel()], key_offsets)] * 2, False), ([(res, res_offs)], False)])
    c.column_operand_table(key_stream, key_offsets, n, [2, 5], out=clause[0][:2])
    mask = wah.bitop_operand_table([(both, both_offs)])
    bins = c.column_operand_table(key_stream, key_offsets, n, list(range(8)))

    def chain():
        wah.bsi_build_device(d_values, k, n, exists=d_exists, scratch=sc_build, out=built, out_offsets=built_offs, check=False)
        wah.bsi_member_device(table, d_set, n, count=d_count, exists=True, scratch=sc_member, out=res, out_offsets=res_offs, check=False)
        wah.bitop_clauses_indexed_device(clause, n, scratch=sc_clause, out=both, out_offsets=both_offs, check=False)
        wah.count_masked_device(mask, bins, n, scratch=sc_count, counts=counts, check=False)

    def query(seed, n_set, swap):
        """New values, set and count in place; the table names the slices in order or with the two top ones swapped.  Returns the
        counts the chain must leave."""
        r = np.random.default_rng(seed)
        values = r.integers(0, 1 << k, 32 * n).astype(np.uint64)
        exists = r.random(32 * n) < 0.85
        entries = np.sort(np.unique(values)[:: max(1, (1 << k) // (3 * max(n_set, 1)))][:n_set])
        listed = np.full(capacity, values[0], np.uint64)  # behind the count: a present value that is not in the set, out of order
        listed[: entries.size] = entries
        d_values.copy_(_dev64(values))
        d_exists.copy_(torch.from_numpy(exists).to(dev))
        d_set.copy_(_dev64(listed))
        d_count.fill_(int(entries.size))
        table.copy_(swapped if swap else plain)
        seen = _swap_top_bits(values, k) if swap else values
        rows = np.isin(seen, entries) & exists & np.isin(keys, [2, 5])
        return [int(((keys == b) & rows).sum()) for b in range(8)]

    def verdicts():
        return (lib.wah_bsi_build_status(sc_build.data_ptr(), n, k + 1, None), lib.wah_bsi_member_status(sc_member.data_ptr(), n, k, None),
                lib.wah_bitop_clauses_status(sc_clause.data_ptr(), n, 3, 2, None), lib.wah_select_status(sc_count.data_ptr(), None))

    want = query(1, 500, False)
    chain()
    assert verdicts() == (0, 0, 0, 0)  # (the first read synchronises: nothing was read back in between)
    assert counts.view(-1).tolist() == want and sum(want) > 0 and want[0] == want[7] == 0
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            chain()
    seen = set()
    for seed, n_set, swap in ((2, 300, False), (3, 40, True), (4, 600, True), (1, 500, False), (5, 0, False)):
        want = query(seed, n_set, swap)
        counts.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert verdicts() == (0, 0, 0, 0)
        assert counts.view(-1).tolist() == want, (seed, n_set, swap)
        seen.add(tuple(want))
    assert len(seen) == 5  # five different answers from one captured chain
    assert not np.array_equal(_swap_top_bits(np.arange(1 << k, dtype=np.uint64), k), np.arange(1 << k, dtype=np.uint64))
