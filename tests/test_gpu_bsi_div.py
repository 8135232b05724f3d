"""GPU tests of wah_bsi_div_indexed_device: `A / B` and `A % B` row by row over two bit-sliced attributes, as a new bit-sliced
attribute in one call (include/wah.h), and its front ends in api.py and columns.py.  Everything is exact: the result's words, their
count and its whole segment index against the CPU oracle's compress() and an indexed compress of the slice matrix that numpy
builds FROM THE VALUES (tests/_div.py); tests/test_div_reference.py proves the model and that every case can fail.

The operands come from columns.bsi_from_values (at 64 bits, which that front end does not take, from api.bsi_build_device, the
call it is built on).  Every call here gets a scratch filled with 0xA5: a slice of the remainder that a step reads or that leaves
without having been written shows.  The sweeps run at 992 words, 2 * 992 (a second segment: the wave's number is not 0 in the
address of its area and of a matrix row) and (WAH_SEG_WAVES + 1) * 992 (a second workgroup with idle waves)."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _div

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6
SEG = 992
SEG_ROWS = 32 * SEG  # the rows of one segment
SEG_WAVES = 4  # WAH_SEG_WAVES: the wavefronts, one segment each, of a workgroup of the walk kernels
MODES = (False, True)  # remainder


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


def _dev_values(values):
    import torch

    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


class Expected:
    """Indexed compressors of whole result matrices, one per matrix size, for the expected segment indexes."""

    def __init__(self, wah):
        self.wah, self.comps = wah, {}

    def of(self, matrix):
        comp = self.comps.get(matrix.size)
        if comp is None:
            comp = self.comps[matrix.size] = self.wah.DeviceCompressor(matrix.size, indexed=True)
        comp.run(_dev(matrix.reshape(-1)))
        return comp.result().clone(), comp.seg_offsets.clone()


@pytest.fixture(scope="module")
def expected(wah):
    return Expected(wah)


def _same(expected, oracle, got, offs, matrix, what):
    """(got, offs) is exactly compress(matrix as one bitmap) and its whole segment index."""
    want = np.ascontiguousarray(oracle.compress(np.ascontiguousarray(matrix.reshape(-1), dtype=np.uint32)), dtype=np.uint32)
    assert got.numel() == want.size, (what, got.numel(), want.size)
    assert np.array_equal(_host(got), want), what
    ref, ref_offs = expected.of(matrix)
    entries = matrix.shape[0] * (matrix.shape[1] // SEG) + 1
    assert offs.numel() >= entries == ref_offs.numel(), what
    assert np.array_equal(offs[:entries].cpu().numpy(), ref_offs.cpu().numpy()), what
    assert int(offs[entries - 1].item()) == want.size and np.array_equal(_host(ref), want), what


def _build(wah, values, bits, n, exists=None):
    """The five-tuple of bsi_from_values for a numpy uint64 column (exists: a numpy bool array or None)."""
    import torch

    x = None if exists is None else torch.from_numpy(exists).cuda()
    if bits <= 63:
        return wah.columns.bsi_from_values(wah, _dev_values(values), bits, n_words_per_column=n, exists=x)
    stream, offs = wah.bsi_build_device(_dev_values(values), bits, n, exists=x)
    return stream, offs, n, bits, x is not None


def _table(wah, order, a, b):
    """The row table in the order the TEST states (_div.row_order): column c of an attribute's own matrix per entry."""
    import torch

    n = a[2]
    parts = [wah.columns.column_operand_table((a if who == "a" else b)[0], (a if who == "a" else b)[1], n, [c]) for who, c in order]
    return torch.cat(parts).contiguous()


def _scratch(wah, n, kb, n_out, flags):
    import torch

    return torch.full((int(wah.lib().wah_bsi_div_scratch_bytes(n, kb, n_out, flags)),), 0xA5, dtype=torch.uint8, device="cuda:0")


def _div_call(wah, a, b, n_out, remainder, have_a, have_b, **kw):
    """One bsi_div_device call over two built attributes, the table in the test's own order."""
    n, ka, kb = a[2], a[3], b[3]
    assert (not have_a or a[4]) and (not have_b or b[4])
    flags = (wah.BSI_EXISTS_A if have_a else 0) | (wah.BSI_EXISTS_B if have_b else 0)
    table = _table(wah, _div.row_order(ka, kb, have_a, have_b), a, b)
    return wah.bsi_div_device(table, ka, kb, n_out, n, remainder=remainder, exists_a=have_a, exists_b=have_b,
                              scratch=_scratch(wah, n, kb, n_out, flags), **kw)


class Pair:
    """Two value columns built as attributes, with and without their existence bitmaps (a row outside one is stored as 0, so the
    attribute without the bitmap is built from the values as they are)."""

    def __init__(self, wah, n, va, ka, vb, kb, xa, xb, existence=_div.EXISTENCE):
        self.va, self.vb, self.ka, self.kb, self.xa, self.xb, self.n = va, vb, ka, kb, xa, xb, n
        need_a, need_b = {h for h, _ in existence}, {h for _, h in existence}
        self.a = {h: _build(wah, va, ka, n, xa if h else None) for h in need_a}
        self.b = {h: _build(wah, vb, kb, n, xb if h else None) for h in need_b}

    def check(self, wah, oracle, expected, n_out, have_a, have_b, what, modes=MODES):
        for remainder in modes:
            got, offs = _div_call(wah, self.a[have_a], self.b[have_b], n_out, remainder, have_a, have_b)
            want = _div.expected_matrix(self.va, self.vb, n_out, remainder, self.xa if have_a else None, self.xb if have_b else None)
            _same(expected, oracle, got, offs, want, (what, remainder, have_a, have_b))


# ---- 1: the sweeps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SEG, SEG * 2, SEG * (SEG_WAVES + 1)])
@pytest.mark.parametrize("ka,kb,n_out", _div.WIDTHS)
def test_sweep_vs_value_model(wah, oracle, expected, n, ka, kb, n_out):
    """Every width triple at every size, both results; all four existence combinations at the smallest size, none and both above
    it."""
    existence = _div.EXISTENCE if n == SEG else ((False, False), (True, True))
    va, vb, xa, xb, planted, _ = _div.case(n, ka, kb, True, True)
    assert ((1 << ka) - 1, 1) in planted and ((1 << ka) - 1, 0) in planted and (0, (1 << kb) - 1) in planted
    pair = Pair(wah, n, va, ka, vb, kb, xa, xb, existence)
    for have_a, have_b in existence:
        pair.check(wah, oracle, expected, n_out, have_a, have_b, (n, ka, kb, n_out))


# ---- 2: chunk edges of the 64-row table walk -------------------------------------------------------------------------------------------
def test_a_starts_inside_the_first_chunk_and_crosses_its_edge(wah, oracle, expected):
    """(40, 41) with A's existence row only: 82 table rows, A's top slice is row 42, its slice of significance 17 row 64 -- the first
    of the second chunk -- and B's image and the remainder, written during the first chunk, are read on both sides of the edge."""
    n, ka, kb = SEG * 2, 40, 41
    order = _div.row_order(ka, kb, True, False)
    assert len(order) == 82 and order[41] == ("b", 0) and order[42] == ("a", 0) and order[64] == ("a", ka - 1 - 17)
    va, vb, xa, xb, _, _ = _div.case(n, ka, kb, True, True, seed=1)
    for remainder in MODES:
        _div.assert_div_matters(va, vb, ka, kb, 40, remainder, xa, None, "chunk edge")
    pair = Pair(wah, n, va, ka, vb, kb, xa, xb, ((True, False),))
    for n_out in (40, 20):
        pair.check(wah, oracle, expected, n_out, True, False, ("chunk edge", n_out))


def test_three_chunks(wah, oracle, expected):
    """(64, 64) with both flags: 130 table rows, B's image spans the first edge, A the second."""
    n, k = SEG * 2, 64
    assert len(_div.row_order(k, k, True, True)) == 130
    va, vb, xa, xb, _, _ = _div.case(n, k, k, True, True, seed=1)
    Pair(wah, n, va, k, vb, k, xa, xb, ((True, True),)).check(wah, oracle, expected, 64, True, True, "three chunks")


# ---- 3: settled and zero slices --------------------------------------------------------------------------------------------------------
ZERO = dict(n=SEG * 2, ka=20, kb=13, n_out=20)


def _zero_in_segment(wah, operand, column, n, seg):
    """Column `column` of the attribute is ONE zero fill in segment `seg`: settled in the gather, never a batch."""
    stream, offs = operand[0], operand[1]
    first = int(offs[column * (n // SEG) + seg].item())
    last = int(offs[column * (n // SEG) + seg + 1].item())
    return last - first == 1 and int(_host(stream[first:last])[0]) >> 30 == 2


@pytest.mark.parametrize("cleared", ["a_top_three", "a_middle", "b_slice", "b_all"])
def test_a_slice_that_is_zero_over_a_whole_segment(wah, oracle, expected, cleared):
    """Slices zeroed in every row of segment 0 and left as they are in segment 1.  a_top_three: the skip runs in one segment and not
    in the other; a_middle: a zero slice of A below a non-zero one, which is not skipped -- the remainder is shifted all the same;
    b_slice: a slice of B's image is zeros, folded from the zeroed LDS image; b_all: every row of segment 0 is NULL, and its
    existence row is empty."""
    z = ZERO
    n, ka, kb, n_out = z["n"], z["ka"], z["kb"], z["n_out"]
    va, vb, xa, xb, _, _ = _div.case(n, ka, kb, True, True, seed=2)
    in_seg0 = np.arange(32 * n) < SEG_ROWS
    which, bits = {"a_top_three": ("a", [ka - 3, ka - 2, ka - 1]), "a_middle": ("a", [7]), "b_slice": ("b", [6]), "b_all": ("b", list(range(kb)))}[cleared]
    keep = ~np.uint64(sum(1 << j for j in bits))
    if which == "a":
        va = np.where(in_seg0, va & keep, va)
    else:
        vb = np.where(in_seg0, vb & keep, vb)
    pair = Pair(wah, n, va, ka, vb, kb, xa, xb, ((False, False), (True, True)))
    k = ka if which == "a" else kb
    for have in (False, True):
        op = (pair.a if which == "a" else pair.b)[have]
        for j in bits:
            assert _zero_in_segment(wah, op, k - 1 - j, n, 0) and not _zero_in_segment(wah, op, k - 1 - j, n, 1)
    want = _div.expected_matrix(va, vb, n_out, False, None, None)
    if cleared == "a_top_three":
        assert not want[:3, :SEG].any() and want[:3, SEG:].any() and want[3, :SEG].any()
    if cleared == "b_all":
        assert not want[:, :SEG].any() and want[n_out, SEG:].any()  # the existence row: empty in segment 0 alone
    for have_a, have_b in ((False, False), (True, True)):
        pair.check(wah, oracle, expected, n_out, have_a, have_b, cleared)


@pytest.mark.parametrize("c", [1, 64, 7, (1 << 13) - 1])
def test_a_constant_divisor(wah, oracle, expected, c):
    """B is a constant: every slice is one fill per segment, all ones or zeros."""
    z = ZERO
    n, ka, kb, n_out = z["n"], z["ka"], z["kb"], z["n_out"]
    va, _, xa, _, _, _ = _div.case(n, ka, kb, True, True, seed=3)
    vb = np.full(va.shape, c, dtype=np.uint64)
    pair = Pair(wah, n, va, ka, vb, kb, xa, None, ((False, False), (True, False)))
    assert pair.b[False][0].numel() == kb * (n // SEG)  # nothing but one fill per slice and segment
    for have_a in (False, True):
        pair.check(wah, oracle, expected, n_out, have_a, False, ("constant divisor", c))


def test_a_constant_dividend_and_a_column_over_itself(wah, oracle, expected):
    z = ZERO
    n, ka, kb, n_out = z["n"], z["ka"], z["kb"], z["n_out"]
    _, vb, _, xb, _, _ = _div.case(n, ka, kb, True, True, seed=3)
    va = np.full(vb.shape, 0b10110011100011110001, dtype=np.uint64)
    pair = Pair(wah, n, va, ka, vb, kb, None, xb, ((False, False), (False, True)))
    assert pair.a[False][0].numel() == ka * (n // SEG)
    for have_b in (False, True):
        pair.check(wah, oracle, expected, n_out, False, have_b, "constant dividend")
    # B / B, the same streams named twice: 1 where B is not zero, and nothing left over
    b = pair.b[True]
    for remainder in MODES:
        got, offs = _div_call(wah, b, b, kb, remainder, True, True)
        want = _div.expected_matrix(vb, vb, kb, remainder, xb, xb)
        ex = xb & (vb != 0)
        assert np.array_equal(want[kb], _bsi.pack_bits(ex)) and not want[: kb - 1].any()
        assert np.array_equal(want[kb - 1], np.zeros(n, np.uint32) if remainder else _bsi.pack_bits(ex))
        _same(expected, oracle, got, offs, want, ("itself", remainder))


# ---- 4: chaining through columns --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attributes(wah):
    """Two attributes over the same 32 * 992 * 2 rows, 20 and 13 bits, both with an existence bitmap, and two more of the same widths
    for the capture that swaps the table."""
    n, ka, kb = SEG * 2, 20, 13
    va, vb, xa, xb, planted, _ = _div.case(n, ka, kb, True, True, seed=4)
    wa, wb, ya, yb, _, _ = _div.case(n, ka, kb, True, True, seed=5)
    return dict(n=n, ka=ka, kb=kb, va=va, vb=vb, xa=xa, xb=xb, planted=planted, a=_build(wah, va, ka, n, xa), b=_build(wah, vb, kb, n, xb),
                wa=wa, wb=wb, ya=ya, yb=yb, a2=_build(wah, wa, ka, n, ya), b2=_build(wah, wb, kb, n, yb))


def test_the_result_goes_into_the_other_calls(wah, oracle, expected, attributes):
    t = attributes
    n, ka, kb, va, vb, xa, xb = t["n"], t["ka"], t["kb"], t["va"], t["vb"], t["xa"], t["xb"]
    ex = _div.existence(vb, xa, xb)
    assert ex.any() and not np.array_equal(ex, xa & xb)
    quotient = wah.columns.divide_columns(wah, t["a"], t["b"])
    rest = wah.columns.modulo_columns(wah, t["a"], t["b"])
    assert quotient[2:] == (n, ka, True) and rest[2:] == (n, min(ka, kb), True)
    _same(expected, oracle, quotient[0], quotient[1], _div.expected_matrix(va, vb, ka, False, xa, xb), "divide_columns")
    _same(expected, oracle, rest[0], rest[1], _div.expected_matrix(va, vb, kb, True, xa, xb), "modulo_columns")
    # q * b + r == a in exactly the rows that exist
    back = wah.columns.add_columns(wah, wah.columns.multiply_columns(wah, quotient, t["b"]), rest)
    equal = wah.columns.compare_columns(wah, back, "==", t["a"])
    assert np.array_equal(_host(equal[0]), oracle.compress(_bsi.pack_bits(ex)))
    assert int(_bsi.unpack_bits(oracle.decompress(_host(equal[0]).copy())[:n]).sum()) == int(ex.sum())
    # `a / b` in a range
    values = _div.expected_values(va, vb, ka, False)
    lo, hi = 3, 1 << 9
    in_range = wah.columns.range_column(wah, quotient, lo, hi)
    selected = (values >= np.uint64(lo)) & (values <= np.uint64(hi)) & ex
    assert selected.any() and not np.array_equal(selected, ex)
    assert np.array_equal(_host(in_range[0]), oracle.compress(_bsi.pack_bits(selected)))
    # MAX(a / b): the planted row of all ones over 1
    largest, count = wah.columns.max_column_where(wah, quotient)
    assert count == int(ex.sum()) and largest == int(values[ex].max()) == (1 << ka) - 1
    # a / 60, a % 60: a constant is never zero, so the rows that exist are A's
    for c in (60, 1, (1 << 22) + 5):
        constant = np.full(va.shape, c, dtype=np.uint64)
        by = wah.columns.divide_column_by(wah, t["a"], c)
        assert by[2:] == (n, ka, True)
        _same(expected, oracle, by[0], by[1], _div.expected_matrix(va, constant, ka, False, xa, None), ("divide_column_by", c))
        bits = min(ka, c.bit_length())
        by = wah.columns.divide_column_by(wah, t["a"], c, remainder=True)
        assert by[2:] == (n, bits, True)
        _same(expected, oracle, by[0], by[1], _div.expected_matrix(va, constant, bits, True, xa, None), ("divide_column_by %", c))
    # fewer slices truncate, more extend, through the front end
    for bits in (9, 30):
        cut = wah.columns.divide_columns(wah, t["a"], t["b"], n_bits=bits)
        _same(expected, oracle, cut[0], cut[1], _div.expected_matrix(va, vb, bits, False, xa, xb), ("n_bits", bits))
        cut = wah.columns.modulo_columns(wah, t["a"], t["b"], n_bits=bits)
        _same(expected, oracle, cut[0], cut[1], _div.expected_matrix(va, vb, bits, True, xa, xb), ("n_bits %", bits))


# ---- 5: graph replay --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remainder", MODES)
def test_graph_replay_over_a_rewritten_table(wah, oracle, expected, attributes, remainder):
    """The table is only ever read by the device: ONE captured call, replayed after the table was overwritten in place with two other
    attributes of the same widths, computes the NEW rows (capture as the multiplication call's test: side stream, warm-up outside,
    check=False; one chain of launches, no parallel branches)."""
    import torch

    t = attributes
    n, ka, kb, k_out = t["n"], t["ka"], t["kb"], 20
    flags = wah.BSI_EXISTS_A | wah.BSI_EXISTS_B
    rows_out = k_out + 1
    sc = _scratch(wah, n, kb, k_out, flags)
    res = torch.empty(wah.max_compressed_words(rows_out * n), dtype=torch.int32, device="cuda:0")
    res_offs = torch.zeros(rows_out * (n // SEG) + 1, dtype=torch.int64, device="cuda:0")
    table = torch.zeros((ka + kb + 2, 3), dtype=torch.int64, device="cuda:0")
    reuse = dict(scratch=sc, out=res, out_offsets=res_offs, check=False)
    front = wah.columns.modulo_columns if remainder else wah.columns.divide_columns
    front(wah, t["a"], t["b"], n_bits=k_out, table=table, **reuse)  # fills the table; the warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _, count, _ = wah.bsi_div_device(table, ka, kb, k_out, n, remainder=remainder, exists_a=True, exists_b=True, **reuse)
    seen = set()
    for first, second, want in ((t["a2"], t["b2"], _div.expected_matrix(t["wa"], t["wb"], k_out, remainder, t["ya"], t["yb"])),
                                (t["a"], t["b2"], _div.expected_matrix(t["va"], t["wb"], k_out, remainder, t["xa"], t["yb"])),
                                (t["a"], t["b"], _div.expected_matrix(t["va"], t["vb"], k_out, remainder, t["xa"], t["xb"]))):
        table.copy_(_table(wah, _div.row_order(ka, kb, True, True), first, second))  # rewrites the table in place
        torch.cuda.synchronize()
        res.fill_(0x5A5A5A5A)
        sc.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bsi_div_status(sc.data_ptr(), n, kb, k_out, flags, None) == 0
        _same(expected, oracle, res[: int(count.item())], res_offs, want, "replay")
        seen.add(want.tobytes())
    assert len(seen) == 3  # different answers from one captured call


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------
def _status(wah, table, ka, kb, n_out, n, remainder, **kw):
    """Enqueue only; the verdict comes from the status call."""
    flags = wah.BSI_EXISTS_A | wah.BSI_EXISTS_B
    sc = _scratch(wah, n, kb, n_out, flags)
    wah.bsi_div_device(table, ka, kb, n_out, n, remainder=remainder, exists_a=True, exists_b=True, scratch=sc, check=False, **kw)
    return int(wah.lib().wah_bsi_div_status(sc.data_ptr(), n, kb, n_out, flags, None))


def test_refusals_come_from_the_status_call(wah, oracle):
    """What only the device sees is reported by the status call, and the verdict depends neither on the data, nor on the result
    asked for, nor on n_out: a broken segment in a slice of A at or above n_out, or in one the skip passes over, is refused like
    one in a slice of B.  The breaks are malformed words in a stream that is read within its bounds: a fill one group short, a fill
    of no groups."""
    import torch

    n, ka, kb = SEG * 2, 20, 13
    calls = [(n_out, remainder) for n_out in (8, 20) for remainder in MODES]
    va, vb, xa, xb, _, _ = _div.case(n, ka, kb, True, True, seed=6)
    va = np.where(np.arange(32 * n) >= SEG_ROWS, va & np.uint64((1 << (ka - 2)) - 1), va)  # A's top two slices are zero in segment 1
    a, b = _build(wah, va, ka, n, xa), _build(wah, vb, kb, n, xb)
    order = _div.row_order(ka, kb, True, True)
    table = _table(wah, order, a, b)
    for n_out, remainder in calls:
        assert _status(wah, table, ka, kb, n_out, n, remainder) == 0
    # a stand-in row: literals at the head of segment 0 and zeros behind them -- one long zero fill; segment 1 all zero -- one fill
    rng = np.random.default_rng(61)
    words = np.zeros(n, np.uint32)
    words[:40] = rng.integers(1, 1 << 32, 40, dtype=np.uint64).astype(np.uint32)
    comp = wah.DeviceCompressor(n, indexed=True)
    comp.run(_dev(words))
    source, source_offs = comp.result().clone(), comp.seg_offsets.clone()
    good = _host(source).copy()
    bounds = [int(v) for v in source_offs.cpu().numpy()]
    fills = [max(range(bounds[s], bounds[s + 1]), key=lambda i: (good[i] >> 30 == 2) * (good[i] & 0x3FFFFFFF)) for s in range(n // SEG)]
    assert all(good[i] >> 30 == 2 and (good[i] & 0x3FFFFFFF) >= 2 for i in fills), "a long zero fill in either segment"
    assert bounds[2] - bounds[1] == 1, "segment 1 of the stand-in is one zero fill"
    # A's slice 10, at or above the smaller n_out; A's slice ka - 2, which the skip passes over in segment 1; B's slice 2
    places = dict(a_above=order.index(("a", ka - 1 - 10)), a_skipped=order.index(("a", 1)), b=order.index(("b", kb - 1 - 2)))

    def with_row(r, stream):
        bad = table.clone()
        bad[r] = wah.bitop_operand_table([(stream, source_offs)])[0]
        return bad

    keep = []  # the tables hold raw pointers
    for r in places.values():  # the stand-in itself is accepted in every place: what is refused below is the break
        for n_out, remainder in calls:
            assert _status(wah, with_row(r, source), ka, kb, n_out, n, remainder) == 0
    for name, edit in (("short fill", lambda w: w - 1), ("empty fill", lambda w: w & 0xC0000000)):
        for where, r, seg in (("a above n_out", places["a_above"], 0), ("a that the skip passes over", places["a_skipped"], 1),
                              ("b", places["b"], 0), ("b, a segment of one fill", places["b"], 1)):
            broken = good.copy()
            broken[fills[seg]] = edit(int(broken[fills[seg]]))
            stream = _dev(broken)
            keep.append(stream)
            bad_table = with_row(r, stream)
            verdicts = [_status(wah, bad_table, ka, kb, n_out, n, remainder) for n_out, remainder in calls]
            assert verdicts == [WAH_ERR_STREAM] * len(calls), (name, where, verdicts)
        with pytest.raises(wah.WahError):
            wah.bsi_div_device(bad_table, ka, kb, 20, n, exists_a=True, exists_b=True)
    # a row without an index, or without a stream
    for r, col in ((places["a_above"], 2), (places["a_skipped"], 2), (0, 2), (places["b"], 0), (1, 0)):
        bad = table.clone()
        bad[r, col] = 0
        assert [_status(wah, bad, ka, kb, n_out, n, remainder) for n_out, remainder in calls] == [WAH_ERR_STREAM] * len(calls), (r, col)
    # an output one word too small, and a sentinel behind the capacity
    want = oracle.compress(np.ascontiguousarray(_div.expected_matrix(va, vb, 20, False, xa, xb).reshape(-1)))
    need = int(want.size)
    assert need > 200
    small = torch.full((need + 63,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert _status(wah, table, ka, kb, 20, n, False, out=small[:need]) == 0
    assert np.array_equal(_host(small[:need]), want) and bool((small[need:] == 0x5A5A5A5A).all())
    small.fill_(0x5A5A5A5A)
    assert _status(wah, table, ka, kb, 20, n, False, out=small[: need - 1]) == WAH_ERR_CAPACITY
    assert bool((small[need - 1:] == 0x5A5A5A5A).all())


# ---- 7: front-end refusals ------------------------------------------------------------------------------------------------------------
def test_front_end_refusals(wah, attributes):
    import torch

    t = attributes
    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(wah.WahError):
        wah.bsi_div_device([(stream, offs)] * 66, 65, 1, 8, SEG)
    with pytest.raises(wah.WahError):
        wah.bsi_div_device([(stream, offs)] * 5, 3, 2, 4, SEG, exists_a=True)  # not 3 + 2 + 1 rows
    with pytest.raises(wah.WahError):
        wah.bsi_div_device([(stream, offs)] * 5, 3, 2, 4, SEG + 1)
    with pytest.raises(wah.WahError):
        wah.bsi_div_device([(stream, offs)] * 5, 3, 2, 65, SEG)
    shorter = _build(wah, t["va"][: 32 * SEG], t["ka"], SEG)
    for front in (wah.columns.divide_columns, wah.columns.modulo_columns):
        with pytest.raises(ValueError):
            front(wah, shorter, t["b"])  # different column lengths
        for bad in (torch.zeros((t["ka"] + t["kb"] + 1, 3), dtype=torch.int64, device="cuda"),      # a row short
                    torch.zeros((t["ka"] + t["kb"] + 2, 3), dtype=torch.int32, device="cuda"),      # not int64
                    torch.zeros((t["ka"] + t["kb"] + 2, 3), dtype=torch.int64)):                    # not on the device
            with pytest.raises(ValueError):
                front(wah, t["a"], t["b"], table=bad)
    with pytest.raises(ValueError):
        wah.columns.divide_column_by(wah, t["a"], 0)
