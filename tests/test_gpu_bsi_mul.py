"""GPU tests of wah_bsi_mul_indexed_device: `A * B` row by row over two bit-sliced attributes, as a new bit-sliced attribute in one
call (include/wah.h), and its front ends in api.py and columns.py.  Everything is exact: the result's words, their count and its
whole segment index against the CPU oracle's compress() and an indexed compress of the slice matrix that numpy builds FROM THE
VALUES (tests/_mul.py); tests/test_mul_reference.py proves the model and that every case can fail.

The operands come from columns.bsi_from_values (at 64 bits, which that front end does not take, from api.bsi_build_device, the
call it is built on).  Every call here gets a scratch filled with 0xA5: a slice of the accumulator that a step reads or that
leaves without having been written shows.  The sweeps run at 992 words, 2 * 992 (a second segment: the wave's number is not 0 in
the address of its area and of a matrix row) and (WAH_SEG_WAVES + 1) * 992 (a second workgroup with idle waves)."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _mul

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6
SEG = 992
SEG_ROWS = 32 * SEG  # the rows of one segment
SEG_WAVES = 4  # WAH_SEG_WAVES: the wavefronts, one segment each, of a workgroup of the walk kernels


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
    """The row table in the order the TEST states (_mul.row_order): column c of an attribute's own matrix per entry."""
    import torch

    n = a[2]
    parts = [wah.columns.column_operand_table((a if who == "a" else b)[0], (a if who == "a" else b)[1], n, [c]) for who, c in order]
    return torch.cat(parts).contiguous()


def _scratch(wah, n, ka, n_out, flags):
    import torch

    return torch.full((int(wah.lib().wah_bsi_mul_scratch_bytes(n, ka, n_out, flags)),), 0xA5, dtype=torch.uint8, device="cuda:0")


def _mul_call(wah, a, b, n_out, have_a, have_b, **kw):
    """One bsi_mul_device call over two built attributes, operands AS GIVEN (no swap), the table in the test's own order."""
    n, ka, kb = a[2], a[3], b[3]
    assert (not have_a or a[4]) and (not have_b or b[4])
    flags = (wah.BSI_EXISTS_A if have_a else 0) | (wah.BSI_EXISTS_B if have_b else 0)
    table = _table(wah, _mul.row_order(ka, kb, have_a, have_b), a, b)
    return wah.bsi_mul_device(table, ka, kb, n_out, n, exists_a=have_a, exists_b=have_b, scratch=_scratch(wah, n, ka, n_out, flags), **kw)


class Pair:
    """Two value columns built as attributes, with and without their existence bitmaps (a row outside one is stored as 0, so the
    attribute without the bitmap is built from the values as they are)."""

    def __init__(self, wah, n, va, ka, vb, kb, xa, xb, existence=_mul.EXISTENCE):
        self.va, self.vb, self.ka, self.kb, self.xa, self.xb, self.n = va, vb, ka, kb, xa, xb, n
        need_a, need_b = {h for h, _ in existence}, {h for _, h in existence}
        self.a = {h: _build(wah, va, ka, n, xa if h else None) for h in need_a}
        self.b = {h: _build(wah, vb, kb, n, xb if h else None) for h in need_b}

    def check(self, wah, oracle, expected, n_out, have_a, have_b, what):
        got, offs = _mul_call(wah, self.a[have_a], self.b[have_b], n_out, have_a, have_b)
        want = _mul.expected_matrix(self.va, self.vb, n_out, self.xa if have_a else None, self.xb if have_b else None)
        _same(expected, oracle, got, offs, want, (what, have_a, have_b))


# ---- 1: the sweeps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SEG, SEG * 2, SEG * (SEG_WAVES + 1)])
@pytest.mark.parametrize("ka,kb,n_out", _mul.WIDTHS)
def test_sweep_vs_value_model(wah, oracle, expected, n, ka, kb, n_out):
    """Every width triple at every size; all four existence combinations at the smallest size, none and both above it."""
    existence = _mul.EXISTENCE if n == SEG else ((False, False), (True, True))
    va, vb, xa, xb, planted, _ = _mul.case(n, ka, kb, True, True)
    assert ((1 << ka) - 1, (1 << kb) - 1) in planted and (0, (1 << kb) - 1) in planted
    pair = Pair(wah, n, va, ka, vb, kb, xa, xb, existence)
    for have_a, have_b in existence:
        pair.check(wah, oracle, expected, n_out, have_a, have_b, (n, ka, kb, n_out))


# ---- 2: chunk edges of the 64-row table walk -------------------------------------------------------------------------------------------
def test_b_starts_inside_the_first_chunk_and_crosses_its_edge(wah, oracle, expected):
    """(40, 41) with A's existence row only: 82 table rows, B's first slice is row 41, its slice 23 row 64 -- the first of the second
    chunk -- and A's image, written during the first chunk, is read on both sides of the edge."""
    n, ka, kb = SEG * 2, 40, 41
    order = _mul.row_order(ka, kb, True, False)
    assert len(order) == 82 and order[41] == ("b", kb - 1) and order[64] == ("b", kb - 1 - 23)
    va, vb, xa, xb, _, _ = _mul.case(n, ka, kb, True, True, seed=1)
    _mul.assert_mul_matters(va, vb, ka, kb, 64, xa, None, "chunk edge")
    pair = Pair(wah, n, va, ka, vb, kb, xa, xb, ((True, False),))
    for n_out in (64, 20):
        pair.check(wah, oracle, expected, n_out, True, False, ("chunk edge", n_out))


def test_three_chunks(wah, oracle, expected):
    """(64, 64) with both flags: 130 table rows, A's image spans the first edge, B the second."""
    n, k = SEG * 2, 64
    assert len(_mul.row_order(k, k, True, True)) == 130
    va, vb, xa, xb, _, _ = _mul.case(n, k, k, True, True, seed=1)
    Pair(wah, n, va, k, vb, k, xa, xb, ((True, True),)).check(wah, oracle, expected, 64, True, True, "three chunks")


# ---- 3: settled and zero slices --------------------------------------------------------------------------------------------------------
ZERO = dict(n=SEG * 2, ka=20, kb=13, n_out=33)


def _zero_in_segment(wah, operand, column, n, seg):
    """Column `column` of the attribute is ONE zero fill in segment `seg`: settled in the gather, never a batch."""
    stream, offs = operand[0], operand[1]
    first = int(offs[column * (n // SEG) + seg].item())
    last = int(offs[column * (n // SEG) + seg + 1].item())
    return last - first == 1 and int(_host(stream[first:last])[0]) >> 30 == 2


@pytest.mark.parametrize("cleared", ["a", "b_middle", "b_first", "b_last", "b_last_two"])
def test_a_slice_that_is_zero_over_a_whole_segment(wah, oracle, expected, cleared):
    """A slice zeroed in every row of segment 0 and left as it is in segment 1.  a: a slice of A -- its image is zeros, folded from
    the zeroed LDS image; b_middle: the step is skipped, its carry slot still written; b_first: the j = 0 path, which never skips;
    b_last (and the last two): the skipped step's carry slot is the product's top slice, which leaves as zeros and not as the
    0xA5 of the scratch."""
    z = ZERO
    n, ka, kb, n_out = z["n"], z["ka"], z["kb"], z["n_out"]
    va, vb, xa, xb, _, _ = _mul.case(n, ka, kb, True, True, seed=2)
    in_seg0 = np.arange(32 * n) < SEG_ROWS
    which, bits = {"a": ("a", [7]), "b_middle": ("b", [6]), "b_first": ("b", [0]), "b_last": ("b", [kb - 1]), "b_last_two": ("b", [kb - 2, kb - 1])}[cleared]
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
    want = _mul.expected_matrix(va, vb, n_out, None, None)
    if cleared.startswith("b_last"):
        assert not want[0, :SEG].any() and want[0, SEG:].any()  # the top slice: empty in segment 0 alone
    for have_a, have_b in ((False, False), (True, True)):
        pair.check(wah, oracle, expected, n_out, have_a, have_b, cleared)


@pytest.mark.parametrize("c", [0, 1, 0b1000000100101, (1 << 13) - 1])
def test_a_constant_multiplier(wah, oracle, expected, c):
    """B is a constant: every slice is one fill per segment, all ones or zeros -- the set bits are fills WITH an effect, the
    others are settled and skipped."""
    z = ZERO
    n, ka, kb, n_out = z["n"], z["ka"], z["kb"], z["n_out"]
    va, _, xa, _, _, _ = _mul.case(n, ka, kb, True, True, seed=3)
    vb = np.full(va.shape, c, dtype=np.uint64)
    pair = Pair(wah, n, va, ka, vb, kb, xa, None, ((False, False), (True, False)))
    assert pair.b[False][0].numel() == kb * (n // SEG)  # nothing but one fill per slice and segment
    for have_a in (False, True):
        pair.check(wah, oracle, expected, n_out, have_a, False, ("constant", c))
    # ... and as A, where its slices become the image
    got, offs = _mul_call(wah, pair.b[False], pair.a[True], n_out, False, True)
    _same(expected, oracle, got, offs, _mul.expected_matrix(vb, va, n_out, None, xa), ("constant as A", c))


# ---- 4: chaining through columns --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attributes(wah):
    """Two attributes over the same 32 * 992 * 2 rows, 13 and 20 bits, both with an existence bitmap, and two more of the same widths
    for the capture that swaps the table."""
    n, ka, kb = SEG * 2, 13, 20
    va, vb, xa, xb, planted, _ = _mul.case(n, ka, kb, True, True, seed=4)
    wa, wb, ya, yb, _, _ = _mul.case(n, ka, kb, True, True, seed=5)
    return dict(n=n, ka=ka, kb=kb, va=va, vb=vb, xa=xa, xb=xb, planted=planted, a=_build(wah, va, ka, n, xa), b=_build(wah, vb, kb, n, xb),
                wa=wa, wb=wb, ya=ya, yb=yb, a2=_build(wah, wa, ka, n, ya), b2=_build(wah, wb, kb, n, yb))


def test_the_result_goes_into_the_other_calls(wah, oracle, expected, attributes):
    t = attributes
    n, ka, kb, va, vb, xa, xb = t["n"], t["ka"], t["kb"], t["va"], t["vb"], t["xa"], t["xb"]
    ex = xa & xb
    product = wah.columns.multiply_columns(wah, t["a"], t["b"])
    assert product[2:] == (n, ka + kb, True)
    want = _mul.expected_matrix(va, vb, ka + kb, xa, xb)
    _same(expected, oracle, product[0], product[1], want, "multiply_columns")
    # commutative, stream for stream: the wider attribute first is swapped behind the narrower
    swapped = wah.columns.multiply_columns(wah, t["b"], t["a"])
    assert swapped[2:] == product[2:] and swapped[0].numel() == product[0].numel() and bool((swapped[0] == product[0]).all())
    entries = (ka + kb + 1) * (n // SEG) + 1
    assert np.array_equal(swapped[1][:entries].cpu().numpy(), product[1][:entries].cpu().numpy())
    values = va * vb
    # `a * b` in a range
    lo, hi = 1 << 20, 1 << 30
    in_range = wah.columns.range_column(wah, product, lo, hi)
    selected = (values >= np.uint64(lo)) & (values <= np.uint64(hi)) & ex
    assert selected.any() and not np.array_equal(selected, ex)
    assert np.array_equal(_host(in_range[0]), oracle.compress(_bsi.pack_bits(selected)))
    # SUM(a * b) WHERE the product is in that range, in Python ints
    total = wah.columns.sum_product_where(wah, t["a"], t["b"], *in_range)
    assert total == sum(int(a) * int(b) for a, b in zip(va[selected], vb[selected])) and total > 1 << 40
    # MAX(a * b): the planted row of both operands all ones
    largest, count = wah.columns.max_column_where(wah, product)
    assert count == int(ex.sum()) and largest == int(values[ex].max()) == ((1 << ka) - 1) * ((1 << kb) - 1)
    # a * b + a
    more = wah.columns.add_columns(wah, product, t["a"])
    assert more[2:] == (n, ka + kb + 1, True)
    _same(expected, oracle, more[0], more[1], _bsi.build_slices(values + va, ka + kb + 1, ex, zero_missing=True), "product + a")
    # fewer slices truncate, more extend, through the front end
    for bits in (9, 40):
        cut = wah.columns.multiply_columns(wah, t["a"], t["b"], n_bits=bits)
        _same(expected, oracle, cut[0], cut[1], _mul.expected_matrix(va, vb, bits, xa, xb), ("n_bits", bits))


# ---- 5: graph replay --------------------------------------------------------------------------------------------------------------------
def test_graph_replay_over_a_rewritten_table(wah, oracle, expected, attributes):
    """The table is only ever read by the device: ONE captured call, replayed after the table was overwritten in place with two other
    attributes of the same widths, computes the NEW rows (capture as the arithmetic call's test: side stream, warm-up outside,
    check=False; one chain of launches, no parallel branches)."""
    import torch

    t = attributes
    n, ka, kb, k_out = t["n"], t["ka"], t["kb"], 33
    flags = wah.BSI_EXISTS_A | wah.BSI_EXISTS_B
    rows_out = k_out + 1
    sc = _scratch(wah, n, ka, k_out, flags)
    res = torch.empty(wah.max_compressed_words(rows_out * n), dtype=torch.int32, device="cuda:0")
    res_offs = torch.zeros(rows_out * (n // SEG) + 1, dtype=torch.int64, device="cuda:0")
    table = torch.zeros((ka + kb + 2, 3), dtype=torch.int64, device="cuda:0")
    reuse = dict(scratch=sc, out=res, out_offsets=res_offs, check=False)
    wah.columns.multiply_columns(wah, t["a"], t["b"], table=table, **reuse)  # fills the table; the warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _, count, _ = wah.bsi_mul_device(table, ka, kb, k_out, n, exists_a=True, exists_b=True, **reuse)
    seen = set()
    for first, second, want in ((t["a2"], t["b2"], _mul.expected_matrix(t["wa"], t["wb"], k_out, t["ya"], t["yb"])),
                                (t["a"], t["b2"], _mul.expected_matrix(t["va"], t["wb"], k_out, t["xa"], t["yb"])),
                                (t["a"], t["b"], _mul.expected_matrix(t["va"], t["vb"], k_out, t["xa"], t["xb"]))):
        table.copy_(_table(wah, _mul.row_order(ka, kb, True, True), first, second))  # rewrites the table in place
        torch.cuda.synchronize()
        res.fill_(0x5A5A5A5A)
        sc.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bsi_mul_status(sc.data_ptr(), n, ka, k_out, flags, None) == 0
        _same(expected, oracle, res[: int(count.item())], res_offs, want, "replay")
        seen.add(want.tobytes())
    assert len(seen) == 3  # different answers from one captured call


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------
def _status(wah, table, ka, kb, n_out, n, **kw):
    """Enqueue only; the verdict comes from the status call."""
    flags = wah.BSI_EXISTS_A | wah.BSI_EXISTS_B
    sc = _scratch(wah, n, ka, n_out, flags)
    wah.bsi_mul_device(table, ka, kb, n_out, n, exists_a=True, exists_b=True, scratch=sc, check=False, **kw)
    return int(wah.lib().wah_bsi_mul_status(sc.data_ptr(), n, ka, n_out, flags, None))


def test_refusals_come_from_the_status_call(wah, oracle):
    """What only the device sees is reported by the status call, and the verdict depends neither on the data nor on n_out: a
    broken segment in a slice of B above n_out, or where A is all zero, is refused like one in a slice of A.  The breaks are
    malformed words in a stream that is read within its bounds: a fill one group short, a fill of no groups."""
    import torch

    n, ka, kb = SEG * 2, 20, 13
    outs = (8, 33)
    va, vb, xa, xb, _, _ = _mul.case(n, ka, kb, True, True, seed=6)
    va = np.where(np.arange(32 * n) >= SEG_ROWS, np.uint64(0), va)  # A is all zero in segment 1
    a, b = _build(wah, va, ka, n, xa), _build(wah, vb, kb, n, xb)
    order = _mul.row_order(ka, kb, True, True)
    table = _table(wah, order, a, b)
    for n_out in outs:
        assert _status(wah, table, ka, kb, n_out, n) == 0
    # a stand-in row: literals at the head of either segment, zeros behind them -- one long zero fill per segment
    rng = np.random.default_rng(61)
    words = np.zeros(n, np.uint32)
    for s in range(n // SEG):
        words[s * SEG: s * SEG + 40] = rng.integers(1, 1 << 32, 40, dtype=np.uint64).astype(np.uint32)
    comp = wah.DeviceCompressor(n, indexed=True)
    comp.run(_dev(words))
    source, source_offs = comp.result().clone(), comp.seg_offsets.clone()
    good = _host(source).copy()
    bounds = [int(v) for v in source_offs.cpu().numpy()]
    fills = [max(range(bounds[s], bounds[s + 1]), key=lambda i: (good[i] >> 30 == 2) * (good[i] & 0x3FFFFFFF)) for s in range(n // SEG)]
    assert all(good[i] >> 30 == 2 and (good[i] & 0x3FFFFFFF) >= 2 for i in fills), "a long zero fill in either segment"
    # A's slice 3; B's slice 10, at or above the smaller n_out; B's slice 2
    places = dict(a=order.index(("a", ka - 1 - 3)), b_above=order.index(("b", kb - 1 - 10)), b_below=order.index(("b", kb - 1 - 2)))

    def with_row(r, stream):
        bad = table.clone()
        bad[r] = wah.bitop_operand_table([(stream, source_offs)])[0]
        return bad

    keep = []  # the tables hold raw pointers
    for r in places.values():  # the stand-in itself is accepted in every place: what is refused below is the break
        for n_out in outs:
            assert _status(wah, with_row(r, source), ka, kb, n_out, n) == 0
    for name, edit in (("short fill", lambda w: w - 1), ("empty fill", lambda w: w & 0xC0000000)):
        for where, r, seg in (("a", places["a"], 0), ("b above n_out", places["b_above"], 0), ("b where A is zero", places["b_below"], 1),
                              ("b above n_out where A is zero", places["b_above"], 1)):
            broken = good.copy()
            broken[fills[seg]] = edit(int(broken[fills[seg]]))
            stream = _dev(broken)
            keep.append(stream)
            bad_table = with_row(r, stream)
            verdicts = [_status(wah, bad_table, ka, kb, n_out, n) for n_out in outs]
            assert verdicts == [WAH_ERR_STREAM] * len(outs), (name, where, verdicts)
        with pytest.raises(wah.WahError):
            wah.bsi_mul_device(bad_table, ka, kb, 33, n, exists_a=True, exists_b=True)
    # a row without an index, or without a stream
    for r, col in ((places["a"], 2), (places["b_above"], 2), (0, 2), (places["b_below"], 0), (1, 0)):
        bad = table.clone()
        bad[r, col] = 0
        assert [_status(wah, bad, ka, kb, n_out, n) for n_out in outs] == [WAH_ERR_STREAM] * len(outs), (r, col)
    # an output one word too small, and a sentinel behind the capacity
    want = oracle.compress(np.ascontiguousarray(_mul.expected_matrix(va, vb, 33, xa, xb).reshape(-1)))
    need = int(want.size)
    assert need > 200
    small = torch.full((need + 63,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert _status(wah, table, ka, kb, 33, n, out=small[:need]) == 0
    assert np.array_equal(_host(small[:need]), want) and bool((small[need:] == 0x5A5A5A5A).all())
    small.fill_(0x5A5A5A5A)
    assert _status(wah, table, ka, kb, 33, n, out=small[: need - 1]) == WAH_ERR_CAPACITY
    assert bool((small[need - 1:] == 0x5A5A5A5A).all())


# ---- 7: front-end refusals ------------------------------------------------------------------------------------------------------------
def test_front_end_refusals(wah, attributes):
    import torch

    t = attributes
    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(wah.WahError):
        wah.bsi_mul_device([(stream, offs)] * 66, 65, 1, 8, SEG)
    with pytest.raises(wah.WahError):
        wah.bsi_mul_device([(stream, offs)] * 5, 3, 2, 4, SEG, exists_a=True)  # not 3 + 2 + 1 rows
    with pytest.raises(wah.WahError):
        wah.bsi_mul_device([(stream, offs)] * 5, 3, 2, 4, SEG + 1)
    with pytest.raises(wah.WahError):
        wah.bsi_mul_device([(stream, offs)] * 5, 3, 2, 65, SEG)
    shorter = _build(wah, t["va"][: 32 * SEG], t["ka"], SEG)
    with pytest.raises(ValueError):
        wah.columns.multiply_columns(wah, shorter, t["b"])  # different column lengths
    for bad in (torch.zeros((t["ka"] + t["kb"] + 1, 3), dtype=torch.int64, device="cuda"),      # a row short
                torch.zeros((t["ka"] + t["kb"] + 2, 3), dtype=torch.int32, device="cuda"),      # not int64
                torch.zeros((t["ka"] + t["kb"] + 2, 3), dtype=torch.int64)):                    # not on the device
        with pytest.raises(ValueError):
            wah.columns.multiply_columns(wah, t["a"], t["b"], table=bad)
    wide_a, wide_b = _build(wah, t["va"], 33, t["n"]), _build(wah, t["vb"], 32, t["n"])
    mask = (t["a"][0], t["a"][1][t["ka"] * (t["n"] // SEG):])
    with pytest.raises(ValueError):
        wah.columns.sum_product_where(wah, wide_a, wide_b, *mask)  # 65 bits: the product would be truncated
