"""GPU tests of wah_bsi_compare_indexed_device: `A op B` row by row over two bit-sliced attributes in one call (include/wah.h), and
its front ends in api.py and columns.py.  Everything is exact: the result's words, their count and its segment index against
compress() of the bitmap computed with numpy FROM THE VALUES (tests/_cmp.py) -- the CPU oracle and an indexed compress of it.

The sweeps run at 1, 31, 992 and 992 * 3 + 5 words over pairs of widths that put the table's edges where the kernel can go wrong:
(41, 40), (40, 41) and (1, 64) have a held A slice in table row 63 and its B slice in row 64, the first of the second chunk of 64
rows; (64, 64) with both existence rows is 130 rows, three chunks.  Wherever there is room for the planted rows the test first
asserts, with numpy alone, that it can fail: each of the six answers is neither empty nor full, all six differ, every single
slice of either attribute changes the answer, and so does either existence row."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _cmp

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6
SEG = 992
MIRROR = {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "==": "==", "!=": "!="}


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


class Pair:
    """Two attributes as indexed compressed slices (existence rows always built), and their tables for any existence combination.
    The tables hold raw pointers: the object stays alive while they are used."""

    def __init__(self, streams, va, ka, vb, kb, xa, xb):
        self.va, self.vb, self.ka, self.kb, self.xa, self.xb = va, vb, ka, kb, xa, xb
        self.ops_a = [streams.of(row) for row in _bsi.build_slices(va, ka, xa)]
        self.ops_b = [streams.of(row) for row in _bsi.build_slices(vb, kb, xb)]

    def rows(self, have_a, have_b):
        return [(self.ops_a if who == "a" else self.ops_b)[i] for who, i in _cmp.row_order(self.ka, self.kb, have_a, have_b)]

    def want(self, op, have_a, have_b):
        return _cmp.expected_compare(self.va, self.vb, op, self.xa if have_a else None, self.xb if have_b else None)


def _check_all(wah, oracle, streams, pair, n, what, existence=_cmp.EXISTENCE):
    for have_a, have_b in existence:
        table = wah.bitop_operand_table(pair.rows(have_a, have_b))
        for op in _cmp.OPS:
            got, offs = wah.bsi_compare_device(table, pair.ka, pair.kb, op, n, exists_a=have_a, exists_b=have_b)
            _same(streams, oracle, got, offs, pair.want(op, have_a, have_b), (what, op, have_a, have_b))


# ---- 1: the sweeps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, SEG, SEG * 3 + 5])
@pytest.mark.parametrize("ka,kb", [(1, 1), (20, 13), (13, 20), (64, 64), (1, 64), (41, 40), (40, 41)])
def test_sweep_vs_value_model(wah, oracle, n, ka, kb):
    """Every existence combination and all six operators; the case first shown to be able to fail wherever the planted rows fit."""
    what = (n, ka, kb)
    if n >= 31:
        va, vb, xa, xb = _cmp.case(n, ka, kb, True, True)
        for have_a, have_b in _cmp.EXISTENCE:
            _cmp.assert_compare_matters(va, vb, ka, kb, xa if have_a else None, xb if have_b else None, (what, have_a, have_b))
    else:  # 32 rows have no room for two planted rows per bit
        rng = np.random.default_rng(100 * ka + kb)
        va = _bsi.uniform_values(rng, 32 * n, ka)
        vb = np.where(rng.random(32 * n) < 0.5, _bsi.uniform_values(rng, 32 * n, kb), va & np.uint64((1 << kb) - 1))
        xa, xb = rng.random(32 * n) < 0.9, rng.random(32 * n) < 0.9
    streams = Streams(wah, n)
    _check_all(wah, oracle, streams, Pair(streams, va, ka, vb, kb, xa, xb), n, what)


# ---- 2: settled rows at the chunk edge ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cleared", ["a", "b"])
def test_settled_rows_at_the_chunk_edge_are_folded(wah, oracle, cleared):
    """(41, 40) at 992 + 31 words (two segments, the second ragged): table row 63 is A's slice of significance 8, row 64 is B's.
    With bit 8 of every A value cleared row 63 is one zero fill per segment -- settled in the gather, never a batch -- and must
    still be held as zeros, not as the slice held before it; with bit 8 of every B value cleared row 64 is settled, and the fold of
    the pair comes from the next row's number."""
    n, ka, kb, sig = SEG + 31, 41, 40, 8
    order = _cmp.row_order(ka, kb, True, True)
    assert order[63] == ("a", ka - 1 - sig) and order[64] == ("b", kb - 1 - sig)
    va, vb, xa, xb = _cmp.case(n, ka, kb, True, True, seed=1)
    bit = np.uint64(1 << sig)
    if cleared == "a":
        va = va & ~bit
    else:
        vb = vb & ~bit
    streams = Streams(wah, n)
    pair = Pair(streams, va, ka, vb, kb, xa, xb)
    settled = pair.ops_a[ka - 1 - sig] if cleared == "a" else pair.ops_b[kb - 1 - sig]
    assert settled[0].numel() == 2 and all(int(w) >> 30 == 2 for w in _host(settled[0]))  # one zero fill per segment
    other = pair.ops_b[kb - 1 - sig] if cleared == "a" else pair.ops_a[ka - 1 - sig]
    assert other[0].numel() > 2
    # a sweep that drops the pair of significance 8 answers differently, and so does one that keeps holding A's slice 9
    def differs(a, b):
        return any(not np.array_equal(_cmp.expected_compare(a, b, op, xa, xb), pair.want(op, True, True)) for op in (">", "=="))

    assert differs(va & ~bit, vb & ~bit)
    assert differs((va & ~bit) | (((va >> np.uint64(sig + 1)) & np.uint64(1)) << np.uint64(sig)), vb)
    _check_all(wah, oracle, streams, pair, n, cleared)


# ---- 3: value kinds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["low", "high", "clustered"])
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("ka,kb", [(20, 20), (64, 40)])
@pytest.mark.parametrize("existence", ["dense", "segment missing in B"])
def test_value_kinds(wah, oracle, kind, which, ka, kb, existence):
    """low: the top 10 slices of one attribute are all zero (settled in the gather, still folded against the other's bits); high: all
    ones (one fill with an effect per segment); clustered: fills with an effect in every slice -- against a uniform attribute, in
    either place.  Existence at density 0.9, once with a whole segment whose rows do not exist in B."""
    n = SEG * 3 + 5
    rows = 32 * n
    rng = np.random.default_rng(1000 * ka + kb + len(kind) + (which == "b"))
    special, plain = (ka, kb) if which == "a" else (kb, ka)
    v_special, v_plain = _bsi.make_values(kind, rng, rows, special), _bsi.uniform_values(rng, rows, plain)
    va, vb = ((v_special, v_plain) if which == "a" else (v_plain, v_special))
    va, vb = va.copy(), vb.copy()
    at = rng.permutation(rows)[:64]  # some equal rows, so that == and != are not trivial
    va[at] = vb[at] = vb[at] & np.uint64((1 << min(ka, kb)) - 1)
    xa, xb = rng.random(rows) < 0.9, rng.random(rows) < 0.9
    xa[at] = xb[at] = True
    if existence == "segment missing in B":
        xb[32 * SEG: 64 * SEG] = False
        assert not _bsi.pack_bits(xb)[SEG: 2 * SEG].any() and _bsi.pack_bits(xb)[2 * SEG:].any()
    streams = Streams(wah, n)
    pair = Pair(streams, va, ka, vb, kb, xa, xb)
    assert pair.want("==", True, True).any() and pair.want("!=", True, True).any()
    assert not np.array_equal(pair.want(">", True, True), pair.want(">=", True, True))
    _check_all(wah, oracle, streams, pair, n, (kind, which, ka, kb, existence), existence=((True, True), (False, False)))


# ---- 4, 5: rows behind the caller's own, and no rows at all ---------------------------------------------------------------------------
def test_rows_without_existence_match_equality(wah, oracle):
    """Without an existence bitmap the rows behind the caller's own hold 0 in both attributes: they match ==, <= and >= and no other
    operator.  With existence rows they match none."""
    n, own = SEG + 7, 1000
    rng = np.random.default_rng(12)
    va, vb = np.zeros(32 * n, np.uint64), np.zeros(32 * n, np.uint64)
    va[:own] = _bsi.uniform_values(rng, own, 12) | np.uint64(1)
    vb[:own] = np.where(rng.random(own) < 0.5, va[:own] & np.uint64(0x1FF), _bsi.uniform_values(rng, own, 9) | np.uint64(1))
    exists = np.arange(32 * n) < own
    streams = Streams(wah, n)
    pair = Pair(streams, va, 12, vb, 9, exists, exists)
    for op in _cmp.OPS:
        behind = _bsi.unpack_bits(pair.want(op, False, False))[own:]
        assert behind.all() if op in ("==", "<=", ">=") else not behind.any(), op
        for have in ((True, False), (False, True), (True, True)):
            assert not _bsi.unpack_bits(pair.want(op, *have))[own:].any() and pair.want(op, *have).any(), (op, have)
    _check_all(wah, oracle, streams, pair, n, "rows behind the caller's own")


def test_empty_bitmap(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    for have_a, have_b in _cmp.EXISTENCE:
        for op in _cmp.OPS:
            got, out_offs = wah.bsi_compare_device([(stream, offs)] * (3 + 2 + have_a + have_b), 3, 2, op, 0, exists_a=have_a, exists_b=have_b)
            assert got.numel() == 0 and int(out_offs[0].item()) == 0


# ---- 6: the column front end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attributes(wah):
    """Two attributes over the same 32 * 992 * 2 rows, built by bsi_from_values: 20 and 13 bits, both with an existence bitmap, and
    a third of 20 bits (B widened) for the capture that swaps the two."""
    import torch

    n, ka, kb = SEG * 2, 20, 13
    va, vb, xa, xb = _cmp.case(n, ka, kb, True, True, seed=2)

    def build(values, bits, exists):
        return wah.columns.bsi_from_values(wah, torch.from_numpy(values.view(np.int64)).cuda(), bits, exists=torch.from_numpy(exists).cuda())

    return dict(n=n, ka=ka, kb=kb, va=va, vb=vb, xa=xa, xb=xb, a=build(va, ka, xa), b=build(vb, kb, xb), b_wide=build(vb, ka, xb))


def test_compare_columns(wah, oracle, attributes):
    import torch

    t = attributes
    n, va, vb, xa, xb = t["n"], t["va"], t["vb"], t["xa"], t["xb"]
    streams = Streams(wah, n)
    want = _cmp.assert_compare_matters(va, vb, t["ka"], t["kb"], xa, xb, "front end")
    got = {}
    for op in _cmp.OPS:
        got[op] = wah.columns.compare_columns(wah, t["a"], op, t["b"])
        _same(streams, oracle, *got[op], want[op], ("compare_columns", op))
        mirrored = wah.columns.compare_columns(wah, t["b"], MIRROR[op], t["a"])
        _same(streams, oracle, *mirrored, want[op], ("compare_columns mirrored", op))
    # `A > B AND lo <= A <= hi`: the comparison is one more predicate beside a range_column result
    lo, hi = (1 << 20) // 4, (3 << 20) // 4
    in_range = _bsi.expected_range(va, lo, hi, xa)
    both_want = want[">"] & in_range
    assert both_want.any() and not np.array_equal(both_want, want[">"]) and not np.array_equal(both_want, in_range)
    rng_stream, rng_offs = wah.columns.range_column(wah, t["a"], lo, hi)
    both, both_offs = wah.columns.filter_columns(wah, [(got[">"][0], got[">"][1], [0], False), (rng_stream, rng_offs, [0], False)], n)
    _same(streams, oracle, both, both_offs, both_want, "A > B AND BETWEEN")
    # != is the negated == predicate within both existence bitmaps
    eq, eq_offs = got["=="]
    ne, ne_offs = wah.columns.filter_columns(wah, [(eq, eq_offs, [0], True), (t["a"][0], t["a"][1], [t["ka"]], False), (t["b"][0], t["b"][1], [t["kb"]], False)], n)
    assert ne.numel() == got["!="][0].numel() and bool((ne == got["!="][0]).all())
    assert np.array_equal(ne_offs.cpu().numpy()[: n // SEG + 1], got["!="][1].cpu().numpy()[: n // SEG + 1])
    # refusals of the front end
    with pytest.raises(ValueError):
        wah.columns.compare_columns(wah, t["a"], "=", t["b"])
    short = wah.columns.bsi_from_values(wah, torch.from_numpy(vb[:5000].view(np.int64).copy()).cuda(), t["kb"], n_words_per_column=SEG)
    with pytest.raises(ValueError):
        wah.columns.compare_columns(wah, t["a"], "<", short)
    table = wah.columns.column_operand_table(t["a"][0], t["a"][1], n, list(range(t["ka"] + 1)))
    with pytest.raises(wah.WahError):
        wah.bsi_compare_device(table, t["ka"], t["kb"], "<", n, exists_a=True, exists_b=True)  # not ka + kb + 2 rows


# ---- 7: graph replay ------------------------------------------------------------------------------------------------------------
def test_graph_replay_with_the_attributes_swapped(wah, oracle, attributes):
    """The table is only ever read by the device: ONE captured call, replayed after the table was rewritten in place to compare B
    with A, gives the mirrored answer (capture as the range call's test: side stream, warm-up outside, check=False)."""
    import torch

    t = attributes
    n, k, va, vb, xa, xb = t["n"], t["ka"], t["va"], t["vb"], t["xa"], t["xb"]
    streams = Streams(wah, n)
    sc = torch.empty(int(wah.lib().wah_bsi_compare_scratch_bytes(n, k, k)), dtype=torch.uint8, device="cuda:0")
    res = torch.empty(wah.max_compressed_words(n), dtype=torch.int32, device="cuda:0")
    res_offs = torch.zeros(n // SEG + 2, dtype=torch.int64, device="cuda:0")
    table = torch.zeros((2 * k + 2, 3), dtype=torch.int64, device="cuda:0")
    reuse = dict(scratch=sc, out=res, out_offsets=res_offs, check=False)
    wah.columns.compare_columns(wah, t["a"], ">", t["b_wide"], table=table, **reuse)  # fills the table; the warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _, count, _ = wah.bsi_compare_device(table, k, k, ">", n, exists_a=True, exists_b=True, **reuse)
    seen = set()
    for first, second, want in ((t["a"], t["b_wide"], _cmp.expected_compare(va, vb, ">", xa, xb)),
                                (t["b_wide"], t["a"], _cmp.expected_compare(vb, va, ">", xb, xa)),
                                (t["a"], t["a"], np.zeros(n, np.uint32))):
        wah.columns.compare_columns(wah, first, "==", second, table=table, **reuse)  # rewrites the table in place (its own call: another operator)
        torch.cuda.synchronize()
        res.fill_(0x5A5A5A5A)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bsi_compare_status(sc.data_ptr(), n, k, k, None) == 0
        _same(streams, oracle, res[: int(count.item())], res_offs[: n // SEG + 1], want, "replay")
        seen.add(want.tobytes())
    assert len(seen) == 3  # different answers from one captured call
    assert np.array_equal(_cmp.expected_compare(vb, va, ">", xb, xa), _cmp.expected_compare(va, vb, "<", xa, xb))


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------
def _status(wah, table, ka, kb, op, n, **kw):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    sc = torch.empty(int(wah.lib().wah_bsi_compare_scratch_bytes(n, ka, kb)), dtype=torch.uint8, device="cuda:0")
    wah.bsi_compare_device(table, ka, kb, op, n, exists_a=True, exists_b=True, scratch=sc, check=False, **kw)
    return int(wah.lib().wah_bsi_compare_status(sc.data_ptr(), n, ka, kb, None))


def test_refusals_come_from_the_status_call(wah, oracle):
    """What only the device sees -- a row whose segment does not add up, an empty fill, a row without an index or a stream, too small
    an output -- is reported by the status call, and the verdict is the same under every operator."""
    import torch

    n, ka, kb = SEG * 4, 12, 9
    rng = np.random.default_rng(43)
    va = _bsi.make_values("clustered", rng, 32 * n, ka)
    vb = np.where(rng.random(32 * n) < 0.5, va & np.uint64((1 << kb) - 1), _bsi.uniform_values(rng, 32 * n, kb))
    xa, xb = rng.random(32 * n) < 0.9, rng.random(32 * n) < 0.9
    streams = Streams(wah, n)
    pair = Pair(streams, va, ka, vb, kb, xa, xb)
    order = _cmp.row_order(ka, kb, True, True)
    good = pair.rows(True, True)
    table = wah.bitop_operand_table(good)
    for op in _cmp.OPS:
        assert _status(wah, table, ka, kb, op, n) == 0
    # a fill of a clustered slice of A, one group shorter: the segment's groups do not add up; and the same fill emptied
    source = pair.ops_a[3]
    words = _host(source[0]).copy()
    fills = np.flatnonzero((words >> 31 == 1) & ((words & 0x3FFFFFFF) >= 2))
    assert fills.size, "a clustered slice has fills"
    at = int(fills[fills.size // 2])
    places = (order.index(("a", 3)), order.index(("b", 4)), order.index(("a", ka)), order.index(("b", kb)), 0, ka + kb - 1)
    for name, word in (("short fill", words[at] - 1), ("empty fill", words[at] & 0xC0000000)):
        broken = words.copy()
        broken[at] = word
        for r in places:  # an A slice, a B slice, either existence row, the first and the last slice
            rows = list(good)
            rows[r] = (_dev(broken), source[1])
            bad_table = wah.bitop_operand_table(rows)
            for op in _cmp.OPS:
                assert _status(wah, bad_table, ka, kb, op, n) == WAH_ERR_STREAM, (name, r, op)
        with pytest.raises(wah.WahError):
            wah.bsi_compare_device(bad_table, ka, kb, ">", n, exists_a=True, exists_b=True)
    # a row without an index, or without a stream
    for r, col in ((0, 2), (places[1], 2), (places[2], 2), (places[3], 2), (5, 0), (places[3], 0)):
        t = table.clone()
        t[r, col] = 0
        for op in _cmp.OPS:
            assert _status(wah, t, ka, kb, op, n) == WAH_ERR_STREAM, (r, col, op)
    # an output one word too small, for a result of many words
    need = int(oracle.compress(pair.want(">", True, True)).size)
    assert need > 200
    out, count, _ = wah.bsi_compare_device(table, ka, kb, ">", n, exists_a=True, exists_b=True, check=False)
    torch.cuda.synchronize()
    assert int(count.item()) == need
    small = torch.full((need + 63,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert _status(wah, table, ka, kb, ">", n, out=small[:need]) == 0
    assert bool((small[:need] == out[:need]).all()) and bool((small[need:] == 0x5A5A5A5A).all())
    small.fill_(0x5A5A5A5A)
    assert _status(wah, table, ka, kb, ">", n, out=small[: need - 1]) == WAH_ERR_CAPACITY
    assert bool((small[need - 1:] == 0x5A5A5A5A).all())


def test_front_end_refuses_bad_tables(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(wah.WahError):
        wah.bsi_compare_device([(stream, offs)] * 66, 65, 1, "<", 0)
    with pytest.raises(wah.WahError):
        wah.bsi_compare_device([(stream, offs)] * 5, 3, 2, "<", 0, exists_a=True)
    with pytest.raises(wah.WahError):
        wah.bsi_compare_device([(stream, offs)] * 5, 3, 2, "<>", 0)
