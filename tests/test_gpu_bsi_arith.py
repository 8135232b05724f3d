"""GPU tests of wah_bsi_arith_indexed_device: `A + B` and `A - B` row by row over two bit-sliced attributes, as a new bit-sliced
attribute in one call (include/wah.h), and its front ends in api.py and columns.py.  Everything is exact: the result's words,
their count and its whole segment index against the CPU oracle's compress() and an indexed compress of the slice matrix that numpy
builds FROM THE VALUES (tests/_arith.py); tests/test_arith_reference.py proves the model and that every case can fail.

The sweeps run at 992 words, 2 * 992 (a second segment: the wave's segment number is not 0 in the address of a matrix row) and
(WAH_SEG_WAVES + 1) * 992 (a second workgroup), over the widths of _arith.WIDTHS: (64, 64, 64) with both existence rows is 130
table rows, three chunks of 64; (20, 13, 8) truncates -- the slices at and above 8 are walked and stored nowhere; (13, 20, 40)
extends."""
import importlib

import numpy as np
import pytest

from tests import _arith, _bsi, _cmp

pytestmark = pytest.mark.gpu

WAH_ERR_CAPACITY, WAH_ERR_STREAM = -4, -6
SEG = 992
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


class Streams:
    """One indexed compressor of n_words, reused for the operands' slices."""

    def __init__(self, wah, n_words):
        self.comp = wah.DeviceCompressor(n_words, indexed=True)

    def of(self, words):
        self.comp.run(_dev(words))
        return self.comp.result().clone(), self.comp.seg_offsets.clone()


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


def _same(expected, oracle, got, offs, matrix, what):
    """(got, offs) is exactly compress(matrix as one bitmap) and its whole segment index."""
    want = np.ascontiguousarray(oracle.compress(np.ascontiguousarray(matrix.reshape(-1), dtype=np.uint32)), dtype=np.uint32)
    assert got.numel() == want.size, (what, got.numel(), want.size)
    assert np.array_equal(_host(got), want), what
    ref, ref_offs = expected.of(matrix)
    assert offs.numel() == matrix.shape[0] * (matrix.shape[1] // SEG) + 1 == ref_offs.numel(), what
    assert np.array_equal(offs.cpu().numpy(), ref_offs.cpu().numpy()), what
    assert int(offs[-1].item()) == want.size and np.array_equal(_host(ref), want), what


class Pair:
    """Two attributes as indexed compressed slices (existence rows always built), and their tables for any existence combination.
    The tables hold raw pointers: the object stays alive while they are used."""

    def __init__(self, streams, va, ka, vb, kb, xa, xb):
        self.va, self.vb, self.ka, self.kb, self.xa, self.xb = va, vb, ka, kb, xa, xb
        self.ops_a = [streams.of(row) for row in _bsi.build_slices(va, ka, xa)]
        self.ops_b = [streams.of(row) for row in _bsi.build_slices(vb, kb, xb)]

    def rows(self, have_a, have_b):
        return [(self.ops_a if who == "a" else self.ops_b)[i] for who, i in _arith.row_order(self.ka, self.kb, have_a, have_b)]

    def want(self, op, n_out, have_a, have_b):
        return _arith.expected_matrix(self.va, self.vb, op, n_out, self.xa if have_a else None, self.xb if have_b else None)


def _check(wah, oracle, expected, pair, op, n_out, n, what, existence=_arith.EXISTENCE):
    for have_a, have_b in existence:
        table = wah.bitop_operand_table(pair.rows(have_a, have_b))
        got, offs = wah.bsi_arith_device(table, pair.ka, pair.kb, op, n_out, n, exists_a=have_a, exists_b=have_b)
        _same(expected, oracle, got, offs, pair.want(op, n_out, have_a, have_b), (what, op, have_a, have_b))


# ---- 1: the sweeps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SEG, SEG * 2, SEG * (SEG_WAVES + 1)])
@pytest.mark.parametrize("ka,kb,n_out", _arith.WIDTHS)
def test_sweep_vs_value_model(wah, oracle, n, ka, kb, n_out):
    """Both operations and every existence combination; the case is first shown to be able to fail."""
    streams, expected = Streams(wah, n), Expected(wah)
    for op in _arith.OPS:
        va, vb, xa, xb, _ = _arith.case(n, ka, kb, op, True, True)
        for have_a, have_b in _arith.EXISTENCE:
            _arith.assert_arith_matters(va, vb, ka, kb, n_out, xa if have_a else None, xb if have_b else None, (n, ka, kb, n_out, have_a, have_b))
        _check(wah, oracle, expected, Pair(streams, va, ka, vb, kb, xa, xb), op, n_out, n, (n, ka, kb, n_out))


# ---- 2, 3: the chunk edge, and settled rows ------------------------------------------------------------------------------------------
EDGE = dict(n=SEG * 2, ka=40, kb=41, n_out=42, sig=31)


def _edge_case(op, seed=0):
    e = EDGE
    order = _arith.row_order(e["ka"], e["kb"], True, False)
    # table row 63 is A's slice of significance 31, row 64 -- the first of the second chunk of 64 rows -- is B's
    assert order[63] == ("a", e["ka"] - 1 - e["sig"]) and order[64] == ("b", e["kb"] - 1 - e["sig"]) and len(order) == 82
    return _arith.case(e["n"], e["ka"], e["kb"], op, True, True, seed=seed)


def _zero_fills(operand, n):
    """The slice is one zero fill per segment: settled in the gather, never a batch."""
    return operand[0].numel() == n // SEG and all(int(w) >> 30 == 2 for w in _host(operand[0]))


@pytest.mark.parametrize("op", _arith.OPS)
def test_chunk_edge(wah, oracle, op):
    """(40, 41, 42) with A's existence row only, at two segments: the held slice crosses from one chunk of 64 table rows to the next."""
    e = EDGE
    va, vb, xa, xb, _ = _edge_case(op)
    _arith.assert_arith_matters(va, vb, e["ka"], e["kb"], e["n_out"], xa, None, "chunk edge")
    streams = Streams(wah, e["n"])
    _check(wah, oracle, Expected(wah), Pair(streams, va, e["ka"], vb, e["kb"], xa, xb), op, e["n_out"], e["n"], "chunk edge", existence=((True, False),))


@pytest.mark.parametrize("op", _arith.OPS)
@pytest.mark.parametrize("cleared", ["a", "b", "both", "tail"])
def test_settled_rows_still_advance_the_carry_and_emit(wah, oracle, op, cleared):
    """A slice that is one zero fill per segment is settled in the gather and never reaches the walk's batches; it is folded from the
    zeroed image all the same.  a: bit 31 of every A value cleared -- the held row, table row 63 with A's existence row; b: bit 31
    of every B value cleared -- the closing row 64; both: bits 31 .. 33 of both cleared while the planted row 2^31 - 1 + 1 carries
    into 31 -- that slice comes from the carry alone, the next from nothing; tail: the top three slices of both cleared -- the last
    table rows are settled and folded behind the walk."""
    e = EDGE
    n, ka, kb, n_out, sig = e["n"], e["ka"], e["kb"], e["n_out"], e["sig"]
    va, vb, xa, xb, planted = _edge_case(op, seed=1)
    bit = np.uint64(1 << sig)
    three = np.uint64(7 << sig)
    if cleared == "a":
        va = va & ~bit
    elif cleared == "b":
        vb = vb & ~bit
    elif cleared == "both":
        va, vb = va & ~three, vb & ~three
    else:
        va, vb = va & np.uint64((1 << (ka - 3)) - 1), vb & np.uint64((1 << (kb - 3)) - 1)
    streams = Streams(wah, n)
    pair = Pair(streams, va, ka, vb, kb, xa, xb)
    a_of, b_of = (lambda s: pair.ops_a[ka - 1 - s]), (lambda s: pair.ops_b[kb - 1 - s])
    if cleared == "a":
        assert _zero_fills(a_of(sig), n) and not _zero_fills(b_of(sig), n)
        # a sweep that keeps holding A's slice 30 instead answers differently
        stale = va | (((va >> np.uint64(sig - 1)) & np.uint64(1)) << np.uint64(sig))
        assert not np.array_equal(_arith.expected_values(stale, vb, op, n_out)[xa], _arith.expected_values(va, vb, op, n_out)[xa])
    elif cleared == "b":
        assert _zero_fills(b_of(sig), n) and not _zero_fills(a_of(sig), n)
    elif cleared == "both":
        assert all(_zero_fills(f(s), n) for f in (a_of, b_of) for s in (sig, sig + 1, sig + 2))
        row = planted[((1 << sig) - 1, 1)]
        assert int(va[row]) == (1 << sig) - 1 and int(vb[row]) == 1
        want = pair.want(op, n_out, True, False)
        if op == "+":  # slice 31 is the carry alone, set in the planted row; slices 32 and 33 come from nothing
            carried = _bsi.unpack_bits(want[n_out - 1 - sig])
            assert carried[row] and not want[n_out - 2 - sig].any() and not want[n_out - 3 - sig].any()
        else:  # the borrow runs through the three zero slices
            assert want[n_out - 1 - sig].any() and np.array_equal(want[n_out - 2 - sig], want[n_out - 1 - sig])
    else:
        assert all(_zero_fills(a_of(s), n) for s in range(ka - 3, ka)) and all(_zero_fills(b_of(s), n) for s in range(kb - 3, kb))
        assert _arith.row_order(ka, kb, True, False)[-1] == ("b", 0) and not _zero_fills(a_of(ka - 4), n)
    _check(wah, oracle, Expected(wah), pair, op, n_out, n, cleared, existence=((True, False), (False, False), (True, True)))


# ---- 4: the tail rows ---------------------------------------------------------------------------------------------------------------
def test_the_carry_slice_of_a_sum_is_set_exactly_where_it_overflows(wah, oracle):
    n, k = SEG * 2, 20
    rows = 32 * n
    rng = np.random.default_rng(20)
    va, vb = _bsi.uniform_values(rng, rows, k - 1), _bsi.uniform_values(rng, rows, k - 1)  # no row overflows 2^k ...
    at = rng.permutation(rows)[:6]
    va[at] = np.array([(1 << k) - 1, 1 << (k - 1), (1 << k) - 1, 1, (1 << k) - 2, 0x80001], dtype=np.uint64)  # ... but these six
    vb[at] = np.array([1, 1 << (k - 1), (1 << k) - 1, (1 << k) - 1, 2, 0x80000], dtype=np.uint64)
    overflow = np.zeros(rows, bool)
    overflow[at] = True
    assert np.array_equal((va + vb) >= np.uint64(1 << k), overflow)
    streams, expected = Streams(wah, n), Expected(wah)
    pair = Pair(streams, va, k, vb, k, np.ones(rows, bool), np.ones(rows, bool))
    got, offs = wah.bsi_arith_device(wah.bitop_operand_table(pair.rows(False, False)), k, k, "+", k + 1, n)
    _same(expected, oracle, got, offs, pair.want("+", k + 1, False, False), "carry slice")
    segs = n // SEG
    top = _host(got[int(offs[0].item()): int(offs[segs].item())])
    assert np.array_equal(top, oracle.compress(_bsi.pack_bits(overflow)))


@pytest.fixture(scope="module")
def attributes(wah):
    """Two attributes over the same 32 * 992 * 2 rows, built by bsi_from_values: 20 and 13 bits, both with an existence bitmap, from
    the SUB case (its planted rows: borrows through every slice, A = B, A = B +- 2^j), and two more of the same widths for the
    capture that swaps the table."""
    import torch

    n, ka, kb = SEG * 2, 20, 13
    va, vb, xa, xb, planted = _arith.case(n, ka, kb, "-", True, True, seed=2)
    wa, wb, ya, yb, _ = _arith.case(n, ka, kb, "+", True, True, seed=3)

    def build(values, bits, exists):
        return wah.columns.bsi_from_values(wah, _dev_values(values), bits, exists=torch.from_numpy(exists).cuda())

    return dict(n=n, ka=ka, kb=kb, va=va, vb=vb, xa=xa, xb=xb, planted=planted, a=build(va, ka, xa), b=build(vb, kb, xb),
                wa=wa, wb=wb, ya=ya, yb=yb, a2=build(wa, ka, ya), b2=build(wb, kb, yb))


def test_the_top_slice_of_a_difference_is_the_less_than_bitmap(wah, oracle, attributes):
    t = attributes
    n, segs = t["n"], t["n"] // SEG
    assert (t["va"] < t["vb"]).any() and (t["va"] > t["vb"]).any()
    diff = wah.columns.subtract_columns(wah, t["a"], t["b"])
    assert diff[2:] == (n, max(t["ka"], t["kb"]) + 1, True)
    less, less_offs = wah.columns.compare_columns(wah, t["a"], "<", t["b"])
    first, last = int(diff[1][0].item()), int(diff[1][segs].item())
    assert last - first == less.numel() and bool((diff[0][first:last] == less).all())
    assert np.array_equal(diff[1][: segs + 1].cpu().numpy() - first, less_offs[: segs + 1].cpu().numpy())
    assert np.array_equal(_host(less), oracle.compress(_cmp.expected_compare(t["va"], t["vb"], "<", t["xa"], t["xb"])))
    _same(Expected(wah), oracle, diff[0], diff[1], _arith.expected_matrix(t["va"], t["vb"], "-", 21, t["xa"], t["xb"]), "subtract_columns")


# ---- 5: chaining through columns --------------------------------------------------------------------------------------------------------
def test_the_result_goes_into_the_other_calls(wah, oracle, attributes):
    import torch

    t = attributes
    n, ka, kb, va, vb, xa, xb = t["n"], t["ka"], t["kb"], t["va"], t["vb"], t["xa"], t["xb"]
    segs, ex = n // SEG, xa & xb
    total = wah.columns.add_columns(wah, t["a"], t["b"])
    assert total[2:] == (n, 21, True)
    _same(Expected(wah), oracle, total[0], total[1], _arith.expected_matrix(va, vb, "+", 21, xa, xb), "add_columns")
    # fetch: every planted row and a random thousand
    rng = np.random.default_rng(8)
    rows = np.concatenate([np.array(sorted(t["planted"].values()), dtype=np.int64), rng.choice(32 * n, size=1000, replace=False).astype(np.int64)])
    values, have = wah.columns.values_at_rows(wah, total, torch.from_numpy(rows).cuda())
    assert np.array_equal(have.cpu().numpy(), ex[rows]) and ex[rows].any() and not ex[rows].all()
    assert np.array_equal(values.cpu().numpy().view(np.uint64), np.where(ex[rows], va[rows] + vb[rows], np.uint64(0)))
    # SUM over the rows that exist in both: the result's own existence bitmap is the mask
    mask = (total[0], total[1][21 * segs:])
    assert wah.columns.sum_column_where(wah, total, *mask) == sum(int(v) for v in (va + vb)[ex])
    # (A - B) + B, cut to A's width, is A again where both exist: stream for stream what the builder makes of those values
    back = wah.columns.add_columns(wah, wah.columns.subtract_columns(wah, t["a"], t["b"]), t["b"], n_bits=ka)
    again = wah.columns.bsi_from_values(wah, _dev_values(va), ka, exists=torch.from_numpy(ex).cuda())
    assert back[2:] == again[2:] == (n, ka, True)
    assert back[0].numel() == again[0].numel() and bool((back[0] == again[0]).all())
    assert np.array_equal(back[1].cpu().numpy(), again[1].cpu().numpy())
    # `a - b <= c` as the docstring of subtract_columns states it
    c = 1000
    diff = wah.columns.subtract_columns(wah, t["a"], t["b"])
    in_range = wah.columns.range_column(wah, diff, 0, c)
    not_less = wah.columns.compare_columns(wah, t["a"], ">=", t["b"])
    got, _ = wah.columns.filter_columns(wah, [(*in_range, [0], False), (*not_less, [0], False)], n)
    want = (va.astype(np.int64) - vb.astype(np.int64) <= c) & (va >= vb) & ex
    assert want.any() and not np.array_equal(want, (va >= vb) & ex)
    assert np.array_equal(_host(got), oracle.compress(_bsi.pack_bits(want)))
    # the k-th largest sum
    largest, selected = wah.columns.kth_column_where(wah, total, 0, largest=True)
    assert selected == int(ex.sum()) and largest == int((va + vb)[ex].max())


# ---- 6: graph replay --------------------------------------------------------------------------------------------------------------------
def test_graph_replay_over_a_rewritten_table(wah, oracle, attributes):
    """The table is only ever read by the device: ONE captured call, replayed after the table was overwritten in place with two other
    attributes of the same widths, computes the NEW rows (capture as the compare call's test: side stream, warm-up outside,
    check=False; one chain of launches, no parallel branches)."""
    import torch

    t = attributes
    n, ka, kb, k_out = t["n"], t["ka"], t["kb"], 21
    flags = wah.BSI_EXISTS_A | wah.BSI_EXISTS_B
    rows_out = k_out + 1
    sc = torch.empty(int(wah.lib().wah_bsi_arith_scratch_bytes(n, k_out, flags)), dtype=torch.uint8, device="cuda:0")
    res = torch.empty(wah.max_compressed_words(rows_out * n), dtype=torch.int32, device="cuda:0")
    res_offs = torch.zeros(rows_out * (n // SEG) + 1, dtype=torch.int64, device="cuda:0")
    table = torch.zeros((ka + kb + 2, 3), dtype=torch.int64, device="cuda:0")
    reuse = dict(scratch=sc, out=res, out_offsets=res_offs, check=False)
    wah.columns.subtract_columns(wah, t["a"], t["b"], table=table, **reuse)  # fills the table; the warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _, count, _ = wah.bsi_arith_device(table, ka, kb, "-", k_out, n, exists_a=True, exists_b=True, **reuse)
    expected = Expected(wah)
    seen = set()
    for first, second, want in ((t["a2"], t["b2"], _arith.expected_matrix(t["wa"], t["wb"], "-", k_out, t["ya"], t["yb"])),
                                (t["a"], t["b2"], _arith.expected_matrix(t["va"], t["wb"], "-", k_out, t["xa"], t["yb"])),
                                (t["a"], t["b"], _arith.expected_matrix(t["va"], t["vb"], "-", k_out, t["xa"], t["xb"]))):
        wah.columns.add_columns(wah, first, second, table=table, **reuse)  # rewrites the table in place (its own call: the other operation)
        torch.cuda.synchronize()
        res.fill_(0x5A5A5A5A)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_bsi_arith_status(sc.data_ptr(), n, k_out, flags, None) == 0
        _same(expected, oracle, res[: int(count.item())], res_offs, want, "replay")
        seen.add(want.tobytes())
    assert len(seen) == 3  # different answers from one captured call


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------------
def _status(wah, table, ka, kb, op, n_out, n, **kw):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    flags = wah.BSI_EXISTS_A | wah.BSI_EXISTS_B
    sc = torch.empty(int(wah.lib().wah_bsi_arith_scratch_bytes(n, n_out, flags)), dtype=torch.uint8, device="cuda:0")
    wah.bsi_arith_device(table, ka, kb, op, n_out, n, exists_a=True, exists_b=True, scratch=sc, check=False, **kw)
    return int(wah.lib().wah_bsi_arith_status(sc.data_ptr(), n, n_out, flags, None))


def test_refusals_come_from_the_status_call(wah, oracle):
    """What only the device sees is reported by the status call, and the verdict depends neither on the operation nor on n_out: a
    broken segment in a slice at or above n_out, which contributes nothing, is refused like one below it."""
    import torch

    n, ka, kb, n_out = SEG * 4, 20, 13, 8
    rng = np.random.default_rng(47)
    va = _bsi.make_values("clustered", rng, 32 * n, ka)
    vb = np.where(rng.random(32 * n) < 0.5, va & np.uint64((1 << kb) - 1), _bsi.uniform_values(rng, 32 * n, kb))
    xa, xb = rng.random(32 * n) < 0.9, rng.random(32 * n) < 0.9
    streams = Streams(wah, n)
    pair = Pair(streams, va, ka, vb, kb, xa, xb)
    order = _arith.row_order(ka, kb, True, True)
    good = pair.rows(True, True)
    table = wah.bitop_operand_table(good)
    for op in _arith.OPS:
        assert _status(wah, table, ka, kb, op, n_out, n) == 0
    # a fill of a clustered slice of A, one group shorter: the segment's groups do not add up; and the same fill emptied
    source = pair.ops_a[ka - 1 - 15]  # significance 15: above n_out
    words = _host(source[0]).copy()
    fills = np.flatnonzero((words >> 31 == 1) & ((words & 0x3FFFFFFF) >= 2))
    assert fills.size, "a clustered slice has fills"
    at = int(fills[fills.size // 2])
    # A's slice 15 and its last one (both at or above n_out), A's slice 3 and B's slice 3 (below), either existence row
    places = (order.index(("a", ka - 1 - 15)), order.index(("a", 0)), order.index(("a", ka - 1 - 3)), order.index(("b", kb - 1 - 3)), 0, 1)
    assert places[0] > 2 + 2 * n_out and places[1] == len(order) - 1
    for name, word in (("short fill", words[at] - 1), ("empty fill", words[at] & 0xC0000000)):
        broken = words.copy()
        broken[at] = word
        for r in places:
            rows = list(good)
            rows[r] = (_dev(broken), source[1])
            bad_table = wah.bitop_operand_table(rows)
            for op in _arith.OPS:
                for k_out in (n_out, 21):
                    assert _status(wah, bad_table, ka, kb, op, k_out, n) == WAH_ERR_STREAM, (name, r, op, k_out)
        with pytest.raises(wah.WahError):
            wah.bsi_arith_device(bad_table, ka, kb, "+", n_out, n, exists_a=True, exists_b=True)
    # a row without an index, or without a stream
    for r, col in ((places[0], 2), (places[3], 2), (0, 2), (places[1], 0), (1, 0)):
        bad = table.clone()
        bad[r, col] = 0
        for op in _arith.OPS:
            assert _status(wah, bad, ka, kb, op, n_out, n) == WAH_ERR_STREAM, (r, col, op)
    # an output one word too small, and a sentinel behind the capacity
    want = oracle.compress(np.ascontiguousarray(pair.want("-", n_out, True, True).reshape(-1)))
    need = int(want.size)
    assert need > 200
    small = torch.full((need + 63,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert _status(wah, table, ka, kb, "-", n_out, n, out=small[:need]) == 0
    assert np.array_equal(_host(small[:need]), want) and bool((small[need:] == 0x5A5A5A5A).all())
    small.fill_(0x5A5A5A5A)
    assert _status(wah, table, ka, kb, "-", n_out, n, out=small[: need - 1]) == WAH_ERR_CAPACITY
    assert bool((small[need - 1:] == 0x5A5A5A5A).all())


def test_front_end_refuses_bad_tables(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(wah.WahError):
        wah.bsi_arith_device([(stream, offs)] * 66, 65, 1, "+", 8, SEG)
    with pytest.raises(wah.WahError):
        wah.bsi_arith_device([(stream, offs)] * 5, 3, 2, "+", 4, SEG, exists_a=True)  # not 3 + 2 + 1 rows
    with pytest.raises(wah.WahError):
        wah.bsi_arith_device([(stream, offs)] * 5, 3, 2, "+", 4, SEG + 1)
    with pytest.raises(wah.WahError):
        wah.bsi_arith_device([(stream, offs)] * 5, 3, 2, "+", 65, SEG)
