"""GPU tests: the indexed calls on FOREIGN operands -- legal streams that compress() never emits (tests/_foreign.py builds
them, tests/test_foreign_reference.py proves them on the CPU): fills that are not maximal, neighbouring fills of one kind,
literals that should have been fills, a whole segment as 1024 one-group words, set pad bits.  include/wah.h promises that
such a stream, once wah_build_index_device has given it an index, goes into every indexed call.

For every foreign operand: its index comes from wah_build_index_device ON THE GPU and equals the CPU restatement, and
wah_validate_device's report equals tests/_walk.py's.  Expected results come from the numpy models of the other test files,
applied to the bitmap that the CPU ORACLE decodes from the foreign stream -- never to anything the library produced.
Everything is exact; a result that is a compressed bitmap is oracle.compress of the expected bitmap word for word, with the
indexed compressor's segment index: non-canonical in, canonical out.

Shapes: 992 words (one segment), 2 x 992 (a segment number in the addresses), (WAH_SEG_WAVES + 1) x 992 (a second
workgroup), 993 (a last segment of 2 groups, 30 pad bits), 2 x 992 + 30 (31 groups, 1 pad bit); and 24 x 992 where a way that
writes 1024 words into a segment ("fills of one", "fillable literals", "mixed") has to stay under the run-merge route's 112
words per segment: there only segment 0 is written that way.

The two routes of wah_bitop_indexed_device / wah_bitop_many_indexed_device go by the operands' lengths, so the SAME foreign
operand A meets the same bitmap B twice: B as compress() wrote it (short: the run merge) and B as fills of one (long: the
decode-based route; foreign against foreign).  Both results must be compress(A op B): the two routes give the same words.

What the file found: operands that set pad bits (a last literal with the pad bits set, a fill of ones over the ragged last
group) came out of BOTH routes of the two-operand call with the pad bits still in the result -- a last literal that kept
them, a fill of ones one group too long -- where the list call, the many-operand call and everything else gave compress() of
the bitmap.  runs_clear_pad (wah_bitop_runs.hip) and the pad mask in IndexedSource::produce (wah_compress.hip) are the fixes.

That the tests bite: libraries with ONE line of the walk (gpu-wah_amd/csrc/wah_list_walk.hpp, then part of wah_bitop_list.hip)
changed, this file run once against each on an MI355X (63 tests; the others passed).

  the all-literal fast path of list_apply_batch takes a zero word for a read past the range:
    `acc[p] = list_combine(r0, w0, m)` -> `acc[p] = w0 ? list_combine(r0, w0, m) : r0`
        test_list_call_with_the_foreign_operand_in_rows_0_63_and_64, all five shapes (batches of 128 zero literals under AND)
  the settled-row shortcut of list_gather trusts the index that a one-word segment is a whole fill:
    `(only & kCountMask) == nvalid &&` dropped from its test
        test_one_group_too_many_or_too_few_is_refused[2014] (the one-word last segment with a group too many is accepted)
  the short / long split of list_apply_batch, a fill of exactly kListShortFill groups applied by its lane AND by the wave:
    `eff0 && n0 > kListShortFill` -> `>=` in the first ballot of list_put_long
        test_list_call_with_the_foreign_operand_in_rows_0_63_and_64, all five shapes, and both shapes of
        test_split_parts_in_one_lane_in_neighbouring_lanes_and_across_a_batch ("split 8" under XOR)
"""
import collections

import numpy as np
import pytest

from tests import _arith, _bsi, _cmp, _foreign as fg, _group, _kth, _masked, _mul, _select
from tests import _switch as sw
from tests import _walk as wk
from tests.test_gpu_bitop_list import FOLD, _dev, _host, _same, wah  # noqa: F401 (wah: the fixture)

pytestmark = pytest.mark.gpu

WAH_ERR_STREAM = -6
ROUTE_RUNS, ROUTE_GROUPS = 1, 2
SEG = sw.SEG_WORDS
U64_MAX = (1 << 64) - 1
OPS = sw.LIST_OPS

WHOLE = (SEG, 2 * SEG, (sw.SEG_WAVES + 1) * SEG)
RAGGED = (SEG + 1, 2 * SEG + 30)
SHAPES = WHOLE + RAGGED
LONG = 24 * SEG                                            # (see above)
LONG_WAYS = ("fills of one", "fillable literals", "mixed")  # 1024 words in a segment, or some hundred


def test_shapes_are_what_they_are_for():
    assert [fg.pad_bits(n) for n in SHAPES] == [0, 0, 0, 30, 1]
    assert [fg.n_groups(n) % 1024 for n in RAGGED] == [2, 31]
    assert sw.SEG_WAVES + 1 == 5 and _select.segments_of(WHOLE[2]) > sw.SEG_WAVES


# ---- foreign operands -------------------------------------------------------------------------------------------------------
Operand = collections.namedtuple("Operand", "way stream data d offs")   # data: what the ORACLE decodes from the stream


class Operands:
    """Foreign operands on the device, each with the index wah_build_index_device gave it; every one is checked on the way in."""

    def __init__(self, wah, oracle):
        self.wah, self.oracle, self.cache = wah, oracle, {}

    def of_stream(self, stream, n, way="?"):
        st = np.ascontiguousarray(stream, dtype=np.uint32)
        data = self.oracle.decompress(st)[:n].copy()
        assert data.size == n, (way, n)
        d, offs = self.on_device(st, n, way)
        return Operand(way, st, data, d, offs)

    def on_device(self, st, n, way):
        d = _dev(st)
        offs, groups = self.wah.build_index_device(d)
        want = wk.index(st)
        assert groups == fg.n_groups(n) and np.array_equal(offs.cpu().numpy(), want), (way, n, "index")
        assert tuple(self.wah.validate_device(d)) == wk.report(st), (way, n, "report")
        return d, offs

    def of_bitmap(self, bitmap, n, way, rng=None, only=None):
        op = self.of_stream(fg.reencode(bitmap, n, way, rng, only), n, way)
        assert np.array_equal(op.data, bitmap), (way, n)
        return op

    def get(self, n, way, j=0, kinds=None, only=None):
        """Operand j of size n in `way`: the bitmap depends on (n, j, kinds, the tail the way needs) alone, so that the same
        bitmap comes in several ways."""
        key = (n, way, j, kinds, only)
        if key not in self.cache:
            tail = fg.tail_for(way, j)
            kinds_ = fg.kinds_for(way, n // SEG) if kinds is None else kinds
            rng = np.random.default_rng(1000 * j + n)
            bitmap = fg.bitmap(n, rng, kinds_[j % len(kinds_):] + kinds_[: j % len(kinds_)], tail)
            self.cache[key] = self.of_bitmap(bitmap, n, way, np.random.default_rng(7 + j), only)
        return self.cache[key]

    def again(self, op, n, way, only=None):
        """The bitmap of `op` written in another way."""
        return self.of_bitmap(op.data, n, way, np.random.default_rng(11), only)


@pytest.fixture(scope="module")
def ops(wah, oracle):
    return Operands(wah, oracle)


def _pair(op):
    return (op.d, op.offs)


SMALL = ("sparse", "zeros", "ones")   # a few words a segment: partners that leave the run-merge route open


def _foreign_a(ops, n, way):
    """The foreign operand A of a bit operation, short enough for the run-merge route: no dense segment, and a long way only in
    segment 0 of 24."""
    if way in LONG_WAYS:
        return LONG, ops.get(LONG, way, 0, kinds=("clustered", "zeros", "ones"), only=(0, ))
    return n, ops.get(n, way, 0, kinds=("zeros", "ones", "clustered", "sparse") if way in fg.TWO_FILL_WAYS else ("clustered", ) + SMALL)


# ---- 1: the index decoder ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_decompress_segments_of_every_way(wah, oracle, ops, n):
    for way in fg.ways_for(n):
        op = ops.get(n, way)
        full = oracle.decompress(op.stream)
        whole = _host(wah.decompress_segments_device(op.d, op.offs, n))
        assert whole.size == full.size and np.array_equal(whole[:n], op.data), (n, way)
        segs = _select.segments_of(n)
        if segs > 1:   # a sub-range that starts at segment 1
            part = _host(wah.decompress_segments_device(op.d, op.offs, n, 1, segs - 1))
            assert part.size == full.size - SEG and np.array_equal(part[: n - SEG], op.data[SEG:]), (n, way)
            one = _host(wah.decompress_segments_device(op.d, op.offs, n, 1, 1))
            assert np.array_equal(one[: min(SEG, n - SEG)], op.data[SEG: 2 * SEG]), (n, way)


# ---- 2: two, three and eight operands, both routes ---------------------------------------------------------------------------
def _route_of(operands, n):
    total = sum(int(o.stream.size) for o in operands)
    return ROUTE_RUNS if total <= sw.RUNS_MAX_WORDS_PER_SEG * _select.segments_of(n) else ROUTE_GROUPS


def _bitop_cases(ops, n, way):
    """[(operands, n)]: A in `way` against B (another bitmap) as compress() wrote it and as fills of one; both orders; three
    and eight operands around A."""
    m, a = _foreign_a(ops, n, way)
    b = ops.get(m, "canonical", 1, kinds=SMALL)
    b_long = ops.again(b, m, "fills of one")
    c = ops.get(m, "split 9", 2, kinds=SMALL)
    tiny = [ops.get(m, ("canonical", "two fills 1", "split 1", "two fills 512", "split 64")[j], 3 + j, kinds=SMALL) for j in range(5)]
    return [([a, b], m), ([b, a], m), ([a, b_long], m), ([b_long, a], m), ([a, a], m),
            ([b, a, c], m), ([a, b_long, c], m), ([b] + tiny[:2] + [a] + tiny[2:] + [c], m), (tiny[:3] + [b_long, c, b, a, tiny[3]], m)]


def _run_bitop(wah, operands, name, n):
    if len(operands) == 2:
        return wah.bitop_indexed_device(name, *_pair(operands[0]), *_pair(operands[1]), n)
    return wah.bitop_many_indexed_device(name, [_pair(o) for o in operands], n)


@pytest.mark.parametrize("n", SHAPES)
def test_bitops_of_two_three_and_eight_on_both_routes(wah, oracle, ops, n):
    """Every way, four operations, 2 / 3 / 8 operands: compress(fold) and its index on the route the lengths choose; the same A
    on both routes gives the same words (both are compared with one compress(fold))."""
    seen = collections.defaultdict(set)
    for way in fg.ways_for(n):
        for operands, m in _bitop_cases(ops, n, way):
            route = _route_of(operands, m)
            seen[way].add((route, len(operands)))
            stack = np.stack([o.data for o in operands])
            for name in OPS:
                got, offs = _run_bitop(wah, operands, name, m)
                assert wah.lib().wah_last_bitop_route() == route, (n, way, name, len(operands), route)
                _same(wah, oracle, got, offs, FOLD[name](stack), (n, way, name, len(operands), "route", route))
    for way, routes in seen.items():   # every way on both routes, with two and with more operands
        assert {r for r, _ in routes} == {ROUTE_RUNS, ROUTE_GROUPS}, (way, routes)
        assert {k for r, k in routes if r == ROUTE_RUNS} >= {2, 3, 8} and {k for r, k in routes if r == ROUTE_GROUPS} >= {2, 3, 8}, (way, routes)


# ---- 3: the operand list ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_list_call_with_the_foreign_operand_in_rows_0_63_and_64(wah, oracle, ops, n):
    """1, 2 and 65 operands (a second chunk of 64 rows), the foreign operand in row 0, 63 and 64, another foreign one beside it,
    the trivial operand everywhere else."""
    trivials = {name: ops.of_bitmap(sw.list_trivial(name, n), n, "canonical") for name in ("and", "or")}
    for way in fg.ways_for(n):
        a = ops.get(n, way, 0)
        b = ops.get(n, "mixed", 1)
        for name in OPS:
            trivial = trivials["and" if name == "and" else "or"]
            tables = [[a], [a, b], [b, a]]
            for row in (0, sw.LIST_CHUNK - 1, sw.LIST_CHUNK):
                rows = [trivial] * (sw.LIST_CHUNK + 1)
                rows[row] = a
                rows[5 if row else 7] = b
                tables.append(rows)
            for rows in tables:
                got, offs = wah.bitop_list_indexed_device(name, [_pair(o) for o in rows], n)
                _same(wah, oracle, got, offs, FOLD[name](np.stack([o.data for o in rows])), (n, way, name, len(rows)))


@pytest.mark.parametrize("n", (SEG, 2 * SEG + 30))
def test_split_parts_in_one_lane_in_neighbouring_lanes_and_across_a_batch(wah, oracle, ops, n):
    """The placement segment of tests/_foreign.py (the two parts of a fill at words 4 | 5, 9 | 10 and 127 | 128 of the segment) under
    every split way, as the list call's row 0 and row 1 and as either operand of the two-operand call; the parts' places are
    asserted again on the very stream that goes to the device."""
    kinds = ("placement", "clustered", "ones")
    b = ops.get(n, "canonical", 1, kinds=("dense", "sparse", "zeros"))
    for way in fg.SPLIT_WAYS:
        a = ops.get(n, way, 0, kinds=kinds)
        k = way[len("split "):]
        k = fg.SPLIT_FILL_GROUPS - 1 if k == "n-1" else int(k)
        for (i, _), kind in zip(fg.PLACED_SPLITS, (sw.FILL1, sw.FILL0, sw.FILL1)):
            assert int(a.stream[i]) == kind | k and int(a.stream[i + 1]) == kind | (fg.SPLIT_FILL_GROUPS - k), (way, i)
        for name in OPS:
            for rows in ([a], [a, b], [b, a], [a, a, b]):
                want = FOLD[name](np.stack([o.data for o in rows]))
                got, offs = wah.bitop_list_indexed_device(name, [_pair(o) for o in rows], n)
                _same(wah, oracle, got, offs, want, (n, way, name, len(rows)))
                if len(rows) == 2:
                    got, offs = wah.bitop_indexed_device(name, *_pair(rows[0]), *_pair(rows[1]), n)
                    _same(wah, oracle, got, offs, want, (n, way, name, "two operands"))


# ---- 4: clauses -------------------------------------------------------------------------------------------------------------
def _clauses_model(clauses, n):
    out = np.full(n, 0xFFFFFFFF, np.uint32)
    for operands, negate in clauses:
        union = np.bitwise_or.reduce(np.stack([o.data for o in operands]))
        out &= ~union if negate else union
    return out


@pytest.mark.parametrize("n", SHAPES)
def test_clauses_with_a_negated_row_of_zero_literals(wah, oracle, ops, n):
    """A negated clause whose only operand is all zeros written as zero literals (and as fills of one, two fills, canonically: the
    same result), alone and beside other clauses of foreign operands."""
    zeros = np.zeros(n, np.uint32)
    results = []
    for way in ("canonical", "fillable literals", "fills of one", "two fills 1", "two fills 512"):
        z = ops.of_bitmap(zeros, n, way)
        assert way == "canonical" or not np.array_equal(z.stream, oracle.compress(zeros)), way
        for k, other_way in enumerate(fg.ways_for(n)):
            a, b = ops.get(n, other_way, 0), ops.get(n, "mixed", 1)
            for clauses in ([([z], True)], [([a, b], False), ([z], True)], [([z], True), ([a], True), ([b, z], False)], [([z, a], True), ([b], False)])[: 4 if k % 4 == 0 else 2]:
                got, offs = wah.bitop_clauses_indexed_device([([_pair(o) for o in operands], neg) for operands, neg in clauses], n)
                _same(wah, oracle, got, offs, _clauses_model(clauses, n), (n, way, other_way, len(clauses)))
        got, _ = wah.bitop_clauses_indexed_device([([_pair(z)], True)], n)
        results.append(_host(got).copy())
    assert all(np.array_equal(r, results[0]) for r in results)


# ---- 5: bit-sliced attributes ------------------------------------------------------------------------------------------------
ZERO_SLICE_WAYS = ("canonical", "two fills 1", "two fills 512", "fillable literals")


def _values(n, k, rng, quiet_segment=True):
    """Values of k bits, constant over runs of some hundred rows with single rows between (slices of fills and literals); in one
    segment the two top bits are zero: those slices are all zero there -- one word, two fills or 1024 zero literals."""
    rows = 32 * n
    runs = rng.integers(300, 1500, rows // 300 + 2)
    v = np.repeat(rng.integers(0, 1 << k, runs.size, dtype=np.uint64), runs)[:rows].copy()
    at = rng.permutation(rows)[: rows // 50]
    v[at] = rng.integers(0, 1 << k, at.size, dtype=np.uint64)
    if quiet_segment:
        s = min(1, _select.segments_of(n) - 1)
        v[_select.SEG_BITS * s: _select.SEG_BITS * (s + 1)] &= np.uint64((1 << (k - 2)) - 1)
    return v


def _exists(n, rng):
    rows = 32 * n
    runs = rng.integers(200, 3000, rows // 200 + 2)
    return np.repeat(np.arange(runs.size) % 4 != 1, runs)[:rows].copy()


class Attribute:
    """A bit-sliced attribute whose rows are foreign streams: the top slice in `top_way`, the others in ways that rotate.  values
    and exists are read back from what the ORACLE decodes."""

    def __init__(self, ops, oracle, n, k, seed, top_way, first_way=0):
        rng = np.random.default_rng(seed)
        matrix = _bsi.build_slices(_values(n, k, rng), k, _exists(n, rng))
        ways = [w for w in fg.ways_for(n) if w != "canonical"]
        streams = fg.rows_foreign(matrix[1:], n, np.random.default_rng(seed + 1), ways, first_way)
        self.rows = [ops.of_bitmap(matrix[0], n, top_way, np.random.default_rng(seed + 2))] + [ops.of_stream(st, n, way) for way, st in streams]
        decoded = np.stack([o.data for o in self.rows])
        assert np.array_equal(decoded, matrix)
        self.k, self.matrix = k, decoded
        self.values, self.exists = _bsi.values_of_slices(decoded, k)

    def pairs(self):
        return [_pair(o) for o in self.rows]


def _all_equal(results, what):
    first = results[0]
    for r in results[1:]:
        assert r[0].size == first[0].size and np.array_equal(r[0], first[0]) and np.array_equal(r[1], first[1]), what


@pytest.mark.parametrize("n", SHAPES)
def test_bsi_range_over_foreign_slices(wah, oracle, ops, n):
    k = 7
    per_way = []
    for j, top_way in enumerate(ZERO_SLICE_WAYS):
        attr = Attribute(ops, oracle, n, k, 40 + n, top_way, j)
        assert not attr.matrix[0][SEG * min(1, _select.segments_of(n) - 1):][:SEG].any()   # the slice that is all zero in a segment
        top = (1 << k) - 1
        bounds = [(0, top), (0, 17), (18, 18), (31, 32), (5, 90), (33, top), (64, 100), (int(attr.values[0]), int(attr.values[0]))]
        out = []
        for exists in (False, True):
            for lo, hi in bounds:
                got, offs = wah.bsi_range_device(attr.pairs()[: k + exists], (lo, hi), n, exists=exists)
                _same(wah, oracle, got, offs, _bsi.expected_range(attr.values, lo, hi, attr.exists if exists else None), (n, top_way, lo, hi, exists))
                out.append(_host(got).copy())
        per_way.append((np.concatenate(out), np.zeros(0)))
    _all_equal(per_way, (n, "the zero slice's way changes the result"))


@pytest.mark.parametrize("n", SHAPES)
def test_bsi_compare_over_foreign_slices(wah, oracle, ops, n):
    ka, kb = 5, 7
    per_way = []
    for j, top_way in enumerate(ZERO_SLICE_WAYS):
        a, b = Attribute(ops, oracle, n, ka, 50 + n, top_way, j), Attribute(ops, oracle, n, kb, 60 + n, ZERO_SLICE_WAYS[(j + 1) % 4], j + 3)
        out = []
        for have_a, have_b in ((False, False), (True, True), (True, False)):
            order = wah.bsi_compare_row_order(ka, kb, have_a, have_b)
            assert order == _cmp.row_order(ka, kb, have_a, have_b)
            table = [_pair((a if who == "a" else b).rows[i]) for who, i in order]
            for op in _cmp.OPS:
                got, offs = wah.bsi_compare_device(table, ka, kb, op, n, exists_a=have_a, exists_b=have_b)
                want = _cmp.expected_compare(a.values, b.values, op, a.exists if have_a else None, b.exists if have_b else None)
                _same(wah, oracle, got, offs, want, (n, top_way, op, have_a, have_b))
                out.append(_host(got).copy())
        per_way.append((np.concatenate(out), np.zeros(0)))
    _all_equal(per_way, (n, "the zero slice's way changes the result"))


@pytest.mark.parametrize("n", WHOLE)
def test_bsi_arith_and_mul_over_foreign_slices(wah, oracle, ops, n):
    """(the two calls take slices of whole segments only: no pad ways)"""
    ka, kb = 4, 5
    per_way = []
    for j, top_way in enumerate(ZERO_SLICE_WAYS):
        a, b = Attribute(ops, oracle, n, ka, 70 + n, top_way, j), Attribute(ops, oracle, n, kb, 80 + n, ZERO_SLICE_WAYS[(j + 2) % 4], j + 5)
        out = []
        for have_a, have_b in ((False, False), (True, True), (False, True)):
            xa, xb = a.exists if have_a else None, b.exists if have_b else None
            order = wah.bsi_arith_row_order(ka, kb, have_a, have_b)
            assert order == _arith.row_order(ka, kb, have_a, have_b)
            table = [_pair((a if who == "a" else b).rows[i]) for who, i in order]
            for op in ("+", "-"):
                n_out = max(ka, kb) + 1
                got, offs = wah.bsi_arith_device(table, ka, kb, op, n_out, n, exists_a=have_a, exists_b=have_b)
                want = _arith.expected_matrix(a.values, b.values, op, n_out, xa, xb)
                _same(wah, oracle, got, offs, want.reshape(-1), (n, top_way, op, have_a, have_b))
                out.append(_host(got).copy())
            order = wah.bsi_mul_row_order(ka, kb, have_a, have_b)
            assert order == _mul.row_order(ka, kb, have_a, have_b)
            table = [_pair((a if who == "a" else b).rows[i]) for who, i in order]
            for n_out in (ka + kb, 6):
                got, offs = wah.bsi_mul_device(table, ka, kb, n_out, n, exists_a=have_a, exists_b=have_b)
                want = _mul.expected_matrix(a.values, b.values, n_out, xa, xb)
                _same(wah, oracle, got, offs, want.reshape(-1), (n, top_way, "*", n_out, have_a, have_b))
                out.append(_host(got).copy())
        per_way.append((np.concatenate(out), np.zeros(0)))
    _all_equal(per_way, (n, "the zero slice's way changes the result"))


# ---- 6: order statistics ----------------------------------------------------------------------------------------------------
def _u64(t):
    return tuple(int(v) & U64_MAX for v in t.reshape(-1).tolist())


def _rows_of(words):
    return _bsi.unpack_bits(words)


QUERIES = ((_kth.ASCENDING, 0, 1), (_kth.DESCENDING, 0, 1), (_kth.QUANTILE, 1, 2), (_kth.ASCENDING, 37, 1), (_kth.QUANTILE, 9, 10), (_kth.ASCENDING, 1 << 40, 1))


@pytest.mark.parametrize("n", SHAPES)
def test_kth_and_grouped_kth_over_foreign_filters_groups_and_slices(wah, oracle, ops, n):
    k = 6
    per_way = []
    rng = np.random.default_rng(90 + n)
    keys = np.repeat(rng.integers(0, 3, 32 * n // 500 + 2), 500)[: 32 * n]
    group_maps = [_bsi.pack_bits(keys == g) for g in range(3)]
    second_filter = fg.bitmap(n, rng, fg.KINDS[:5], "ones")
    for j, top_way in enumerate(ZERO_SLICE_WAYS):
        attr = Attribute(ops, oracle, n, k, 95 + n, top_way, j)
        ways = [w for w in fg.ways_for(n) if w != "canonical"]
        filt = [ops.of_stream(st, n, way) for way, st in fg.rows_foreign([attr.matrix[k], second_filter], n, rng, ways, j + 1)]
        groups = [ops.of_stream(st, n, way) for way, st in fg.rows_foreign(group_maps, n, rng, ways, j + 4)]
        slices = attr.pairs()[:k]
        out = []
        for n_filters in (0, 1, 2):
            selected = np.ones(32 * n, bool)
            for f in filt[:n_filters]:
                selected &= _rows_of(f.data)
            for query in QUERIES:
                got = _u64(wah.bsi_kth_device([_pair(f) for f in filt[:n_filters]] + slices, query, n, n_filters))
                assert got == _kth.model(attr.values, selected, *query), (n, top_way, n_filters, query)
                out.append(got)
            got = wah.bsi_kth_grouped_device([_pair(f) for f in filt[:n_filters]], [_pair(g) for g in groups], slices, list(QUERIES), n).cpu().numpy()
            for g, group in enumerate(groups):
                for q, query in enumerate(QUERIES):
                    assert _u64(got[g, q]) == _kth.model(attr.values, selected & _rows_of(group.data), *query), (n, top_way, n_filters, g, query)
            out.append(_u64(got))
        per_way.append(out)
    assert all(p == per_way[0] for p in per_way)


# ---- 7: fetch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_fetch_of_rows_in_segments_of_every_way(wah, oracle, ops, n):
    """Both modes; every table is six bitmaps in ONE way (so the listed rows lie in segments whose slices are fills of one, zero
    literals, split fills ...), and one table of all ways mixed."""
    import torch

    rng = np.random.default_rng(3 + n)
    rows = np.unique(np.concatenate([rng.integers(0, 32 * n, 300), [0, 30, 31, 32 * n - 1, 32 * n - 2], np.arange(31744 - 3, min(31744 + 3, 32 * n))]))
    rows = np.sort(np.concatenate([rows[rows < 32 * n], rows[:5]])).astype(np.int64)   # (non-descending: a few rows twice)
    d_rows = torch.from_numpy(rows).cuda()
    tables = [[ops.get(n, way, j) for j in range(6)] for way in fg.ways_for(n)]
    tables.append([ops.get(n, way, 1) for way in fg.ways_for(n)])
    for table in tables:
        bits = np.stack([_rows_of(o.data)[rows] for o in table])                        # [k, listed rows], from the decoded bitmaps
        k = len(table)
        want_bits = [sum(int(bits[j, i]) << (k - 1 - j) for j in range(k)) for i in range(rows.size)]
        want_first = [int(np.flatnonzero(bits[:, i])[0]) if bits[:, i].any() else U64_MAX for i in range(rows.size)]
        pairs = [_pair(o) for o in table]
        assert list(_u64(wah.fetch_device(pairs, d_rows, n, wah.FETCH_BITS))) == want_bits, (n, table[0].way)
        assert list(_u64(wah.fetch_device(pairs, d_rows, n, wah.FETCH_FIRST))) == want_first, (n, table[0].way)


# ---- 8: counts, positions, masked counts, grouped sums ----------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_counts_and_positions_of_every_way(wah, oracle, ops, n):
    table = [ops.get(n, way, j % 3) for j, way in enumerate(fg.ways_for(n))]
    counts = wah.count_device([_pair(o) for o in table], n).cpu().tolist()
    assert counts == [_select.ref_count(o.data, n) for o in table]
    for o in table:
        want = _select.ref_positions(o.data, n)
        got, total = wah.positions_device(o.d, o.offs, n)
        assert total == want.size and np.array_equal(got.cpu().numpy(), want), (n, o.way)
        # windows that start inside a fill of ones, at its first and its last row (a split fill: inside either part)
        inside = np.flatnonzero(np.diff(want) == 1)
        for first in sorted({0, max(want.size - 1, 0)} | ({int(inside[0]), int(inside[inside.size // 2]) + 7, int(inside[-1])} if inside.size else set())):
            got, total = wah.positions_device(o.d, o.offs, n, first=first, limit=70)
            assert total == want.size and np.array_equal(got.cpu().numpy(), want[first: first + 70]), (n, o.way, first)


@pytest.mark.parametrize("n", SHAPES)
def test_a_window_that_starts_inside_the_second_part_of_a_split_fill(wah, oracle, ops, n):
    for way in fg.SPLIT_WAYS + (("pad: split one-fill", ) if fg.pad_bits(n) else ()):
        o = ops.get(n, way, 0)
        second = [int(t) for t in fg.noncanonical_words(o.stream) if int(o.stream[t]) >= sw.FILL1]   # second parts of fills of ones
        assert second, (n, way)
        starts = wk._walk(o.stream)[4]
        want = _select.ref_positions(o.data, n)
        for t in (second[0], second[-1]):
            first = int(np.searchsorted(want, 31 * int(starts[t]))) + 3     # the rank of the fourth row of that part
            if first >= want.size:
                first = want.size - 1
            got, total = wah.positions_device(o.d, o.offs, n, first=first, limit=40)
            assert total == want.size and np.array_equal(got.cpu().numpy(), want[first: first + 40]), (n, way, t)


@pytest.mark.parametrize("n", SHAPES)
def test_masked_counts_and_grouped_sums_over_foreign_masks_and_operands(wah, oracle, ops, n):
    """Masks and operands in every way; the one-word mask (all ones: the shortcut) against the same mask as two fills, as fills of
    one and as literals."""
    ones = np.full(n, 0xFFFFFFFF, np.uint32)
    mask_ways = ("canonical", "two fills 1", "two fills 512", "fills of one", "fillable literals") + (fg.PAD_WAYS if fg.pad_bits(n) else ())
    masks = [ops.of_bitmap(ones, n, way) for way in mask_ways] + [ops.get(n, way, 1) for way in fg.ways_for(n)]
    operands = [ops.get(n, way, 2 + j % 2) for j, way in enumerate(fg.ways_for(n))]
    got = wah.count_masked_device([_pair(m) for m in masks], [_pair(o) for o in operands], n).cpu().tolist()
    want = [[_masked.ref_counts(m.data, o.data, n) for o in operands] for m in masks]
    assert got == want
    assert all(row == got[0] for row in got[: len(mask_ways)])                          # the mask of all ones, however it is written
    # GROUP BY over a foreign attribute under foreign filters: rows, counts and sums
    k = 5
    attr = Attribute(ops, oracle, n, k, 120 + n, "fillable literals", 2)
    rng = np.random.default_rng(130 + n)
    keys = np.repeat(rng.integers(0, 4, 32 * n // 700 + 2), 700)[: 32 * n]
    ways = [w for w in fg.ways_for(n) if w != "canonical"]
    groups = [ops.of_stream(st, n, way) for way, st in fg.rows_foreign([_bsi.pack_bits(keys == g) for g in range(4)], n, rng, ways, 3)]
    for filters in ([], [masks[1]], [masks[len(mask_ways)], attr.rows[k]]):
        rows, counts, sums = wah.group_sum_device([_pair(f) for f in filters], [_pair(g) for g in groups], attr.pairs()[:k], [k], n)
        want_rows, want_counts, want_sums = _group.ref_group([f.data for f in filters], [[g.data] for g in groups], attr.matrix[:k], [k], n)
        assert rows.cpu().tolist() == want_rows and counts.cpu().tolist() == want_counts, (n, len(filters))
        assert [[tuple(int(v) & U64_MAX for v in pair) for pair in grp] for grp in sums.cpu().tolist()] == [[_group.split128(s) for s in grp] for grp in want_sums]
        for g, group in enumerate(groups):                                               # ... and the sums from the VALUES
            sel = _rows_of(group.data)
            for f in filters:
                sel = sel & _rows_of(f.data)
            assert want_sums[g][0] == int(attr.values[sel].sum(dtype=np.uint64)), (n, g)


# ---- 9: the refusal stays ---------------------------------------------------------------------------------------------------
def _list_status(wah, name, pairs, n):
    import torch

    table = wah.bitop_operand_table(pairs)
    sc = torch.empty(int(wah.lib().wah_bitop_list_scratch_bytes(n, table.shape[0])), dtype=torch.uint8, device="cuda:0")
    wah.bitop_list_indexed_device(name, table, n, scratch=sc, check=False)
    return int(wah.lib().wah_bitop_list_status(sc.data_ptr(), n, table.shape[0], None))


def _two_status(wah, name, a, b, n):
    import torch

    sc = torch.empty(int(wah.lib().wah_bitop_indexed_scratch_bytes(n)), dtype=torch.uint8, device="cuda:0")
    wah.bitop_indexed_device(name, *a, *b, n, scratch=sc, check=False)
    return int(wah.lib().wah_bitop_indexed_status(sc.data_ptr(), n, None)), int(wah.lib().wah_last_bitop_route())


@pytest.mark.parametrize("n", (2 * SEG, 2 * SEG + 30))
def test_one_group_too_many_or_too_few_is_refused(wah, oracle, ops, n):
    """Every way with one group too many and one too few in its non-canonical part (tests/_foreign.py: off_by_one; the index is
    hand-made: to the builder such a stream is another bitmap, or has a fill across a segment): WAH_ERR_STREAM from the list
    call and from the two-operand call on the run-merge route, under every operation and in either operand; the intact stream
    beside it is accepted."""
    import torch

    for way in fg.ways_for(n):
        m, a = _foreign_a(ops, n, way)
        b = ops.get(m, "canonical", 1, kinds=SMALL)
        assert _list_status(wah, "or", [_pair(a), _pair(b)], m) == 0
        assert _two_status(wah, "or", _pair(a), _pair(b), m) == (0, ROUTE_RUNS), (n, way)
        for delta in (1, -1):
            stream, index, t = fg.off_by_one(a.stream, way, delta)
            d = _dev(np.concatenate([stream, wk.PADDING]))[: stream.size]             # (what lies behind it would change the verdict if it were read)
            bad = (d, torch.from_numpy(index).cuda())
            for name in OPS:
                assert _list_status(wah, name, [bad, _pair(b)], m) == WAH_ERR_STREAM, (n, way, delta, name)
                assert _list_status(wah, name, [_pair(b), bad], m) == WAH_ERR_STREAM, (n, way, delta, name)
                assert _two_status(wah, name, bad, _pair(b), m) == (WAH_ERR_STREAM, ROUTE_RUNS), (n, way, delta, name)
                assert _two_status(wah, name, _pair(b), bad, m) == (WAH_ERR_STREAM, ROUTE_RUNS), (n, way, delta, name)
