"""Shared helpers of the column-to-column comparison tests (wah_bsi_compare_indexed_device), numpy only: a model that answers
`A op B` from the VALUES, an independent restatement of the table order, the eq / gt / hold sweep over the slice matrices of
tests/_bsi.py, a generator of value pairs in which every slice of either attribute decides a row, and the vacuity guard."""
import numpy as np

from tests import _bsi

OPS = ("<", "<=", ">", ">=", "==", "!=")
_MODEL = {"<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal, "==": np.equal, "!=": np.not_equal}
EXISTENCE = ((False, False), (True, False), (False, True), (True, True))  # none / A / B / both
WIDTHS = ((1, 1), (1, 64), (64, 1), (64, 64), (20, 13), (13, 20), (41, 40), (40, 41))


def expected_compare(va, vb, op, xa=None, xb=None):
    """The model: rows with va op vb (uint64, unsigned) that exist in both attributes -- from the values, never from slices."""
    match = _MODEL[op](va, vb)
    for x in (xa, xb):
        if x is not None:
            match = match & x
    return _bsi.pack_bits(match)


def row_order(ka, kb, exists_a, exists_b):
    """The table order, restated from the widths: the wider attribute's surplus slices alone, then pairs (A, B) of equal
    significance, then A's existence row, then B's.  Entries are (attribute, row of that attribute's own slice matrix)."""
    order = []
    if ka > kb:
        order += [("a", i) for i in range(ka - kb)]
    else:
        order += [("b", i) for i in range(kb - ka)]
    shared = min(ka, kb)
    for i in range(shared):
        order += [("a", ka - shared + i), ("b", kb - shared + i)]
    return order + ([("a", ka)] if exists_a else []) + ([("b", kb)] if exists_b else [])


def table_rows(slices_a, ka, slices_b, kb, exists_a, exists_b, order=None):
    """The decoded rows of the table, in table order (slices_*: _bsi.build_slices matrices, the existence row last if any)."""
    order = row_order(ka, kb, exists_a, exists_b) if order is None else order
    return [(slices_a if who == "a" else slices_b)[i] for who, i in order]


def sweep(slices_a, ka, slices_b, kb, op, exists_a=False, exists_b=False):
    """The fold as the interface states it, over the table's rows in order: hold = A's slice where B has one of that significance;
    at B's slice (a = hold, or 0 where A has none) and at an A slice that B lacks (b = 0): gt |= eq & a & ~b, eq &= ~(a ^ b);
    an existence row ANDs into gt, eq and ex; the negated operators are taken within ex."""
    n = slices_a.shape[1]
    ones = np.full(n, _bsi.ONES, np.uint32)
    eq, gt, ex, hold = ones.copy(), np.zeros(n, np.uint32), ones.copy(), np.zeros(n, np.uint32)
    top = max(ka, kb)
    for sig in range(top - 1, -1, -1):
        in_a, in_b = sig < ka, sig < kb
        if in_a and in_b:
            hold = slices_a[ka - 1 - sig]
        if in_b:
            a, b = (hold if in_a else np.zeros(n, np.uint32)), slices_b[kb - 1 - sig]
        else:
            a, b = slices_a[ka - 1 - sig], np.zeros(n, np.uint32)
        gt = gt | (eq & a & ~b)
        eq = eq & ~(a ^ b)
    for have, row in ((exists_a, slices_a[ka] if exists_a else None), (exists_b, slices_b[kb] if exists_b else None)):
        if have:
            gt, eq, ex = gt & row, eq & row, ex & row
    result = {">": gt, ">=": gt | eq, "==": eq, "!=": ~eq, "<=": ~gt, "<": ~(gt | eq)}[op]
    return result & ex


def _mask(k):
    return np.uint64((1 << k) - 1)


def value_pair(rng, rows, ka, kb):
    """(va, vb, planted): A uniform over ka bits, about four tenths of the rows masked to min(ka, kb) bits; B = A's low kb bits,
    except three tenths of the rows uniform over kb bits; and for every bit j of either attribute one row where A and B are equal
    but for that bit, in each direction the widths allow (A has it and B does not: j < ka; B has it and A does not: j < kb).
    planted: the rows so written, which the caller makes exist.  Needs room: rows >= 2 * (ka + kb)."""
    shared = min(ka, kb)
    va = _bsi.uniform_values(rng, rows, ka)
    va = np.where(rng.random(rows) < 0.4, va & _mask(shared), va)
    vb = np.where(rng.random(rows) < 0.3, _bsi.uniform_values(rng, rows, kb), va & _mask(kb))
    pairs = []
    for j in range(max(ka, kb)):
        bit = np.uint64(1 << j)
        base = _bsi.uniform_values(rng, 2, shared) & ~bit
        if j < ka:
            pairs.append((base[0] | bit, base[0]))
        if j < kb:
            pairs.append((base[1], base[1] | bit))
    assert len(pairs) <= rows, "no room for the planted rows"
    planted = rng.permutation(rows)[: len(pairs)]
    va, vb = va.copy(), vb.copy()
    va[planted] = np.array([p[0] for p in pairs], dtype=np.uint64)
    vb[planted] = np.array([p[1] for p in pairs], dtype=np.uint64)
    assert int(va.max()) <= int(_mask(ka)) and int(vb.max()) <= int(_mask(kb))
    return va, vb, planted


def case(n_words, ka, kb, exists_a, exists_b, seed=0):
    """The headline case of a size and a pair of widths: value_pair and existence bitmaps of density 0.9 (None where the attribute
    has none) in which the planted rows exist.  Deterministic.  Returns (va, vb, xa, xb)."""
    rng = np.random.default_rng(104729 * ka + 1009 * kb + n_words + 7 * seed)
    rows = 32 * n_words
    va, vb, planted = value_pair(rng, rows, ka, kb)
    xa, xb = rng.random(rows) < 0.9, rng.random(rows) < 0.9
    xa[planted] = True
    xb[planted] = True
    return va, vb, (xa if exists_a else None), (xb if exists_b else None)


def assert_compare_matters(va, vb, ka, kb, xa, xb, what):
    """The vacuity guard, numpy alone: each of the six expected bitmaps is neither empty nor full, all six differ, complementing any
    single slice of A or of B changes the `>` or the `==` answer, and so does dropping either existence row.  Returns the six."""
    want = {op: expected_compare(va, vb, op, xa, xb) for op in OPS}
    for op, w in want.items():
        assert w.any() and not (w == _bsi.ONES).all(), (what, op, "empty or full")
    assert len({w.tobytes() for w in want.values()}) == len(OPS), (what, "two operators give one answer")

    def changed(a, b, ea, eb):
        return any(not np.array_equal(expected_compare(a, b, op, ea, eb), want[op]) for op in (">", "=="))

    for j in range(ka):
        assert changed(va ^ np.uint64(1 << j), vb, xa, xb), (what, "slice", j, "of A does not matter")
    for j in range(kb):
        assert changed(va, vb ^ np.uint64(1 << j), xa, xb), (what, "slice", j, "of B does not matter")
    if xa is not None:
        assert changed(va, vb, None, xb), (what, "A's existence row does not matter")
    if xb is not None:
        assert changed(va, vb, xa, None), (what, "B's existence row does not matter")
    return want
