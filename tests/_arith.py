"""Shared helpers of the column arithmetic tests (wah_bsi_arith_indexed_device), numpy only: a model that answers `A + B` and
`A - B` from the VALUES, an independent restatement of the table order, the ex / carry / hold sweep over the slice matrices of
tests/_bsi.py, a generator of value pairs in which every carry matters, and the vacuity guard.

What the guard can ask follows from the semantics, not from any implementation:
  * an input slice at or above n_out cannot change (A op B) mod 2^n_out, so only the slices below n_out are flipped;
  * the slices of an ADD above max(ka, kb) are a zero extension: they are asserted EMPTY, every other output slice (for SUB all
    of them: the borrow and its sign extension) is asserted neither empty nor full."""
import numpy as np

from tests import _bsi, _cmp

OPS = ("+", "-")
EXISTENCE = _cmp.EXISTENCE  # none / A / B / both
# (ka, kb, n_out): the last two truncate and extend
WIDTHS = ((1, 1, 2), (20, 13, 21), (13, 20, 21), (64, 64, 64), (63, 63, 64), (1, 64, 64), (64, 1, 64), (40, 41, 42), (20, 13, 8), (13, 20, 40))


def _mask(k):
    return np.uint64((1 << k) - 1)


def expected_values(va, vb, op, n_out):
    """(va op vb) mod 2^n_out: uint64 arithmetic wraps mod 2^64, which every n_out <= 64 divides, then the mask."""
    with np.errstate(over="ignore"):
        r = va + vb if op == "+" else va - vb
    return r & _mask(n_out)


def both(xa, xb):
    """The AND of the existence bitmaps that are there (bool arrays), None without any."""
    if xa is None:
        return xb
    return xa if xb is None else xa & xb


def expected_matrix(va, vb, op, n_out, xa=None, xb=None):
    """The model: the decoded slice matrix of the result, most significant slice first, the existence row last, rows that do not
    exist stored as 0 -- from the values, never from slices."""
    return _bsi.build_slices(expected_values(va, vb, op, n_out), n_out, both(xa, xb), zero_missing=True)


def row_order(ka, kb, exists_a, exists_b):
    """The table order, restated from the widths: A's existence row, then B's; min(ka, kb) pairs (A, B) from the least significant
    slice up; then the wider attribute's surplus slices alone, upwards.  Entries are (attribute, row of that attribute's own slice
    matrix), row 0 the MOST significant slice."""
    order = ([("a", ka)] if exists_a else []) + ([("b", kb)] if exists_b else [])
    shared = min(ka, kb)
    for i in range(shared):
        order += [("a", ka - 1 - i), ("b", kb - 1 - i)]
    who, k = ("a", ka) if ka > kb else ("b", kb)
    return order + [(who, k - 1 - i) for i in range(shared, k)]


def table_rows(slices_a, ka, slices_b, kb, exists_a, exists_b):
    """The decoded rows of the table, in table order (slices_*: _bsi.build_slices matrices, the existence row last if any)."""
    return [(slices_a if who == "a" else slices_b)[i] for who, i in row_order(ka, kb, exists_a, exists_b)]


def sweep(slices_a, ka, slices_b, kb, op, n_out, exists_a=False, exists_b=False):
    """The fold as the interface states it, over the table's rows in order: an existence row ANDs into ex; A's slice where B has
    one of that significance is held; the closing row of a significance (B's slice, or A's alone with b = 0, or B's alone with
    a = 0) does b ^= flip, sum = a ^ b ^ carry, carry = (a & b) | (carry & (a ^ b)) and emits sum & ex as matrix row
    n_out - 1 - sig if sig < n_out.  Behind the rows the carry alone: ADD emits carry & ex and clears it, SUB emits ~carry & ex.
    Then the ex row, if there is one."""
    n = slices_a.shape[1]
    zeros, ones = np.zeros(n, np.uint32), np.full(n, _bsi.ONES, np.uint32)
    sub = op == "-"
    ex, carry, hold = ones.copy(), (ones.copy() if sub else zeros.copy()), zeros.copy()
    flip = ones if sub else zeros
    n_ex = int(bool(exists_a)) + int(bool(exists_b))
    out = np.zeros((n_out + (1 if n_ex else 0), n), np.uint32)
    written = set()
    order = row_order(ka, kb, exists_a, exists_b)
    rows = [(slices_a if who == "a" else slices_b)[i] for who, i in order]
    for j, ((who, i), acc) in enumerate(zip(order, rows)):
        if j < n_ex:
            ex = ex & acc
            continue
        sig = (ka if who == "a" else kb) - 1 - i
        if who == "a" and sig < kb:
            hold = acc
            continue
        a, b = (acc, zeros) if who == "a" else ((hold if sig < ka else zeros), acc)
        b = b ^ flip
        total = a ^ b ^ carry
        carry = (a & b) | (carry & (a ^ b))
        if sig < n_out:
            out[n_out - 1 - sig] = total & ex
            written.add(n_out - 1 - sig)
    for sig in range(max(ka, kb), n_out):
        out[n_out - 1 - sig] = (~carry if sub else carry) & ex
        written.add(n_out - 1 - sig)
        if not sub:
            carry = zeros
    if n_ex:
        out[n_out] = ex
        written.add(n_out)
    assert written == set(range(out.shape[0])), "every matrix row is written exactly by one step"
    return out


def planted_pairs(ka, kb, op):
    """The rows that make every carry matter, as (A, B) Python ints that fit the widths.  Both operations: A = 2^j - 1, B = 1 for
    every j (adding ripples through j slices; subtracting clears one bit).  SUB also: A = 0, B = 1 (a borrow through every slice),
    A = B, and A = B + 2^j, A = B - 2^j for every j both widths allow."""
    pairs = [((1 << j) - 1, 1) for j in range(1, ka + 1)]
    if op == "-":
        pairs += [(0, 1), (5 % (1 << min(ka, kb)), 5 % (1 << min(ka, kb)))]
        base = (0x5A5A5A5A5A5A5A5A >> 1) & ((1 << min(ka, kb)) - 1)
        for j in range(max(ka, kb)):
            bit = 1 << j
            low = base & ~bit
            if (low | bit) < 1 << ka:
                pairs.append((low | bit, low))  # A = B + 2^j
            if (low | bit) < 1 << kb:
                pairs.append((low, low | bit))  # A = B - 2^j
    return pairs


def case(n_words, ka, kb, op, exists_a, exists_b, seed=0):
    """The headline case of a size, a pair of widths and an operation: the uniform pair of _cmp.value_pair (its planted rows kept),
    the rows of planted_pairs in rows of their own, and existence bitmaps of density 0.9 (None where the attribute has none) in
    which every planted row exists.  Deterministic.  Returns (va, vb, xa, xb, planted): planted maps (A, B) to its row."""
    rng = np.random.default_rng(15485863 * ka + 32452843 * kb + n_words + 7 * seed + (op == "-"))
    rows = 32 * n_words
    va, vb, taken = _cmp.value_pair(rng, rows, ka, kb)
    pairs = planted_pairs(ka, kb, op)
    free = np.ones(rows, bool)
    free[taken] = False
    candidates = np.flatnonzero(free)
    assert len(pairs) <= candidates.size, "no room for the planted rows"
    at = candidates[rng.permutation(candidates.size)[: len(pairs)]]
    va[at] = np.array([p[0] for p in pairs], dtype=np.uint64)
    vb[at] = np.array([p[1] for p in pairs], dtype=np.uint64)
    assert int(va.max()) <= int(_mask(ka)) and int(vb.max()) <= int(_mask(kb))
    xa, xb = rng.random(rows) < 0.9, rng.random(rows) < 0.9
    for x in (xa, xb):
        x[taken] = True
        x[at] = True
    return va, vb, (xa if exists_a else None), (xb if exists_b else None), {p: int(r) for p, r in zip(pairs, at)}


def _stored(va, vb, op, n_out, xa, xb):
    """The values the result stores (rows that do not exist: 0) and its existence bitmap: two results have one slice matrix exactly
    when these agree."""
    ex = both(xa, xb)
    v = expected_values(va, vb, op, n_out)
    return (v if ex is None else np.where(ex, v, np.uint64(0))), ex


def assert_arith_matters(va, vb, ka, kb, n_out, xa, xb, what):
    """The vacuity guard, numpy alone, for both operations at once: every expected output slice is neither empty nor full (the zero
    extension of an ADD: empty), complementing any single input slice below n_out changes the result, dropping either existence
    row changes it, and ADD and SUB differ."""
    stored = {}
    for op in OPS:
        v, ex = stored[op] = _stored(va, vb, op, n_out, xa, xb)
        for sig in range(n_out):
            bits = (v >> np.uint64(sig)) & np.uint64(1)
            if op == "+" and sig > max(ka, kb):
                assert not bits.any(), (what, op, "slice", sig, "of a zero extension is set")
            else:
                assert bits.any() and not bits.all(), (what, op, "slice", sig, "empty or full")
        if ex is not None:
            assert ex.any() and not ex.all(), (what, "the existence row is empty or full")

        def changed(a, b, ea, eb):
            w, wx = _stored(a, b, op, n_out, ea, eb)
            return not np.array_equal(w, v) or (wx is None) != (ex is None) or (ex is not None and not np.array_equal(wx, ex))

        for j in range(min(ka, n_out)):
            assert changed(va ^ np.uint64(1 << j), vb, xa, xb), (what, op, "slice", j, "of A does not matter")
        for j in range(min(kb, n_out)):
            assert changed(va, vb ^ np.uint64(1 << j), xa, xb), (what, op, "slice", j, "of B does not matter")
        if xa is not None:
            assert changed(va, vb, None, xb), (what, op, "A's existence row does not matter")
        if xb is not None:
            assert changed(va, vb, xa, None), (what, op, "B's existence row does not matter")
    assert not np.array_equal(stored["+"][0], stored["-"][0]), (what, "ADD and SUB give one answer")
