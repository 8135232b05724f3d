"""Shared helpers of the column multiplication tests (wah_bsi_mul_indexed_device), numpy only: a model that answers `A * B` from the
VALUES, an independent restatement of the table order, the shift-and-add sweep over the slice matrices of tests/_bsi.py as the
interface states it (A's image, the accumulator P whose carry slot nobody has written yet, the skip of a zero slice of B), and
the value pairs of the GPU tests with their planted rows."""
import numpy as np

from tests import _bsi, _cmp

EXISTENCE = _cmp.EXISTENCE  # none / A / B / both
# (ka, kb, n_out): (1, 1, 1), (40, 41, 64), (40, 41, 20) and the three of 64 bits and more truncate, (5, 3, 12) extends
WIDTHS = ((1, 1, 2), (1, 1, 1), (3, 5, 8), (8, 8, 16), (20, 13, 33), (13, 20, 33), (32, 32, 64), (33, 31, 64), (64, 64, 64), (64, 1, 64),
          (1, 64, 64), (40, 41, 64), (40, 41, 20), (5, 3, 12))


def _mask(k):
    return np.uint64((1 << k) - 1)


def expected_values(va, vb, n_out):
    """(va * vb) mod 2^n_out: uint64 multiplication wraps mod 2^64, which every n_out <= 64 divides, then the mask."""
    with np.errstate(over="ignore"):
        return (va * vb) & _mask(n_out)


def both(xa, xb):
    """The AND of the existence bitmaps that are there (bool arrays), None without any."""
    if xa is None:
        return xb
    return xa if xb is None else xa & xb


def expected_matrix(va, vb, n_out, xa=None, xb=None):
    """The model: the decoded slice matrix of the product, most significant slice first, the existence row last, rows that do not
    exist stored as 0 -- from the values, never from slices."""
    return _bsi.build_slices(expected_values(va, vb, n_out), n_out, both(xa, xb), zero_missing=True)


def row_order(ka, kb, exists_a, exists_b):
    """The table order, restated from the widths: A's existence row, then B's; A's slices from the least significant up; B's slices
    from the least significant up.  Entries are (attribute, row of that attribute's own slice matrix), row 0 the MOST significant
    slice, row k the existence bitmap."""
    order = []
    if exists_a:
        order.append(("a", ka))
    if exists_b:
        order.append(("b", kb))
    order.extend(("a", i) for i in reversed(range(ka)))
    order.extend(("b", i) for i in reversed(range(kb)))
    return order


def table_rows(slices_a, ka, slices_b, kb, exists_a, exists_b):
    """The decoded rows of the table, in table order (slices_*: _bsi.build_slices matrices, the existence row last if any)."""
    return [(slices_a if who == "a" else slices_b)[i] for who, i in row_order(ka, kb, exists_a, exists_b)]


def sweep(slices_a, ka, slices_b, kb, n_out, exists_a=False, exists_b=False, skip_zero=True):
    """The fold as the interface states it, over the table's rows in order: an existence row ANDs into ex; A's slice i goes into
    the image; B's slice j, with carry = 0, does for i = 0 .. ka - 1 while i + j < n_out
        x = A_i & b;  p = P[i + j];  t = p ^ x;  P[i + j] = t ^ carry;  carry = (p & x) | (carry & t)
    and then P[ka + j] = carry where ka + j < n_out; B's slice 0 reads no P; a slice of B that is all zero (skip_zero) writes
    P[ka + j] = 0 alone.  P starts as None in every slice: a step that reads a slice nobody has written fails here.  Behind the
    rows P[sig] & ex is matrix row n_out - 1 - sig, zeros at and above ka + kb, then the ex row, if there is one."""
    n = slices_a.shape[1]
    zeros, ones = np.zeros(n, np.uint32), np.full(n, _bsi.ONES, np.uint32)
    ex = ones.copy()
    image, prod = [None] * ka, [None] * n_out
    n_ex = int(bool(exists_a)) + int(bool(exists_b))
    order = row_order(ka, kb, exists_a, exists_b)
    rows = [(slices_a if who == "a" else slices_b)[i] for who, i in order]
    for r, ((who, i), acc) in enumerate(zip(order, rows)):
        if r < n_ex:
            ex = ex & acc
            continue
        if who == "a":
            assert r - n_ex == ka - 1 - i, "A's slices come first, least significant first"
            image[ka - 1 - i] = acc
            continue
        j = kb - 1 - i
        assert r - n_ex - ka == j and all(s is not None for s in image), "A is complete before B's first slice"
        b, carry = acc, zeros
        if j != 0 and skip_zero and not b.any():
            if ka + j < n_out:
                assert prod[ka + j] is None, "the carry slot is nobody's yet"
                prod[ka + j] = zeros
            continue
        for s in range(ka):
            if s + j >= n_out:
                break
            x = image[s] & b
            if j == 0:
                assert prod[s] is None
                prod[s] = x
                continue
            p = prod[s + j]
            assert p is not None, ("step", j, "reads slice", s + j, "which nobody has written")
            t = p ^ x
            prod[s + j] = t ^ carry
            carry = (p & x) | (carry & t)
        if ka + j < n_out:
            assert prod[ka + j] is None, "the carry slot is nobody's yet"
            prod[ka + j] = carry
    out = np.zeros((n_out + (1 if n_ex else 0), n), np.uint32)
    for sig in range(n_out):
        if sig < ka + kb:
            assert prod[sig] is not None, ("slice", sig, "was never written")
            out[n_out - 1 - sig] = prod[sig] & ex
        else:
            assert prod[sig] is None
    if n_ex:
        out[n_out] = ex
    return out


def planted_pairs(ka, kb):
    """The rows in which the edges show, as (A, B) Python ints that fit the widths: both all ones (the longest carries), either
    operand 0, all ones times 1, and single powers of two in either operand against all ones and against a power of two."""
    top_a, top_b = (1 << ka) - 1, (1 << kb) - 1
    pairs = [(top_a, top_b), (0, top_b), (top_a, 0), (0, 0), (top_a, 1), (1, top_b)]
    pairs += [(1 << i, top_b) for i in range(ka)] + [(top_a, 1 << j) for j in range(kb)]
    pairs += [(1 << i, 1 << ((5 * i + 3) % kb)) for i in range(ka)]
    return list(dict.fromkeys(pairs))


def case(n_words, ka, kb, exists_a, exists_b, seed=0):
    """The headline case of a size and a pair of widths: uniform values, the rows of planted_pairs in rows of their own, and
    existence bitmaps of density 0.9 (None where the attribute has none) in which every planted row exists but the first two of
    `absent`: one planted all-ones row is absent from A's bitmap alone, one from B's alone.  Deterministic.  Returns (va, vb, xa,
    xb, planted, absent): planted maps (A, B) to its row, absent is the two rows."""
    rng = np.random.default_rng(49979687 * ka + 67867967 * kb + n_words + 7 * seed)
    rows = 32 * n_words
    va, vb = _bsi.uniform_values(rng, rows, ka).copy(), _bsi.uniform_values(rng, rows, kb).copy()
    pairs = planted_pairs(ka, kb)
    assert len(pairs) + 2 <= rows, "no room for the planted rows"
    at = rng.permutation(rows)[: len(pairs) + 2]
    va[at[:-2]] = np.array([p[0] for p in pairs], dtype=np.uint64)
    vb[at[:-2]] = np.array([p[1] for p in pairs], dtype=np.uint64)
    va[at[-2:]], vb[at[-2:]] = _mask(ka), _mask(kb)
    assert int(va.max()) <= int(_mask(ka)) and int(vb.max()) <= int(_mask(kb))
    xa, xb = rng.random(rows) < 0.9, rng.random(rows) < 0.9
    for x in (xa, xb):
        x[at] = True
    xa[at[-2]] = False
    xb[at[-1]] = False
    return va, vb, (xa if exists_a else None), (xb if exists_b else None), {p: int(r) for p, r in zip(pairs, at)}, (int(at[-2]), int(at[-1]))


def assert_mul_matters(va, vb, ka, kb, n_out, xa, xb, what):
    """The vacuity guard, numpy alone, asking what the semantics allow: with `width` the bits of the largest product, (2^ka - 1) *
    (2^kb - 1) -- ka + kb, one fewer where an operand has one bit -- every product slice below min(n_out, width) is neither
    empty nor full and every slice at or above width is empty; complementing an input slice below n_out changes the result
    (bit i of A reaches bit i + the lowest set bit of B: some row has B odd); dropping either existence row changes it."""
    def stored(a, b, ea, eb):
        ex = both(ea, eb)
        v = expected_values(a, b, n_out)
        return (v if ex is None else np.where(ex, v, np.uint64(0))), ex

    v, ex = stored(va, vb, xa, xb)
    width = (((1 << ka) - 1) * ((1 << kb) - 1)).bit_length()
    for sig in range(n_out):
        bits = (v >> np.uint64(sig)) & np.uint64(1)
        if sig >= width:
            assert not bits.any(), (what, "slice", sig, "of a zero extension is set")
        else:
            assert bits.any() and not bits.all(), (what, "slice", sig, "empty or full")
    if ex is not None:
        assert ex.any() and not ex.all(), (what, "the existence row is empty or full")

    def changed(a, b, ea, eb):
        w, wx = stored(a, b, ea, eb)
        return not np.array_equal(w, v) or (wx is None) != (ex is None) or (ex is not None and not np.array_equal(wx, ex))

    for j in range(min(ka, n_out)):
        assert changed(va ^ np.uint64(1 << j), vb, xa, xb), (what, "slice", j, "of A does not matter")
    for j in range(min(kb, n_out)):
        assert changed(va, vb ^ np.uint64(1 << j), xa, xb), (what, "slice", j, "of B does not matter")
    if xa is not None:
        assert changed(va, vb, None, xb), (what, "A's existence row does not matter")
    if xb is not None:
        assert changed(va, vb, xa, None), (what, "B's existence row does not matter")
