"""Shared helpers of the column division tests (wah_bsi_div_indexed_device), numpy only: a model that answers `A / B` and `A % B`
from the VALUES (a row with B = 0 has no result), an independent restatement of the table order, the restoring long division
over the slice matrices of tests/_bsi.py as the interface states it (B's image, the shifted remainder R and R - B = T, the
quotient bit that says which of the two the next step reads, the skip of the dividend's leading zero slices), seven WRONG models
with one error each, and the value pairs of the GPU tests with their planted rows."""
import numpy as np

from tests import _bsi, _cmp

EXISTENCE = _cmp.EXISTENCE  # none / A / B / both
# (ka, kb, n_out): (40, 41, 20) truncates, (5, 3, 12) extends
WIDTHS = ((1, 1, 1), (3, 5, 3), (5, 3, 5), (8, 8, 8), (20, 13, 20), (13, 20, 13), (32, 32, 32), (33, 31, 33), (64, 64, 64), (64, 1, 64),
          (1, 64, 1), (40, 41, 20), (5, 3, 12))
WRONG = ("zero_divisor_kept", "narrow_ripple", "not_restored", "a_least_significant_first", "skip_after_nonzero", "truncated_dividend",
         "unblended_remainder")


def _mask(k):
    return np.uint64((1 << k) - 1)


def expected_values(va, vb, n_out, remainder):
    """floor(va / vb) or va mod vb, mod 2^n_out, in uint64; where vb == 0 the value is 0 (the row does not exist)."""
    safe = np.where(vb != 0, vb, np.uint64(1))
    v = (va % safe) if remainder else (va // safe)
    return np.where(vb != 0, v, np.uint64(0)) & _mask(n_out)


def existence(vb, xa=None, xb=None):
    """xa & xb & (vb != 0) as a bool array: the result's existence row, which is always there."""
    ex = vb != 0
    for x in (xa, xb):
        if x is not None:
            ex = ex & x
    return ex


def expected_matrix(va, vb, n_out, remainder, xa=None, xb=None):
    """The model: the decoded slice matrix of the result, most significant slice first, the existence row ALWAYS last, rows that do
    not exist stored as 0 -- from the values, never from slices."""
    return _bsi.build_slices(expected_values(va, vb, n_out, remainder), n_out, existence(vb, xa, xb), zero_missing=True)


def natural_width(ka, kb, remainder):
    """The bits of the largest result: the quotient reaches 2^ka - 1 (B = 1), the remainder min(2^ka - 1, 2^kb - 2)."""
    top_a, top_b = (1 << ka) - 1, (1 << kb) - 1
    return min(top_a, top_b - 1).bit_length() if remainder else ka


def row_order(ka, kb, exists_a, exists_b):
    """The table order, restated from the widths: A's existence row, then B's; B's slices from the least significant up; A's
    slices from the most significant down.  Entries are (attribute, row of that attribute's own slice matrix), row 0 the MOST
    significant slice, row k the existence bitmap."""
    order = []
    if exists_a:
        order.append(("a", ka))
    if exists_b:
        order.append(("b", kb))
    order.extend(("b", i) for i in reversed(range(kb)))
    order.extend(("a", i) for i in range(ka))
    return order


def table_rows(slices_a, ka, slices_b, kb, exists_a, exists_b):
    """The decoded rows of the table, in table order (slices_*: _bsi.build_slices matrices, the existence row last if any)."""
    return [(slices_a if who == "a" else slices_b)[i] for who, i in row_order(ka, kb, exists_a, exists_b)]


def sweep(slices_a, ka, slices_b, kb, n_out, remainder, exists_a=False, exists_b=False, skip=True, wrong=None, stats=None):
    """The fold as the interface states it, over the table's rows in order: an existence row ANDs into ex; B's slice s goes into
    the image and ORs into nz, and behind B's last slice ex &= nz; A's slice i (i = ka - 1 down to 0), with Re[s] = q ? T[s] : R[s]
    the remainder the step before left, does Rn[0] = A_i, Rn[s + 1] = Re[s] for s < kb, borrow = 0, and for s = 0 .. kb with b = B_s
    (0 at s = kb)
        Tn[s] = Rn[s] ^ b ^ borrow;  borrow = (~Rn[s] & b) | (~(Rn[s] ^ b) & borrow)
    then q = ~borrow, R = Rn, T = Tn; q & ex is quotient slice i.  While every slice of A so far was all zero (skip) the step stores
    a zero quotient slice and touches nothing; the first step that runs takes Re as zeros; and B's slices above its last one that
    is not all zero are left out of every ripple (skip too).  R and T start as None in every slice: a step that reads a slice
    nobody has written fails here.  Behind the rows: QUOTIENT zeros at and above ka; REMAINDER Re[sig] & ex for sig < min(kb,
    n_out), zeros above; then the ex row.  wrong: one of WRONG, a model with that one error.  stats: a dict that receives the
    number of skipped steps."""
    assert wrong is None or wrong in WRONG
    n = slices_a.shape[1]
    zeros, ones = np.zeros(n, np.uint32), np.full(n, _bsi.ONES, np.uint32)
    ex, nz = ones.copy(), zeros.copy()
    image, R, T, q = [None] * kb, [None] * (kb + 1), [None] * (kb + 1), None
    quot = [None] * ka
    started, skipped, kb_run, ripple = False, 0, kb, kb + 1
    n_ex = int(bool(exists_a)) + int(bool(exists_b))
    order = row_order(ka, kb, exists_a, exists_b)
    rows = [(slices_a if who == "a" else slices_b)[i] for who, i in order]
    if wrong == "a_least_significant_first":
        rows[n_ex + kb:] = rows[n_ex + kb:][::-1]

    def blended(s):
        assert R[s] is not None and T[s] is not None, ("slice", s, "of the remainder was never written")
        if wrong == "not_restored":
            return T[s]
        return (T[s] & q) | (R[s] & ~q)

    for r, ((who, col), acc) in enumerate(zip(order, rows)):
        if r < n_ex:
            ex = ex & acc
            continue
        if who == "b":
            s = kb - 1 - col
            assert r - n_ex == s, "B's slices come first, least significant first"
            image[s] = acc
            nz = nz | acc
            if s == kb - 1 and wrong != "zero_divisor_kept":
                ex = ex & nz
            continue
        i = ka - 1 - col
        assert r - n_ex - kb == col and all(s is not None for s in image), "B is complete before A's first slice, A comes from the top"
        if not started:  # B's slices that take part: up to its last one that is not all zero
            kb_run = max([s + 1 for s in range(kb) if image[s].any()] + [1]) if skip else kb
            ripple = kb_run if wrong == "narrow_ripple" else kb_run + 1
        if wrong == "truncated_dividend" and i >= n_out:
            quot[i] = zeros
            continue
        zero = not acc.any()
        if skip and zero and (not started or wrong == "skip_after_nonzero"):
            quot[i] = zeros
            skipped += 1
            continue
        re = [zeros] * kb_run if not started else [blended(s) for s in range(kb_run)]
        started = True
        rn = [acc] + re
        borrow, tn = zeros, []
        for s in range(ripple):
            b = image[s] if s < kb_run else zeros
            tn.append(rn[s] ^ b ^ borrow)
            borrow = (~rn[s] & b) | (~(rn[s] ^ b) & borrow)
        q = ~borrow
        R, T = rn + [None] * (kb - kb_run), tn + [None] * (kb + 1 - ripple)
        quot[i] = q
    if stats is not None:
        stats["skipped"] = skipped
    out = np.zeros((n_out + 1, n), np.uint32)
    for sig in range(n_out):
        if not remainder:
            if sig < ka:
                assert quot[sig] is not None, ("quotient slice", sig, "was never written")
                out[n_out - 1 - sig] = quot[sig] & ex
        elif started and sig < kb_run:
            out[n_out - 1 - sig] = (R[sig] if wrong == "unblended_remainder" else blended(sig)) & ex
    out[n_out] = ex
    return out


def planted_pairs(ka, kb):
    """The rows in which the edges show, as (A, B) Python ints that fit the widths: the largest quotient, a zero dividend, both all
    ones, a zero divisor with and without a dividend, the largest remainder where it fits, a single power of two in the dividend
    over 1 (every quotient slice) and over all ones (every remainder slice), all ones over every power of two (a shift)."""
    top_a, top_b = (1 << ka) - 1, (1 << kb) - 1
    pairs = [(top_a, 1), (0, top_b), (top_a, top_b), (top_a, 0), (0, 0)]
    if 0 < top_b - 1 <= top_a:
        pairs.append((top_b - 1, top_b))
    pairs += [(1 << i, 1) for i in range(ka)] + [(1 << i, top_b) for i in range(ka)] + [(top_a, 1 << j) for j in range(kb)]
    return list(dict.fromkeys(pairs))


def draw(rng, rows, k):
    """A uniform value of k bits shifted right by a per-row random 0 .. k - 1: results of every width."""
    return _bsi.uniform_values(rng, rows, k) >> rng.integers(0, k, rows).astype(np.uint64)


def case(n_words, ka, kb, exists_a, exists_b, seed=0):
    """The headline case of a size and a pair of widths: values of every width (draw), B = 0 in one row of sixteen (and in no other
    but a planted one: a draw that comes out as 0 is 1, or a narrow B would be 0 in a third of the rows), the rows of
    planted_pairs in rows of their own, and existence bitmaps of density 0.9 (None where the attribute has none) in which every
    planted row exists but the two of `absent`: one row of both operands all ones is absent from A's bitmap alone, one from B's
    alone.  Deterministic.  Returns (va, vb, xa, xb, planted, absent): planted maps (A, B) to its row."""
    rng = np.random.default_rng(49979687 * ka + 67867967 * kb + n_words + 7 * seed + 3)
    rows = 32 * n_words
    va, vb = draw(rng, rows, ka).copy(), draw(rng, rows, kb).copy()
    vb[vb == 0] = 1  # (a narrow B shifted down is 0 in a third of the rows: the zero divisors are the forced ones alone)
    vb[rng.random(rows) < 1.0 / 16.0] = 0
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


def assert_div_matters(va, vb, ka, kb, n_out, remainder, xa, xb, what):
    """The vacuity guard, numpy alone, asking what the semantics allow: at least three quarters of the rows have B != 0; every
    output slice below min(n_out, natural_width) is neither empty nor full and every slice at or above the natural width is empty;
    the existence row differs from xa & xb (some row that exists in both has B = 0); complementing any input slice changes the
    result (`A % B` with a one-bit B is 0 whatever A holds: there A's slices cannot matter and are not asked); dropping either
    existence row changes it."""
    def stored(a, b, ea, eb):
        return expected_values(a, b, n_out, remainder) * existence(b, ea, eb).astype(np.uint64), existence(b, ea, eb)

    v, ex = stored(va, vb, xa, xb)
    assert 4 * int((vb != 0).sum()) >= 3 * vb.size, (what, "too many zero divisors")
    width = natural_width(ka, kb, remainder)
    for sig in range(n_out):
        bits = (v >> np.uint64(sig)) & np.uint64(1)
        if sig >= width:
            assert not bits.any(), (what, "slice", sig, "above the natural width is set")
        else:
            assert bits.any() and not bits.all(), (what, "slice", sig, "empty or full")
    operands = np.ones(va.shape, bool)
    for x in (xa, xb):
        if x is not None:
            operands = operands & x
    assert ex.any() and not np.array_equal(ex, operands), (what, "the existence row is that of the operands")

    def changed(a, b, ea, eb):
        w, wx = stored(a, b, ea, eb)
        return not np.array_equal(w, v) or not np.array_equal(wx, ex)

    if width:
        for j in range(ka):
            assert changed(va ^ np.uint64(1 << j), vb, xa, xb), (what, "slice", j, "of A does not matter")
    for j in range(kb):
        assert changed(va, vb ^ np.uint64(1 << j), xa, xb), (what, "slice", j, "of B does not matter")
    if xa is not None:
        assert changed(va, vb, None, xb), (what, "A's existence row does not matter")
    if xb is not None:
        assert changed(va, vb, xa, None), (what, "B's existence row does not matter")
