"""Shared helpers of the bit-sliced index tests (wah_bsi_range_indexed_device): a numpy model that answers a range predicate from
the VALUES, a slice builder, two numpy restatements of the slice sweep, value generators, the bound edge cases and the vacuity
guard.  A bitmap of n_words words has 32 * n_words rows, row p at word p // 32, bit p % 32 (LSB first); values are numpy uint64."""
import numpy as np

U64_MAX = (1 << 64) - 1
ONES = np.uint32(0xFFFFFFFF)


def pack_bits(bits):
    """A bool array of 32 * n rows -> the n uint32 words of its bitmap."""
    bits = np.ascontiguousarray(bits, dtype=bool)
    assert bits.size % 32 == 0
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def unpack_bits(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").astype(bool)


def expected_range(values, lo, hi, exists=None):
    """The model: rows with lo <= value <= hi (Python ints, both inclusive) that exist -- from the values, never from slices."""
    if lo > U64_MAX or hi < 0 or lo > hi:
        match = np.zeros(values.shape, bool)
    else:
        match = (values >= np.uint64(max(lo, 0))) & (values <= np.uint64(min(hi, U64_MAX)))
    return pack_bits(match if exists is None else match & exists)


def build_slices(values, n_bits, exists=None, zero_missing=False):
    """The decoded slice matrix [n_bits (+ 1), rows / 32]: row i holds bit n_bits - 1 - i of every value (row 0: the MOST significant
    bit), the existence bitmap comes last when there is one.  zero_missing: rows that do not exist are stored with the value 0."""
    v = values if exists is None or not zero_missing else np.where(exists, values, np.uint64(0))
    rows = [pack_bits((v >> np.uint64(n_bits - 1 - i)) & np.uint64(1)) for i in range(n_bits)]
    if exists is not None:
        rows.append(pack_bits(exists))
    return np.stack(rows)


def values_of_slices(slices, n_bits):
    """The inverse of build_slices: the uint64 values (and the existence row, or None)."""
    v = np.zeros(32 * slices.shape[1], np.uint64)
    for i in range(n_bits):
        v |= unpack_bits(slices[i]).astype(np.uint64) << np.uint64(n_bits - 1 - i)
    return v, (unpack_bits(slices[n_bits]) if slices.shape[0] > n_bits else None)


def _clamp(lo, hi, n_bits):
    top = (1 << n_bits) - 1
    return lo > hi or lo > top, min(hi, top)


def sweep(slices, n_bits, lo, hi, has_exists=False):
    """The O'Neil & Quass sweep as the interface states it, most significant slice first, four bitmaps of state:
    GT |= EQlo & B if lo's bit is 0; EQlo &= B or ~B; LT |= EQhi & ~B if hi's bit is 1; EQhi &= B or ~B;
    result = (GT | EQlo) & (LT | EQhi) [& exists].  An empty range is all zeros; hi is clamped to the slices' width."""
    n = slices.shape[1]
    none, hi = _clamp(lo, hi, n_bits)
    if none:
        return np.zeros(n, np.uint32)
    gt, lt = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    eq_lo, eq_hi = np.full(n, ONES, np.uint32), np.full(n, ONES, np.uint32)
    for i in range(n_bits):
        b, sig = slices[i], n_bits - 1 - i
        if not (lo >> sig) & 1:
            gt |= eq_lo & b
        eq_lo &= b if (lo >> sig) & 1 else ~b
        if (hi >> sig) & 1:
            lt |= eq_hi & ~b
        eq_hi &= b if (hi >> sig) & 1 else ~b
    result = (gt | eq_lo) & (lt | eq_hi)
    return result & slices[n_bits] if has_exists else result


def sweep_three(slices, n_bits, lo, hi, has_exists=False):
    """The same sweep with the state the kernel keeps: GT and LT share one bitmap that is only fed behind the first bit in which
    the bounds differ, and result = IN | EQlo | EQhi."""
    n = slices.shape[1]
    none, hi = _clamp(lo, hi, n_bits)
    inside = np.zeros(n, np.uint32)
    eq_lo, eq_hi = np.full(n, ONES, np.uint32), np.full(n, ONES, np.uint32)
    diverged = False
    for i in range(n_bits):
        b, sig = slices[i], n_bits - 1 - i
        l, h = (lo >> sig) & 1, (hi >> sig) & 1
        if diverged and not l:
            inside |= eq_lo & b
        if diverged and h:
            inside |= eq_hi & ~b
        eq_lo &= b if l else ~b
        eq_hi &= b if h else ~b
        diverged = diverged or l != h
    result = inside | eq_lo | eq_hi
    if has_exists:
        result &= slices[n_bits]
    return np.zeros(n, np.uint32) if none else result


# ---- values -------------------------------------------------------------------------------------------------------------------
def uniform_values(rng, rows, n_bits):
    """Uniform over the full width: every slice is incompressible."""
    return np.frombuffer(rng.bytes(8 * rows), dtype=np.uint64) >> np.uint64(64 - n_bits)


def make_values(kind, rng, rows, n_bits):
    """uniform; low: the top 10 bits zero (slices settled in the gather); high: the top 10 bits one; clustered: constant over runs
    of some thousand rows (fills with an effect).  Widths below 12 bits keep at least two free bits."""
    top = min(10, max(n_bits - 2, 0))
    if kind == "uniform":
        return uniform_values(rng, rows, n_bits)
    if kind == "low":
        return uniform_values(rng, rows, n_bits) >> np.uint64(top)
    if kind == "high":
        mask = ((1 << top) - 1) << (n_bits - top)
        return (uniform_values(rng, rows, n_bits) >> np.uint64(top)) | np.uint64(mask)
    if kind == "clustered":
        runs = rng.integers(1500, 6000, rows // 1500 + 2)
        v = np.repeat(uniform_values(rng, runs.size, n_bits), runs)[:rows]
        assert v.size == rows
        return np.ascontiguousarray(v)
    raise ValueError(kind)


def plant(values, rng, wanted, exists=None, free=None):
    """Write every value of `wanted` into a row of its own (distinct random rows, made to exist; free: a bool mask of the rows that
    may be taken): the rows a bound's neighbours need."""
    wanted = sorted(set(int(w) for w in wanted))
    candidates = np.arange(values.size) if free is None else np.flatnonzero(free)
    assert len(wanted) <= candidates.size
    at = candidates[rng.permutation(candidates.size)[: len(wanted)]]
    values = values.copy()
    values[at] = np.array(wanted, dtype=np.uint64)
    if exists is not None:
        exists = exists.copy()
        exists[at] = True
    return values, exists


def neighbours(lo, hi, n_bits):
    """lo, hi and both with every single bit flipped."""
    return [lo, hi] + [lo ^ (1 << j) for j in range(n_bits)] + [hi ^ (1 << j) for j in range(n_bits)]


def assert_range_matters(values, n_bits, lo, hi, exists, what):
    """The vacuity guard, numpy alone: the expected bitmap is neither all zeros nor all ones, flipping any single bit of lo or of hi
    changes it, and so does dropping the existence row."""
    want = expected_range(values, lo, hi, exists)
    assert want.any() and not (want == ONES).all(), what
    for j in range(n_bits):
        assert not np.array_equal(expected_range(values, lo ^ (1 << j), hi, exists), want), (what, "bit", j, "of lo does not matter")
        assert not np.array_equal(expected_range(values, lo, hi ^ (1 << j), exists), want), (what, "bit", j, "of hi does not matter")
    if exists is not None:
        assert not np.array_equal(expected_range(values, lo, hi, None), want), (what, "the existence row does not matter")
    return want


def bound_cases(values, n_bits):
    """(name, lo, hi) for every edge the interface names, around the values at hand."""
    top = (1 << n_bits) - 1
    present = sorted(set(int(v) for v in values[:: max(values.size // 64, 1)]))
    mid = present[len(present) // 2]
    q1, q3 = present[len(present) // 4], present[(3 * len(present)) // 4]
    everything = set(int(v) for v in values)
    absent = next((c for c in range(mid, min(mid + 4096, top + 1)) if c not in everything), None)
    below = min(mid, top - 1)
    cases = [("eq present", mid, mid), ("lo 0", 0, mid), ("hi max", mid, top), ("all", 0, top), ("quartiles", q1, q3),
             ("lo > hi", max(q3, 1), min(q1, max(q3, 1) - 1)), ("lo = hi + 1", below + 1, below), ("eq 0", 0, 0), ("eq max", top, top)]
    if absent is not None:
        cases.append(("eq absent", absent, absent))
    if n_bits >= 8:
        prefix = mid & ~0x3F
        cases.append(("long shared prefix", prefix | 0x05, prefix | 0x2B))
    if n_bits >= 3:
        half = 1 << (n_bits - 1)
        cases.append(("differ in the top bit", half - 3, half + 2))
        cases.append(("differ in the top bit, wide", q1 & (half - 1), half | (q3 & (half - 1))))
    if n_bits < 64:
        cases += [("hi = 2^k", mid, 1 << n_bits), ("hi = 2^64 - 1", q1, U64_MAX), ("hi beyond, lo 0", 0, (1 << n_bits) + 12345 if n_bits < 63 else U64_MAX),
                  ("lo = 2^k", 1 << n_bits, U64_MAX), ("lo beyond, lo > hi too", (1 << n_bits) + 5, (1 << n_bits) + 3 if n_bits < 63 else 1 << 63)]
    else:
        cases += [("eq 2^64 - 1", U64_MAX, U64_MAX), ("0 .. 2^64 - 1", 0, U64_MAX), ("mid .. 2^64 - 1", mid, U64_MAX), ("2^64 - 1 .. 0", U64_MAX, 0),
                  ("2^63 .. 2^64 - 1", 1 << 63, U64_MAX)]
    return cases


def headline(n_words, n_bits, with_exists, kind="uniform", empty=None):
    """The headline case of a size and a width: values of `kind`, an existence bitmap of density 0.9, a range from about three tenths
    to about seven tenths of the width with irregular bits, and the bounds' neighbours planted so that every bit of either bound
    decides at least one row (assert_range_matters).  empty: (first, end) rows that do not exist at all.  Returns (values, exists or None, lo, hi); deterministic."""
    rng = np.random.default_rng(7919 * n_bits + n_words)
    rows = 32 * n_words
    values = make_values(kind, rng, rows, n_bits)
    exists = rng.random(rows) < 0.9 if with_exists else None
    top = (1 << n_bits) - 1
    lo, hi = (top * 3) // 10, (top * 7) // 10
    if n_bits >= 8:
        lo, hi = lo ^ (0x5A & top), hi ^ (0xA5 & top)
    if n_bits <= 2:
        lo, hi = 1, top - (n_bits == 2)  # 1 .. 1 of 0 .. 1, 1 .. 2 of 0 .. 3
    free = np.ones(rows, bool)
    if empty is not None:
        exists[empty[0]: empty[1]] = False
        free[empty[0]: empty[1]] = False
    values, exists = plant(values, rng, neighbours(lo, hi, n_bits), exists, free)
    if exists is not None:  # a row inside the range that does not exist
        inside = np.flatnonzero((values >= np.uint64(lo)) & (values <= np.uint64(hi)) & (values != np.uint64(lo)) & (values != np.uint64(hi)))
        if inside.size == 0:
            inside = np.flatnonzero((values >= np.uint64(lo)) & (values <= np.uint64(hi)))
            extra = np.flatnonzero(~((values >= np.uint64(lo)) & (values <= np.uint64(hi))))[:1]
            values[extra] = np.uint64(lo)
            exists[extra] = False
        else:
            exists[inside[0]] = False
    return values, exists, lo, hi
