"""Shared helpers of the order-statistics tests (wah_bsi_kth_indexed_device: include/wah.h): the model that answers a query from
the VALUES, a numpy restatement of the digit-wise radix select over the slices, the query and filter cases, and input builders.
A bitmap of n_words words has 32 * n_words rows (tests/_bsi.py); values are numpy uint64, results five Python ints
(found, value, total, less, equal)."""
import numpy as np

from tests import _bsi

U64_MAX = (1 << 64) - 1
ASCENDING, DESCENDING, QUANTILE = 0, 1, 2


def rank_of(kind, a, b, total):
    """The rank from the bottom a query names among `total` rows, in Python ints, or None when it names no row."""
    if total == 0:
        return None
    if kind == ASCENDING:
        return a if a < total else None
    if kind == DESCENDING:
        return total - 1 - a if a < total else None
    if kind == QUANTILE and b > 0 and a <= b:
        return a * (total - 1) // b
    return None


def model(values, selected, kind, a, b):
    """From the values, never from slices: np.sort(values[selected])[rank], less and equal by comparison."""
    chosen = values if selected is None else values[selected]
    total = int(chosen.size)
    rank = rank_of(kind, a, b, total)
    if rank is None:
        return (0, 0, total, 0, 0)
    value = np.sort(chosen)[rank]
    return (1, int(value), total, int((chosen < value).sum()), int((chosen == value).sum()))


class Model:
    """model() for many queries over one selection: one sort, then the counts by binary search in it (test_kth_reference.py holds
    it against model())."""

    def __init__(self, values, selected=None):
        self.sorted = np.sort(values if selected is None else values[selected])
        self.total = int(self.sorted.size)

    def __call__(self, kind, a, b):
        rank = rank_of(kind, a, b, self.total)
        if rank is None:
            return (0, 0, self.total, 0, 0)
        value = self.sorted[rank]
        less = int(np.searchsorted(self.sorted, value, "left"))
        return (1, int(value), self.total, less, int(np.searchsorted(self.sorted, value, "right")) - less)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)).sum(dtype=np.int64))


def radix_select(slices, n_bits, filters, kind, a, b, digit, seen=None):
    """The kernels' algorithm on decoded bitmaps: digits of `digit` slices, most significant first, the last one possibly
    shorter.  Per digit: eq = AND of the filters and of B or ~B of every slice above the digit, by the prefix; a histogram of
    popcount(eq & pattern) over the digit's patterns; the bucket that holds the rank.  seen: a set that collects (digit width,
    bucket) of every decision, for the vacuity guard."""
    n = slices.shape[1]
    base = np.full(n, _bsi.ONES, np.uint32)
    for f in filters:
        base &= f
    prefix, rank, less, total, found, equal = 0, None, 0, 0, False, 0
    for first in range(0, n_bits, digit):
        end = min(first + digit, n_bits)
        width = end - first
        eq = base.copy()
        for i in range(first):
            eq &= slices[i] if (prefix >> (n_bits - 1 - i)) & 1 else ~slices[i]
        hist = []
        for pattern in range(1 << width):
            m = eq.copy()
            for i in range(first, end):
                m &= slices[i] if (pattern >> (end - 1 - i)) & 1 else ~slices[i]
            hist.append(popcount(m))
        if first == 0:
            total = sum(hist)
            rank = rank_of(kind, a, b, total)
            found = rank is not None
        bucket = 0
        if found:
            below = 0
            for bucket, h in enumerate(hist):
                if rank < below + h:
                    equal = h
                    break
                below += h
            rank -= below
            less += below
            if seen is not None:
                seen.add((width, bucket))
        prefix |= bucket << (n_bits - end)
    return (1, prefix, total, less, equal) if found else (0, 0, total, 0, 0)


def query_cases(total, spread=False):
    """(name, kind, a, b) for every query the interface names, around `total` selected rows; spread: sixteen ranks across them
    too, so that every bucket of a digit gets picked."""
    cases = [("rank 0 up", ASCENDING, 0, 1), ("rank 0 down", DESCENDING, 0, 1), ("last up", ASCENDING, max(total - 1, 0), 1),
             ("last down", DESCENDING, max(total - 1, 0), 1), ("rank total up", ASCENDING, total, 1), ("rank total down", DESCENDING, total, 1),
             ("rank 2^64 - 1 up", ASCENDING, U64_MAX, 0), ("rank 2^64 - 1 down", DESCENDING, U64_MAX, 0),
             ("third up", ASCENDING, total // 3, 1), ("third down", DESCENDING, total // 3, 1),
             ("min", QUANTILE, 0, 1), ("median", QUANTILE, 1, 2), ("max", QUANTILE, 1, 1), ("2^64 - 1 / 2^64 - 1", QUANTILE, U64_MAX, U64_MAX),
             ("(2^64 - 2) / (2^64 - 1)", QUANTILE, U64_MAX - 1, U64_MAX), ("0.99", QUANTILE, 99, 100),
             ("b = 0", QUANTILE, 0, 0), ("a > b", QUANTILE, 3, 2), ("kind 3", 3, 0, 1), ("kind 2^64 - 1", U64_MAX, 0, 1)]
    if spread:
        cases += [("rank %d/16" % i, ASCENDING, total * i // 16, 1) for i in range(1, 16)]
    return cases


def tie_values(rows, n_bits, boundary):
    """Two values whose ties straddle a segment boundary: the low one up to row `boundary` + 7, the high one from there."""
    top = (1 << n_bits) - 1
    low, high = top // 3, top // 3 + 1 if n_bits > 1 else 1
    v = np.full(rows, low, np.uint64)
    v[min(boundary + 7, rows - 1):] = high
    return v


def value_sets(rng, rows, n_bits, boundary):
    """name -> values: the four kinds of make_values, all rows equal, and the two-valued ties."""
    out = {kind: _bsi.make_values(kind, rng, rows, n_bits) for kind in ("uniform", "low", "high", "clustered")}
    out["equal"] = np.full(rows, ((1 << n_bits) - 1) * 5 // 7, np.uint64)
    out["ties"] = tie_values(rows, n_bits, boundary)
    return out


def mask_sets(rng, rows):
    """name -> bool rows: the masks the interface names (one row, dense, none, all)."""
    one = np.zeros(rows, bool)
    one[rows * 2 // 3] = True
    return {"one row": one, "dense": rng.random(rows) < 0.6, "zeros": np.zeros(rows, bool), "ones": np.ones(rows, bool),
            "sparse": rng.random(rows) < 0.01}
