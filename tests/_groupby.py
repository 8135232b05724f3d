"""Shared helpers of the group-by tests (wah_bsi_group_by_indexed_device, include/wah.h): a numpy model that answers COUNT and
SUM per bucket from the VALUES, the kernel's steps restated in numpy from the SLICES, seven wrong models of that restatement, and
the builders of the named cases.  A bitmap of n words has 32 * n rows, row p at word p // 32, bit p % 32; keys and values are numpy
uint64, a lookup is uint32.  Everything is integer-exact: counts and sums are Python ints.

A case is a dict: n (words), n_rows, ks (key slices), vs (value slices, 0: count only), keys, exists (the key's existence bitmap
or None), vals (or None), filters (a list of bool arrays), lookup (uint32 [n_keys] or None), n_buckets, and prefill: None, or
(counts, sums) -- Python ints per bucket, "other" included, the sums as whole 128-bit numbers -- that WAH_GROUP_BY_ACCUMULATE adds
into."""
import numpy as np

from tests import _bsi

SEG_WORDS, SEG_GROUPS, SEG_BITS = 992, 1024, 31 * 1024
HALF_GROUPS, HALF_ROWS = 512, 31 * 512
GRID_ITEMS = 512     # kGroupByGridItems of wah_group_by.hip: workgroups at the most
LDS_BUCKETS = 2048   # kGroupByLdsBuckets: buckets, "other" included, up to which an item adds in LDS
DROP = 0xFFFFFFFF
M64 = (1 << 64) - 1
WRONG = ("rows behind n_rows counted", "other dropped", "map read behind n_keys", "last run of a lane lost", "carry dropped",
         "both halves count the whole segment", "existence ignored under a filter")


# ---- the value model -------------------------------------------------------------------------------------------------------------
def buckets_of(case, keys):
    """The bucket of every key: through the lookup where there is one, "other" (n_buckets) for a key behind it or a bucket at or
    above n_buckets."""
    nb = case["n_buckets"]
    k = keys.astype(np.int64)
    if case["lookup"] is None:
        b = k
    else:
        inside = k < case["lookup"].size
        b = np.full(k.shape, nb, np.int64)
        b[inside] = case["lookup"][k[inside]].astype(np.int64)
    return np.where(b < nb, b, nb)


def selected(case):
    rows = 32 * case["n"]
    sel = np.arange(rows) < case["n_rows"]
    if case["exists"] is not None:
        sel &= case["exists"]
    for f in case["filters"]:
        sel &= f
    return sel


def expected(case):
    """The model: (counts, sums) as lists of Python ints per bucket, "other" last; sums is None for count only.  From the values,
    never from slices."""
    nb = case["n_buckets"]
    sel = selected(case)
    b = buckets_of(case, case["keys"][sel])
    counts = [int(c) for c in np.bincount(b, minlength=nb + 1)]
    sums = None
    if case["vs"]:
        sums = [0] * (nb + 1)
        v = case["vals"][sel]
        order = np.argsort(b, kind="stable")
        bs, vsorted = b[order], v[order]
        if bs.size:  # (values are below 2^32 and rows below 2^32: a bucket's sum fits uint64)
            assert bs.size < 1 << 32 and case["vs"] <= 32
            starts = np.flatnonzero(np.r_[True, bs[1:] != bs[:-1]])
            for at, total in zip(starts, np.add.reduceat(vsorted, starts)):
                sums[int(bs[at])] = int(total)
    if case["prefill"] is not None:
        counts = [(c + p) & M64 for c, p in zip(counts, case["prefill"][0])]
        if sums is not None:
            sums = [(s + p) & ((1 << 128) - 1) for s, p in zip(sums, case["prefill"][1])]
    return counts, sums


# ---- the kernel's steps ------------------------------------------------------------------------------------------------------------
def _words_of(slices, width):
    """One word per row out of a decoded slice matrix [width, words], most significant slice first: the fold."""
    v = np.zeros(32 * slices.shape[1], np.uint64)
    for i in range(width):
        v |= _bsi.unpack_bits(slices[i]).astype(np.uint64) << np.uint64(width - 1 - i)
    return v


class _Outputs:
    """counts and (low, high) sums in device memory: 64-bit words, the adds the kernel's atomics are."""

    def __init__(self, case, wrong):
        nb = case["n_buckets"]
        pre = case["prefill"]
        self.counts = [0] * (nb + 1) if pre is None else [int(c) for c in pre[0]]
        self.low = [0] * (nb + 1) if pre is None else [int(s) & M64 for s in pre[1]]
        self.high = [0] * (nb + 1) if pre is None else [int(s) >> 64 for s in pre[1]]
        self.val, self.wrong = case["vs"] != 0, wrong

    def add(self, b, count, total):
        self.counts[b] = (self.counts[b] + count) & M64
        if self.val and total:
            old = self.low[b]
            self.low[b] = (old + total) & M64
            if self.low[b] < old and self.wrong != "carry dropped":  # old + x < old: the returning add's carry
                self.high[b] = (self.high[b] + 1) & M64

    def result(self):
        return self.counts, ([lo + (hi << 64) for lo, hi in zip(self.low, self.high)] if self.val else None)


def kernel(case, wrong=None):
    """wah_group_by.hip restated: the items (a segment, with a value attribute a segment and a half of its groups), the key and
    value words out of the slices, the selection image (all ones clipped to n_rows, ANDed with the existence row and the filters),
    the lanes' groups of 31 rows with their runs of equal consecutive buckets merged, the adds of the route -- per item in LDS
    buckets that are flushed with one add each, or per run into the outputs -- and the carry into the high sum word."""
    n, nb, vs = case["n"], case["n_buckets"], case["vs"]
    groups = (32 * n + 30) // 31
    n_seg = -(-groups // SEG_GROUPS)
    rows_all = n_seg * SEG_BITS

    def padded(a, dtype):
        out = np.zeros(rows_all, dtype)
        out[: min(a.size, rows_all)] = a[:rows_all]
        return out

    key_slices = _bsi.build_slices(case["keys"], case["ks"])
    keys = padded(_words_of(key_slices, case["ks"]), np.uint64)
    vals = padded(_words_of(_bsi.build_slices(case["vals"], vs), vs), np.uint64) if vs else np.zeros(rows_all, np.uint64)
    limit = 32 * n if wrong == "rows behind n_rows counted" else case["n_rows"]
    image = np.arange(rows_all) < limit  # the preset: all ones, clipped
    if case["exists"] is not None and not (wrong == "existence ignored under a filter" and case["filters"]):
        image &= padded(case["exists"], bool)
    for f in case["filters"]:
        image &= padded(f, bool)
    lookup = case["lookup"]
    out = _Outputs(case, wrong)
    lds = nb + 1 <= LDS_BUCKETS
    halves = 2 if vs else 1
    for t in range(n_seg * halves):
        seg, half = divmod(t, halves)
        lo = seg * SEG_BITS + (half * HALF_ROWS if vs else 0)
        hi = lo + (HALF_ROWS if vs else SEG_BITS)
        if wrong == "both halves count the whole segment":
            lo, hi = seg * SEG_BITS, (seg + 1) * SEG_BITS
        rows = lo + np.flatnonzero(image[lo:hi])
        k = keys[rows].astype(np.int64)
        if lookup is None:
            b = k
        elif wrong == "map read behind n_keys":
            b = np.r_[lookup.astype(np.int64), np.zeros(1 << 12, np.int64)][np.minimum(k, lookup.size + (1 << 12) - 1)]
        else:
            b = np.where(k < lookup.size, lookup.astype(np.int64)[np.minimum(k, lookup.size - 1)], DROP)
        b = np.where(b < nb, b, nb)
        lane = rows // 31  # a lane takes one group of 31 rows and visits them in order
        first = np.r_[True, (lane[1:] != lane[:-1]) | (b[1:] != b[:-1])] if rows.size else np.zeros(0, bool)
        starts = np.flatnonzero(first)
        ends = np.r_[starts[1:], rows.size]
        v = vals[rows]
        item_counts, item_sums = {}, {}
        for at, end in zip(starts, ends):
            if wrong == "last run of a lane lost" and (end == rows.size or lane[end] != lane[at]):
                continue
            bucket, count, total = int(b[at]), int(end - at), int(v[at:end].sum())
            if wrong == "other dropped" and bucket == nb:
                continue
            if lds:
                item_counts[bucket] = item_counts.get(bucket, 0) + count
                item_sums[bucket] = item_sums.get(bucket, 0) + total
            else:
                out.add(bucket, count, total)
        for bucket in sorted(item_counts):  # the flush: the item's non-zero buckets
            out.add(bucket, item_counts[bucket], item_sums[bucket])
    return out.result()


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def make_case(n, ks, vs, n_filters=0, with_exists=False, n_rows=None, n_buckets=None, lookup=None, pattern="random", seed=0, prefill=None):
    rng = np.random.default_rng(7919 * ks + 31 * vs + n + seed)
    rows = 32 * n
    if n_buckets is None:
        n_buckets = min(1 << ks, 1 << 12) if lookup is None else max(int(lookup[lookup != DROP].max()) + 1 if (lookup != DROP).any() else 1, 1)
    domain = 1 << ks
    if pattern == "random":
        keys = _bsi.uniform_values(rng, rows, ks)
        if ks > 12:  # half of the keys inside the buckets, the rest anywhere in the width
            keys = np.where(rng.random(rows) < 0.5, rng.integers(0, min(domain, 2 * n_buckets), rows, dtype=np.uint64), keys)
    elif pattern == "one key":
        keys = np.full(rows, min(domain - 1, 5), np.uint64)
    elif pattern == "alternating":
        keys = np.where(np.arange(rows) % 2 == 0, np.uint64(domain - 1 if domain <= n_buckets else 1), np.uint64(0))
    elif pattern == "sorted":
        keys = np.sort(rng.integers(0, min(domain, n_buckets + 3), rows, dtype=np.uint64))
    else:
        raise ValueError(pattern)
    vals = _bsi.uniform_values(rng, rows, vs) if vs else None
    exists = rng.random(rows) < 0.9 if with_exists else None
    filters = [rng.random(rows) < 0.7 for _ in range(n_filters)]
    return dict(n=n, n_rows=rows if n_rows is None else n_rows, ks=ks, vs=vs, keys=keys, exists=exists, vals=vals, filters=filters,
                lookup=None if lookup is None else np.asarray(lookup, np.uint32), n_buckets=n_buckets, prefill=prefill)


SIZES = (1, 31, SEG_WORDS, SEG_WORDS * 3 + 5)
KEY_WIDTHS, VALUE_WIDTHS, FILTER_COUNTS = (1, 8, 11, 12, 32), (0, 1, 17, 32), (0, 1, 3)
BIG = SEG_WORDS * 3 + 5


def carry_prefill(n_buckets):
    """Counts of 7 and a low sum word of 2^64 - 1 under a high word of 3, in every bucket."""
    return [7] * (n_buckets + 1), [(3 << 64) | M64] * (n_buckets + 1)


def named_cases():
    """name -> case: what tests/test_groupby_reference.py proves the restatement and the wrong models on, and
    tests/test_gpu_bsi_group_by.py runs on the device."""
    cases = {}
    i = 0
    for ks in KEY_WIDTHS:  # every pair of widths at 31 words
        for vs in VALUE_WIDTHS:
            cases[f"widths {ks} x {vs}"] = make_case(31, ks, vs, FILTER_COUNTS[i % 3], i % 2 == 1)
            i += 1
    for n in SIZES:  # every size with every number of filters, with and without an existence row
        for j, n_filters in enumerate(FILTER_COUNTS):
            for with_exists in (False, True):
                ks, vs = KEY_WIDTHS[(j + with_exists) % 5], VALUE_WIDTHS[(j + 2 * with_exists + (n > 31)) % 4]
                cases[f"size {n}: {n_filters} filters{' exists' if with_exists else ''}"] = make_case(n, ks, vs, n_filters, with_exists, seed=1)
    edges = (32 * BIG, 32 * BIG - 1, 31 * 1000 - 1, 31 * 1000, 31 * 1000 + 1, SEG_BITS - 1, SEG_BITS, SEG_BITS + 1, 2 * SEG_BITS + HALF_ROWS, 1, 0)
    for n_rows in edges:  # on and beside a group and a segment edge
        cases[f"n_rows {n_rows}"] = make_case(BIG, 8, 17, 1, False, n_rows=n_rows, seed=2)
        cases[f"n_rows {n_rows} count only"] = make_case(BIG, 11, 0, 0, n_rows % 2 == 0, n_rows=n_rows, n_buckets=LDS_BUCKETS, seed=2)
    for nb in (1, LDS_BUCKETS - 1, LDS_BUCKETS):  # the LDS route's last bucket count, the global route's first
        for vs in (0, 17):
            cases[f"buckets {nb} x {vs}"] = make_case(SEG_WORDS + 5, 11, vs, 1, True, n_buckets=nb, seed=3)
    cases["buckets 4096 under a 32-slice key"] = make_case(SEG_WORDS + 5, 32, 32, 1, True, n_buckets=1 << 12, seed=3)
    for pattern in ("one key", "alternating", "sorted"):
        for nb in (256, 1 << 12):
            cases[f"pattern {pattern} x {nb}"] = make_case(SEG_WORDS + 5, 12, 32, 0, False, n_buckets=nb, pattern=pattern, seed=4)
    rng = np.random.default_rng(5)
    full = rng.integers(0, 300, 1 << 12).astype(np.uint32)
    full[rng.random(full.size) < 0.2] = DROP
    full[7], full[8], full[9] = 256, 257, 299  # at and above n_buckets
    cases["map: drops and entries at and above n_buckets"] = make_case(SEG_WORDS + 5, 12, 17, 1, True, n_buckets=256, lookup=full, seed=5)
    cases["map: n_keys below the domain"] = make_case(SEG_WORDS + 5, 12, 17, 0, False, n_buckets=300, lookup=full[:1000], seed=5)
    cases["map: one key"] = make_case(31, 8, 0, 0, False, n_buckets=3, lookup=np.array([2], np.uint32), seed=5)
    cases["map: global route"] = make_case(SEG_WORDS + 5, 12, 32, 1, False, n_buckets=1 << 12,
                                           lookup=rng.integers(0, (1 << 12) + 9, 3000).astype(np.uint32), seed=5)
    for nb, name in ((64, "lds"), (1 << 12, "global")):  # a prefilled low sum word of 2^64 - 1 carries
        cases[f"carry {name}"] = make_case(SEG_WORDS + 5, 12, 32, 1, False, n_buckets=nb, prefill=carry_prefill(nb), seed=6)
    return cases


def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.choice([1, 5, 31, 40, SEG_WORDS, SEG_WORDS + 3]))
    ks, vs = int(rng.integers(1, 33)), int(rng.choice([0, 0, 1, 9, 32]))
    lookup = None
    if rng.random() < 0.5:
        lookup = rng.integers(0, 40, int(rng.integers(1, 300))).astype(np.uint32)
        lookup[rng.random(lookup.size) < 0.2] = DROP
    nb = int(rng.choice([1, 2, 33, LDS_BUCKETS - 1, LDS_BUCKETS, 5000]))
    return make_case(n, ks, vs, int(rng.integers(0, 4)), bool(rng.random() < 0.5), n_rows=int(rng.integers(0, 32 * n + 1)), n_buckets=nb, lookup=lookup,
                     seed=seed, prefill=carry_prefill(nb) if rng.random() < 0.3 else None)


# the named case on which a wrong model has to change the answer
CAUGHT_BY = {
    "rows behind n_rows counted": f"n_rows {32 * BIG - 1} count only",  # (no filter, no existence row: the last row is selected)
    "other dropped": "buckets 1 x 17",
    "map read behind n_keys": "map: n_keys below the domain",
    "last run of a lane lost": "pattern one key x 256",
    "carry dropped": "carry global",
    "both halves count the whole segment": "widths 8 x 17",
    "existence ignored under a filter": "size 992: 1 filters exists",
}
