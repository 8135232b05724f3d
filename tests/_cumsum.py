"""Shared helpers of the running-sum tests (wah_bsi_cumsum_indexed_device, include/wah.h).  The call is stated three times:
  (a) values_of / expected: a numpy model that answers from the VALUES, the existence bitmap and the filters as unpacked bits, in
      uint64 with an explicit mod, so that sums beyond 2^63 stay exact;
  (b) compressed: that model's slice matrix through the oracle's compress(), with the segment index the call has to leave;
  (c) kernel: the steps of csrc/wah_cumsum.hip restated from the SLICES -- segment totals by weighted popcounts, their exclusive
      scan, block totals, the step scan with its carry, exclusive / all-rows / the clip at n_rows --
and WRONG names seven wrong models of (c), each with one error.  A bitmap of n words has 32 * n rows, row p at word p // 32, bit
p % 32; values are numpy uint64.

A case is a dict: n (words, a multiple of 992), n_rows, kv (value slices, 0: every selected row counts 1), values (uint64 [32 n]),
exists (the value's existence bitmap or None), filters (a list of bool arrays), k_out (result slices), exclusive and all_rows.  An
answer is the result's decoded slice matrix [k_out (+ 1 without all_rows), n], most significant slice first, the selection last."""
import numpy as np

from tests import _bsi

SEG_WORDS, SEG_GROUPS, SEG_BITS = 992, 1024, 31 * 1024
BLOCK_ROWS, BLOCK_WORDS, BLOCKS = 2048, 64, 16  # a segment: fifteen blocks and a half one
HALF_START = 15 * BLOCK_ROWS                     # 30 720: the half block's first row
GRID_ITEMS = 512                                 # kCumsumGridItems of wah_cumsum.hip: workgroups at the most
MAX_FILTERS = 64                                 # WAH_GROUP_MAX_FILTERS
TOP32 = (1 << 32) - 1
WRONG = ("carry between steps dropped", "block totals in wavefront order", "half block counted as a whole one", "segment base in 32 bits",
         "exclusive taken as inclusive at a segment's first row", "unselected rows not carried under all_rows",
         "rows at or behind n_rows not cleared")


def rows_out(case):
    return case["k_out"] + (0 if case["all_rows"] else 1)


def size_bound(n_bits_val, n_rows):
    """The width no running sum of n_rows values of n_bits_val bits passes: what columns.cumsum_column defaults to (a count: 0 bits)."""
    return min(64, n_bits_val + int(n_rows).bit_length())


# ---- (a) the value model -------------------------------------------------------------------------------------------------------------
def selection(case):
    rows = 32 * case["n"]
    sel = np.arange(rows) < case["n_rows"]
    if case["exists"] is not None:
        sel &= case["exists"]
    for f in case["filters"]:
        sel &= f
    return sel


def values_of(case):
    """(running values uint64 mod 2^k_out, selection bool): from the values and the unpacked bitmaps, never from slices."""
    rows = 32 * case["n"]
    sel = selection(case)
    x = np.where(sel, case["values"] if case["kv"] else np.uint64(1), np.uint64(0)).astype(np.uint64)
    run = np.cumsum(x, dtype=np.uint64)  # (mod 2^64: the sum is carried in 64 bits)
    if case["exclusive"]:
        run = run - x
    keep = (np.arange(rows) < case["n_rows"]) if case["all_rows"] else sel
    mask = np.uint64((1 << case["k_out"]) - 1)  # the explicit mod
    return np.where(keep, run, np.uint64(0)) & mask, sel


def expected(case):
    """The model's slice matrix."""
    values, sel = values_of(case)
    return _bsi.build_slices(values, case["k_out"], None if case["all_rows"] else sel)


# ---- (b) the compressed matrix -------------------------------------------------------------------------------------------------------
def compressed(oracle, matrix):
    """(stream, index): compress() of the matrix as ONE bitmap and the first word of every one of its segments, then the count --
    what the call leaves in d_out and d_out_offsets.  A fill never crosses a segment, so the stream is the segments' own streams
    back to back."""
    flat = np.ascontiguousarray(matrix.reshape(-1), dtype=np.uint32)
    parts = [np.asarray(oracle.compress(flat[i: i + SEG_WORDS]), dtype=np.uint32) for i in range(0, flat.size, SEG_WORDS)]
    stream = np.asarray(oracle.compress(flat), dtype=np.uint32)
    assert np.array_equal(np.concatenate(parts), stream)
    return stream, np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)


# ---- (c) the kernel's steps ------------------------------------------------------------------------------------------------------------
def _popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8)).sum())


def kernel(case, wrong=None):
    """wah_cumsum.hip restated.  First launch: per segment the selection image (all ones clipped to n_rows, ANDed with the existence
    row and the filters) and the total, the sum over the slices of popcount(slice AND selection) << significance.  Second: the
    exclusive scan of the totals, mod 2^64.  Third: the value words folded out of the slices, fifteen blocks of 2048 rows and the
    half block of 1024, lane l of step t owning row 2048 blk + 64 t + l; the block totals; per block the base is the segment's plus
    the totals of the blocks in front; per step an inclusive scan of the 64 lanes plus the carry of the steps in front; minus the
    row's own value when exclusive; zero for an unselected row unless all_rows and for a row at or behind n_rows; the result
    slices most significant first, then the ballots of the selection."""
    n, kv, k_out = case["n"], case["kv"], case["k_out"]
    assert n % SEG_WORDS == 0
    rows, segs = 32 * n, n // SEG_WORDS
    slices = _bsi.build_slices(case["values"], kv, case["exists"], zero_missing=True) if kv else None
    image = np.arange(rows) < case["n_rows"]
    if case["exists"] is not None:
        image = image & (_bsi.unpack_bits(slices[kv]) if kv else case["exists"])
    for f in case["filters"]:
        image = image & f
    sel_words = _bsi.pack_bits(image)
    # the totals: no per-row fold
    totals = []
    for seg in range(segs):
        w = slice(seg * SEG_WORDS, (seg + 1) * SEG_WORDS)
        if kv:
            totals.append(sum(_popcount(slices[i][w] & sel_words[w]) << (kv - 1 - i) for i in range(kv)))
        else:
            totals.append(_popcount(sel_words[w]))
    bases, run = [], 0
    for t in totals:
        bases.append(run & TOP32 if wrong == WRONG[3] else run)
        run = (run + t) & ((1 << 64) - 1)
    # the rows
    if kv:
        words = np.zeros(rows, np.uint64)
        for i in range(kv):  # the fold: slice i lands at bit kv - 1 - i of the row's word
            words |= _bsi.unpack_bits(slices[i]).astype(np.uint64) << np.uint64(kv - 1 - i)
    else:
        words = np.ones(rows, np.uint64)
    x_all = np.where(image, words, np.uint64(0))
    clip = rows if wrong == WRONG[6] else case["n_rows"]
    mask = np.uint64((1 << k_out) - 1)
    matrix = np.zeros((rows_out(case), n), np.uint32)
    late = []  # the stores of a half block that is not cut: they land last
    order = [b for w in range(8) for b in (w, w + 8)] if wrong == WRONG[1] else list(range(BLOCKS))
    for seg in range(segs):
        block_totals = []
        for blk in range(BLOCKS):
            steps = 16 if blk == BLOCKS - 1 and wrong != WRONG[2] else 32
            r = seg * SEG_BITS + blk * BLOCK_ROWS + np.arange(64 * steps)
            block_totals.append(int(x_all[np.minimum(r, rows - 1)][r < (seg + 1) * SEG_BITS].sum(dtype=np.uint64)))
        for blk in range(BLOCKS):
            half = blk == BLOCKS - 1
            steps = 16 if half and wrong != WRONG[2] else 32
            r = seg * SEG_BITS + blk * BLOCK_ROWS + np.arange(64 * steps)  # step t, lane l: 64 t + l
            inside = r < (seg + 1) * SEG_BITS                               # (steps that do not exist hold nothing)
            rr = np.minimum(r, rows - 1)
            x = np.where(inside, x_all[rr], np.uint64(0)).reshape(steps, 64)
            on = (image[rr] & inside).reshape(steps, 64)
            base = (bases[seg] + sum(block_totals[b] for b in order[: order.index(blk)])) & ((1 << 64) - 1)
            scan = np.cumsum(x, axis=1, dtype=np.uint64)           # the wave scan of a step
            step_totals = scan[:, 63]
            carry = np.uint64(base) + (np.cumsum(step_totals, dtype=np.uint64) - step_totals)  # the steps in front
            if wrong == WRONG[0]:
                carry = np.full(steps, base, np.uint64)
            run = carry[:, None] + scan
            if case["exclusive"]:
                own = x.copy()
                if wrong == WRONG[4] and blk == 0:
                    own[0, 0] = 0  # the segment's first row
                run = run - own
            keep = on | (case["all_rows"] and wrong != WRONG[5])
            keep = keep & (r < clip).reshape(steps, 64)
            run = (np.where(keep, run, np.uint64(0)) & mask).reshape(-1)
            first = seg * SEG_WORDS + blk * BLOCK_WORDS
            for i in range(rows_out(case)):
                ballots = _bsi.pack_bits(((run >> np.uint64(k_out - 1 - i)) & np.uint64(1)).astype(bool)) if i < k_out else _bsi.pack_bits(on.reshape(-1))
                if half and steps == 32:
                    late.append((i, first, ballots))
                else:
                    matrix[i, first: first + 2 * steps] = ballots
    for i, first, ballots in late:
        end = min(first + 64, n)
        matrix[i, first:end] = ballots[: end - first]
    return matrix


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def make_case(n, kv, k_out, n_rows=None, with_exists=False, n_filters=0, exclusive=False, all_rows=False, seed=0, values=None, filters=None):
    rng = np.random.default_rng(7919 * kv + 104729 * k_out + n + 31 * n_filters + seed)
    rows = 32 * n
    if values is None:
        values = _bsi.uniform_values(rng, rows, kv) if kv else np.zeros(rows, np.uint64)
    exists = rng.random(rows) < 0.9 if with_exists else None
    if filters is None:  # together they keep about one half of the rows
        keep = 0.5 ** (1.0 / n_filters) if n_filters else 1.0
        filters = [rng.random(rows) < keep for _ in range(n_filters)]
    return dict(n=n, n_rows=rows if n_rows is None else n_rows, kv=kv, values=np.ascontiguousarray(values, dtype=np.uint64), exists=exists,
                filters=list(filters), k_out=k_out, exclusive=exclusive, all_rows=all_rows)


SIZES = (SEG_WORDS, 2 * SEG_WORDS, 3 * SEG_WORDS)
VAL_WIDTHS, OUT_WIDTHS = (0, 1, 7, 32), (1, 32, 33, 64)
MODES = ((False, False), (True, False), (False, True), (True, True))  # (exclusive, all_rows)
BIG = 3 * SEG_WORDS
ROW_EDGES = (63, 64, 65, 31, 32, 33, 2047, 2048, 2049, HALF_START - 1, HALF_START, HALF_START + 1, SEG_BITS - 1, SEG_BITS, SEG_BITS + 1, 2 * SEG_BITS)


def _rows(n, at):
    f = np.zeros(32 * n, bool)
    f[np.asarray(at, dtype=np.int64)] = True
    return f


def named_cases():
    """name -> case: what tests/test_cumsum_reference.py proves the three statements and the wrong models on, and
    tests/test_gpu_bsi_cumsum.py runs on the device."""
    cases = {}
    i = 0
    for kv in VAL_WIDTHS:  # every pair of widths; the sizes, the modes, an existence row and a filter in turn
        for k_out in OUT_WIDTHS:
            exclusive, all_rows = MODES[i % 4]
            cases[f"widths {kv} x {k_out}"] = make_case(SIZES[i % 3], kv, k_out, None, i % 2 == 1, (i // 2) % 2 if kv else 1, exclusive, all_rows)  # (a count has a filter)
            i += 1
    for j, n_rows in enumerate(ROW_EDGES):
        exclusive, all_rows = MODES[j % 4]
        cases[f"n_rows {n_rows}"] = make_case(BIG, 7, 24, n_rows, j % 3 == 0, j % 2, exclusive, all_rows, seed=2)
    for with_exists in (False, True):
        for exclusive, all_rows in MODES:
            name = f"flags{' exists' if with_exists else ''}{' exclusive' if exclusive else ''}{' all_rows' if all_rows else ''}"
            cases[name] = make_case(2 * SEG_WORDS, 7, 23, 2 * SEG_BITS - 777, with_exists, 1, exclusive, all_rows, seed=3)
    for n_filters in (0, 1, MAX_FILTERS):
        cases[f"filters {n_filters}"] = make_case(2 * SEG_WORDS, 12, 28, None, True, n_filters, seed=4)
    cases["count under 64 filters"] = make_case(2 * SEG_WORDS, 0, 16, None, False, MAX_FILTERS, True, True, seed=4)
    # sums that leave 32 bits
    rows = 32 * BIG
    cases["all ones of 32 bits"] = make_case(BIG, 32, 48, values=np.full(rows, TOP32, np.uint64))
    cases["all ones of 32 bits exclusive"] = make_case(BIG, 32, 48, exclusive=True, all_rows=True, values=np.full(rows, TOP32, np.uint64))
    v = np.zeros(rows, np.uint64)
    v[5000], v[SEG_BITS], v[SEG_BITS + 1], v[2 * SEG_BITS + 70] = TOP32, 1, TOP32, 12345  # 2^32 is passed exactly at segment 1's first row
    cases["2^32 at a segment's first row"] = make_case(BIG, 32, 40, values=v)
    cases["2^32 at a segment's first row all_rows"] = make_case(BIG, 32, 40, all_rows=True, values=v)
    cases["truncated sum"] = make_case(2 * SEG_WORDS, 32, 33, None, True, 1, seed=5)  # the true sum needs 48 bits
    # selections
    for kv, what in ((9, "values"), (0, "count")):
        for exclusive, all_rows in ((False, False), (True, True)):
            tail = f"{what}{' exclusive all_rows' if all_rows else ''}"
            k_out = size_bound(kv, rows)
            cases[f"empty selection {tail}"] = make_case(BIG, kv, k_out, None, False, 0, exclusive, all_rows, 6, filters=[np.zeros(rows, bool)])
            cases[f"every row {tail}"] = make_case(BIG, kv, k_out, None, False, 0, exclusive, all_rows, 6, filters=[np.ones(rows, bool)])
            cases[f"each segment's last row {tail}"] = make_case(BIG, kv, k_out, None, False, 0, exclusive, all_rows, 6,
                                                                  filters=[_rows(BIG, [SEG_BITS - 1, 2 * SEG_BITS - 1, 3 * SEG_BITS - 1])])
            cases[f"alternating rows {tail}"] = make_case(BIG, kv, k_out, None, False, 0, exclusive, all_rows, 6, filters=[np.arange(rows) % 2 == 1])
            middle = np.ones(rows, bool)
            middle[SEG_BITS: 2 * SEG_BITS] = False
            cases[f"empty middle segment {tail}"] = make_case(BIG, kv, k_out, None, False, 0, exclusive, all_rows, 6, filters=[middle])
    return cases


def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.choice(SIZES[:2]))
    kv, k_out = int(rng.integers(0, 33)), int(rng.integers(1, 65))
    return make_case(n, kv, k_out, int(rng.integers(0, 32 * n + 1)), bool(rng.random() < 0.5), int(rng.integers(0, 4)), bool(rng.random() < 0.5),
                     bool(rng.random() < 0.5), seed=seed)


# the named case on which a wrong model has to change the answer
CAUGHT_BY = {
    WRONG[0]: "filters 0",
    WRONG[1]: "filters 0",
    WRONG[2]: "every row values",
    WRONG[3]: "all ones of 32 bits",
    WRONG[4]: "all ones of 32 bits exclusive",
    WRONG[5]: "each segment's last row count exclusive all_rows",
    WRONG[6]: "n_rows 65",
}
