"""Shared helpers of the partitioned running-sum tests (wah_bsi_cumsum_parts_indexed_device, include/wah.h).  As tests/_cumsum.py
does for the plain call, the call is stated three times:
  (a) values_of / expected: a numpy model that answers from the VALUES, the unpacked bitmaps and the STARTS, in uint64 with an
      explicit mod;
  (b) compressed (tests/_cumsum.py's): that model's slice matrix through the oracle's compress(), with its segment index;
  (c) kernel: the steps of csrc/wah_cumsum.hip's partitioned kernels restated from the SLICES -- per segment whether it holds a start
      and the weighted popcounts of its TAIL, the segmented scan of those records in rounds of 8192 with a pair as the carry, block
      pairs and their fold, steps of 64 rows without a head (the plain step) and with heads (the scan minus its exclusive value at
      the lane's own head lane) --
and WRONG names seven wrong models of (c), each with one error.

A case is a case of tests/_cumsum.py with one more entry: starts, a bool array of 32 n rows."""
import numpy as np

from tests import _bsi, _cumsum as cs

SEG_WORDS, SEG_BITS = cs.SEG_WORDS, cs.SEG_BITS
BLOCK_ROWS, BLOCK_WORDS, BLOCKS, HALF_START = cs.BLOCK_ROWS, cs.BLOCK_WORDS, cs.BLOCKS, cs.HALF_START
SCAN_ROUND = 8192  # entries of one round of the scan kernel
M64 = (1 << 64) - 1
TOP32 = cs.TOP32
WRONG = ("a start at an unselected row is ignored", "the incoming base is added behind a start inside the segment",
         "a segment without a start drops what came into the segment in front", "an exclusive start row shows the previous partition's total",
         "the head lane is off by one at lane 0", "with two heads in a step every lane uses the first",
         "a block's tail is taken from its first start")

rows_out = cs.rows_out
compressed = cs.compressed


# ---- (a) the value model -------------------------------------------------------------------------------------------------------------
def effective_starts(case):
    return case["starts"] & (np.arange(32 * case["n"]) < case["n_rows"])


def values_of(case):
    """(running values uint64 mod 2^k_out, selection bool): from the values, the unpacked bitmaps and the starts."""
    rows = 32 * case["n"]
    sel = cs.selection(case)
    x = np.where(sel, case["values"] if case["kv"] else np.uint64(1), np.uint64(0)).astype(np.uint64)
    run = np.cumsum(x, dtype=np.uint64)  # (mod 2^64)
    st = effective_starts(case)
    last = np.maximum.accumulate(np.where(st, np.arange(rows), 0))  # s(p), 0 where there is none
    front = np.where(np.cumsum(st) > 0, (run - x)[last], np.uint64(0))  # the sum in front of s(p)
    run = run - front
    if case["exclusive"]:
        run = run - x
    keep = (np.arange(rows) < case["n_rows"]) if case["all_rows"] else sel
    mask = np.uint64((1 << case["k_out"]) - 1)  # the explicit mod
    return np.where(keep, run, np.uint64(0)) & mask, sel


def expected(case):
    values, sel = values_of(case)
    return _bsi.build_slices(values, case["k_out"], None if case["all_rows"] else sel)


# ---- (c) the kernels' steps ----------------------------------------------------------------------------------------------------------
def _fold(x, y):
    """(has_start, sum) pairs, x in front of y."""
    return (x[0] | y[0], y[1] if y[0] else (x[1] + y[1]) & M64)


def scan_records(records, wrong=None):
    """The scan kernel: what flows into every segment, in rounds of SCAN_ROUND entries with a pair as the carry."""
    incoming, carry = [], (False, 0)
    for i0 in range(0, len(records), SCAN_ROUND):
        run = carry
        for rec in records[i0: i0 + SCAN_ROUND]:
            incoming.append(run[1])
            run = (run[0] | rec[0], rec[1]) if wrong == WRONG[2] and not rec[0] else _fold(run, rec)
        carry = run
    return incoming


def kernel(case, wrong=None):
    n, kv, k_out = case["n"], case["kv"], case["k_out"]
    assert n % SEG_WORDS == 0
    rows, segs = 32 * n, n // SEG_WORDS
    slices = _bsi.build_slices(case["values"], kv, case["exists"], zero_missing=True) if kv else None
    image = np.arange(rows) < case["n_rows"]
    if case["exists"] is not None:
        image = image & (_bsi.unpack_bits(slices[kv]) if kv else case["exists"])
    for f in case["filters"]:
        image = image & f
    st = _bsi.unpack_bits(_bsi.pack_bits(case["starts"])) & (np.arange(rows) < case["n_rows"])  # the starts image, clipped
    if wrong == WRONG[0]:
        st = st & image
    # first launch: a record per segment
    records = []
    for seg in range(segs):
        lo, hi, w = seg * SEG_BITS, (seg + 1) * SEG_BITS, slice(seg * SEG_WORDS, (seg + 1) * SEG_WORDS)
        at = np.flatnonzero(st[lo:hi])
        tail = image[lo:hi].copy()
        if at.size:
            tail[: at[-1]] = False  # "rows at or behind the last start" ANDed into the selection
        tail_words = _bsi.pack_bits(tail)
        if kv:
            total = sum(cs._popcount(slices[i][w] & tail_words) << (kv - 1 - i) for i in range(kv))
        else:
            total = cs._popcount(tail_words)
        records.append((bool(at.size), total & M64))
    incoming = scan_records(records, wrong)
    # third launch: the rows
    if kv:
        words = np.zeros(rows, np.uint64)
        for i in range(kv):
            words |= _bsi.unpack_bits(slices[i]).astype(np.uint64) << np.uint64(kv - 1 - i)
    else:
        words = np.ones(rows, np.uint64)
    x_all = np.where(image, words, np.uint64(0))
    mask = np.uint64((1 << k_out) - 1)
    matrix = np.zeros((rows_out(case), n), np.uint32)
    lanes = np.arange(64)
    for seg in range(segs):
        blocks = []
        for blk in range(BLOCKS):
            steps = 16 if blk == BLOCKS - 1 else 32
            r = seg * SEG_BITS + blk * BLOCK_ROWS + np.arange(64 * steps)
            inside = r < rows
            rr = np.minimum(r, rows - 1)
            x = np.where(inside, x_all[rr], np.uint64(0))
            heads = st[rr] & inside
            on = image[rr] & inside
            at = np.flatnonzero(heads)
            first = 0 if not at.size else int(at[0] if wrong == WRONG[6] else at[-1])
            blocks.append(dict(steps=steps, r=r, x=x.reshape(steps, 64), heads=heads.reshape(steps, 64), on=on.reshape(steps, 64),
                               pair=(bool(at.size), int(x[first:].sum(dtype=np.uint64)))))
        for blk, b in enumerate(blocks):
            base = (False, incoming[seg])
            for front in blocks[:blk]:
                base = _fold(base, front["pair"])
            carry = base[1]
            if wrong == WRONG[1] and base[0]:
                carry = (carry + incoming[seg]) & M64
            steps, x = b["steps"], b["x"]
            run = np.zeros((steps, 64), np.uint64)
            for t in range(steps):
                s = np.cumsum(x[t], dtype=np.uint64)  # the wave scan
                own = x[t] if case["exclusive"] else np.uint64(0)
                hm = b["heads"][t]
                if not hm.any():  # the plain step
                    run[t] = np.uint64(carry) + s - own
                    carry = (carry + int(s[63])) & M64
                    continue
                e = s - x[t]  # the exclusive scan
                head_at = np.where(hm, lanes, -1)
                hl = np.maximum.accumulate(head_at)  # the last head at or in front of the lane, -1: none
                if wrong == WRONG[3] and case["exclusive"]:  # ... strictly in front of it
                    hl = np.concatenate([[-1], hl[:-1]])
                if wrong == WRONG[4]:
                    hl = np.where(hl == 0, -1, hl)
                if wrong == WRONG[5]:
                    hl = np.where(hl >= 0, int(np.flatnonzero(hm)[0]), -1)
                run[t] = np.where(hl >= 0, s - e[np.maximum(hl, 0)], np.uint64(carry) + s) - own
                carry = int(s[63] - e[int(np.flatnonzero(hm)[-1])])
            keep = (b["on"] | case["all_rows"]) & (b["r"] < case["n_rows"]).reshape(steps, 64)
            run = (np.where(keep, run, np.uint64(0)) & mask).reshape(-1)
            first = seg * SEG_WORDS + blk * BLOCK_WORDS
            for i in range(rows_out(case)):
                bits = ((run >> np.uint64(k_out - 1 - i)) & np.uint64(1)).astype(bool) if i < k_out else b["on"].reshape(-1)
                matrix[i, first: first + 2 * steps] = _bsi.pack_bits(bits)
    return matrix


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def make_case(n, kv, k_out, starts, **kw):
    """tests/_cumsum.py's make_case and the starts: a bool array, a list of rows, or a density."""
    case = cs.make_case(n, kv, k_out, **kw)
    rows = 32 * n
    if isinstance(starts, float):
        starts = np.random.default_rng(int(1e6 * starts) + n + kv + 64 * k_out).random(rows) < starts
    elif not (isinstance(starts, np.ndarray) and starts.dtype == bool):
        at = np.asarray(starts, dtype=np.int64)
        starts = np.zeros(rows, bool)
        starts[at] = True
    case["starts"] = starts
    return case


SIZES = cs.SIZES
BIG = cs.BIG
VAL_WIDTHS, OUT_WIDTHS = (0, 1, 26, 27, 32), (1, 32, 33, 64)
MODES = cs.MODES
SEAMS = (63, 64, 65, 2047, 2048, 16383, 16384, HALF_START, SEG_BITS - 1, SEG_BITS)


def named_cases():
    """name -> case: what tests/test_cumsum_parts_reference.py proves the statements and the wrong models on, and
    tests/test_gpu_bsi_cumsum_parts.py runs on the device."""
    cases = {}
    rows = 32 * BIG
    # where the starts are
    for i, n in enumerate(SIZES):
        exclusive, all_rows = MODES[i % 4]
        cases[f"a start at row 0 only, {i + 1} segments"] = make_case(n, 7, 24, [0], n_filters=i % 2, exclusive=exclusive, all_rows=all_rows, seed=11)
        cases[f"no start, {i + 1} segments"] = make_case(n, 7, 24, [], n_filters=1, exclusive=all_rows, all_rows=exclusive, seed=12)
        cases[f"every row a start, {i + 1} segments"] = make_case(n, 9, 12, np.ones(32 * n, bool), n_filters=i % 2, exclusive=i == 1, all_rows=i == 2, seed=13)
    for exclusive, all_rows in MODES:
        tail = f"{' exclusive' if exclusive else ''}{' all_rows' if all_rows else ''}"
        cases[f"starts at the seams{tail}"] = make_case(BIG, 7, 24, SEAMS + tuple(SEG_BITS + r for r in SEAMS), n_filters=1, exclusive=exclusive,
                                                          all_rows=all_rows, seed=14)
        cases[f"each seam alone{tail}"] = make_case(BIG, 0, 16, SEAMS[::2] if exclusive else SEAMS[1::2], exclusive=exclusive, all_rows=all_rows,
                                                      filters=[np.ones(rows, bool)])
        two = [64 * 5, 64 * 5 + 63, 64 * 40 + 1, 64 * 40 + 2, SEG_BITS + 64 * 9, SEG_BITS + 64 * 9 + 63]
        three = [64 * 7, 64 * 7 + 17, 64 * 7 + 63, HALF_START + 64 * 3, HALF_START + 64 * 3 + 30, HALF_START + 64 * 3 + 31]
        cases[f"two starts in a step{tail}"] = make_case(2 * SEG_WORDS, 7, 24, two, n_filters=1, exclusive=exclusive, all_rows=all_rows, seed=15)
        cases[f"three starts in a step{tail}"] = make_case(2 * SEG_WORDS, 27, 40, three, exclusive=exclusive, all_rows=all_rows, seed=15)
        middle = np.ones(rows, bool)
        middle[SEG_BITS: 2 * SEG_BITS] = False
        cases[f"a start in segment 0, segment 1 empty{tail}"] = make_case(BIG, 9, 30, [100], exclusive=exclusive, all_rows=all_rows, filters=[middle], seed=16)
        cases[f"a start in segment 1 only{tail}"] = make_case(BIG, 9, 30, [SEG_BITS + 5000], n_filters=1, exclusive=exclusive, all_rows=all_rows, seed=17)
        f = np.random.default_rng(18).random(rows) < 0.5
        at = np.flatnonzero(~f)[:: 97]
        cases[f"starts at unselected rows{tail}"] = make_case(BIG, 7, 24, at, exclusive=exclusive, all_rows=all_rows, filters=[f], seed=18)
        n_rows = SEG_BITS + 4000
        cases[f"starts at and behind n_rows{tail}"] = make_case(BIG, 7, 24, [3000, n_rows - 1, n_rows, n_rows + 1, n_rows + 64, 2 * SEG_BITS + 9], n_rows=n_rows,
                                                                  n_filters=1, exclusive=exclusive, all_rows=all_rows, seed=19)
    # widths: every pair, the sizes, the modes, an existence row, a filter and the density of the starts in turn
    i = 0
    for kv in VAL_WIDTHS:
        for k_out in OUT_WIDTHS:
            exclusive, all_rows = MODES[i % 4]
            cases[f"widths {kv} x {k_out}"] = make_case(SIZES[i % 3], kv, k_out, (1 / 16, 1 / 700, 1 / 9000)[(i // 2) % 3], with_exists=i % 2 == 1,
                                                        n_filters=(i // 2) % 2 if kv else 1, exclusive=exclusive, all_rows=all_rows)
            i += 1
    # partition sums that leave 32 bits
    ones = np.full(rows, TOP32, np.uint64)
    far = list(range(777, rows, 20011))
    cases["partition sums past 2^32"] = make_case(BIG, 32, 48, far, values=ones)
    cases["partition sums past 2^32 exclusive all_rows"] = make_case(BIG, 32, 48, far, exclusive=True, all_rows=True, values=ones)
    cases["partition sums past 2^32 truncated"] = make_case(BIG, 32, 33, far, values=ones, n_filters=1)
    for with_exists in (False, True):
        for exclusive, all_rows in MODES:
            name = f"flags{' exists' if with_exists else ''}{' exclusive' if exclusive else ''}{' all_rows' if all_rows else ''}"
            cases[name] = make_case(2 * SEG_WORDS, 7, 23, 1 / 300, n_rows=2 * SEG_BITS - 777, with_exists=with_exists, n_filters=1, exclusive=exclusive,
                                    all_rows=all_rows, seed=3)
    for n_filters in (0, 1, cs.MAX_FILTERS):
        cases[f"filters {n_filters}"] = make_case(2 * SEG_WORDS, 12, 28, 1 / 1000, with_exists=True, n_filters=n_filters, seed=4)
    cases["count under 64 filters"] = make_case(2 * SEG_WORDS, 0, 16, 1 / 50, n_filters=cs.MAX_FILTERS, exclusive=True, all_rows=True, seed=4)
    return cases


def random_case(seed):
    rng = np.random.default_rng(seed)
    case = cs.random_case(seed)
    case["starts"] = rng.random(32 * case["n"]) < float(rng.choice([0.0, 1 / 20000, 1 / 300, 1 / 8, 1.0]))
    return case


# ---- long bitmaps: expected from tests/_long.py's run model ------------------------------------------------------------------------------
def long_expected(oracle, filt, starts, n_rows, empty=None, put=None):
    """The call's result for bitmaps too long to exist decoded (tests/_long.py: LongBitmap): a filter of constant ones with a few live
    segments, starts of constant zeros with a few live segments, no value slices, a 2-bit result and all_rows -- every row in front
    of n_rows holds the number of selected rows since its partition's start mod 4.  A segment of ones adds 31 744, a multiple of 4,
    so between two live segments every constant segment of a result slice is the same 1024 literals, given by the count mod 4 that
    flows into it; a segment at or behind n_rows is one zero fill.  The live segments -- the filter's and those that hold a start --
    are computed row by row.  empty(total) makes the int32 output and put(words) moves numpy words to where it lives (defaults:
    numpy).  Returns (stream int32, index int64, what flows into every segment)."""
    from tests import _long as lg

    empty = empty or (lambda total: np.empty(total, np.int32))
    put = put or (lambda words: words)
    a = filt.n_segments
    assert starts.n_segments == a and SEG_BITS % 4 == 0 and set(filt.defaults().tolist()) == {1} and not starts.defaults().any()
    live = sorted(set(filt.live) | set(starts.live))
    cut = n_rows // SEG_BITS
    assert cut in live or n_rows % SEG_BITS == 0
    incoming = np.zeros(a + 1, np.int64)
    words, run, prev = {}, 0, 0
    for s in live + [a]:
        incoming[prev: s + 1] = run + SEG_BITS * np.arange(s + 1 - prev)  # constant segments of ones
        if s == a:
            break
        row = s * SEG_BITS + np.arange(SEG_BITS)
        bits = filt.seg_bits(s).astype(np.int64) * (row < n_rows)
        st = starts.seg_bits(s).astype(bool) & (row < n_rows)
        total = np.cumsum(bits)
        last = np.maximum.accumulate(np.where(st, np.arange(SEG_BITS), 0))
        value = total - np.where(np.cumsum(st) > 0, (total - bits)[last], -int(incoming[s]))
        run = int(value[-1])
        value = np.where(row < n_rows, value & 3, 0)
        words[s] = [np.asarray(oracle.compress(_bsi.pack_bits(((value >> b) & 1).astype(bool))), dtype=np.uint32).view(np.int32) for b in (1, 0)]
        prev = s + 1
    phase_words = {p: [put(np.asarray(oracle.compress(_bsi.pack_bits((((p + 1 + np.arange(SEG_BITS)) >> b) & 1).astype(bool))), dtype=np.uint32).view(np.int32))
                       for b in (1, 0)] for p in range(4)}
    assert all(w.shape[0] == 1024 for ws in phase_words.values() for w in ws)
    lengths = np.where(np.arange(a) < cut, 1024, 1).astype(np.int64)
    lengths = np.stack([lengths, lengths.copy()])
    for s, pair in words.items():
        lengths[0, s], lengths[1, s] = pair[0].size, pair[1].size
    index = np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64)
    want = empty(int(index[-1]))
    zero_fill = int(np.array([lg.FILL | lg.SEG_GROUPS], np.uint32).view(np.int32)[0])
    for j in range(2):
        first = 0
        for s in live + [a]:  # the constant segments [first, s) -- all in front of the cut or all behind it -- then the live segment s
            if s > first:
                lo, hi = int(index[j * a + first]), int(index[j * a + s])
                if first < cut:
                    want[lo:hi].reshape(-1, 1024)[:] = phase_words[int(incoming[first]) & 3][j]
                else:
                    want[lo:hi] = zero_fill
            if s < a:
                at = int(index[j * a + s])
                want[at: at + words[s][j].size] = put(words[s][j])
            first = s + 1
    return want, index, incoming


# the named case on which a wrong model has to change the answer
CAUGHT_BY = {
    WRONG[0]: "starts at unselected rows",
    WRONG[1]: "starts at the seams",
    WRONG[2]: "a start in segment 0, segment 1 empty",
    WRONG[3]: "two starts in a step exclusive",
    WRONG[4]: "two starts in a step",
    WRONG[5]: "three starts in a step",
    WRONG[6]: "three starts in a step",
}
