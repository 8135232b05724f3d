"""Shared helpers of the partition-total tests (wah_bsi_total_parts_indexed_device, include/wah.h).  As tests/_cumsum_parts.py does
for the partitioned running sum, the call is stated three times:
  (a) values_of / expected: a numpy model that answers from the VALUES, the unpacked bitmaps and the STARTS, in uint64 with an
      explicit mod: partition id = cumsum(starts), the totals by np.add.at, broadcast back;
  (b) compressed (tests/_cumsum.py's): that model's slice matrix through the oracle's compress(), with its segment index;
  (c) kernel: the steps of csrc/wah_cumsum.hip's total_parts kernels restated from the SLICES -- per segment a record (has_start, head,
      tail) from weighted popcounts under two masks, both scans of the records in rounds of 8192 with a pair as the carry (the
      backward one from the end, its short round last), block triples and their folds in both directions, the forward pass of a
      block's steps (the partitioned call's inclusive step) and the backward pass with its wave-uniform `after` --
and WRONG names seven wrong models of (c), each with one error.

A case is a tests/_cumsum_parts.py make_case case with exclusive False."""
import numpy as np

from tests import _bsi, _cumsum as cs, _cumsum_parts as cp

SEG_WORDS, SEG_BITS = cs.SEG_WORDS, cs.SEG_BITS
BLOCK_ROWS, BLOCK_WORDS, BLOCKS, HALF_START = cs.BLOCK_ROWS, cs.BLOCK_WORDS, cs.BLOCKS, cs.HALF_START
SCAN_ROUND = cp.SCAN_ROUND
RECORD_BYTES = 24  # (head, tail, has_start): what include/wah.h states for the scratch
M64 = cp.M64
TOP32 = cs.TOP32
WRONG = ("the backward inflow is taken past a segment that holds a start", "a segment without a start drops what flows in from behind it",
         "a head at lane 0 takes the step's own r instead of the previous step's", "with two heads in a step every lane uses the last",
         "a block's head is taken up to its last start", "the backward carry of the short last round is lost",
         "an unselected start row is ignored")

rows_out = cs.rows_out
compressed = cs.compressed
effective_starts = cp.effective_starts


# ---- (a) the value model -------------------------------------------------------------------------------------------------------------
def values_of(case):
    """(totals uint64 mod 2^k_out, selection bool): from the values, the unpacked bitmaps and the starts."""
    assert not case["exclusive"]
    rows = 32 * case["n"]
    sel = cs.selection(case)
    x = np.where(sel, case["values"] if case["kv"] else np.uint64(1), np.uint64(0)).astype(np.uint64)
    part = np.cumsum(effective_starts(case))  # the partition of every row; the rows at and behind n_rows lie in the last one and add 0
    totals = np.zeros(int(part[-1]) + 1, np.uint64)
    np.add.at(totals, part, x)  # (mod 2^64)
    keep = (np.arange(rows) < case["n_rows"]) if case["all_rows"] else sel
    mask = np.uint64((1 << case["k_out"]) - 1)  # the explicit mod
    return np.where(keep, totals[part], np.uint64(0)) & mask, sel


def expected(case):
    values, sel = values_of(case)
    return _bsi.build_slices(values, case["k_out"], None if case["all_rows"] else sel)


# ---- (c) the kernels' steps ----------------------------------------------------------------------------------------------------------
def scan_records(records, wrong=None):
    """The scan kernel on records (has_start, head, tail): (what flows into every segment from the front, ... from behind).  Forward
    it is tests/_cumsum_parts.py's scan of (has_start, tail).  Backward entry k of a round is record n - 1 - k: the rounds start
    at the end and the short one is the last; a record in front of a run takes the run's sum and folds its own head over it."""
    n = len(records)
    forward = cp.scan_records([(f, t) for f, _, t in records])
    backward, carry = [0] * n, (False, 0)
    for k0 in range(0, n, SCAN_ROUND):
        run = carry
        if wrong == WRONG[5] and k0 > 0 and k0 + SCAN_ROUND > n:
            run = (False, 0)
        for k in range(k0, min(k0 + SCAN_ROUND, n)):
            f, h, _ = records[n - 1 - k]
            backward[n - 1 - k] = run[1]
            if wrong == WRONG[0]:
                run = (run[0] | f, (run[1] + h) & M64)
            elif wrong == WRONG[1] and not f:
                run = (run[0], h)
            else:
                run = cp._fold(run, (f, h))  # (the mirrored operator: the nearer item is the one folded last)
        carry = run
    return forward, backward


def kernel(case, wrong=None):
    n, kv, k_out = case["n"], case["kv"], case["k_out"]
    assert n % SEG_WORDS == 0 and not case["exclusive"]
    rows, segs = 32 * n, n // SEG_WORDS
    slices = _bsi.build_slices(case["values"], kv, case["exists"], zero_missing=True) if kv else None
    image = np.arange(rows) < case["n_rows"]
    if case["exists"] is not None:
        image = image & (_bsi.unpack_bits(slices[kv]) if kv else case["exists"])
    for f in case["filters"]:
        image = image & f
    st = _bsi.unpack_bits(_bsi.pack_bits(case["starts"])) & (np.arange(rows) < case["n_rows"])  # the starts image, clipped
    if wrong == WRONG[6]:
        st = st & image
    # first launch: a record per segment, every popcount under two masks
    records = []
    for seg in range(segs):
        lo, hi, w = seg * SEG_BITS, (seg + 1) * SEG_BITS, slice(seg * SEG_WORDS, (seg + 1) * SEG_WORDS)
        at = np.flatnonzero(st[lo:hi])
        head, tail = image[lo:hi].copy(), image[lo:hi].copy()
        if at.size:
            head[at[0]:] = False   # "rows in front of the first start"
            tail[: at[-1]] = False  # "rows at or behind the last start"
        sums = []
        for words in (_bsi.pack_bits(head), _bsi.pack_bits(tail)):
            if kv:
                sums.append(sum(cs._popcount(slices[i][w] & words) << (kv - 1 - i) for i in range(kv)) & M64)
            else:
                sums.append(cs._popcount(words))
        records.append((bool(at.size), sums[0], sums[1]))
    # second launch: both scans
    incoming, behind = scan_records(records, wrong)
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
            head_to = x.size if not at.size else int(at[-1] if wrong == WRONG[4] else at[0])
            tail_from = 0 if not at.size else int(at[-1])
            blocks.append(dict(steps=steps, r=r, x=x.reshape(steps, 64), heads=heads.reshape(steps, 64), on=on.reshape(steps, 64), f=bool(at.size),
                               head=int(x[:head_to].sum(dtype=np.uint64)), tail=int(x[tail_from:].sum(dtype=np.uint64))))
        for blk, b in enumerate(blocks):
            base = (False, incoming[seg])
            for front in blocks[:blk]:
                base = cp._fold(base, (front["f"], front["tail"]))
            back = behind[seg]
            for far in reversed(blocks[blk + 1:]):  # the heads of the blocks behind up to the first with a start
                back = far["head"] if far["f"] else (back + far["head"]) & M64
            steps, x = b["steps"], b["x"]
            # the forward pass: the segmented running sum of every row
            carry = base[1]
            run = np.zeros((steps, 64), np.uint64)
            for t in range(steps):
                s = np.cumsum(x[t], dtype=np.uint64)  # the wave scan
                hm = b["heads"][t]
                if not hm.any():  # the plain step
                    run[t] = np.uint64(carry) + s
                    carry = (carry + int(s[63])) & M64
                    continue
                e = s - x[t]  # the exclusive scan
                hl = np.maximum.accumulate(np.where(hm, lanes, -1))  # the last head at or in front of the lane, -1: none
                run[t] = np.where(hl >= 0, s - e[np.maximum(hl, 0)], np.uint64(carry) + s)
                carry = int(s[63] - e[int(np.flatnonzero(hm)[-1])])
            # the backward pass
            after = (carry + back) & M64  # (the carry is the running sum at the block's last row)
            total = np.zeros((steps, 64), np.uint64)
            for t in range(steps - 1, -1, -1):
                hm = b["heads"][t]
                if not hm.any():  # one select
                    total[t] = np.uint64(after)
                    continue
                at = np.flatnonzero(hm)
                nxt = np.minimum.accumulate(np.where(hm, lanes, 64)[::-1])[::-1]  # the first head at or behind the lane
                nxt = np.concatenate([nxt[1:], [64]])                              # ... behind it; 64: none
                if wrong == WRONG[3]:
                    nxt = np.where(nxt < 64, int(at[-1]), 64)
                total[t] = np.where(nxt < 64, run[t][np.clip(nxt - 1, 0, 63)], np.uint64(after))
                first = int(at[0])
                if first > 0:
                    after = int(run[t][first - 1])
                elif wrong == WRONG[2]:
                    after = int(run[t][63])
                elif t > 0:
                    after = int(run[t - 1][63])
                else:
                    after = base[1]
            keep = (b["on"] | case["all_rows"]) & (b["r"] < case["n_rows"]).reshape(steps, 64)
            out = (np.where(keep, total, np.uint64(0)) & mask).reshape(-1)
            first = seg * SEG_WORDS + blk * BLOCK_WORDS
            for i in range(rows_out(case)):
                bits = ((out >> np.uint64(k_out - 1 - i)) & np.uint64(1)).astype(bool) if i < k_out else b["on"].reshape(-1)
                matrix[i, first: first + 2 * steps] = _bsi.pack_bits(bits)
    return matrix


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def make_case(n, kv, k_out, starts, **kw):
    assert "exclusive" not in kw
    return cp.make_case(n, kv, k_out, starts, **kw)


SIZES = cs.SIZES
BIG = cs.BIG
VAL_WIDTHS, OUT_WIDTHS = cp.VAL_WIDTHS, cp.OUT_WIDTHS
SEAMS = cp.SEAMS
ROUND_SEGMENTS = SCAN_ROUND + 2  # 8194: two more than a round of either scan


def named_cases():
    """name -> case: what tests/test_total_parts_reference.py proves the statements and the wrong models on, and
    tests/test_gpu_bsi_total_parts.py runs on the device."""
    cases = {}
    rows = 32 * BIG
    for i, n in enumerate(SIZES):
        cases[f"no start, {i + 1} segments"] = make_case(n, 7, 24, [], n_filters=1, all_rows=i == 1, seed=12)
        cases[f"every row a start, {i + 1} segments"] = make_case(n, 9, 12, np.ones(32 * n, bool), n_filters=i % 2, all_rows=i == 2, seed=13)
    both = SEAMS + tuple(SEG_BITS + r for r in SEAMS)
    for j, r in enumerate(both):  # each seam alone, in segment 0 and in segment 1: a count, which every row changes
        select = dict(filters=[np.ones(rows, bool)]) if j % 3 else dict(n_filters=1)
        cases[f"a start at row {r} alone"] = make_case(BIG, 0, 17, [r], all_rows=j % 2 == 1, seed=j, **select)
    for all_rows in (False, True):
        tail = " all_rows" if all_rows else ""
        cases[f"starts at the seams{tail}"] = make_case(BIG, 7, 24, both, n_filters=1, all_rows=all_rows, seed=14)
        two = [64 * 5, 64 * 5 + 63, 64 * 40 + 1, 64 * 40 + 2, SEG_BITS + 64 * 9, SEG_BITS + 64 * 9 + 63]
        three = [64 * 7, 64 * 7 + 17, 64 * 7 + 63, HALF_START + 64 * 3, HALF_START + 64 * 3 + 30, HALF_START + 64 * 3 + 31]
        cases[f"two starts in a step{tail}"] = make_case(2 * SEG_WORDS, 7, 24, two, n_filters=1, all_rows=all_rows, seed=15)
        cases[f"three starts in a step{tail}"] = make_case(2 * SEG_WORDS, 27, 40, three, all_rows=all_rows, seed=15)
        n_rows = 2 * SEG_BITS + 4000
        cases[f"starts at a block's, a segment's and the table's ends{tail}"] = make_case(
            BIG, 7, 24, [3 * BLOCK_ROWS, SEG_BITS, SEG_BITS + 9 * BLOCK_ROWS, n_rows - 1], n_rows=n_rows, n_filters=1, all_rows=all_rows, seed=20)
        cases[f"a partition over three segments{tail}"] = make_case(BIG, 9, 30, [100], n_filters=1, all_rows=all_rows, seed=16)
        middle = np.ones(rows, bool)
        middle[SEG_BITS: 2 * SEG_BITS] = False
        cases[f"a partition over three segments, the middle one empty{tail}"] = make_case(BIG, 9, 30, [100], all_rows=all_rows, filters=[middle], seed=16)
        cases[f"a start in segment 1 only{tail}"] = make_case(BIG, 9, 30, [SEG_BITS + 5000], n_filters=1, all_rows=all_rows, seed=17)
        f = np.random.default_rng(18).random(rows) < 0.5
        at = np.flatnonzero(~f)[:: 97]
        cases[f"starts at unselected rows{tail}"] = make_case(BIG, 7, 24, at, all_rows=all_rows, filters=[f], seed=18)
        n_rows = SEG_BITS + 4000
        cases[f"starts at and behind n_rows{tail}"] = make_case(BIG, 7, 24, [3000, n_rows - 1, n_rows, n_rows + 1, n_rows + 64, 2 * SEG_BITS + 9], n_rows=n_rows,
                                                                  n_filters=1, all_rows=all_rows, seed=19)
        empty = np.ones(rows, bool)
        empty[5000:9000] = False
        cases[f"a partition without a selected row{tail}"] = make_case(BIG, 7, 24, [777, 5000, 9000, SEG_BITS + 1], all_rows=all_rows, filters=[empty], seed=21)
    # widths: every pair, the sizes, all_rows, an existence row, a filter and the density of the starts in turn
    i = 0
    for kv in VAL_WIDTHS:
        for k_out in OUT_WIDTHS:
            cases[f"widths {kv} x {k_out}"] = make_case(SIZES[i % 3], kv, k_out, (1 / 16, 1 / 700, 1 / 9000)[(i // 2) % 3], with_exists=i % 2 == 1,
                                                        n_filters=(i // 2) % 2 if kv else 1, all_rows=i % 4 >= 2)
            i += 1
    # totals that leave 32 bits
    ones = np.full(rows, TOP32, np.uint64)
    far = list(range(777, rows, 20011))
    cases["totals past 2^32"] = make_case(BIG, 32, 48, far, values=ones)
    cases["totals past 2^32 all_rows"] = make_case(BIG, 32, 48, far, all_rows=True, values=ones, n_filters=1)
    cases["totals past 2^32 truncated"] = make_case(BIG, 32, 33, far, values=ones, n_filters=1)
    for with_exists in (False, True):
        for all_rows in (False, True):
            name = f"flags{' exists' if with_exists else ''}{' all_rows' if all_rows else ''}"
            cases[name] = make_case(2 * SEG_WORDS, 7, 23, 1 / 300, n_rows=2 * SEG_BITS - 777, with_exists=with_exists, n_filters=1, all_rows=all_rows, seed=3)
    for n_filters in (0, 1, cs.MAX_FILTERS):
        cases[f"filters {n_filters}"] = make_case(2 * SEG_WORDS, 12, 28, 1 / 1000, with_exists=True, n_filters=n_filters, seed=4)
    cases["count under 64 filters"] = make_case(2 * SEG_WORDS, 0, 16, 1 / 50, n_filters=cs.MAX_FILTERS, all_rows=True, seed=4)
    return cases


def random_case(seed):
    case = cp.random_case(seed)
    case["exclusive"] = False
    return case


def round_seam_records(seed=8194):
    """ROUND_SEGMENTS records with starts in the first four and the last four segments and sums that fill 62 bits: both scans' round
    seams lie inside the one long partition, the forward one behind record 8191, the backward one in front of record 2."""
    rng = np.random.default_rng(seed)
    return [(i < 4 or i >= ROUND_SEGMENTS - 4, int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 62))) for i in range(ROUND_SEGMENTS)]


# ---- long bitmaps: expected from tests/_long.py's run model ------------------------------------------------------------------------------
def long_expected(oracle, filt, starts, n_rows, empty=None, put=None):
    """The call's result for bitmaps too long to exist decoded (tests/_long.py: LongBitmap): a filter of constant ones with a few live
    segments, starts of constant zeros with a few live segments, no value slices, a 2-bit result and all_rows -- every row in front
    of n_rows holds the number of selected rows of its partition mod 4.  A constant segment holds no start, so all its rows lie in
    one partition and every one of its result slices is ONE fill, of ones or of zeros, by the partition's size; a segment at or
    behind n_rows is a zero fill.  Only the live segments -- the filter's and those that hold a start -- are computed row by row;
    the partitions' sizes are added up from the runs, a constant segment in front of n_rows giving 31 744.  Nothing is decoded.
    empty(total) makes the int32 output and put(words) moves numpy words to where it lives (defaults: numpy).  Returns (stream
    int32, index int64, the partitions' sizes in order)."""
    from tests import _long as lg

    empty = empty or (lambda total: np.empty(total, np.int32))
    put = put or (lambda words: words)
    a = filt.n_segments
    assert starts.n_segments == a and set(filt.defaults().tolist()) == {1} and not starts.defaults().any()
    live = sorted(set(filt.live) | set(starts.live))
    cut = n_rows // SEG_BITS
    assert cut in live or n_rows % SEG_BITS == 0
    sizes, run = [], 0       # the closed partitions' sizes; the open one's so far
    first_part, per_row = {}, {}  # per live segment: the partition open at its row 0, and the rows' partitions relative to it
    prev = 0
    for s in live + [a]:
        run += SEG_BITS * max(0, min(s, cut) - prev)  # the constant segments [prev, s) in front of n_rows, all ones
        if s == a:
            break
        row = s * SEG_BITS + np.arange(SEG_BITS)
        bits = filt.seg_bits(s).astype(np.int64) * (row < n_rows)
        st = starts.seg_bits(s).astype(bool) & (row < n_rows)
        ids = np.cumsum(st)
        sums = np.bincount(ids, weights=bits, minlength=int(ids[-1]) + 1).astype(np.int64)
        first_part[s], per_row[s] = len(sizes), ids
        run += int(sums[0])
        for more in sums[1:]:
            sizes.append(run)
            run = int(more)
        prev = s + 1
    sizes.append(run)
    sizes = np.asarray(sizes, np.int64)
    words = {}
    for s in live:
        row = s * SEG_BITS + np.arange(SEG_BITS)
        value = np.where(row < n_rows, sizes[first_part[s] + per_row[s]] & 3, 0)
        words[s] = [np.asarray(oracle.compress(_bsi.pack_bits(((value >> b) & 1).astype(bool))), dtype=np.uint32).view(np.int32) for b in (1, 0)]
    fills = np.array([lg.FILL | lg.SEG_GROUPS, lg.FILL | lg.ONE | lg.SEG_GROUPS], np.uint32).view(np.int32)
    assert np.array_equal(np.asarray(oracle.compress(np.full(SEG_WORDS, 0xFFFFFFFF, np.uint32)), dtype=np.uint32).view(np.int32), fills[1:])
    lengths = np.ones((2, a), np.int64)
    for s, pair in words.items():
        lengths[0, s], lengths[1, s] = pair[0].size, pair[1].size
    index = np.concatenate([[0], np.cumsum(lengths.reshape(-1))]).astype(np.int64)
    want = empty(int(index[-1]))
    for j, b in enumerate((1, 0)):
        first = 0
        for s in live + [a]:  # the constant segments [first, s), all in one partition: the one open at s's row 0, or the last one
            if s > first:
                size = int(sizes[first_part[s]] if s < a else sizes[-1])
                mid = min(max(cut, first), s)  # in front of n_rows the partition's bit, behind it zeros
                lo, at, hi = int(index[j * a + first]), int(index[j * a + first]) + (mid - first), int(index[j * a + s])
                want[lo:at] = int(fills[(size >> b) & 1])
                want[at:hi] = int(fills[0])
            if s < a:
                at = int(index[j * a + s])
                want[at: at + words[s][j].size] = put(words[s][j])
            first = s + 1
    return want, index, sizes


# the named case on which a wrong model has to change the answer ("records": round_seam_records() through scan_records alone -- the
# kernels' restatement of 8194 segments row by row would be 260 million rows)
CAUGHT_BY = {
    WRONG[0]: "a start in segment 1 only",
    WRONG[1]: "a partition over three segments",
    WRONG[2]: "two starts in a step",
    WRONG[3]: "three starts in a step",
    WRONG[4]: "three starts in a step",
    WRONG[5]: "records",
    WRONG[6]: "starts at unselected rows",
}
