"""Thresholds, shapes and references for tests/test_gpu_full_grid.py: the sizes at which a wavefront of from_positions_kernel,
from_positions_check_kernel, fetch_check_kernel and bsi_slices_kernel takes a SECOND item and carries state into it.  No GPU, no
library: tests/test_grid_reference.py proves everything here on the CPU.

All four kernels cap their grid at what the chip holds at once.  The caps are read out of the sources (as _fetch.grid_waves()
does), and every shape is written in terms of them: a cap that moves fails tests/test_grid_reference.py by name and does not
quietly shrink what the GPU tests reach.

runs() restates how from_positions_kernel shares its (list, segment) items out in contiguous runs.  The three builder shapes
give every item one of five row counts -- 0, 1, 64, 65, about 300: the three routes of the kernel at their edges
(_rows.route_of) -- and put a row on the first and on the last position of the segment half of the time, so a slice of the
list that begins or ends one row early or late moves a row into the neighbouring segment and changes the words of two
segments.  The conditions that keep the GPU tests from being vacuous are asserted here (assert_shape), two numpy models of what
a wrong carry would build among them (model_lo_is_list_start, model_stale_list)."""
import functools
import math
import os
import re

import numpy as np

from tests import _bsi, _rows, _select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-wah_amd", "csrc")
FROM_POSITIONS_SOURCE = os.path.join(CSRC, "wah_from_positions.hip")
FETCH_SOURCE = os.path.join(CSRC, "wah_bitop_list.hip")
BSI_BUILD_SOURCE = os.path.join(CSRC, "wah_bsi_build.hip")

SEG_GROUPS, SEG_WORDS, SEG_BITS = _select.SEG_GROUPS, _select.SEG_WORDS, _select.SEG_BITS
FILL = _select.FILL
KINDS = (0, 1, 64, 65, 300)  # rows of an item; 300 stands for "about 300" (200 .. 399, at most what the segment holds)


# ---- thresholds, from the sources -----------------------------------------------------------------------------------------------
def _source(path):
    with open(path) as f:
        return f.read()


def _constant(path, name):
    m = re.search(r"constexpr u(?:32|64) %s = (\d+);" % re.escape(name), _source(path))
    assert m, f"{name} is no longer a plain constant of {os.path.basename(path)}: revisit the shapes of tests/_grid.py"
    return int(m.group(1))


def _most(path, launcher):
    """The grid cap of a launcher: the product behind the first `constexpr u64 most =` of its body."""
    text = _source(path)
    at = text.find(f"hipError_t {launcher}(")
    assert at >= 0, f"{launcher} is no longer in {os.path.basename(path)}: revisit the shapes of tests/_grid.py"
    m = re.compile(r"constexpr u64 most = (\d+)u \* (\d+)u;").search(text, at)
    nxt = text.find("hipError_t ", at + 1)
    assert m and (nxt < 0 or m.start() < nxt), f"{launcher} no longer caps its grid at `most = a * b`: revisit the shapes of tests/_grid.py"
    return int(m.group(1)) * int(m.group(2))


def _block(path, kernel):
    m = re.search(r"__launch_bounds__\((\d+)\) void %s\(" % re.escape(kernel), _source(path))
    assert m, f"{kernel} no longer states its workgroup size as a number: revisit the shapes of tests/_grid.py"
    return int(m.group(1))


@functools.lru_cache(None)
def thresholds():
    """What one trip of each capped grid covers."""
    fp_waves = _constant(FROM_POSITIONS_SOURCE, "kFpWaves")
    bsi_waves = _constant(BSI_BUILD_SOURCE, "kBsiBuildWaves")
    block_words, block_rows = _constant(BSI_BUILD_SOURCE, "kBsiBlockWords"), _constant(BSI_BUILD_SOURCE, "kBsiBlockRows")
    assert block_rows == 32 * block_words, "a block of the slices kernel is no longer 32 rows a word: revisit the BSI shape of tests/_grid.py"
    t = dict(
        fp_waves=fp_waves,
        fp_grid=_most(FROM_POSITIONS_SOURCE, "launch_from_positions_segments"),
        check_threads=_most(FROM_POSITIONS_SOURCE, "launch_from_positions_check") * _block(FROM_POSITIONS_SOURCE, "from_positions_check_kernel"),
        fetch_check_rows=_most(FETCH_SOURCE, "launch_fetch_check") * _block(FETCH_SOURCE, "fetch_check_kernel"),
        bsi_block_words=block_words, bsi_block_rows=block_rows,
        bsi_blocks=_most(BSI_BUILD_SOURCE, "launch_bsi_slices") * bsi_waves)
    t["items"] = t["fp_grid"] * fp_waves            # (list, segment) items of one trip of from_positions_kernel
    t["bsi_rows"] = t["bsi_blocks"] * block_rows    # rows of one trip of bsi_slices_kernel
    return t


# ---- how from_positions_kernel shares its items out ----------------------------------------------------------------------------
def runs(n_lists, n_segments):
    """(per, runs): run w is the list of (list, segment) items of wavefront w, in the order it takes them."""
    t = thresholds()
    n_items = n_lists * n_segments
    want = -(-n_items // t["fp_waves"])
    n_waves = max(1, min(want, t["fp_grid"])) * t["fp_waves"]
    per = -(-n_items // n_waves)
    out = []
    for w in range(n_waves):
        begin, end = min(w * per, n_items), min(w * per + per, n_items)
        out.append([divmod(item, n_segments) for item in range(begin, end)])
    return per, out


# ---- the three builder shapes -----------------------------------------------------------------------------------------------------
def _shape_table():
    items = thresholds()["items"]
    return {"two": (2976, (items + 28) // 3, 2), "three": (2981, (2 * items + 16) // 4, 3), "lists": (992, 3 * items + 5, 4)}


SHAPES = ("two", "three", "lists")


def segment_span(seg, n_words):
    """(first position, positions, groups) of segment seg of a bitmap of n_words words."""
    first = seg * SEG_BITS
    return first, min(SEG_BITS, 32 * n_words - first), min(SEG_GROUPS, _select.groups_of(n_words) - seg * SEG_GROUPS)


def _item_rows(rng, kind, first, positions):
    """`kind` rows of one segment, ascending: the first position with probability 1/2, the last one with probability 1/2, the
    others one in each of equal strides of what lies between."""
    take_first, take_last = rng.random() < 0.5, rng.random() < 0.5
    k = min(rng.integers(200, 400) if kind == 300 else kind, positions)
    if k == 0:
        return np.empty(0, np.int64)
    if k == positions:
        return first + np.arange(positions, dtype=np.int64)
    if k == 1:
        take_last = take_last and not take_first
    inner = k - take_first - take_last
    stride = (positions - 2) // inner if inner else 0
    assert inner == 0 or stride >= 1
    mid = 1 + np.arange(inner, dtype=np.int64) * stride + rng.integers(0, max(stride, 1), inner)
    return first + np.concatenate([[0] if take_first else [], mid, [positions - 1] if take_last else []]).astype(np.int64)


class Shape:
    """One builder input: .lists (row arrays), .item_rows (the rows of item list * S + segment), .kinds (the row count drawn
    for every item), .per and .runs of runs()."""

    def __init__(self, name):
        self.name = name
        self.n_words, self.n_lists, want_per = _shape_table()[name]
        self.segments = _select.segments_of(self.n_words)
        self.per, self.runs = runs(self.n_lists, self.segments)
        assert self.per == want_per, f"shape {name}: a run holds {self.per} items and no longer {want_per}: revisit _shape_table"
        assert math.gcd(self.per, self.segments) == 1, f"shape {name}: the runs' first segments do not rotate"
        rng = np.random.default_rng([len(name), self.n_words, self.n_lists])
        p = (1 / 3, 1 / 6, 1 / 6, 1 / 6, 1 / 6) if name == "lists" else None
        n_items = self.n_lists * self.segments
        self.kinds = np.asarray(KINDS)[rng.choice(len(KINDS), size=n_items, p=p)]
        self.item_rows = []
        for item in range(n_items):
            first, positions, _ = segment_span(item % self.segments, self.n_words)
            self.item_rows.append(_item_rows(rng, int(self.kinds[item]), first, positions))
        s = self.segments
        self.lists = [np.concatenate(self.item_rows[c * s: (c + 1) * s]) for c in range(self.n_lists)]

    @property
    def n_items(self):
        return self.n_lists * self.segments


@functools.lru_cache(None)
def shape(name):
    return Shape(name)


def _same_rows(a, b):
    return sum(not np.array_equal(x, y) for x, y in zip(a, b))


def model_lo_is_list_start(sh):
    """The rows every item would build if a slice began at the LIST's first row instead of the carried end of the slice in front
    of it (`: slice_end` read as `: lb`): the list's rows of earlier segments come in too, and the kernel's clamp puts every one
    of them on the last bit of the segment's last group.  Only items behind the first of a run, in a segment other than 0, carry."""
    out = list(sh.item_rows)
    for run in sh.runs:
        for c, seg in run[1:]:
            if seg and any(sh.item_rows[c * sh.segments + s].size for s in range(seg)):
                first, _, groups = segment_span(seg, sh.n_words)
                out[c * sh.segments + seg] = np.union1d(sh.item_rows[c * sh.segments + seg], [first + 31 * groups - 1])
    return out


def model_stale_list(sh):
    """The rows every item would build if a run kept the bounds of the list it began in behind a list end (the crossing without
    `have_list = false`): every later list of the run is built from that first list's rows, segment for segment."""
    out = list(sh.item_rows)
    for run in sh.runs:
        for c, seg in run:
            if c != run[0][0]:
                out[c * sh.segments + seg] = sh.item_rows[run[0][0] * sh.segments + seg]
    return out


def assert_shape(sh):
    """What keeps the GPU tests of a shape from being vacuous.  Returns the figures."""
    name, s = sh.name, sh.segments
    assert sh.per >= 2, name
    assert sum(len(r) for r in sh.runs) == sh.n_items and max(len(r) for r in sh.runs) == sh.per, name
    for item, rows in enumerate(sh.item_rows):
        first, positions, _ = segment_span(item % s, sh.n_words)
        assert rows.size == min(sh.kinds[item], positions) or (sh.kinds[item] == 300 and 200 <= rows.size < 400), (name, item)
        assert rows.size == 0 or (first <= rows[0] and rows[-1] < first + positions and np.all(np.diff(rows) > 0)), (name, item)
    inside, across, late = set(), set(), 0
    for run in sh.runs:
        for (c0, s0), (c1, s1) in zip(run, run[1:]):
            pair = (int(sh.kinds[c0 * s + s0]), int(sh.kinds[c1 * s + s1]))
            (inside if c0 == c1 else across).add(pair)
        if run and run[0][1] and any(sh.item_rows[run[0][0] * s + e].size for e in range(run[0][1])):
            late += 1
    every = {(a, b) for a in KINDS for b in KINDS}
    if name != "lists":
        assert inside == every and across == every, (name, sorted(every - inside), sorted(every - across))
        assert late >= 100, (name, late)
        firsts = {run[0][1] for run in sh.runs if run}
        assert firsts == set(range(s)), (name, firsts)
        if sh.n_words % SEG_WORDS:  # the ragged last segment in every place of a run
            places = {i for run in sh.runs for i, (_, seg) in enumerate(run) if seg == s - 1}
            assert places == set(range(sh.per)), (name, places)
    else:
        assert across == every and not inside, name
        empty = sum(r.size == 0 for r in sh.lists)
        assert 0.3 < empty / sh.n_lists < 0.37, (name, empty)
    edge_first = sum(r.size > 0 and r[0] % SEG_BITS == 0 for r in sh.item_rows)
    edge_last = sum(r.size > 0 and r[-1] == sum(segment_span(i % s, sh.n_words)[:2]) - 1 for i, r in enumerate(sh.item_rows))
    filled = sum(r.size > 0 for r in sh.item_rows)
    assert 0.4 < edge_first / filled < 0.6 and 0.4 < edge_last / filled < 0.6, (name, edge_first, edge_last, filled)
    stale = _same_rows(model_stale_list(sh), sh.item_rows)
    assert stale >= 100, (name, "a stale list changes", stale, "segments")
    lo = _same_rows(model_lo_is_list_start(sh), sh.item_rows)
    assert lo >= 100 or s == 1, (name, "a slice from the list's first row changes", lo, "segments")
    return dict(late=late, stale=stale, lo=lo)


# ---- lists of no row or one row: the closed form ---------------------------------------------------------------------------------
def one_row_reference(positions, n_words):
    """(stream, index) of one call whose list c is empty (positions[c] < 0) or holds the one row positions[c]: per segment one
    zero-fill of its groups, and in the row's segment the literal with a zero-fill for the groups on either side of it that
    there are (the word count is _rows.one_row_words)."""
    p = np.asarray(positions, np.int64)
    segments, groups = _select.segments_of(n_words), _select.groups_of(n_words)
    in_seg = np.minimum(SEG_GROUPS, groups - SEG_GROUPS * np.arange(segments, dtype=np.int64))
    g = np.where(p >= 0, p // 31, 0)
    seg, local = g // SEG_GROUPS, g % SEG_GROUPS
    has = p >= 0
    left, right = has & (local > 0), has & (local < in_seg[seg] - 1)
    words = np.ones((p.size, segments), np.int64)
    words[np.flatnonzero(has), seg[has]] = 1 + left[has] + right[has]
    index = np.concatenate([[0], np.cumsum(words.reshape(-1))]).astype(np.int64)
    stream = (FILL | np.tile(in_seg, p.size)).astype(np.uint32)  # every segment one zero-fill ...
    stream = np.repeat(stream, words.reshape(-1))
    at = index[np.flatnonzero(has) * segments + seg[has]]         # ... but the row's: [gap] literal [gap]
    lit = at + left[has]
    stream[at[left[has]]] = (FILL | local[has][left[has]]).astype(np.uint32)
    stream[lit] = (np.int64(1) << (p[has] % 31)).astype(np.uint32)
    stream[lit[right[has]] + 1] = (FILL | (in_seg[seg[has]] - 1 - local[has])[right[has]]).astype(np.uint32)
    return stream, index


def one_row_lists(positions):
    return [np.array([q], np.int64) if q >= 0 else np.empty(0, np.int64) for q in np.asarray(positions, np.int64).tolist()]


# ---- the check pass of the builder: a second trip of the rows loop, of the ends loop ------------------------------------------------
CHECK_ROWS_WORDS = 6 * SEG_WORDS


@functools.lru_cache(None)
def check_rows_lists():
    """Four lists over 6 segments, more rows than one trip of the check pass covers by over 4096; the last list boundary -- a legal
    descent -- lies behind the first trip.  (A list holds at most 32 * n_words = 190 464 rows, so it takes three lists to get
    there and a fourth one behind the boundary.)"""
    trip = thresholds()["check_threads"]
    sizes = [180000, 180000, trip + 5712 - 360000, 10000]
    assert 0 < sizes[2] <= 32 * CHECK_ROWS_WORDS, "the check pass covers another number of rows a trip: revisit check_rows_lists"
    rng = np.random.default_rng(77)
    lists = [np.sort(rng.choice(32 * CHECK_ROWS_WORDS, size=k, replace=False)).astype(np.int64) for k in sizes]
    rows, ends = _rows.flatten(lists)
    assert rows.size > trip + 4096 and ends[2] > trip + 1 and ends[2] < rows.size - 2
    assert rows[ends[2] - 1] > rows[ends[2]]  # the boundary is a descent
    return lists


CHECK_ENDS_WORDS = SEG_WORDS


@functools.lru_cache(None)
def check_ends_positions():
    """The one row (or -1: none) of each of trip + 12 lists over one segment.  The three lists around list index `trip` and the
    last three hold one row each, ascending from list to list: no descent there, so an end that is wrong there is seen by the
    ends loop ALONE (the rows loop asks the ends only where rows descend)."""
    trip = thresholds()["check_threads"]
    n_lists = trip + 12
    rng = np.random.default_rng(78)
    p = rng.integers(0, SEG_BITS, n_lists)
    p[rng.random(n_lists) < 1 / 3] = -1
    p[trip - 1: trip + 2] = (100, 200, 300)
    p[-3:] = (1000, 2000, 3000)
    return p


# ---- the fetch call's check pass ----------------------------------------------------------------------------------------------------
FETCH_WORDS, FETCH_BITS_WIDE, FETCH_KEYS = 3 * SEG_WORDS, 20, 5


@functools.lru_cache(None)
def fetch_case():
    """(values, exists, keys, rows): a 20-bit attribute with existence bytes and a key column of five values over three segments,
    and trip + 200 listed rows, non-descending, with duplicates, in all three segments."""
    trip = thresholds()["fetch_check_rows"]
    rng = np.random.default_rng(79)
    count = 32 * FETCH_WORDS
    values = _bsi.uniform_values(rng, count, FETCH_BITS_WIDE)
    exists = rng.random(count) < 0.8
    keys = rng.integers(0, FETCH_KEYS, count)
    rows = np.sort(rng.integers(0, count, trip + 200)).astype(np.int64)
    rows[0], rows[-1] = 0, count - 1
    return values, exists, keys, rows


# ---- the slices kernel: a second block for some wavefronts ------------------------------------------------------------------------
def bsi_shape():
    """(n_words, n_rows): half a block more than 8199 blocks of words -- wavefronts 0 to 7 take a second block, the last one half
    full --; the rows fill blocks 8192 to 8194, 77 rows of block 8195, and leave the blocks behind it to the zeros."""
    t = thresholds()
    n_words = SEG_WORDS * 529
    n_rows = t["bsi_rows"] + 3 * t["bsi_block_rows"] + 77
    blocks = n_words / t["bsi_block_words"]
    assert t["bsi_blocks"] + 7 < blocks < t["bsi_blocks"] + 8 and blocks % 1 == 0.5, "the slices kernel's trip moved: revisit bsi_shape"
    assert n_rows < 32 * n_words - 4 * t["bsi_block_rows"]
    return n_words, n_rows


@functools.lru_cache(None)
def bsi_case(n_bits, with_exists):
    n_words, n_rows = bsi_shape()
    rng = np.random.default_rng([n_words, n_bits, int(with_exists)])
    values = _bsi.uniform_values(rng, n_rows, n_bits)
    exists = rng.random(n_rows) < 0.7 if with_exists else None
    return values, exists


def bsi_slice_row(values, n_bits, i, n_words):
    """Row i of the expected slice matrix alone (bit n_bits - 1 - i of every value), for columns without existence bytes."""
    bits = np.zeros(32 * n_words, bool)
    bits[: values.size] = (values >> np.uint64(n_bits - 1 - i)) & np.uint64(1)
    return _bsi.pack_bits(bits)


def assert_second_trip_matters(row, what):
    """A slice row has a set and a clear bit among the real rows of the second trip."""
    n_words, n_rows = bsi_shape()
    t = thresholds()
    bits = _bsi.unpack_bits(row[t["bsi_blocks"] * t["bsi_block_words"]:])[: n_rows - t["bsi_rows"]]
    assert bits.size == n_rows - t["bsi_rows"] and bits.any() and not bits.all(), what
