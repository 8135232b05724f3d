"""Shared helpers of the grouped order-statistics tests (wah_bsi_kth_grouped_indexed_device: include/wah.h).  No GPU, no library:
tests/test_kthg_reference.py proves everything here on the CPU.

  * the model answers from the VALUES: per group _kth.Model(values, filters & group), asked every query;
  * restate() is the kernels' algorithm in numpy, lane by lane (a LANE is a (group, query) pair, number g * Q + q): per pass the
    items (segment, lane), each the AND of the filters and of its group's rows over its segment, the short cut of an item that
    selects nothing there, the one kind of item that takes no short cut because it CHECKS the slices (lane 0 in the last pass),
    a histogram per lane, and the decision per lane; item_of() and wave_items() say which wavefront takes which item;
  * the builders of the shapes both test files use, and the conditions that keep them from being vacuous (assert_* below);
  * the grid cap of the pass launcher, read out of the source as tests/_grid.py reads `most`: a cap that moves fails by name.

Rows are bool arrays of 32 * n_words entries; a result is five Python ints (found, value, total, less, equal)."""
import functools
import os
import re

import numpy as np

from tests import _bsi, _grid, _kth, _select

SEG_WORDS, SEG_BITS = _select.SEG_WORDS, _select.SEG_BITS
ASC, DESC, QUANT = _kth.ASCENDING, _kth.DESCENDING, _kth.QUANTILE
MIN_MEDIAN_MAX = [(QUANT, 0, 1), (QUANT, 1, 2), (QUANT, 1, 1)]
PASS_WAVES = 4  # wavefronts of a workgroup of the pass kernel (kSegDecodeWaves)


# ---- constants, from the sources ----------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def digit_bits():
    text = _grid._source(os.path.join(_grid.CSRC, "wah_internal.hpp"))
    m = re.search(r"#define WAH_BSI_KTH_DIGIT_BITS (\d+)", text)
    assert m, "WAH_BSI_KTH_DIGIT_BITS is no longer a plain define of wah_internal.hpp: revisit tests/_kthg.py"
    return int(m.group(1))


@functools.lru_cache(None)
def grid_cap():
    """Workgroups of bsi_kth_group_pass_kernel at the most."""
    return _grid._most(_grid.FETCH_SOURCE, "launch_bsi_kth_group_pass")


def grid_waves(n_items):
    """Wavefronts of the pass launch over n_items items."""
    want = -(-n_items // PASS_WAVES)
    return max(1, min(want, grid_cap())) * PASS_WAVES


def wave_items(n_items):
    """The item numbers every wavefront of the pass launch takes, in its order: a whole grid apart."""
    waves = grid_waves(n_items)
    return [list(range(w, n_items, waves)) for w in range(waves)]


def item_of(i, lanes, n_items):
    """(segment, lane) of item i of n_items: the lane runs fastest, and segment s holds lane l at place (l + s // R) % lanes, R the
    segments one trip of the grid covers -- the turn that keeps a wavefront from having one lane in all its items."""
    per_trip = max(1, grid_waves(n_items) // lanes)
    seg, place = divmod(i, lanes)
    return seg, (place - seg // per_trip) % lanes


# ---- a case -----------------------------------------------------------------------------------------------------------------------
class Case:
    """values: uint64 per row; filters: bool rows, ANDed; groups: per group its R bool rows, ANDed; queries: (kind, a, b)."""

    def __init__(self, name, n_words, n_bits, values, filters, groups, queries):
        self.name, self.n_words, self.n_bits, self.values = name, n_words, n_bits, values
        self.filters, self.groups, self.queries = list(filters), [list(g) for g in groups], list(queries)
        self.rows = 32 * n_words
        self.rows_per_group = len(self.groups[0])
        assert values.size == self.rows and all(len(g) == self.rows_per_group for g in self.groups)
        assert all(r.size == self.rows for r in self.filters) and all(r.size == self.rows for g in self.groups for r in g)

    @property
    def lanes(self):
        return len(self.groups) * len(self.queries)

    def selected(self, g):
        s = np.ones(self.rows, bool)
        for r in self.filters + self.groups[g]:
            s &= r
        return s

    def slices(self):
        """bool [n_bits, rows], the most significant slice first"""
        return np.stack([((self.values >> np.uint64(self.n_bits - 1 - i)) & np.uint64(1)).astype(bool) for i in range(self.n_bits)])

    @functools.lru_cache(None)
    def model(self):
        """[G][Q] results, from the values"""
        out = []
        for g in range(len(self.groups)):
            m = _kth.Model(self.values, self.selected(g))
            out.append([m(*q) for q in self.queries])
        return out


# ---- the kernels' algorithm -----------------------------------------------------------------------------------------------------------
def restate(case, trace=None):
    """[G][Q] results by the lane-wise radix select over the slices.  trace: a dict that collects, for the guards,
    counted / skipped: per pass the (segment, lane) items that counted, and those that took the short cut;
    checked: the segments whose slices the checking items walked; picks: (digit width, bucket) of every decision;
    prefix0: per lane the prefix behind pass 0."""
    digit, n_bits, rows = digit_bits(), case.n_bits, case.rows
    slices = case.slices()
    n_q, lanes = len(case.queries), case.lanes
    n_seg = -(-rows // SEG_BITS)
    base = np.ones(rows, bool)
    for f in case.filters:
        base &= f
    group_sel = []
    for g in case.groups:
        s = base.copy()
        for r in g:
            s &= r
        group_sel.append(s)
    state = [dict(prefix=0, rank=None, less=0, total=0, found=False, equal=0) for _ in range(lanes)]
    passes = -(-n_bits // digit)
    if trace is not None:
        trace.update(counted=[set() for _ in range(passes)], skipped=[set() for _ in range(passes)], checked=set(), picks=set(), prefix0=[])
    for p in range(passes):
        first, end = p * digit, min(p * digit + digit, n_bits)
        last = end == n_bits
        hist = np.zeros((lanes, 1 << digit), np.int64)
        for seg in range(n_seg):
            lo, hi = seg * SEG_BITS, min(rows, (seg + 1) * SEG_BITS)
            number = np.zeros(hi - lo, np.int64)  # the digit of every row of the segment
            for i in range(first, end):
                number |= slices[i, lo:hi].astype(np.int64) << (end - 1 - i)
            for lane in range(lanes):  # the lane runs fastest
                eq = group_sel[lane // n_q][lo:hi]
                checks = last and lane == 0
                if not eq.any() and not checks:  # the short cut: behind the filter and group sweeps
                    if trace is not None:
                        trace["skipped"][p].add((seg, lane))
                    continue
                if trace is not None:
                    trace["counted"][p].add((seg, lane))
                    if checks:
                        trace["checked"].add(seg)
                eq = eq.copy()
                prefix = state[lane]["prefix"]
                for i in range(first):
                    eq &= slices[i, lo:hi] if (prefix >> (n_bits - 1 - i)) & 1 else ~slices[i, lo:hi]
                hist[lane] += np.bincount(number[eq], minlength=1 << digit)
        for lane in range(lanes):
            st, h = state[lane], [int(v) for v in hist[lane]]
            if p == 0:
                st["total"] = sum(h)
                st["rank"] = _kth.rank_of(*case.queries[lane % n_q], st["total"])
                st["found"] = st["rank"] is not None
            bucket = 0
            if st["found"]:
                below = 0
                for bucket, count in enumerate(h):
                    if st["rank"] < below + count:
                        st["equal"] = count
                        break
                    below += count
                st["rank"] -= below
                st["less"] += below
                if trace is not None:
                    trace["picks"].add((end - first, bucket))
            st["prefix"] |= bucket << (n_bits - end)
            if p == 0 and trace is not None:
                trace["prefix0"].append(st["prefix"])
    flat = [(1, st["prefix"], st["total"], st["less"], st["equal"]) if st["found"] else (0, 0, st["total"], 0, 0) for st in state]
    return [flat[g * n_q: (g + 1) * n_q] for g in range(len(case.groups))]


# ---- builders ---------------------------------------------------------------------------------------------------------------------
SIZES = [31, SEG_WORDS, 1000, SEG_WORDS * 9 + 17]
WIDTHS = [1, 4, 5, 9, 20, 64]


def _filters(rng, rows, n_filters):
    """none; the existence bitmap; existence and a mask"""
    return [rng.random(rows) < p for p in (0.9, 0.4)[:n_filters]]


def _product_groups(keys, counts):
    """The Cartesian product of the keys' values, row-major: one row per key and group."""
    picks = np.stack(np.meshgrid(*[np.arange(k) for k in counts], indexing="ij"), -1).reshape(-1, len(counts))
    return [[keys[r] == v for r, v in enumerate(pick)] for pick in picks]


@functools.lru_cache(None)
def keyed(n_words, n_bits, n_filters, counts=(3,), queries="mmm"):
    """Uniform values over the full width; one random key per entry of counts with one value more than it has groups, so some rows
    belong to no group; the groups are the product of the keys' values.  queries: "mmm" (MIN, median, MAX), "min" alone, or
    "spread": _kth.query_cases(total of group 0, spread=True)."""
    rng = np.random.default_rng([n_words, n_bits, n_filters, len(counts)])
    rows = 32 * n_words
    values = _bsi.uniform_values(rng, rows, n_bits)
    keys = [rng.integers(0, k + 1, rows) for k in counts]
    filters, groups = _filters(rng, rows, n_filters), _product_groups(keys, counts)
    case = Case(f"keyed {n_words} x {n_bits}, {n_filters} filters, {counts}, {queries}", n_words, n_bits, values, filters, groups, [(QUANT, 0, 1)])
    if queries == "mmm":
        case.queries = list(MIN_MEDIAN_MAX)
    elif queries == "spread":
        case.queries = [(kind, a, b) for _, kind, a, b in _kth.query_cases(int(case.selected(0).sum()), spread=True)]
    return case


@functools.lru_cache(None)
def overlapping():
    """Four groups over one key of four values: {0, 1}, {1, 2}, {0, 1} again through the SAME row twice (R = 2: the row and itself),
    and one that selects nothing (two disjoint rows)."""
    n_words, n_bits = SEG_WORDS * 2 + 3, 9
    rng = np.random.default_rng(8)
    rows = 32 * n_words
    values = _bsi.uniform_values(rng, rows, n_bits)
    key = rng.integers(0, 4, rows)
    a, b = np.isin(key, [0, 1]), np.isin(key, [1, 2])
    everything = np.ones(rows, bool)
    groups = [[a, everything], [b, everything], [a, a], [key == 0, key == 3]]
    return Case("overlapping", n_words, n_bits, values, _filters(rng, rows, 1), groups, MIN_MEDIAN_MAX)


CLUSTERED_TAIL = 300  # rows of the last group: all of them in the ragged last segment


@functools.lru_cache(None)
def clustered(n_filters=1):
    """Keys sorted in row order: group g is ONE run of rows, so its row is one zero-fill in most segments.  The runs end inside
    segments; the last group has its CLUSTERED_TAIL rows in the ragged last segment alone."""
    n_words, n_bits = SIZES[-1], 20
    rng = np.random.default_rng(9)
    rows = 32 * n_words
    values = _bsi.uniform_values(rng, rows, n_bits)
    ends = [0, int(2.5 * SEG_BITS), int(5.2 * SEG_BITS), rows - CLUSTERED_TAIL, rows]
    assert ends[3] > 9 * SEG_BITS
    groups = []
    for lo, hi in zip(ends, ends[1:]):
        r = np.zeros(rows, bool)
        r[lo:hi] = True
        groups.append([r])
    return Case("clustered", n_words, n_bits, values, _filters(rng, rows, n_filters), groups, MIN_MEDIAN_MAX)


SECOND_ITEM_GROUPS, SECOND_ITEM_QUERIES = 35, 2


@functools.lru_cache(None)
def second_item():
    """The smallest lanes x segments above what one trip of the capped grid covers, for a cap of 1024 workgroups of four
    wavefronts: 70 lanes x 60 segments = 4200 items, so 104 wavefronts take a second item, of another lane.  Five slices: two
    passes, the second one a short digit."""
    n_segments = -(-(grid_cap() * PASS_WAVES + 1) // (SECOND_ITEM_GROUPS * SECOND_ITEM_QUERIES))
    n_words, n_bits = SEG_WORDS * n_segments, 5
    rng = np.random.default_rng(10)
    rows = 32 * n_words
    values = _bsi.uniform_values(rng, rows, n_bits)
    key = rng.integers(0, SECOND_ITEM_GROUPS, rows)
    groups = [[key == g] for g in range(SECOND_ITEM_GROUPS)]
    return Case("second item", n_words, n_bits, values, [], groups, [(QUANT, 1, 3), (DESC, 5, 1)])


def shapes():
    """name -> case: every shape the reference test holds restate() against the model on."""
    out = {}
    for n in SIZES:
        for n_bits in (5, 9):
            out[f"size {n}, {n_bits} bits"] = keyed(n, n_bits, 1)
    for n_bits in WIDTHS:
        out[f"width {n_bits}"] = keyed(1000, n_bits, 2)
    out["two keys"] = keyed(SIZES[-1], 9, 1, (2, 3))
    out["one lane"] = keyed(1000, 9, 1, (1,), "min")
    out["no filter"] = keyed(SIZES[-1], 20, 0)
    out["spread"] = keyed(SEG_WORDS * 2 + 5, 9, 1, (3,), "spread")
    out["overlapping"] = overlapping()
    out["clustered"] = clustered()
    out["second item"] = second_item()
    return out


# ---- what keeps the tests from being vacuous ---------------------------------------------------------------------------------------
def assert_groups_differ(case):
    """The answers differ between groups: a kernel that reads another lane's state or histogram fails."""
    m = case.model()
    found = [g for g in range(len(m)) if all(r[0] for r in m[g])]
    assert len(found) >= 2, case.name
    assert len({tuple(m[g]) for g in found}) == len(found), case.name


def assert_second_item(case):
    """More items than one trip of the grid, and a wavefront whose second item is another lane's."""
    n_seg = -(-case.rows // SEG_BITS)
    n_items = n_seg * case.lanes
    assert n_items > grid_cap() * PASS_WAVES, (n_items, grid_cap())
    runs = [r for r in wave_items(n_items) if len(r) > 1]
    assert runs and all(item_of(r[0], case.lanes, n_items)[1] != item_of(r[1], case.lanes, n_items)[1] for r in runs), "no lane change inside a wavefront's run"
    assert sorted(item_of(i, case.lanes, n_items) for i in range(n_items)) == [(s, l) for s in range(n_seg) for l in range(case.lanes)]
    assert n_items - case.lanes <= grid_cap() * PASS_WAVES, "not the smallest such shape: a whole segment fewer is still above the cap"
    return len(runs)
