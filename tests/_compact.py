"""Reference, model and named cases for wah_compact_indexed_device (include/wah.h): the rows a mask bitmap selects -- or, under
WAH_COMPACT_DELETE, does not select -- of every column of an index, moved together into new indexed bitmaps.  No GPU, no library:
tests/test_compact_reference.py proves everything here on the CPU, tests/test_gpu_compact.py holds the kernels against the
reference.

Three statements of one thing:
  model()      row by row on unpacked bits: bits[:n_rows][selected], zero padded -- the definition;
  reference()  the model, compressed per column by the oracle and indexed by _select.index_of, laid out as _splice.reference;
  arithmetic() what compact_segments_kernel does, restated: the selected rows in front of every source segment (the ranks), per
               output segment a destination image of 1024 groups, per source segment that holds a selected row the mask's and the
               column's image, and per group, 64 groups to a step: the selected mask bits, their prefix with a carry across
               steps, the column's bits under them moved together, and their deposit at destination bit rank + prefix - base,
               clipped to the output segment, into at most two destination groups.
arithmetic() takes the name of a WRONG model too: each one changes an answer on a named case (WRONG_MODELS).
A Case names the mask, the columns, the row limit, the flag, and optionally the way (tests/_foreign.py) a stream is written in."""
import functools

import numpy as np

from tests import _foreign, _select

SEG_GROUPS, SEG_WORDS, SEG_BITS = _select.SEG_GROUPS, _select.SEG_WORDS, _select.SEG_BITS
M31 = 0x7FFFFFFF
FILL0, FILL1 = 0x80000000, 0xC0000000
STEP = 64       # groups of a source segment per step of the kernel: one per lane
SEG_WAVES = 4   # WAH_SEG_WAVES: the wavefronts of a workgroup of compact_segments_kernel
GRID_CAP = 256 * 3  # workgroups of compact_segments_kernel at the most (launch_compact_segments: 48 KiB of LDS each)
WRONG_MODELS = ("seam off by one", "pad rows selected under DELETE", "second destination group dropped", "carry lost between steps")


def bits_of(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")


def words_of(bits):
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def random_words(n_words, density, seed):
    rng = np.random.default_rng([n_words, int(density * 1000), seed])
    return words_of((rng.random(32 * n_words) < density).astype(np.uint8))


def clustered_words(n_words, seed, longest=400):
    """Runs of either kind, a few bits to a few groups long."""
    rng = np.random.default_rng([n_words, seed, longest])
    bits = np.zeros(32 * n_words, np.uint8)
    at, v = 0, int(rng.integers(0, 2))
    while at < bits.size:
        n = int(rng.integers(1, longest))
        bits[at: at + n] = v
        at, v = at + n, 1 - v
    return words_of(bits)


def chosen_rows(n_words, rows):
    """The bitmap of n_words words with exactly the listed rows set."""
    return _select.bitmap_of(np.asarray(rows, dtype=np.int64), n_words)


class Case:
    """name; n_words, n_rows: the source bitmaps and how many of their positions are rows; n_words_out; delete; mask: bitmap
    words; columns: a list of bitmap words; mask_way / column_ways: how a stream is written (tests/_foreign.py), None: as
    compress() writes it; set_pad: the streams written in a pad way carry SET pad bits (the models then see them set too)."""

    def __init__(self, name, n_words, n_rows, n_words_out, mask, columns, delete=False, mask_way=None, column_ways=None, set_pad=False):
        self.name, self.n_words, self.n_rows, self.n_words_out, self.delete = name, int(n_words), int(n_rows), int(n_words_out), bool(delete)
        self.mask = np.ascontiguousarray(mask, dtype=np.uint32)
        self.columns = [np.ascontiguousarray(c, dtype=np.uint32) for c in columns]
        assert self.mask.size == self.n_words and all(c.size == self.n_words for c in self.columns), name
        assert 0 <= self.n_rows <= 32 * self.n_words, name
        self.n_columns = len(self.columns)
        self.mask_way = mask_way
        self.column_ways = column_ways if column_ways is not None else [None] * self.n_columns
        self.set_pad = set_pad

    def selected(self):
        """The selected rows, ascending."""
        m = bits_of(self.mask)[: self.n_rows]
        return np.flatnonzero(m == (0 if self.delete else 1))

    @property
    def total_rows(self):
        return int(self.selected().size)

    def _stream(self, oracle, words, way, salt):
        if way is None or way == "canonical":
            return np.ascontiguousarray(oracle.compress(words), dtype=np.uint32)
        return _foreign.reencode(words, self.n_words, way, np.random.default_rng([salt, 5]))

    def mask_stream(self, oracle):
        return self._stream(oracle, self.mask, self.mask_way, 0)

    def column_stream(self, oracle, c):
        return self._stream(oracle, self.columns[c], self.column_ways[c], c + 1)


# ---- (a) the definition ---------------------------------------------------------------------------------------------------------
def model(case, c):
    """Column c of the output: n_words_out words (the selected rows must fit: T <= 32 * n_words_out)."""
    sel = case.selected()
    assert sel.size <= 32 * case.n_words_out, case.name
    out = np.zeros(32 * case.n_words_out, np.uint8)
    out[: sel.size] = bits_of(case.columns[c])[: case.n_rows][sel]
    return words_of(out)


# ---- (b) the call's output --------------------------------------------------------------------------------------------------------
def reference(oracle, case):
    """(stream, index, T) of the call: the columns' compress() streams back to back, n_columns * S + 1 index entries counted from
    the first word of the whole (the layout of _splice.reference), and the number of selected rows."""
    segments = _select.segments_of(case.n_words_out)
    streams, index, at = [], [], 0
    for c in range(case.n_columns):
        st = np.ascontiguousarray(oracle.compress(model(case, c)), dtype=np.uint32)
        own = _select.index_of(st)
        assert own.size == segments + 1, (own.size, segments)
        index.append(own[:-1] + at)
        streams.append(st)
        at += st.size
    index.append(np.array([at], np.int64))
    return np.concatenate(streams), np.concatenate(index).astype(np.int64), case.total_rows


# ---- (c) the kernel's arithmetic, restated ----------------------------------------------------------------------------------------
def source_image(words, n_words, seg, set_pad=False):
    """The 1024 groups list_walk leaves for segment `seg` of a source under OR into zeros: its groups, zeros behind the last
    one; set_pad: with the pad bits of the last group set, as a foreign stream may have them."""
    g = _foreign.unpack(np.asarray(words, np.uint32)[:n_words]).copy()
    if set_pad:
        g[-1] |= np.uint32(M31 ^ (M31 >> _foreign.pad_bits(n_words)))
    img = np.zeros(SEG_GROUPS, np.uint32)
    part = g[seg * SEG_GROUPS: (seg + 1) * SEG_GROUPS]
    img[: part.size] = part
    return img


def selected_groups(case, seg, wrong=None):
    """compact_selected for the 1024 groups of source segment `seg`: the mask image's groups -- under DELETE the walk is under AND
    into ones, so groups behind the bitmap's last stay ones --, complemented under DELETE, below the row limit."""
    img = source_image(case.mask, case.n_words, seg, case.set_pad and case.mask_way in _foreign.PAD_WAYS)
    valid = min(SEG_GROUPS, _select.groups_of(case.n_words) - seg * SEG_GROUPS)
    if case.delete:
        img[valid:] = M31
        img = ~img & np.uint32(M31)
    n_rows = case.n_rows
    if wrong == "pad rows selected under DELETE" and case.delete and n_rows == 32 * case.n_words:
        n_rows = 31 * _select.groups_of(case.n_words)  # the pad bits of the last group count as rows
    seg_rows = min(max(n_rows - seg * SEG_BITS, 0), SEG_BITS)
    nb = np.clip(seg_rows - 31 * np.arange(SEG_GROUPS, dtype=np.int64), 0, 31)
    return img & ((np.int64(1) << nb) - 1).astype(np.uint32)


def ranks(case, wrong=None):
    """The selected rows in front of every source segment, then T: what the rank pass and its scan leave."""
    counts = [int(np.unpackbits(selected_groups(case, s, wrong).view(np.uint8)).sum()) for s in range(_select.segments_of(case.n_words))]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def extract(x, m):
    """The bits of x at the set bits of m moved together, lowest first (PEXT)."""
    v = k = 0
    while m:
        low = m & -m
        if x & low:
            v |= 1 << k
        k += 1
        m ^= low
    return v


def arithmetic(case, c, wrong=None):
    """Column c of the case by the kernel's road (wrong: one of WRONG_MODELS, or None).  Returns the output bitmap's words."""
    assert wrong is None or wrong in WRONG_MODELS
    starts = ranks(case, wrong)
    total = int(starts[-1])
    groups = _select.groups_of(case.n_words_out)
    out = []
    for seg in range(_select.segments_of(case.n_words_out)):
        base = seg * SEG_BITS
        dst = [0] * (SEG_GROUPS + 1)
        limit = min(base + SEG_BITS, total)
        room = limit - base
        if wrong == "seam off by one" and limit == base + SEG_BITS:
            room -= 1
        for ss in range(starts.size - 1):
            st, en = int(starts[ss]), int(starts[ss + 1])
            if en <= st or en <= base or st >= limit:
                continue
            sel = selected_groups(case, ss, wrong)
            col = source_image(case.columns[c], case.n_words, ss, case.set_pad and case.column_ways[c] in _foreign.PAD_WAYS)
            cnt = np.array([bin(int(v)).count("1") for v in sel], np.int64)
            first, carry = st - base, 0
            for s0 in range(0, SEG_GROUPS, STEP):
                step_cnt = cnt[s0: s0 + STEP]
                excl = np.cumsum(step_cnt) - step_cnt
                for lane in np.flatnonzero(step_cnt):
                    g = s0 + int(lane)
                    d, n = first + carry + int(excl[lane]), int(step_cnt[lane])
                    if d >= room or d + n <= 0:
                        continue
                    v = extract(int(col[g]), int(sel[g]))
                    if d < 0:
                        v >>= -d
                        n += d
                        d = 0
                    if d + n > room:
                        n = room - d
                    v &= (1 << n) - 1
                    dg, off = divmod(d, 31)
                    dst[dg] |= (v << off) & M31
                    if off + n > 31 and wrong != "second destination group dropped":
                        dst[dg + 1] |= v >> (31 - off)
                if wrong != "carry lost between steps":
                    carry += int(step_cnt.sum())
        assert dst[SEG_GROUPS] == 0
        out.append(np.array(dst[: min(SEG_GROUPS, groups - seg * SEG_GROUPS)], np.uint32))
    return _select.pack(np.concatenate(out))[: case.n_words_out]


# ---- the bound, the scratch -----------------------------------------------------------------------------------------------------
def max_words(n_words_out, n_columns, source_words):
    g, s = _select.groups_of(n_words_out), _select.segments_of(n_words_out)
    return min(n_columns * g, n_columns * (s + 1) + 2 * source_words, (1 << 64) - 1)


def scratch_bytes(n_words, n_words_out, n_columns):
    def round256(x):
        return (x + 255) // 256 * 256

    def levels(entries):
        level1 = -(-entries // 4096)
        return round256(8 * level1) + round256(8 * -(-level1 // 4096))

    r = _select.segments_of(n_words) + 1
    return 1024 + round256(8 * r) + levels(n_columns * _select.segments_of(n_words_out) + 1) + levels(r)


def read_source_words(oracle, case):
    """The words of the column segments the call reads -- those that hold a selected row --, over all columns: what source_words
    may be set to."""
    starts = ranks(case)
    total = 0
    for c in range(case.n_columns):
        idx = _foreign.segment_ranges(case.column_stream(oracle, c))[0]
        total += sum(idx[s + 1] - idx[s] for s in range(starts.size - 1) if starts[s + 1] > starts[s])
    return total


# ---- the named cases --------------------------------------------------------------------------------------------------------------
def _columns(n_words, seed):
    """Dense, sparse and clustered."""
    return [random_words(n_words, 0.5, seed), random_words(n_words, 0.002, seed + 1), clustered_words(n_words, seed + 2)]


def _out_words(rows):
    return max(-(-((rows + 31) // 32) // SEG_WORDS), 1) * SEG_WORDS


def half(delete=False):
    return Case("one segment at density 1/2" + (", DELETE" if delete else ""), SEG_WORDS, SEG_BITS, SEG_WORDS, random_words(SEG_WORDS, 0.5, 1),
                _columns(SEG_WORDS, 2), delete)


def all_ones(delete, n_words=SEG_WORDS + 1):
    """The mask all ones: the identity, or under DELETE nothing at all."""
    return Case(f"mask of ones{', DELETE' if delete else ''}", n_words, 32 * n_words, n_words, np.full(n_words, 0xFFFFFFFF, np.uint32),
                _columns(n_words, 5), delete)


def all_zeros(delete, n_words=SEG_WORDS + 1):
    """The mask empty: T = 0, or under DELETE the identity."""
    return Case(f"mask of zeros{', DELETE' if delete else ''}", n_words, 32 * n_words, n_words, np.zeros(n_words, np.uint32), _columns(n_words, 8), delete)


ROW_LIMITS = (31 * 700 + 7, 32 * 700, 31 * 1024 + 7, 7, 1)


def row_limit(n_rows, delete):
    """n_rows in the middle of a group and of a word: what lies behind it -- set mask bits, set column bits -- is no row."""
    n = 2 * SEG_WORDS
    return Case(f"{n_rows} rows of {32 * n}{', DELETE' if delete else ''}", n, n_rows, _out_words(n_rows), random_words(n, 0.5, 11),
                [random_words(n, 0.5, 12), np.full(n, 0xFFFFFFFF, np.uint32)], delete)


def pad_rows(delete, way="pad: literal"):
    """n_rows = 32 * n_words of a ragged bitmap whose foreign streams carry SET pad bits: the pad bits are no rows.  Under DELETE
    the mask is canonical: its CLEAR pad bits are the ones that would select."""
    n = SEG_WORDS + 1
    ones = np.full(n, 0xFFFFFFFF, np.uint32)
    mask = random_words(n, 0.5, 13)
    mask[-2:] = 0 if delete else 0xFFFFFFFF
    return Case(f"set pad bits, {way}{', DELETE' if delete else ''}", n, 32 * n, n, mask, [ones, random_words(n, 0.5, 14) | np.uint32(0x80000000)], delete,
                mask_way=None if delete else "pad: literal", column_ways=[way, "pad: literal"], set_pad=True)


def no_rows(delete):
    return Case(f"n_rows = 0{', DELETE' if delete else ''}", SEG_WORDS, 0, SEG_WORDS, random_words(SEG_WORDS, 0.5, 15), _columns(SEG_WORDS, 16), delete)


@functools.lru_cache(None)
def seam():
    """Three source segments that select 31 744 + 5 rows: the second one feeds two output segments, and the row that becomes the
    first of output segment 1 lies at a multiple of neither 31 nor 32."""
    n = 3 * SEG_WORDS
    rng = np.random.default_rng(21)
    per_segment = (9000, SEG_BITS - 9000 + 2, 3)  # the rows 31 744 and 31 745 of the output come out of source segment 1
    rows = np.concatenate([s * SEG_BITS + np.sort(rng.choice(SEG_BITS, k, replace=False)) for s, k in enumerate(per_segment)])
    return Case("a seam inside a source segment", n, 32 * n, 2 * SEG_WORDS, chosen_rows(n, rows), _columns(n, 22) + [np.full(n, 0xFFFFFFFF, np.uint32)])


def exactly(total, n_words_out, name):
    """T exactly `total`, out of two source segments at density about 1/2."""
    n = 3 * SEG_WORDS
    rng = np.random.default_rng([total, n_words_out])
    rows = np.sort(rng.choice(32 * n, total, replace=False))
    return Case(name, n, 32 * n, n_words_out, chosen_rows(n, rows), [random_words(n, 0.5, 23), np.full(n, 0xFFFFFFFF, np.uint32)])


def one_segment_of_rows():
    return exactly(SEG_BITS, 2 * SEG_WORDS, "T = 31744")


def full_output():
    return exactly(32 * (SEG_WORDS + 1), SEG_WORDS + 1, "T = 32 * n_words_out")


def overfull_output():
    """One row more than the output holds: refused by the device (the models do not apply)."""
    return exactly(32 * (SEG_WORDS + 1) + 1, SEG_WORDS + 1, "T = 32 * n_words_out + 1")


@functools.lru_cache(None)
def seventy_sources():
    """One selected row in each of 70 source segments: an output segment that draws from more sources than a wavefront has lanes."""
    s = 70
    n = s * SEG_WORDS
    rows = [k * SEG_BITS + (997 * k + 13) % SEG_BITS for k in range(s)]
    col = chosen_rows(n, rows[::2] + [r + 1 for r in rows[1::2]])
    return Case("one row from each of 70 segments", n, 32 * n, SEG_WORDS, chosen_rows(n, rows), [col, np.full(n, 0xFFFFFFFF, np.uint32)])


def fill_mask_segments(delete):
    """Mask segments that are single fill words of either kind between literal ones."""
    n = 5 * SEG_WORDS
    mask = random_words(n, 0.3, 31)
    mask[SEG_WORDS: 2 * SEG_WORDS] = 0
    mask[2 * SEG_WORDS: 3 * SEG_WORDS] = 0xFFFFFFFF
    mask[4 * SEG_WORDS:] = 0xFFFFFFFF if delete else 0
    return Case(f"mask segments of one fill{', DELETE' if delete else ''}", n, 32 * n - 100, 4 * SEG_WORDS, mask, _columns(n, 32), delete)


def fill_columns():
    """Columns that are single fills under a literal mask."""
    n = 2 * SEG_WORDS
    return Case("columns of one fill", n, 32 * n, n, random_words(n, 0.4, 33), [np.zeros(n, np.uint32), np.full(n, 0xFFFFFFFF, np.uint32)])


def sparse_mask(delete):
    """A 0.1 % mask over four segments: every output group gathers from many source groups."""
    n = 4 * SEG_WORDS
    return Case(f"a sparse mask{', DELETE' if delete else ''}", n, 32 * n - 5, n if delete else SEG_WORDS, random_words(n, 0.001, 34), _columns(n, 35), delete)


def step_edges():
    """Selected rows that straddle the kernel's steps of 64 groups: the last bit of group 63, the first of group 64, and a
    column that differs exactly there -- a carry lost between steps puts them elsewhere."""
    n = SEG_WORDS
    rows = [31 * 63 + 30, 31 * 64, 31 * 64 + 1, 31 * 127 + 30, 31 * 128, 31 * 1023 + 30]
    return Case("rows at the edges of steps", n, 32 * n, n, chosen_rows(n, rows), [chosen_rows(n, rows[1::2]), chosen_rows(n, rows[::2])])


def foreign(way, n_words=2 * SEG_WORDS + 1):
    """Mask and columns re-encoded in one of the ways of tests/_foreign.py (not a pad way)."""
    rng = np.random.default_rng(41)
    mask = _foreign.bitmap(n_words, rng)
    cols = [_foreign.bitmap(n_words, np.random.default_rng(42)), _foreign.bitmap(n_words, np.random.default_rng(43), tail="ones")]
    return Case(f"foreign streams, {way}", n_words, 32 * n_words - 3, n_words, mask, cols, mask_way=way, column_ways=[way, way])


def named_cases():
    """Every case the CPU test proves and the GPU test runs."""
    out = [half(), half(True)] + [f(d) for f in (all_ones, all_zeros) for d in (False, True)]
    out += [row_limit(r, d) for r in ROW_LIMITS for d in (False, True)]
    out += [pad_rows(d) for d in (False, True)] + [pad_rows(True, w) for w in _foreign.PAD_WAYS[1:]]
    out += [no_rows(False), no_rows(True), seam(), one_segment_of_rows(), full_output(), seventy_sources()]
    out += [fill_mask_segments(False), fill_mask_segments(True), fill_columns(), sparse_mask(False), sparse_mask(True), step_edges()]
    return out


def full_grid_columns():
    """How many columns of one output segment pass the capped grid: a wavefront takes a second item."""
    return GRID_CAP * SEG_WAVES + 1
