"""Reference, model and named cases for wah_update_indexed_device (include/wah.h): per column the blend of two indexed bitmaps
under a mask bitmap -- then_c where the mask selects a row below n_rows, else_c everywhere else -- as new indexed bitmaps.  No GPU,
no library: tests/test_update_reference.py proves everything here on the CPU, tests/test_gpu_update.py holds the kernels against
the reference.

Three statements of one thing:
  model()      bit by bit on unpacked bits: where(mask & (p < n_rows), then, else) -- the definition;
  reference()  the model, compressed per column by the oracle and indexed by _select.index_of, laid out as _compact.reference;
  arithmetic() what update_segments_kernel does, restated: per segment the mask's image of 1024 groups clipped to the rows below
               n_rows, the else entry's image (a constant: the image filled), where the clipped mask selects a row the then
               entry's image, the blend (dst & ~sel) | (then & sel) group by group, and the pad bits of the last group cleared.
               It returns GROUPS, pad bits and all: what a word array cannot show.
arithmetic() takes the name of a WRONG model too: each one changes an answer on a named case (WRONG_MODELS).
A side of a case holds per column the bitmap's words or the int 0 or 1, a constant; a way (tests/_foreign.py) says how a stream is
written, None: as compress() writes it.  A stream written in a pad way carries SET pad bits."""
import numpy as np

from tests import _foreign, _select
from tests._compact import bits_of, chosen_rows, clustered_words, random_words, words_of

SEG_GROUPS, SEG_WORDS, SEG_BITS = _select.SEG_GROUPS, _select.SEG_WORDS, _select.SEG_BITS
M31 = 0x7FFFFFFF
FILL0, FILL1 = 0x80000000, 0xC0000000
ONES = 0xFFFFFFFF
SEG_WAVES = 4       # WAH_SEG_WAVES: the wavefronts of a workgroup of update_segments_kernel
GRID_CAP = 256 * 3  # workgroups of update_segments_kernel at the most (launch_update_segments: 48 KiB of LDS each)
WRONG_MODELS = ("rows at or behind n_rows updated", "pad bits carried", "constant ones written outside the mask",
                "then and else swapped where the mask segment is a fill")


class Case:
    """name; n_words, n_rows; mask: bitmap words; else_ / then: per column bitmap words or the constant 0 or 1; mask_way /
    else_ways / then_ways: how a stream is written (tests/_foreign.py), None: as compress() writes it."""

    def __init__(self, name, n_words, n_rows, mask, else_, then, mask_way=None, else_ways=None, then_ways=None):
        self.name, self.n_words, self.n_rows = name, int(n_words), int(n_rows)
        self.mask = np.ascontiguousarray(mask, dtype=np.uint32)
        self.sides = {"else": [self._entry(e) for e in else_], "then": [self._entry(e) for e in then]}
        self.n_columns = len(else_)
        assert len(then) == self.n_columns and self.n_columns >= 1 and self.mask.size == self.n_words, name
        assert 0 <= self.n_rows <= 32 * self.n_words, name
        self.mask_way = mask_way
        self.ways = {"else": else_ways or [None] * self.n_columns, "then": then_ways or [None] * self.n_columns}

    def _entry(self, e):
        if isinstance(e, (int, np.integer)):
            assert e in (0, 1)
            return int(e)
        e = np.ascontiguousarray(e, dtype=np.uint32)
        assert e.size == self.n_words
        return e

    def constant(self, side, c):
        """The constant's bit, or None for a stream."""
        e = self.sides[side][c]
        return e if isinstance(e, int) else None

    def words(self, side, c):
        """The entry's bitmap words, a constant's written out."""
        e = self.sides[side][c]
        return np.full(self.n_words, ONES if e else 0, np.uint32) if isinstance(e, int) else e

    def _stream(self, oracle, words, way, salt):
        if way is None or way == "canonical":
            return np.ascontiguousarray(oracle.compress(words), dtype=np.uint32)
        return _foreign.reencode(words, self.n_words, way, np.random.default_rng([salt, 5]))

    def mask_stream(self, oracle):
        return self._stream(oracle, self.mask, self.mask_way, 0)

    def stream(self, oracle, side, c):
        """The entry's stream; None for a constant."""
        if self.constant(side, c) is not None:
            return None
        return self._stream(oracle, self.sides[side][c], self.ways[side][c], 2 * c + 1 + (side == "then"))

    def selection(self):
        """The mask's bits below n_rows, zeros behind them."""
        m = bits_of(self.mask).copy()
        m[self.n_rows:] = 0
        return m


# ---- (a) the definition ---------------------------------------------------------------------------------------------------------
def model(case, c):
    """Column c of the output as bitmap words."""
    return words_of(np.where(case.selection() == 1, bits_of(case.words("then", c)), bits_of(case.words("else", c))).astype(np.uint8))


# ---- (b) the call's output --------------------------------------------------------------------------------------------------------
def reference(oracle, case):
    """(stream, index) of the call: the columns' compress() streams back to back and n_columns * S + 1 index entries counted from
    the first word of the whole."""
    segments = _select.segments_of(case.n_words)
    streams, index, at = [], [], 0
    for c in range(case.n_columns):
        st = np.ascontiguousarray(oracle.compress(model(case, c)), dtype=np.uint32)
        own = _select.index_of(st)
        assert own.size == segments + 1, (own.size, segments)
        index.append(own[:-1] + at)
        streams.append(st)
        at += st.size
    index.append(np.array([at], np.int64))
    return np.concatenate(streams), np.concatenate(index).astype(np.int64)


# ---- (c) the kernel's arithmetic, restated ----------------------------------------------------------------------------------------
def source_image(words, n_words, seg, set_pad):
    """The 1024 groups list_walk leaves for segment `seg` of a source under OR into zeros: its groups, zeros behind the last one;
    set_pad: with the pad bits of the last group set, as a stream written in a pad way has them."""
    g = _foreign.unpack(np.asarray(words, np.uint32)[:n_words]).copy()
    if set_pad:
        g[-1] |= np.uint32(M31 ^ (M31 >> _foreign.pad_bits(n_words)))
    img = np.zeros(SEG_GROUPS, np.uint32)
    part = g[seg * SEG_GROUPS: (seg + 1) * SEG_GROUPS]
    img[: part.size] = part
    return img


def entry_image(case, side, c, seg):
    """The image of an else or a then entry: a stream's groups, or all 1024 groups filled with the constant."""
    k = case.constant(side, c)
    if k is not None:
        return np.full(SEG_GROUPS, M31 if k else 0, np.uint32)
    return source_image(case.sides[side][c], case.n_words, seg, case.ways[side][c] in _foreign.PAD_WAYS)


def row_bits(n_rows, seg):
    """group_row_bits (wah_device.hpp) for the 1024 groups of segment `seg`: the bits of every group that are rows."""
    seg_rows = min(max(n_rows - seg * SEG_BITS, 0), SEG_BITS)
    nb = np.clip(seg_rows - 31 * np.arange(SEG_GROUPS, dtype=np.int64), 0, 31)
    return ((np.int64(1) << nb) - 1).astype(np.uint32)


def clipped_mask(case, seg, wrong=None):
    img = source_image(case.mask, case.n_words, seg, case.mask_way in _foreign.PAD_WAYS)
    return img if wrong == "rows at or behind n_rows updated" else img & row_bits(case.n_rows, seg)


def selecting_segments(case):
    """The segments in which the clipped mask selects a row: where a then entry is read."""
    return [s for s in range(_select.segments_of(case.n_words)) if clipped_mask(case, s).any()]


def arithmetic(case, c, wrong=None):
    """Column c of the case by the kernel's road (wrong: one of WRONG_MODELS, or None).  Returns the output bitmap's GROUPS."""
    assert wrong is None or wrong in WRONG_MODELS
    groups = _select.groups_of(case.n_words)
    last_bits = 32 * case.n_words - 31 * (groups - 1)
    out = []
    for seg in range(_select.segments_of(case.n_words)):
        valid = min(SEG_GROUPS, groups - seg * SEG_GROUPS)
        sel = clipped_mask(case, seg, wrong)
        dst = entry_image(case, "else", c, seg)
        if sel.any() or wrong is not None:
            then = entry_image(case, "then", c, seg)
            raw = source_image(case.mask, case.n_words, seg, False)[:valid]
            if wrong == "then and else swapped where the mask segment is a fill" and (not raw.any() or (raw == M31).all()):
                dst, then = then, dst
            if wrong == "constant ones written outside the mask" and case.constant("then", c) == 1 and sel.any():
                dst = dst | then
            else:
                dst = (dst & ~sel) | (then & sel)
        dst = dst[:valid].copy()
        if seg + 1 == _select.segments_of(case.n_words) and wrong != "pad bits carried":
            dst[-1] &= np.uint32((1 << last_bits) - 1)
        out.append(dst)
    return np.concatenate(out)


def model_groups(case, c):
    """The model's column c as groups, the pad bits zero: what arithmetic() must return."""
    return _foreign.unpack(model(case, c))


# ---- the bound, the scratch -----------------------------------------------------------------------------------------------------
def max_words(n_words, n_columns, mask_words, source_words):
    return min(n_columns * _select.groups_of(n_words), source_words + n_columns * (mask_words + 3), (1 << 64) - 1)


def scratch_bytes(n_words, n_columns):
    def round256(x):
        return (x + 255) // 256 * 256

    level1 = -(-(n_columns * _select.segments_of(n_words) + 1) // 4096)
    return 1024 + round256(8 * level1) + round256(8 * -(-level1 // 4096))


def read_words(oracle, case):
    """(mask_words, source_words) of what the call reads: the mask's stream; every else stream whole and of every then stream the
    segments in which the clipped mask selects a row, constants nothing."""
    selecting = selecting_segments(case)
    total = 0
    for c in range(case.n_columns):
        st = case.stream(oracle, "else", c)
        total += 0 if st is None else st.size
        st = case.stream(oracle, "then", c)
        if st is not None:
            idx = _foreign.segment_ranges(st)[0]
            total += sum(idx[s + 1] - idx[s] for s in selecting)
    return int(case.mask_stream(oracle).size), int(total)


# ---- the named cases --------------------------------------------------------------------------------------------------------------
def _columns(n_words, seed):
    """Dense, sparse and clustered."""
    return [random_words(n_words, 0.5, seed), random_words(n_words, 0.002, seed + 1), clustered_words(n_words, seed + 2)]


ROW_LIMITS = (0, 1, 7, 31 * 700 + 7, 32 * 700, 31744, 31745)


def row_limit(n_rows, n_words=2 * SEG_WORDS):
    """n_rows in the middle of a group and of a word, at a segment's edge and one behind it: the mask and both sides hold set bits
    behind it."""
    n_rows = 32 * n_words if n_rows is None else n_rows
    return Case(f"{n_rows} rows of {32 * n_words}", n_words, n_rows, random_words(n_words, 0.5, 11),
                [random_words(n_words, 0.5, 12), np.zeros(n_words, np.uint32), np.full(n_words, ONES, np.uint32)],
                [random_words(n_words, 0.5, 13), np.full(n_words, ONES, np.uint32), np.zeros(n_words, np.uint32)])


def mask_of_zeros(n_words=SEG_WORDS + 1):
    """Nothing is selected: the result is compress() of the else columns, and no then entry is read."""
    return Case("mask of zeros", n_words, 32 * n_words, np.zeros(n_words, np.uint32), _columns(n_words, 21), _columns(n_words, 24))


def mask_of_ones(n_words=SEG_WORDS + 1):
    return Case("mask of ones", n_words, 32 * n_words, np.full(n_words, ONES, np.uint32), _columns(n_words, 27), _columns(n_words, 30))


def fill_mask_segments():
    """Every mask segment one fill word: zeros, ones, zeros; rows end inside the segment of ones."""
    n = 3 * SEG_WORDS
    mask = np.zeros(n, np.uint32)
    mask[SEG_WORDS: 2 * SEG_WORDS] = ONES
    return Case("mask segments of one fill", n, 2 * SEG_BITS - 100, mask, _columns(n, 33), _columns(n, 36))


def seam_rows():
    """Single selected rows on the seams of groups, of the kernel's steps of 64 groups (lanes 63 / 0) and of segments, the sides
    differing exactly there."""
    n = 2 * SEG_WORDS + 1
    rows = [0, 30, 31, 61, 62, 31 * 63 + 30, 31 * 64, 31 * 127 + 30, 31 * 128, SEG_BITS - 1, SEG_BITS, 2 * SEG_BITS - 1, 2 * SEG_BITS, 32 * n - 1]
    return Case("single rows on seams", n, 32 * n, chosen_rows(n, rows),
                [chosen_rows(n, rows[1::2]), np.zeros(n, np.uint32), random_words(n, 0.5, 41)],
                [chosen_rows(n, rows[::2]), np.full(n, ONES, np.uint32), random_words(n, 0.5, 42)])


def constants(name, n_words=SEG_WORDS + 1, n_rows=None, density=0.3):
    """then: constants on the then side; else: on the else side; both: on both, every pairing."""
    n_rows = 32 * n_words - 3 if n_rows is None else n_rows
    cols = _columns(n_words, 45)
    else_, then = {"then": (cols + cols[:1], [0, 1, 1, 0]), "else": ([0, 1, 1, 0], cols + cols[:1]), "both": ([0, 0, 1, 1], [0, 1, 0, 1])}[name]
    return Case(f"constants: {name}", n_words, n_rows, random_words(n_words, density, 44), else_, then)


def same_operand():
    """One operand given as else and as then: the column comes out as compress() of it, whatever the mask."""
    n = 2 * SEG_WORDS
    cols = _columns(n, 51)
    return Case("the same operand on both sides", n, 32 * n - 40, random_words(n, 0.5, 50), cols, cols)


def sparse_mask():
    """A 0.1 % mask over three segments, one of which it leaves out."""
    n = 3 * SEG_WORDS
    mask = random_words(n, 0.001, 55)
    mask[SEG_WORDS: 2 * SEG_WORDS] = 0
    return Case("a sparse mask", n, 32 * n - 5, mask, _columns(n, 56), _columns(n, 59))


def foreign(way, who, n_words=2 * SEG_WORDS + 1):
    """The mask, the else or the then operand (who) re-encoded in one of the ways of tests/_foreign.py (not a pad way)."""
    mask = _foreign.bitmap(n_words, np.random.default_rng(61))
    else_ = [_foreign.bitmap(n_words, np.random.default_rng(62)), _foreign.bitmap(n_words, np.random.default_rng(63), tail="ones")]
    then = [_foreign.bitmap(n_words, np.random.default_rng(64), tail="random"), _foreign.bitmap(n_words, np.random.default_rng(65))]
    ways = {"mask_way": way} if who == "mask" else {f"{who}_ways": [way, way]}
    return Case(f"foreign {who}, {way}", n_words, 32 * n_words - 3, mask, else_, then, **ways)


def set_pad_bits(way="pad: literal"):
    """A ragged bitmap whose streams carry SET pad bits on every side: the output's pad bits are zero."""
    n = SEG_WORDS + 1
    ones = np.full(n, ONES, np.uint32)
    mask = random_words(n, 0.5, 71)
    mask[-2:] = ONES
    return Case(f"set pad bits, {way}", n, 32 * n, mask, [ones, random_words(n, 0.5, 72) | np.uint32(0x80000000)],
                [random_words(n, 0.5, 73) | np.uint32(0x80000000), ones], mask_way=way, else_ways=[way, "pad: literal"], then_ways=["pad: literal", way])


def foreign_cases():
    return [foreign(way, who) for who in ("mask", "else", "then") for way in _foreign.WAYS[1:]]


def named_cases():
    """Every case the CPU test proves and the GPU test runs."""
    out = [row_limit(r) for r in ROW_LIMITS + (None,)] + [row_limit(None, SEG_WORDS + 1), row_limit(7, 3 * SEG_WORDS)]
    out += [mask_of_zeros(), mask_of_ones(), fill_mask_segments(), seam_rows(), sparse_mask(), same_operand()]
    out += [constants(name) for name in ("then", "else", "both")] + [constants("both", 2 * SEG_WORDS, 32 * 700)]
    out += [set_pad_bits(way) for way in _foreign.PAD_WAYS]
    return out


def full_grid_columns():
    """How many columns of one segment pass the capped grid: a wavefront takes a second item."""
    return GRID_CAP * SEG_WAVES + 1
