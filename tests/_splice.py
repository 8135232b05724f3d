"""Reference, model and named cases for wah_splice_indexed_device (include/wah.h): row ranges of indexed bitmaps concatenated
into new indexed bitmaps.  No GPU, no library: tests/test_splice_reference.py proves everything here on the CPU,
tests/test_gpu_splice.py holds the kernels against the reference.

Three statements of one thing:
  model()        the concatenation bit by bit in numpy: the definition;
  reference()    the model, compressed per column by the oracle and indexed by _select.index_of, laid out as _rows.reference;
  group_move()   what splice_segments_kernel does, restated: per output segment a destination image of 1024 groups, per piece
                 and source segment a source image, and destination group d taking
                 ((S[d + q] >> r) | (S[d + q + 1] << (31 - r))) & 0x7FFFFFFF under the mask of the bits the source range covers.
A Case names the pieces, the source bitmaps of every (piece, column), and optionally the way (tests/_foreign.py) a source's
stream is written in."""
import functools
import os

import numpy as np

from tests import _foreign, _grid, _select

SEG_GROUPS, SEG_WORDS, SEG_BITS = _select.SEG_GROUPS, _select.SEG_WORDS, _select.SEG_BITS
M31 = 0x7FFFFFFF
FILL0, FILL1 = 0x80000000, 0xC0000000
MAX_PIECES = 1 << 16
SEG_WAVES = 4  # WAH_SEG_WAVES: the wavefronts of a workgroup of splice_segments_kernel, one item each
KINDS = ("dense", "sparse", "clustered", "ones")


# ---- bitmaps ------------------------------------------------------------------------------------------------------------------
def source(kind, n_words, seed):
    """n_words bitmap words of one of the four kinds."""
    rng = np.random.default_rng([KINDS.index(kind), n_words, seed])
    if kind == "ones":
        return np.full(n_words, 0xFFFFFFFF, np.uint32)
    if kind == "dense":
        return rng.integers(0, 1 << 32, n_words, dtype=np.uint64).astype(np.uint32)
    bits = np.zeros(32 * n_words, np.uint8)
    if kind == "sparse":
        bits[rng.integers(0, bits.size, max(bits.size // 700, 1))] = 1
    else:  # clustered: runs of either kind, a few bits to a few groups long
        at, v = 0, int(rng.integers(0, 2))
        while at < bits.size:
            n = int(rng.integers(1, 400))
            bits[at: at + n] = v
            at, v = at + n, 1 - v
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def bits_of(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")


def words_of(bits):
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


# ---- the definition -----------------------------------------------------------------------------------------------------------
def model(pieces, n_words_out):
    """pieces: [(bitmap words or None, first_row, n_rows)] of ONE column.  The output bitmap's n_words_out words."""
    out = np.zeros(32 * n_words_out, np.uint8)
    at = 0
    for words, first, n in pieces:
        if n:
            out[at: at + n] = bits_of(words)[first: first + n]
            at += n
    return words_of(out)


class Case:
    """name; n_words_out; pieces [(n_words, first_row, n_rows)]; sources[p][c]: the bitmap of (piece p, column c) or None (a
    piece of no rows); ways[p][c]: how its stream is written (tests/_foreign.py), None: as compress() writes it."""

    def __init__(self, name, n_words_out, pieces, sources, ways=None):
        self.name, self.n_words_out = name, int(n_words_out)
        self.pieces = [tuple(int(v) for v in p) for p in pieces]
        self.sources = sources
        self.n_columns = len(sources[0])
        assert all(len(row) == self.n_columns for row in sources) and len(sources) == len(self.pieces), name
        self.ways = ways if ways is not None else [[None] * self.n_columns for _ in self.pieces]

    @property
    def total_rows(self):
        return sum(p[2] for p in self.pieces)

    def column(self, c):
        return [(self.sources[p][c], first, n) for p, (_, first, n) in enumerate(self.pieces)]

    def stream_of(self, oracle, p, c):
        """The stream operand (p, c) is handed to the call as."""
        words, way = self.sources[p][c], self.ways[p][c]
        if way is None or way == "canonical":
            return np.ascontiguousarray(oracle.compress(words), dtype=np.uint32)
        return _foreign.reencode(words, self.pieces[p][0], way, np.random.default_rng([p, c, 5]))


def reference(oracle, case):
    """(stream, index) of the call: the columns' compress() streams back to back, and n_columns * S + 1 index entries counted
    from the first word of the whole (the layout of _rows.reference)."""
    segments = _select.segments_of(case.n_words_out)
    streams, index, at = [], [], 0
    for c in range(case.n_columns):
        st = np.ascontiguousarray(oracle.compress(model(case.column(c), case.n_words_out)), dtype=np.uint32)
        own = _select.index_of(st)
        assert own.size == segments + 1, (own.size, segments)
        index.append(own[:-1] + at)
        streams.append(st)
        at += st.size
    index.append(np.array([at], np.int64))
    return np.concatenate(streams), np.concatenate(index).astype(np.int64)


# ---- the kernel's group move, restated ------------------------------------------------------------------------------------------
def source_image(words, n_words, seg, set_pad=False):
    """The 1024 groups list_walk leaves for segment `seg` of a source: its groups, zeros behind the last one; set_pad: with the
    pad bits of the last group set, as a foreign stream may have them."""
    g = _foreign.unpack(np.asarray(words, np.uint32)[:n_words]).copy()
    if set_pad:
        g[-1] |= np.uint32(M31 ^ (M31 >> _foreign.pad_bits(n_words)))
    img = np.zeros(SEG_GROUPS, np.uint32)
    part = g[seg * SEG_GROUPS: (seg + 1) * SEG_GROUPS]
    img[: part.size] = part
    return img


def move(src, dst, sb, db, length):
    """splice_move: `length` bits of image src from bit sb on ORed into image dst from bit db on.  Returns (q, r)."""
    delta = sb - db
    q = delta // 31 if delta >= 0 else -((30 - delta) // 31)
    r = delta - 31 * q
    assert 0 <= r < 31 and q == delta // 31
    d = np.arange(SEG_GROUPS, dtype=np.int64)
    padded = np.concatenate([np.zeros(SEG_GROUPS + 1, np.uint64), src.astype(np.uint64), np.zeros(SEG_GROUPS + 2, np.uint64)])
    x, y = padded[d + q + SEG_GROUPS + 1], padded[d + q + SEG_GROUPS + 2]
    v = ((x >> np.uint64(r)) | (y << np.uint64(31 - r))) & np.uint64(M31)
    lo, hi = np.clip(db - 31 * d, 0, 31), np.clip(db + length - 31 * d, 0, 31)
    mask = np.where(hi > lo, ((np.int64(1) << hi) - 1) & ~((np.int64(1) << lo) - 1), 0).astype(np.uint64)
    dst |= (v & mask).astype(np.uint32)
    return q, r


def group_move(case, c, set_pad=False, trace=None):
    """Column c of the case by the kernel's road.  trace: a list that receives one (output segment, piece, source segment, q, r)
    per move.  Returns the output bitmap's words."""
    starts = np.concatenate([[0], np.cumsum([p[2] for p in case.pieces])])
    total = int(starts[-1])
    groups = _select.groups_of(case.n_words_out)
    out = []
    for seg in range(_select.segments_of(case.n_words_out)):
        base = seg * SEG_BITS
        dst = np.zeros(SEG_GROUPS, np.uint32)
        limit = min(base + SEG_BITS, total)
        for p, (n_words, first, n) in enumerate(case.pieces):
            st, en = int(starts[p]), int(starts[p + 1])
            if n == 0 or en <= base or st >= limit:
                continue
            d0, d1 = max(st, base), min(en, limit)
            s0 = first + d0 - st
            s1 = s0 + d1 - d0
            ss = s0 // SEG_BITS
            while ss * SEG_BITS < s1:
                t0, t1 = max(s0, ss * SEG_BITS), min(s1, (ss + 1) * SEG_BITS)
                src = source_image(case.sources[p][c], n_words, ss, set_pad)
                q, r = move(src, dst, t0 - ss * SEG_BITS, d0 + t0 - s0 - base, t1 - t0)
                if trace is not None:
                    trace.append((seg, p, ss, q, r))
                ss += 1
        out.append(dst[: min(SEG_GROUPS, groups - seg * SEG_GROUPS)])
    return _select.pack(np.concatenate(out))[: case.n_words_out]


# ---- the bound, the scratch, the grid -------------------------------------------------------------------------------------------
def max_words(n_words_out, n_columns, n_pieces, source_words):
    g, s = _select.groups_of(n_words_out), _select.segments_of(n_words_out)
    return min(n_columns * g, n_columns * (s + 1) + 2 * n_pieces * n_columns + 2 * source_words, (1 << 64) - 1)


def scratch_bytes(n_words_out, n_columns, n_pieces):
    def round256(x):
        return (x + 255) // 256 * 256

    entries = n_columns * _select.segments_of(n_words_out) + 1
    level1 = -(-entries // 4096)
    level2 = -(-level1 // 4096)
    return 1024 + round256(8 * (n_pieces + 1)) + round256(8 * level1) + round256(8 * level2)


def touched_source_words(oracle, case):
    """The words of the source segments the call reads, over all (piece, column): what source_words may be set to."""
    total = 0
    for p, (n_words, first, n) in enumerate(case.pieces):
        if n == 0:
            continue
        for c in range(case.n_columns):
            st = case.stream_of(oracle, p, c)
            idx = _foreign.segment_ranges(st)[0]
            for ss in range(first // SEG_BITS, (first + n - 1) // SEG_BITS + 1):
                total += idx[ss + 1] - idx[ss]
    return total


def met_source_words(oracle, case):
    """The source words whose groups hold a spliced row, over all (piece, column): a tighter count than the touched segments',
    and the one the argument for the bound charges (include/wah.h)."""
    total = 0
    for p, (n_words, first, n) in enumerate(case.pieces):
        if n == 0:
            continue
        for c in range(case.n_columns):
            _, _, cnt, start = _select._walk(case.stream_of(oracle, p, c))
            total += int(np.count_nonzero((31 * start < first + n) & (31 * (start + cnt) > first)))
    return total


def grid_cap():
    """Workgroups of splice_segments_kernel at the most, read out of the source as _grid._most reads the others."""
    return _grid._most(os.path.join(_grid.CSRC, "wah_splice.hip"), "launch_splice_segments")


# ---- the named cases --------------------------------------------------------------------------------------------------------------
def _columns(n_words, seed, kinds=KINDS):
    return [source(k, n_words, seed + i) for i, k in enumerate(kinds)]


def identity(n_words, way=None):
    srcs = _columns(n_words, 1)
    ways = None
    if way is not None:
        ways = [[way if way not in _foreign.PAD_WAYS[1:] or kind == "ones" else "pad: literal" for kind in KINDS]]
    return Case(f"identity {n_words} words" + (f", {way}" if way else ""), n_words, [(n_words, 0, 32 * n_words)], [srcs], ways)


IDENTITY_WORDS = (992, 1984, 993, 1)
SHIFTS = (0, 1, 30, 31, 32, 61, 62, 31743)
FRONTS = (1, 30, 31, 32)


def shift(f):
    return Case(f"shift {f}", SEG_WORDS, [(2 * SEG_WORDS, f, SEG_BITS)], [_columns(2 * SEG_WORDS, 2)])


def front(b):
    """A first piece of b rows in front of a second one that starts at its row 0: a negative delta."""
    return Case(f"front {b}", SEG_WORDS, [(31, 7, b), (SEG_WORDS, 0, SEG_BITS - b)], [_columns(31, 3), _columns(SEG_WORDS, 4)])


def one_row_pieces():
    """65 pieces of one row each, from 65 sources: more pieces in one output segment than a wavefront has lanes."""
    n = 65
    pieces = [(1 + p % 3, (5 * p) % 32, 1) for p in range(n)]
    return Case("65 pieces of one row", 3, pieces, [_columns(1 + p % 3, 10 + p) for p in range(n)])


def short_pieces():
    pieces = [(31, 3, 30), (31, 40, 31), (31, 100, 32), (31, 0, 30), (31, 31, 31), (31, 62, 32)]
    return Case("pieces of 30, 31 and 32 rows", 31, pieces, [_columns(31, 20 + p) for p in range(len(pieces))])


def edge_pieces():
    """A piece that ends exactly on an output segment edge, the next one beginning there."""
    pieces = [(SEG_WORDS, 0, SEG_BITS), (SEG_WORDS, 17, 5000)]
    return Case("a piece ending on a segment edge", 2 * SEG_WORDS, pieces, [_columns(SEG_WORDS, 30), _columns(SEG_WORDS, 31)])


def straddle():
    """The second piece crosses the output's segment edge (its row 30 744) and its source's segment edge (its row 11 744)."""
    pieces = [(SEG_WORDS, 5, 1000), (2 * SEG_WORDS, 20000, 40000)]
    return Case("a piece across an output edge and a source edge", 2 * SEG_WORDS, pieces, [_columns(SEG_WORDS, 32), _columns(2 * SEG_WORDS, 33)])


def _ones(n_words):
    return [np.full(n_words, 0xFFFFFFFF, np.uint32)]


def ones_one_fill():
    return Case("two runs of ones: one fill", SEG_WORDS, [(31, 0, 100), (SEG_WORDS, 3, SEG_BITS - 100)], [_ones(31), _ones(SEG_WORDS)])


def ones_two_fills():
    return Case("ones across a segment edge: two fills", 2 * SEG_WORDS, [(31, 0, 100), (2 * SEG_WORDS, 3, 2 * SEG_BITS - 100)],
                [_ones(31), _ones(2 * SEG_WORDS)])


def ones_literal():
    return Case("ones ending inside a group", SEG_WORDS, [(31, 0, 100), (SEG_WORDS, 3, 1000)], [_ones(31), _ones(SEG_WORDS)])


def ragged_sources():
    """The last real row of sources of 1, 31 and 993 words."""
    pieces = [(1, 20, 12), (31, 900, 92), (993, 31000, 32 * 993 - 31000)]
    return Case("the last rows of ragged sources", 993, pieces, [_columns(1, 40), _columns(31, 41), _columns(993, 42)])


def ragged_out(n_words_out):
    rows = min(32 * n_words_out, 700)
    return Case(f"{n_words_out} words out", n_words_out, [(31, 5, rows // 2), (993, 31000, rows - rows // 2)], [_columns(31, 43), _columns(993, 44)])


def full_out():
    """T == 32 * n_words_out exactly, in a ragged output: the pad bits behind it stay clear."""
    return Case("T fills a ragged output", 993, [(31, 0, 32), (2 * SEG_WORDS, 31, 32 * 992)], [_ones(31) + _columns(31, 45), _ones(2 * SEG_WORDS) + _columns(2 * SEG_WORDS, 46)])


def empty():
    """T == 0: every piece empty, every operand null."""
    return Case("no rows at all", 993, [(0, 0, 0), (5, 99999, 0)], [[None, None], [None, None]])


def pad_tail(way="pad: literal"):
    """A foreign source with SET pad bits whose last rows are followed by the zero tail."""
    srcs = [np.full(993, 0xFFFFFFFF, np.uint32), source("dense", 993, 47) | np.uint32(0x80000000)]
    return Case(f"set pad bits in front of the tail, {way}", SEG_WORDS, [(993, 32 * 993 - 500, 500)], [srcs],
                [[way, "pad: literal"]])


def transposable():
    """Three columns, two pieces, six different sources."""
    pieces = [(SEG_WORDS, 100, 3000), (SEG_WORDS, 1, 900)]
    return Case("3 columns x 2 pieces", SEG_WORDS, pieces, [_columns(SEG_WORDS, 50, KINDS[:3]), _columns(SEG_WORDS, 53, KINDS[:3])])


def second_workgroup():
    """S = WAH_SEG_WAVES + 1 output segments of one column: a second workgroup."""
    s = SEG_WAVES + 1
    pieces = [(s * SEG_WORDS, 11, s * SEG_BITS - 11 - 1000), (31, 0, 900)]
    return Case("one more segment than a workgroup has waves", s * SEG_WORDS, pieces, [[source("clustered", s * SEG_WORDS, 60)], [source("dense", 31, 61)]])


@functools.lru_cache(None)
def full_grid():
    """cap * 4 + 1 one-segment columns over sparse sources: a wavefront takes a second item."""
    k = grid_cap() * SEG_WAVES + 1
    rng = np.random.default_rng(70)
    srcs = []
    for c in range(k):
        bits = rng.integers(0, SEG_BITS, 1 + c % 3)
        srcs.append(_select.bitmap_of(bits, SEG_WORDS))
    return Case("a second item per wavefront", SEG_WORDS, [(SEG_WORDS, 3, SEG_BITS - 3)], [srcs])


def doubled_literals():
    """Isolated literals with bits 0 and 30 set, shifted by one: every literal becomes two, and 2 * source_words is needed."""
    g = np.zeros(SEG_GROUPS, np.uint32)
    g[1::8] = (1 << 30) | 1
    return Case("every literal becomes two", SEG_WORDS, [(SEG_WORDS, 1, SEG_BITS - 1)], [[_select.pack(g)]])


def all_literals():
    """Dense sources: the n_columns * G arm of the bound is the smaller one."""
    return Case("dense: the groups bound", SEG_WORDS, [(SEG_WORDS, 9, SEG_BITS - 9)], [[source("dense", SEG_WORDS, 80), source("dense", SEG_WORDS, 81)]])


def named_cases():
    """Every case the CPU test proves and the GPU test runs (the identity cases in their foreign ways are the GPU test's own)."""
    out = [identity(n) for n in IDENTITY_WORDS] + [shift(f) for f in SHIFTS] + [front(b) for b in FRONTS]
    out += [one_row_pieces(), short_pieces(), edge_pieces(), straddle(), ones_one_fill(), ones_two_fills(), ones_literal(), ragged_sources()]
    out += [ragged_out(n) for n in (1, 993, 1000)] + [full_out(), empty(), pad_tail(), transposable(), second_workgroup(), doubled_literals(), all_literals()]
    return out
