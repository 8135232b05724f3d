"""A segment-sparse model of bitmaps that are too long to exist decoded, and exact references of the indexed calls on it
(include/wah.h).  No GPU, no library: tests/test_long_reference.py proves every reference here against the dense numpy models of
the other helper modules on bitmaps of at most 40 segments; tests/test_gpu_long_bitmaps.py holds the kernels against them at sizes
where row numbers, group numbers, word offsets, ranks and counts pass 2^31, 2^32 and 2^36.

A LongBitmap is n_segments segments (1 segment = 992 words = 1024 groups = 31 744 rows).  Every segment has a DEFAULT, all zero or
all one, given as a few runs of segments; a small dict of LIVE segments holds 992 decoded words each and overrides the default.
Nothing here ever makes an array of rows or words of the whole bitmap: per-segment arrays (one entry a segment, a few MB) are the
largest things built, everything that counts is a Python int or int64 / uint64."""
import functools

import numpy as np

from tests import _select as sel

FILL, ONE = sel.FILL, sel.ONE
SEG_WORDS, SEG_GROUPS, SEG_BITS = sel.SEG_WORDS, sel.SEG_GROUPS, sel.SEG_BITS
U64_MAX = (1 << 64) - 1
ASCENDING, DESCENDING, QUANTILE = 0, 1, 2

# the two sizes of the GPU tests
A_SEGMENTS = 135_400              # 4.298e9 rows: rows 2^31 and 2^32 exist
B_SEGMENTS = 4_330_000            # words and groups pass 2^32, rows pass 2^36
A_NAMED = (0, 67_649, 67_650, 67_651, 135_299, 135_300, 135_301, 135_399)
B_NAMED = (0, 1, 4_194_303, 4_194_304, 4_329_603, 4_329_604, 4_329_998, 4_329_999)
A_ROWS = (0, 2**31 - 1, 2**31, 2**32 - 1, 2**32, A_SEGMENTS * SEG_BITS - 1)   # rows every size-A operand of `marked` sets


def _bits(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")


def _words(bits):
    return np.packbits(np.ascontiguousarray(bits, dtype=np.uint8), bitorder="little").view("<u4").astype(np.uint32)


class LongBitmap:
    """n_segments segments, the last one of last_words <= 992 words (a ragged last segment has to be live; the bits behind its
    words are zero).  default: 0, 1, or (starts, bits): segment runs, run i from segment starts[i] (starts[0] == 0, ascending)
    with bit bits[i].  live: segment -> np.uint32[992]."""

    def __init__(self, n_segments, default=0, live=None, last_words=SEG_WORDS):
        self.n_segments, self.last_words = int(n_segments), int(last_words)
        assert self.n_segments >= 1 and 1 <= self.last_words <= SEG_WORDS
        starts, bits = ([0], [default]) if np.isscalar(default) else default
        self.starts, self.bits = np.asarray(starts, dtype=np.int64), np.asarray(bits, dtype=np.uint8)
        assert self.starts[0] == 0 and np.all(np.diff(self.starts) > 0) and self.starts[-1] < self.n_segments and self.bits.max() <= 1
        self.live = {}
        for s, w in sorted((live or {}).items()):
            w = np.ascontiguousarray(w, dtype=np.uint32)
            assert 0 <= s < self.n_segments and w.shape == (SEG_WORDS,)
            self.live[int(s)] = w
        if self.last_words < SEG_WORDS:
            last = self.live.get(self.n_segments - 1)
            assert last is not None and not last[self.last_words:].any(), "a ragged last segment is live and zero behind its words"

    # ---- sizes
    @property
    def n_words(self):
        return (self.n_segments - 1) * SEG_WORDS + self.last_words

    @property
    def n_bits(self):
        return 32 * self.n_words

    # ---- the parts
    def default_of(self, segments):
        return self.bits[np.searchsorted(self.starts, segments, side="right") - 1]

    def defaults(self):
        """The default of every segment: uint8 [n_segments]."""
        return np.repeat(self.bits, np.diff(np.concatenate([self.starts, [self.n_segments]])))

    def live_segments(self):
        return np.array(sorted(self.live), dtype=np.int64)

    def words(self, s):
        w = self.live.get(int(s))
        return w if w is not None else np.full(SEG_WORDS, 0xFFFFFFFF if self.default_of(s) else 0, np.uint32)

    def seg_bits(self, s):
        return _bits(self.words(s))

    def decoded(self):
        """The whole bitmap's words: for bitmaps of a few dozen segments only."""
        assert self.n_segments <= 64
        return np.concatenate([self.words(s) for s in range(self.n_segments)])[: self.n_words]

    @classmethod
    def of_words(cls, words, live=None):
        """The model of a short decoded bitmap: every segment live unless `live` names the live ones (the others must be constant)."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        n_seg = -(-words.size // SEG_WORDS)
        padded = np.concatenate([words, np.zeros(n_seg * SEG_WORDS - words.size, np.uint32)]).reshape(n_seg, SEG_WORDS)
        keep = range(n_seg) if live is None else live
        bits = []
        for s in range(n_seg):
            bits.append(int(padded[s, 0] & 1))
            assert s in keep or np.all(padded[s] == (0xFFFFFFFF if bits[-1] else 0))
        return cls(n_seg, (list(range(n_seg)), bits), {s: padded[s] for s in keep}, words.size - (n_seg - 1) * SEG_WORDS)

    # ---- the stream
    def stream_index(self, oracle, split=1):
        """(stream uint32, index int64 [n_segments + 1]): every constant segment ONE fill of its 1024 groups, never merged across
        segments, every live segment compress() of its words; the index holds the running word counts.  split > 1 (a power of
        two): a constant segment as `split` equal fills -- a stream compress() never emits, which the calls take all the same,
        and the way to an operand of many words a segment that still exists only compressed."""
        assert SEG_GROUPS % split == 0
        seg = self.live_segments()
        parts = [np.ascontiguousarray(oracle.compress(self.live[s][: self.last_words if s == self.n_segments - 1 else SEG_WORDS]),
                                      dtype=np.uint32) for s in seg.tolist()]
        words_in = np.full(self.n_segments, split, np.int64)
        words_in[seg] = [p.size for p in parts]
        index = np.concatenate([[0], np.cumsum(words_in)]).astype(np.int64)
        stream = np.repeat(np.uint32(FILL | (SEG_GROUPS // split)) | (self.defaults().astype(np.uint32) * np.uint32(ONE)), words_in)
        for s, p in zip(seg.tolist(), parts):
            stream[index[s]: index[s + 1]] = p
        return stream, index

    def expected_stream_index(self, oracle):
        """What a call that emits canonical per-segment streams returns for this bitmap: compress() never joins fills across a
        segment edge and writes a constant segment as one fill, so it is stream_index() -- a live segment that happens to be
        constant compresses to the same single fill."""
        return self.stream_index(oracle)

    # ---- count, positions, bits
    def segment_counts(self):
        """Set bits per segment: int64 [n_segments]."""
        c = self.defaults().astype(np.int64) * SEG_BITS
        for s, w in self.live.items():
            c[s] = int(_bits(w).sum(dtype=np.int64))
        return c

    def count(self):
        return int(self.segment_counts().sum(dtype=np.int64))

    def positions(self, first=0, limit=None):
        """The row numbers of the set bits of ranks [first, first + limit), ascending: int64."""
        cum = np.concatenate([[0], np.cumsum(self.segment_counts())]).astype(np.int64)
        total = int(cum[-1])
        last = total if limit is None else min(total, first + limit)
        if first >= last:
            return np.zeros(0, np.int64)
        assert last - first <= 1 << 24, "a window for a test, not a bitmap"
        ranks = np.arange(first, last, dtype=np.int64)
        seg = np.searchsorted(cum, ranks, side="right") - 1
        out = seg * SEG_BITS + (ranks - cum[seg])  # right for a segment of ones
        for s in np.unique(seg).tolist():
            if s in self.live:
                mine = seg == s
                out[mine] = s * SEG_BITS + np.flatnonzero(_bits(self.live[s]))[ranks[mine] - cum[s]]
        return out

    def bits_at(self, rows):
        """Bit rows[i]: uint8."""
        rows = np.asarray(rows, dtype=np.int64)
        assert np.all(rows >= 0) and np.all(rows < self.n_bits)
        seg, at = rows // SEG_BITS, rows % SEG_BITS
        out = self.default_of(seg).astype(np.uint8)
        for s in np.unique(seg).tolist():
            if s in self.live:
                mine = seg == s
                out[mine] = _bits(self.live[s])[at[mine]]
        return out

    def bit(self, row):
        return int(self.bits_at([row])[0])

    def bits_range(self, a, b):
        """Bits of rows [a, b): uint8, b - a at most a few segments."""
        assert 0 <= a <= b <= self.n_segments * SEG_BITS and b - a <= 4 * SEG_BITS
        if a == b:
            return np.zeros(0, np.uint8)
        s0, s1 = a // SEG_BITS, (b - 1) // SEG_BITS
        return np.concatenate([self.seg_bits(s) for s in range(s0, s1 + 1)])[a - s0 * SEG_BITS: b - s0 * SEG_BITS]


# ---- row by row over several bitmaps ---------------------------------------------------------------------------------------------
def rowwise(fn, bitmaps, n_out=1):
    """fn: a list of uint8 arrays (one per bitmap, a bit per row) -> a list of n_out such arrays, row by row.  Applied to the live
    segments' rows and, for the constant ones, to one row per run of equal defaults.  Returns n_out LongBitmaps."""
    first = bitmaps[0]
    assert all(b.n_segments == first.n_segments and b.last_words == first.last_words for b in bitmaps)
    starts = np.unique(np.concatenate([b.starts for b in bitmaps]))
    run_bits = [np.ascontiguousarray(r, dtype=np.uint8) & 1 for r in fn([b.default_of(starts).astype(np.uint8) for b in bitmaps])]
    assert len(run_bits) == n_out
    lives = [dict() for _ in range(n_out)]
    for s in sorted(set().union(*[b.live for b in bitmaps])):
        res = fn([b.seg_bits(s) for b in bitmaps])
        for j in range(n_out):
            bits = np.ascontiguousarray(res[j], dtype=np.uint8) & 1
            if s == first.n_segments - 1:
                bits[32 * first.last_words:] = 0
            lives[j][s] = _words(bits)
    return [LongBitmap(first.n_segments, (starts, run_bits[j]), lives[j], first.last_words) for j in range(n_out)]


_BITOPS = {"and": lambda a, b: a & b, "or": lambda a, b: a | b, "xor": lambda a, b: a ^ b, "andnot": lambda a, b: a & (b ^ 1)}


def bitop(op, bitmaps):
    """A op B op C ... left to right ("andnot": A AND NOT B AND NOT C ...)."""
    def fn(rows):
        acc = rows[0]
        for r in rows[1:]:
            acc = _BITOPS[op](acc, r)
        return [acc]

    return rowwise(fn, bitmaps)[0]


def invert(bitmap):
    return rowwise(lambda rows: [rows[0] ^ 1], [bitmap])[0]


def clauses(clause_list):
    """AND over clauses of [NOT] (OR of the clause's bitmaps): clause_list is [(bitmaps, negate)]."""
    flat = [b for ops, _ in clause_list for b in ops]

    def fn(rows):
        acc, at = None, 0
        for ops, negate in clause_list:
            any_ = rows[at]
            for r in rows[at + 1: at + len(ops)]:
                any_ = any_ | r
            at += len(ops)
            any_ = any_ ^ 1 if negate else any_
            acc = any_ if acc is None else acc & any_
        return [acc]

    return rowwise(fn, flat)[0]


# ---- a bit-sliced column: a list of slices, MOST significant first, and an existence bitmap or None --------------------------------
def _values(rows):
    k, v = len(rows), np.zeros(rows[0].shape, np.uint64)
    for i, r in enumerate(rows):
        v |= r.astype(np.uint64) << np.uint64(k - 1 - i)
    return v


def _slices(values, k):
    return [((values >> np.uint64(k - 1 - i)) & np.uint64(1)).astype(np.uint8) for i in range(k)]


def value_at(slices, exists, row):
    """The value at a row as a Python int, None where the row does not exist."""
    if exists is not None and not exists.bit(row):
        return None
    return sum(s.bit(row) << (len(slices) - 1 - i) for i, s in enumerate(slices))


def range_predicate(slices, lo, hi, exists=None):
    """lo <= value <= hi [AND exists], lo and hi Python ints."""
    k = len(slices)

    def fn(rows):
        v = _values(rows[:k])
        if lo > U64_MAX or hi < 0 or lo > hi:
            match = np.zeros(v.shape, np.uint8)
        else:
            match = ((v >= np.uint64(max(lo, 0))) & (v <= np.uint64(min(hi, U64_MAX)))).astype(np.uint8)
        return [match & rows[k] if exists is not None else match]

    return rowwise(fn, list(slices) + ([exists] if exists is not None else []))[0]


_CMP = {"<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal, "==": np.equal, "!=": np.not_equal}


def _two_columns(sa, sb, xa, xb):
    return list(sa) + list(sb) + [x for x in (xa, xb) if x is not None]


def _both(rows, ka, kb, xa, xb):
    """The AND of the existence rows that are there, or None."""
    extra = rows[ka + kb:]
    if not extra:
        return None
    return extra[0] if len(extra) == 1 else extra[0] & extra[1]


def compare(sa, sb, op, xa=None, xb=None):
    """A op B row by row, unsigned [AND the existence bitmaps that are there]."""
    ka, kb = len(sa), len(sb)

    def fn(rows):
        match = _CMP[op](_values(rows[:ka]), _values(rows[ka: ka + kb])).astype(np.uint8)
        have = _both(rows, ka, kb, xa, xb)
        return [match if have is None else match & have]

    return rowwise(fn, _two_columns(sa, sb, xa, xb))[0]


def arith(sa, sb, op, n_out, xa=None, xb=None):
    """(A op B) mod 2^n_out for op "+", "-", "*": the n_out slices, most significant first, then with an existence bitmap their
    AND as the last slice; rows that do not exist are stored as 0."""
    ka, kb = len(sa), len(sb)
    have_any = xa is not None or xb is not None

    def fn(rows):
        va, vb = _values(rows[:ka]), _values(rows[ka: ka + kb])
        with np.errstate(over="ignore"):
            r = (va + vb if op == "+" else va - vb if op == "-" else va * vb) & np.uint64((1 << n_out) - 1)
        have = _both(rows, ka, kb, xa, xb)
        if have is None:
            return _slices(r, n_out)
        return _slices(np.where(have != 0, r, np.uint64(0)), n_out) + [have]

    return rowwise(fn, _two_columns(sa, sb, xa, xb), n_out + (1 if have_any else 0))


def value_counts(slices, mask=None):
    """value -> rows that hold it among the rows of `mask` (a LongBitmap, None: all rows), as Python ints: a constant segment
    contributes 31 744 rows of its one value in closed form, a live one is counted by numpy on its decoded rows."""
    k = len(slices)
    maps = list(slices) + ([mask] if mask is not None else [])
    first = maps[0]
    starts = np.unique(np.concatenate([b.starts for b in maps]))
    ends = np.concatenate([starts[1:], [first.n_segments]])
    live = np.array(sorted(set().union(*[b.live for b in maps])), dtype=np.int64)
    constant = (ends - starts) - (np.searchsorted(live, ends) - np.searchsorted(live, starts))  # constant segments of every run
    run_values = _values([b.default_of(starts).astype(np.uint8) for b in slices])
    run_mask = np.ones(starts.size, np.uint8) if mask is None else mask.default_of(starts)
    out = {}
    for v, m, c in zip(run_values.tolist(), run_mask.tolist(), constant.tolist()):
        if m and c:
            out[v] = out.get(v, 0) + c * SEG_BITS
    for s in live.tolist():
        v = _values([b.seg_bits(s) for b in slices])
        keep = np.ones(SEG_BITS, bool) if mask is None else mask.seg_bits(s).astype(bool)
        if s == first.n_segments - 1:
            keep[32 * first.last_words:] = False
        for value, c in zip(*[a.tolist() for a in np.unique(v[keep], return_counts=True)]):
            out[value] = out.get(value, 0) + c
    assert len(maps) == k + (mask is not None)
    return out


def sum_count(slices, mask=None, exists=None):
    """(SUM(value), COUNT(value), COUNT(*)) over the rows of mask, the first two over those that exist: Python ints."""
    both = mask if exists is None else exists if mask is None else bitop("and", [mask, exists])
    counts = value_counts(slices, both)
    rows = slices[0].n_bits if mask is None else mask.count()
    return sum(v * c for v, c in counts.items()), sum(counts.values()), rows


def rank_of(kind, a, b, total):
    """The rank from the bottom that a query names among `total` rows, or None when it names no row."""
    if total == 0:
        return None
    if kind == ASCENDING:
        return a if a < total else None
    if kind == DESCENDING:
        return total - 1 - a if a < total else None
    if kind == QUANTILE and b > 0 and a <= b:
        return a * (total - 1) // b
    return None


class Ranks:
    """The order statistics of a column under a mask: (found, value, total, less, equal) for a query, in Python ints."""

    def __init__(self, slices, mask=None):
        self.table = sorted(value_counts(slices, mask).items())
        self.total = sum(c for _, c in self.table)

    def __call__(self, kind, a, b=1):
        rank = rank_of(kind, a, b, self.total)
        if rank is None:
            return (0, 0, self.total, 0, 0)
        less = 0
        for value, c in self.table:
            if rank < less + c:
                return (1, value, self.total, less, c)
            less += c
        raise AssertionError("a rank below the total names a value")


def top_rows(slices, mask, k):
    """The rows of the k largest values under the mask as columns.top_rows lists them: the rows strictly above the k-th value in
    row order, then the first of its ties in row order."""
    found, t, total, less, equal = Ranks(slices, mask)(DESCENDING, k - 1)
    assert found
    better = total - less - equal
    top = (1 << len(slices)) - 1
    parts = [bitop("and", [range_predicate(slices, t + 1, top), mask]).positions(0, better)] if better else []
    return np.concatenate(parts + [bitop("and", [range_predicate(slices, t, t), mask]).positions(0, k - better)])


# ---- splice ----------------------------------------------------------------------------------------------------------------------
def splice(pieces, n_segments_out, last_words=SEG_WORDS):
    """pieces: [(LongBitmap, first_row, n_rows)] of ONE column.  The output holds the pieces' row ranges back to back and zeros
    behind them.  Output segments that hold the image of a live source segment, of an edge between two default runs of a source or
    of a piece's first or last row are computed bit by bit; every other one lies inside one piece and images constant rows of one
    default, or lies behind all pieces: its default is its first row's bit."""
    n_rows_out = ((n_segments_out - 1) * SEG_WORDS + last_words) * 32
    pieces = [(src, int(first), int(n)) for src, first, n in pieces if n]
    starts, at = [], 0
    for src, first, n in pieces:
        assert 0 <= first and first + n <= src.n_bits
        starts.append(at)
        at += n
    assert at <= n_rows_out
    starts_a = np.array(starts + [at], dtype=np.int64)

    def out_bits(a, b):  # rows [a, b) of the output
        out = np.zeros(b - a, np.uint8)
        for (src, first, n), st in zip(pieces, starts):
            lo, hi = max(a, st), min(b, st + n)
            if lo < hi:
                out[lo - a: hi - a] = src.bits_range(first + lo - st, first + hi - st)
        return out

    marks = {0, n_segments_out - 1} if last_words < SEG_WORDS else set()
    for (src, first, n), st in zip(pieces, starts):
        rows = {first, first + n - 1}
        for s in src.live:
            rows.update((max(s * SEG_BITS, first), min((s + 1) * SEG_BITS, first + n) - 1))
        for s in src.starts.tolist():
            rows.update((s * SEG_BITS - 1, s * SEG_BITS))
        marks.update((r - first + st) // SEG_BITS for r in rows if first <= r < first + n)
        marks.add((st + n) // SEG_BITS)
    marks = sorted(m for m in marks if 0 <= m < n_segments_out)
    live = {m: _words(out_bits(m * SEG_BITS, (m + 1) * SEG_BITS)) for m in marks}
    if last_words < SEG_WORDS:
        live[n_segments_out - 1][last_words:] = 0
    run_starts = sorted({0} | {m + 1 for m in marks if m + 1 < n_segments_out})
    run_bits = [int(out_bits(s * SEG_BITS, s * SEG_BITS + 1)[0]) for s in run_starts]
    assert starts_a[-1] == at
    return LongBitmap(n_segments_out, (run_starts, run_bits), live, last_words)


# ---- streams of several bitmaps back to back ---------------------------------------------------------------------------------------
def expected_streams(oracle, bitmaps):
    """(stream, index) of a call that returns several bitmaps: their canonical streams back to back and n * S + 1 index entries
    counted from the first word of the whole."""
    streams, index, at = [], [], 0
    for b in bitmaps:
        st, own = b.expected_stream_index(oracle)
        streams.append(st)
        index.append(own[:-1] + at)
        at += st.size
    index.append(np.array([at], np.int64))
    return np.concatenate(streams), np.concatenate(index).astype(np.int64)


def decode_live(oracle, stream, index, segments, n_segments, last_words=SEG_WORDS):
    """segment -> its 992 decoded words, for the named segments only, by the oracle's decode of that segment's words."""
    out = {}
    for s in segments:
        n = last_words if s == n_segments - 1 else SEG_WORDS
        w = np.ascontiguousarray(oracle.decompress(stream[index[s]: index[s + 1]]), dtype=np.uint32)
        assert w.size >= n and not w[n:].any()
        out[s] = np.concatenate([w[:n], np.zeros(SEG_WORDS - n, np.uint32)])
    return out


# ---- builders --------------------------------------------------------------------------------------------------------------------
def random_segment(rng, density=0.5):
    bits = (rng.random(SEG_BITS) < density).astype(np.uint8)
    return _words(bits)


def marked(n_segments, named, rows, seed, default=0, density=0.5, extra=2):
    """A bitmap whose live segments are `named` plus `extra` seeded others, random at `density`, with the listed rows SET."""
    rng = np.random.default_rng(seed)
    segs = sorted(set(named) | {int(s) for s in rng.integers(2, n_segments - 2, extra)})
    live = {s: random_segment(rng, density) for s in segs}
    for r in rows:
        s, at = divmod(int(r), SEG_BITS)
        assert s in live, (r, s)
        live[s][at >> 5] |= np.uint32(1 << (at & 31))
    return LongBitmap(n_segments, default, live)


def column(n_segments, named, n_bits, seed, constant_value, extra=2):
    """A bit-sliced column of n_bits slices whose constant segments hold constant_value -- an int, or (starts, values): runs of
    segments with a value each -- and whose live ones (the same segments in every slice) hold seeded random values."""
    rng = np.random.default_rng(seed)
    segs = sorted(set(named) | {int(s) for s in rng.integers(2, n_segments - 2, extra)})
    values = {s: rng.integers(0, 1 << n_bits, SEG_BITS, dtype=np.uint64) for s in segs}
    starts, consts = ([0], [constant_value]) if isinstance(constant_value, int) else constant_value
    return [LongBitmap(n_segments, (starts, [(c >> (n_bits - 1 - i)) & 1 for c in consts]),
                       {s: _words(((v >> np.uint64(n_bits - 1 - i)) & np.uint64(1)).astype(np.uint8)) for s, v in values.items()})
            for i in range(n_bits)]


def from_rows(n_segments, rows):
    """The bitmap of a list of row numbers: zeros, live where a row lies."""
    rows = np.asarray(rows, dtype=np.int64)
    live = {}
    for s in np.unique(rows // SEG_BITS).tolist():
        bits = np.zeros(SEG_BITS, np.uint8)
        bits[rows[rows // SEG_BITS == s] % SEG_BITS] = 1
        live[s] = _words(bits)
    return LongBitmap(n_segments, 0, live)


def below(n_segments, row):
    """Rows 0 .. row - 1 set: two runs of defaults and the one live segment that holds `row`."""
    s, at = divmod(int(row), SEG_BITS)
    bits = np.zeros(SEG_BITS, np.uint8)
    bits[:at] = 1
    return LongBitmap(n_segments, ([0, s], [1, 0]) if s else 0, {s: _words(bits)})


# ---- the operands of the GPU tests: made here so that tests/test_long_reference.py can prove what their names claim ----------------
def named_of(n_segments):
    return A_NAMED if n_segments == A_SEGMENTS else B_NAMED


def edge_rows(n_segments):
    """The rows every `operand` sets: the first and the last, and both sides of every edge the size is there for."""
    last = n_segments * SEG_BITS - 1
    if n_segments == A_SEGMENTS:
        return A_ROWS
    group, word = 31 * 2**32, 32 * 2**32  # the first row of group 2^32, of decoded word 2^32
    return (0, group - 1, group, word - 1, word, last)


@functools.lru_cache(maxsize=None)
def operand(n_segments, j):
    """Operand j of a size: the named live segments but one (all of them for j == 0), two seeded others, defaults and densities
    that differ from operand to operand; the edge rows that lie in its live segments are set."""
    named = named_of(n_segments)
    mine = named if j == 0 else tuple(s for i, s in enumerate(named) if i != j % len(named))
    rows = [r for r in edge_rows(n_segments) if r // SEG_BITS in mine]
    return marked(n_segments, mine, rows, 100 + j, default=(0, 1, 0)[j % 3], density=(0.5, 0.02, 0.97, 0.5)[j % 4])


def fetch_rows(n_segments, per_edge):
    """Ascending rows with runs on both sides of every edge row, in the seeded and in constant segments, the last row, duplicates."""
    n_bits = n_segments * SEG_BITS
    rows = []
    for e in edge_rows(n_segments):
        rows += [r for r in range(e - per_edge, e + per_edge + 1) if 0 <= r < n_bits]
    rng = np.random.default_rng(n_segments)
    for s in sorted(operand(n_segments, 0).live)[-4:] + [5, n_segments // 3]:
        rows += (s * SEG_BITS + rng.integers(0, SEG_BITS, 6)).tolist()
    rows += rows[::7] + [n_bits - 1, n_bits - 1]
    return np.sort(np.array(rows, dtype=np.int64))


def row_lists(n_segments, n_lists):
    """Strictly ascending row lists for the from-positions call: across the edges, in the last segment, one row every few
    thousand segments; then an empty one."""
    n_bits = n_segments * SEG_BITS
    edges = edge_rows(n_segments)
    rng = np.random.default_rng(7)
    lists = [np.unique(np.concatenate([np.arange(e - 20, e + 21) for e in edges[1:5]] + [np.arange(n_bits - 33, n_bits)])),
             np.unique(np.concatenate([[0], n_bits - SEG_BITS + rng.integers(0, SEG_BITS, 50)])),
             np.unique(np.concatenate([np.arange(17, n_bits, n_bits // 130), list(edges)])),
             np.zeros(0, np.int64)]
    return [np.asarray(x, dtype=np.int64) for x in lists[:n_lists]]


COLUMN_40 = 0xABCDE12345   # the value the constant segments of the 40-bit column hold


@functools.lru_cache(maxsize=None)
def column_40():
    return column(A_SEGMENTS, A_NAMED, 40, 40, COLUMN_40)


@functools.lru_cache(maxsize=None)
def groups_at_2_32():
    """Two groups whose rows split at row 2^32."""
    g0 = below(A_SEGMENTS, 2**32)
    return g0, invert(g0)


@functools.lru_cache(maxsize=None)
def columns_12():
    """Two 12-bit columns with existence bitmaps for compare / add / subtract: constant segments hold 1000 in A, and in B 1000 up
    to segment 60 000 and 3000 behind it; live segments are random."""
    a = column(A_SEGMENTS, A_NAMED, 12, 12, 1000)
    b = column(A_SEGMENTS, A_NAMED[1:], 12, 13, ([0, 60_000], [1000, 3000]))
    return a, b, operand(A_SEGMENTS, 1), operand(A_SEGMENTS, 4)   # (both existence bitmaps default to one)


@functools.lru_cache(maxsize=None)
def splice_cases():
    """name -> (segments of the output, [(the piece's source per column, first_row, n_rows)]).  Two columns at size A, one at B."""
    a, b = A_SEGMENTS, B_SEGMENTS
    mostly_ones = marked(a, (3, 135_350), [], 55, default=1, extra=0)
    middle = marked(b, B_NAMED + (2_164_900, 2_164_901), [], 56, extra=0)   # live segments inside the piece taken from row 2^36 on
    return {
        "a piece lands at 2^32 - 7": (a, [((operand(a, 0), operand(a, 2)), 1234, 2**32 - 7 - 2_000_000),
                                          ((operand(a, 1), operand(a, 3)), 2**32 - 100, 2_000_000),
                                          ((operand(a, 2), operand(a, 5)), 2**31 - 5, 1_000_000)]),
        "a piece of more than 2^32 rows": (a, [((LongBitmap(a, 1), mostly_ones), 3, 2**32 + 1000),
                                               ((operand(a, 0), operand(a, 1)), 2**32 - 100, 3_000_000)]),
        "source rows above 2^36": (b, [((LongBitmap(b, 1), ), 7, 2**36 + 99), ((middle, ), 2**36 + 12_345, 10_000_000)])}


@functools.lru_cache(maxsize=None)
def top_case():
    """(slices, mask): a 12-bit column that holds 5 everywhere but in two live segments behind row 2^32, under the kth mask."""
    return column(A_SEGMENTS, (135_301, 135_399), 12, 77, 5, extra=0), operand(A_SEGMENTS, 1)


KTH_LOW, KTH_HIGH, KTH_TUNED =7, 4000, 100_000   # the two constant values of the kth column; the segment that tunes the split


@functools.lru_cache(maxsize=None)
def kth_case():
    """(slices, mask): a 12-bit column whose constant segments hold KTH_LOW up to a segment R and KTH_HIGH behind it, under a mask
    of ones with random live segments; R and the rows of segment KTH_TUNED that hold KTH_LOW (the others hold 4095) are chosen so
    that EXACTLY 2^32 selected rows hold a value <= KTH_LOW: rank 2^32 - 1 is KTH_LOW, rank 2^32 is the next value up."""
    mask = operand(A_SEGMENTS, 1)
    assert mask.default_of(KTH_TUNED) == 1 and KTH_TUNED not in mask.live
    rng = np.random.default_rng(12)
    values = {s: rng.integers(0, 1 << 12, SEG_BITS, dtype=np.uint64) for s in A_NAMED}

    def build(r, t):
        tuned = np.full(SEG_BITS, 4095, np.uint64)
        tuned[:t] = KTH_LOW
        both = dict(values)
        both[KTH_TUNED] = tuned
        return [LongBitmap(A_SEGMENTS, ([0, r], [(KTH_LOW >> (11 - i)) & 1, (KTH_HIGH >> (11 - i)) & 1]),
                           {s: _words(((v >> np.uint64(11 - i)) & np.uint64(1)).astype(np.uint8)) for s, v in both.items()}) for i in range(12)]

    def at_most_low(slices):
        return sum(c for v, c in value_counts(slices, mask).items() if v <= KTH_LOW)

    r = 135_290
    for _ in range(8):
        short = 2**32 - at_most_low(build(r, 0))
        if 0 <= short < SEG_BITS:
            slices = build(r, short)
            assert at_most_low(slices) == 2**32
            return slices, mask
        r += short // SEG_BITS
    raise AssertionError("no split at 2^32")
