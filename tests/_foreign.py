"""Legal re-encodings of a bitmap that compress() never emits: foreign operands for the indexed calls.

TEST INFRASTRUCTURE (tests/test_foreign_reference.py proves every way with the oracle on the CPU,
tests/test_gpu_foreign_operands.py runs the streams through the indexed kernels).

include/wah.h promises that a stream "written by the reference, read back from storage" gets a segment index from
wah_build_index_device and may then be used by every indexed call.  The index builder asks three things of a stream: no fill
crosses a segment of 1024 groups, no fill is empty, a segment's words make up exactly its groups.  compress() and the oracle
give more than that -- maximal fills, never a literal that could be a fill, never a set pad bit -- and every operand the rest
of the suite hands to an indexed kernel is one of theirs.  reencode() writes the SAME bitmap in the ways that are legal and
not canonical:

  way                  a segment's words                                        what it is for
  -------------------  -------------------------------------------------------  ---------------------------------------------
  canonical            as oracle.compress                                       the control
  fills of one         every fill group its own count-1 fill word (an all-zero  `w1 - w0 > nvalid` at equality, the short-fill
                       segment: 1024 words)                                     path in every lane, 8 batches of fills
  split k              every maximal fill of n >= 2 groups as two fills of one  the short / long split at kListShortFill, two
    k = 1, 8, 9, 64,   kind, k and n - k (left whole where k does not fit)      fills of one kind in one lane's pair, in
    n - 1                                                                       neighbouring lanes, across a batch edge
  fillable literals    every zero / all-ones group as literal 0 / 0x7FFFFFFF    the all-literal fast paths against reads past
                                                                                the range, begin_row on a row of zeros
  two fills 1 / 512    a one-word segment as two fills: 1 + rest, half + half   the gather's settled shortcut NOT taken
  mixed                per run one of the above, by a seeded rng                everything side by side in one batch
  pad: literal         ragged n_words: the last group a literal with every pad  the pad rule of every call, both routes of the
                       bit set                                                  two-operand call
  pad: one-fill        a fill of ones that runs over the ragged last group
  pad: split one-fill  the same, the last group a count-1 one-fill of its own

A bitmap of n_words words has G = ceil(32 n_words / 31) groups; where 31 G > 32 n_words the last group has pad bits (the
highest 31 G - 32 n_words of its 31), which compress() leaves clear and the pad ways set.  An operand with set pad bits is the
same bitmap: the pad is not part of it.
"""
import numpy as np

from tests import _switch as sw
from tests import _walk as wk

M31, FILL0, FILL1, SEG, SEG_WORDS = sw.M31, sw.FILL0, sw.FILL1, sw.SEG_GROUPS, sw.SEG_WORDS
BATCH = sw.LIST_BATCH

SPLITS = (1, 8, 9, 64, "n-1")
WAYS = ("canonical", "fills of one") + tuple(f"split {k}" for k in SPLITS) + ("fillable literals", "two fills 1", "two fills 512", "mixed")
PAD_WAYS = ("pad: literal", "pad: one-fill", "pad: split one-fill")
SPLIT_WAYS = tuple(w for w in WAYS if w.startswith("split"))
TWO_FILL_WAYS = ("two fills 1", "two fills 512")
# the counter of wah_validate_device (tests/_walk.py: report) a way must move: index into the 7-tuple
UNMERGED, FILLABLE = 5, 3
EXPECTED_COUNTER = {"fills of one": UNMERGED, "fillable literals": FILLABLE, "two fills 1": UNMERGED, "two fills 512": UNMERGED,
                    "pad: split one-fill": UNMERGED, **{w: UNMERGED for w in SPLIT_WAYS}}

# segments of every kind a bitmap index holds, and "placement": the split-fill placement segment (placement_layout)
KINDS = ("clustered", "zeros", "sparse", "ones", "dense", "placement")
TAILS = ("zeros", "ones", "random")


# ---- groups <-> words -------------------------------------------------------------------------------------------------------
def n_groups(n_words):
    return (32 * n_words + 30) // 31


def pad_bits(n_words):
    """Bits of the last group that lie behind the bitmap's last bit (0: the last group is whole)."""
    return 31 * n_groups(n_words) - 32 * n_words


def unpack(words):
    """The inverse of _switch.pack: the ceil(32 n / 31) groups of a bitmap of n words (the last one's pad bits zero)."""
    w = np.ascontiguousarray(words, dtype="<u4")
    g = n_groups(w.size)
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    bits = np.concatenate([bits, np.zeros(31 * g - bits.size, np.uint8)]).reshape(g, 31).astype(np.uint32)
    return (bits << np.arange(31, dtype=np.uint32)).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def runs(groups):
    """[(kind, first group, n)] of the maximal runs of one segment's groups: "zeros", "ones", or "lit" (literals in a row)."""
    g = np.asarray(groups, np.uint32)
    kind = np.where(g == 0, 0, np.where(g == M31, 1, 2))
    cut = np.flatnonzero(np.diff(kind)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [g.size]])
    return [(("zeros", "ones", "lit")[int(kind[a])], int(a), int(b - a)) for a, b in zip(starts, ends)]


# ---- the ways ---------------------------------------------------------------------------------------------------------------
def _fill_words(way, word, n, whole_segment, rng):
    """The words of one maximal fill of n groups (word: FILL0 or FILL1) under `way`."""
    if way == "mixed":
        way = ("canonical", "fills of one", "fillable literals", f"split {int(rng.integers(1, n))}" if n >= 2 else "canonical")[int(rng.integers(0, 4))]
    if way == "fills of one":
        return [word | 1] * n
    if way == "fillable literals":
        return [M31 if word == FILL1 else 0] * n
    if way.startswith("split"):
        k = way[len("split "):]
        k = n - 1 if k == "n-1" else int(k)
        return [word | k, word | (n - k)] if 1 <= k < n else [word | n]
    if way in TWO_FILL_WAYS and whole_segment and n >= 2:
        k = 1 if way == "two fills 1" else n // 2
        return [word | k, word | (n - k)]
    return [word | n]


def segment_words(groups, way, rng):
    """One segment's groups in the named way (not a pad way)."""
    out = []
    for kind, at, n in runs(groups):
        if kind == "lit":
            out.extend(int(v) for v in groups[at: at + n])
        else:
            out.extend(_fill_words(way, FILL1 if kind == "ones" else FILL0, n, n == len(groups), rng))
    return out


def reencode(words, n_words, way, rng=None, only=None):
    """The bitmap words[:n_words] as a WAH stream (uint32) whose every segment is written in `way`: no fill crosses a segment,
    none is empty, a segment's words make up exactly its groups.  The pad ways write every segment canonically but for the end
    of the last one, and need pad bits there (and, for the two one-fill ways, a bitmap whose last two groups are all ones).
    only: the segment numbers that are written in `way`, the others canonically (a long way in a stream that stays short)."""
    assert way in WAYS + PAD_WAYS, way
    g = unpack(np.asarray(words, np.uint32)[:n_words])
    pad = pad_bits(n_words)
    out = []
    for s in range(0, g.size, SEG):
        seg = g[s: s + SEG].copy()
        if way not in PAD_WAYS or s + SEG < g.size:
            out.extend(segment_words(seg, way if way not in PAD_WAYS and (only is None or s // SEG in only) else "canonical", rng))
            continue
        assert pad, "a pad way needs a ragged n_words"
        valid = M31 >> pad
        if way == "pad: literal":
            out.extend(segment_words(seg[:-1], "canonical", rng))
            out.append(int(seg[-1]) | (M31 ^ valid))
            continue
        assert seg.size >= 2 and seg[-1] == valid and seg[-2] == M31, "the one-fill pad ways need a bitmap that ends in ones"
        seg[-1] = M31
        tail = segment_words(seg, "canonical", rng)
        if way == "pad: split one-fill":
            tail[-1:] = [tail[-1] - 1, FILL1 | 1]
        out.extend(tail)
    return np.array(out, np.uint32)


def segment_ranges(stream):
    """Word-by-word restatement of wah_build_index_device (tests/test_walk_reference.py: _py_index) that also proves the
    index's preconditions: returns [first word of every segment ..., len(stream)]; asserts that no fill is empty or crosses a
    segment.  Every segment's words then sum to exactly its groups (1024, the last one what is left)."""
    pos, offsets = 0, []
    for i, x in enumerate(int(v) for v in stream):
        n = x & sw.COUNT_MASK if x & FILL0 else 1
        assert n != 0 and pos % SEG + n <= SEG, (i, hex(x), pos)
        if pos % SEG == 0:
            offsets.append(i)
        pos += n
    return offsets + [len(stream)], pos


def noncanonical_words(stream):
    """Indices of the words compress() would not have written: a fill behind a fill of its kind inside a segment, a literal
    that could be a fill (the two counters of the checker that are about single words)."""
    st, fill, cnt, _, pos = wk._walk(stream)
    _, same = wk._behind_a_fill_of_its_kind(st, fill, cnt)
    return np.flatnonzero((same & ((pos & np.uint64(SEG - 1)) != 0)) | (~fill & ((st == 0) | (st == M31))))


def off_by_one(stream, way, delta):
    """(stream, index, word) of a stream that must be REFUSED: the foreign stream with one group too many (delta 1) or too few
    (-1) in its non-canonical part -- a fill's count moved by one; a literal, or a fill of one group, written twice or left
    out.  The pad ways take the stream's last word, the control its last fill.  The index is hand-made (to the builder the
    stream is another bitmap, or has a fill across a segment): the segment starts of the intact stream, moved with the words behind the one that changed."""
    assert delta in (1, -1)
    offsets, _ = segment_ranges(stream)
    if way in PAD_WAYS:
        t = len(stream) - 1
    elif way == "canonical":
        t = int(np.flatnonzero(stream & np.uint32(FILL0))[-1])
    else:
        at = noncanonical_words(stream)
        t = int(at[at.size // 2])
    st, x, moved = [int(v) for v in stream], int(stream[t]), 0
    if x & FILL0 and (delta > 0 or (x & sw.COUNT_MASK) >= 2):
        st[t] = x + delta
    elif delta > 0:
        st.insert(t, x)
        moved = 1
    else:
        del st[t]
        moved = -1
    return np.array(st, np.uint32), np.array([o + (moved if o > t else 0) for o in offsets], np.int64), t


# ---- bitmaps ----------------------------------------------------------------------------------------------------------------
SPLIT_FILL_GROUPS = 100  # of the three placed fills of placement_layout: every k of SPLITS fits


def placement_layout():
    """A whole segment in which, under every split way, the two parts of a fill lie (a) in one lane's pair of a 128-word batch
    (words 4 and 5), (b) in neighbouring lanes (words 9 and 10), (c) across the edge of two batches (words 127 and 128); a
    lane holds words 2 l and 2 l + 1 of its batch.  The placed fills are of ones, zeros, ones -- each has an effect under some
    operation -- and a long fill of zeros ends the segment.  placement_words() gives the indices, asserted by the CPU test."""
    n = SPLIT_FILL_GROUPS
    return [("lit", 4), ("ones", n), ("lit", 3), ("zeros", n), ("lit", 116), ("ones", n), ("lit", 10), ("zeros", SEG - 3 * n - 133)]


PLACED_SPLITS = ((4, "one lane's pair"), (9, "neighbouring lanes"), (BATCH - 1, "across the batch edge"))


def _clustered(n, rng):
    """Fills of 2 to 200 groups of either kind in turn with one or two literals between them: some 25 words in 1024 groups."""
    layout, left, k = [], n, int(rng.integers(0, 2))
    while left:
        m = min(int(rng.integers(2, 200)), left)
        layout.append((("zeros", "ones")[k & 1], m))
        left -= m
        k += 1
        if left:
            m = min(int(rng.integers(1, 3)), left)
            layout.append(("lit", m))
            left -= m
    return layout


def _groups_of_kind(kind, n, rng):
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "ones":
        return np.full(n, M31, np.uint32)
    if kind == "clustered":
        return sw.list_groups(_clustered(n, rng), rng)
    if kind == "placement":
        assert n == SEG
        return sw.list_groups(placement_layout(), rng)
    if kind == "sparse":  # single set bits, two of them in neighbouring groups
        g = np.zeros(n, np.uint32)
        at = rng.permutation(n - 1)[: min(6, n - 1)]
        g[at] = np.uint32(1) << rng.integers(0, 31, at.size).astype(np.uint32)
        g[at[0] + 1] = 5
        return g
    assert kind == "dense", kind
    g = sw.literals(rng, n)  # random literals around a few fill groups: lone ones, a pair, a run of three
    for at, m, v in ((3, 1, 0), (n // 4, 2, M31), (n // 2, 3, 0), (n - 2, 1, M31)):
        if at + m <= n:
            g[at: at + m] = v
    return g


def bitmap(n_words, rng, kinds=KINDS, tail="zeros"):
    """n_words bitmap words: whole segments of `kinds` in turn, and, where n_words is no multiple of 992, a short last segment
    that is all zeros, all ones (the bits the bitmap has) or random literals."""
    whole, rest = divmod(n_groups(n_words), SEG)
    parts = [_groups_of_kind(kinds[s % len(kinds)], SEG, rng) for s in range(whole)]
    if rest:
        assert tail in TAILS, tail
        parts.append(np.zeros(rest, np.uint32) if tail == "zeros" else np.full(rest, M31, np.uint32) if tail == "ones" else sw.literals(rng, rest) | np.uint32(1))
    g = np.concatenate(parts)
    g[-1] &= np.uint32(M31 >> pad_bits(n_words))
    words = sw.pack(g)
    assert not words[n_words:].any()
    return np.ascontiguousarray(words[:n_words])


def kinds_for(way, n_segments):
    """Segment kinds, in turn, under which `way` changes a bitmap of n_segments whole segments: the two-fill ways need a
    one-word segment, the others a segment with fills of two and more groups -- first, so that one segment is enough."""
    if way in TWO_FILL_WAYS:
        return ("zeros", "ones", "clustered", "zeros", "dense")
    return ("clustered", "zeros", "sparse", "ones", "dense") if n_segments < 6 else KINDS


def tail_for(way, j=0):
    """The short last segment a way needs: ones for the one-fill pad ways; otherwise zeros, ones, random by j."""
    return "ones" if way in PAD_WAYS[1:] else TAILS[j % 3]


def ways_for(n_words):
    """Every way a bitmap of n_words words can be written in: the pad ways only where the last group has pad bits."""
    return WAYS + (PAD_WAYS if pad_bits(n_words) else ())


def rows_foreign(rows, n_words, rng, ways=None, first=0):
    """The rows of a decoded matrix [k, n_words] (slices, masks, group rows) as foreign streams, the ways rotating over the rows
    from `first`: [(way, stream)].  A pad way that a row cannot take (its bitmap does not end in ones) becomes "pad: literal"."""
    ways = ways_for(n_words)[1:] if ways is None else ways
    out = []
    for j, row in enumerate(rows):
        way = ways[(first + j) % len(ways)]
        if way in PAD_WAYS[1:]:
            g = unpack(row[:n_words])
            if not (g.size >= 2 and g[-1] == (M31 >> pad_bits(n_words)) and g[-2] == M31):
                way = "pad: literal"
        out.append((way, reencode(row, n_words, way, rng)))
    return out
