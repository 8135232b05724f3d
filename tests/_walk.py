"""Foreign streams that sit ON the edges of the tiled walk of wah_aux.hip (wah_validate_device, wah_build_index_device,
wah_merge_fills_device), and vectorised references of the three calls.

TEST INFRASTRUCTURE (tests/test_walk_reference.py proves the references equal to the word-by-word restatements and every
constructor to have the property it states; tests/test_gpu_walk_kernels.py runs the streams through the kernels).

The walk: a workgroup takes a tile of 4096 words, each of its 256 threads 16 consecutive ones, a wave 1024.  A word's group
position is the wave scan + the sums of the waves in front + the tile's base; its predecessor comes from the same thread, from
LDS (first word of a thread) or from global memory (first word of a tile).  The merger adds suffix minima of "first kept
position" over lanes, waves and tiles, a scan kernel that takes 1024 tiles a round with a carry in each direction, and the rule
that no run merges across a multiple of 2^29 groups.  The constructors build WAH words directly -- these are streams, not
bitmaps -- and return Probe(name, stream, facts): `facts` is what the stream was built for, asserted on the CPU by restating
the kernel's predicate.

The references are numpy, exact in uint64, without a Python loop over words: report() the checker's 7-tuple, merged() the
merger's words, index() the segment index or the reason why there is none.
"""
import collections

import numpy as np

from tests import _switch as sw

FILL0, FILL1, M31, COUNT_MASK = sw.FILL0, sw.FILL1, sw.M31, sw.COUNT_MASK
KIND = 0x40000000
SEG = sw.SEG_GROUPS

TILE = sw.THRESHOLDS["kScanTileWords"][0]                 # words a workgroup walks
WAVES = sw.THRESHOLDS["kExpandWaves"][0]
THREADS = 64 * WAVES
PER_THREAD = TILE // THREADS                              # 16
PER_WAVE = TILE // WAVES                                  # 1024
BLOCK_SHIFT = sw.THRESHOLDS["kMergeBlockShift"][0]
BLOCK = 1 << BLOCK_SHIFT
SCAN_TILES = sw.THRESHOLDS["merge scan tiles"][0][0]      # tiles a round of merge_scan_kernel
ALIGN = sw.THRESHOLDS["walk vector load alignment"][0] + 1

# the stream's first byte behind a 16-byte boundary: only 0 (and whole tiles) takes the 16-byte loads
PLACEMENT_BYTES = tuple(range(0, ALIGN, 4))
# word index -> whose first word it is; "inside a thread" is the control
WALK_EDGES = (("inside a thread", 5 * PER_THREAD + 7), ("thread", 5 * PER_THREAD), ("last thread of a wave", 63 * PER_THREAD),
              ("wave", PER_WAVE), ("last wave", (WAVES - 1) * PER_WAVE), ("tile", TILE), ("third tile", 2 * TILE))
END_WORDS = (1, PER_THREAD - 1, PER_THREAD, PER_THREAD + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1)
RUN_LENGTHS = (2, PER_THREAD - 1, PER_THREAD, PER_THREAD + 1, PER_WAVE, TILE, 3 * TILE + 5)
SCAN_ROUND_TILE_COUNTS = (SCAN_TILES - 1, SCAN_TILES, SCAN_TILES + 1, 2 * SCAN_TILES, 2 * SCAN_TILES + 1)
BLOCK_MULTIPLES = (1, 9)                                  # k 2^29: the first boundary, and one beyond 2^32 groups
TAIL = 37                                                 # ordinary words behind a probe
# what lies behind the stream's end in the device buffer: words that would move every counter if they were read
PADDING = np.array([FILL0 | 7, FILL0 | 9, 0, M31, FILL0, FILL1 | 2000, FILL1 | 3, 12345], np.uint32)

Probe = collections.namedtuple("Probe", "name stream facts")


# ---- the references ---------------------------------------------------------------------------------------------------------
def _walk(stream):
    """(words, is a fill, count, groups, group position) of every word, positions exact in uint64."""
    st = np.ascontiguousarray(stream, dtype=np.uint32)
    fill = (st & np.uint32(FILL0)) != 0
    cnt = (st & np.uint32(COUNT_MASK)).astype(np.uint64)
    n = np.where(fill, cnt, np.uint64(1))
    end = np.cumsum(n, dtype=np.uint64)
    return st, fill, cnt, n, end - n


def groups(stream):
    """The stream's group total."""
    n = _walk(stream)[3]
    return int(n.sum(dtype=np.uint64)) if n.size else 0


def _behind_a_fill_of_its_kind(st, fill, cnt):
    """Per word: it is a non-empty fill, and so is the word in front of it, of the same kind."""
    full = fill & (cnt != 0)
    same = np.zeros(st.size, bool)
    same[1:] = full[1:] & full[:-1] & (((st[1:] ^ st[:-1]) & np.uint32(KIND)) == 0)
    return full, same


def report(stream):
    """wah_validate_device's report: (groups, decoded words, empty fills, literals that could be fills, fills across a segment
    boundary, fills that could have been merged with the one in front inside their segment, none of the four)."""
    st, fill, cnt, n, pos = _walk(stream)
    g = int(n.sum(dtype=np.uint64)) if st.size else 0
    full, same = _behind_a_fill_of_its_kind(st, fill, cnt)
    in_seg = pos & np.uint64(SEG - 1)
    empty = int(np.count_nonzero(fill & (cnt == 0)))
    lit = int(np.count_nonzero(~fill & ((st == 0) | (st == M31))))
    cross = int(np.count_nonzero(full & (in_seg + cnt > SEG)))
    unmerged = int(np.count_nonzero(same & (in_seg != 0)))
    return g, (31 * g + 31) // 32, empty, lit, cross, unmerged, not (empty or lit or cross or unmerged)


def dropped(stream):
    """Per word: wah_merge_fills_device drops it -- an empty fill, or a fill behind a non-empty fill of its kind with which it
    lies inside one block of 2^29 groups."""
    st, fill, cnt, n, pos = _walk(stream)
    full, same = _behind_a_fill_of_its_kind(st, fill, cnt)
    before = np.zeros(st.size, np.uint64)
    before[1:] = cnt[:-1]
    first, last = pos.copy(), pos + cnt - np.uint64(1)
    first[same] -= before[same]                                # (only where `same`: pos >= the count of the word in front)
    one_block = (first >> np.uint64(BLOCK_SHIFT)) == (last >> np.uint64(BLOCK_SHIFT))
    return (fill & (cnt == 0)) | (same & one_block)


def merged(stream):
    """wah_merge_fills_device's output: the kept words, every kept non-empty fill running up to the next kept word (the
    stream's end behind the last)."""
    st, fill, cnt, n, pos = _walk(stream)
    keep = ~dropped(st)
    out = st[keep].copy()
    at = pos[keep]
    run = np.diff(np.concatenate([at, np.array([n.sum(dtype=np.uint64)], np.uint64)]))
    is_fill = fill[keep]                                        # (a kept fill is never empty)
    assert not np.any(run[is_fill] > COUNT_MASK), "a merged count outgrew 30 bits"
    out[is_fill] = (out[is_fill] & np.uint32(FILL1)) | run[is_fill].astype(np.uint32)
    return out


def index(stream):
    """wah_build_index_device: the int64 offsets (first word of every segment, then the stream's length), or the reason for
    refusing the stream (a str): an empty fill, or a word across a segment boundary."""
    st, fill, cnt, n, pos = _walk(stream)
    if np.any(n == 0):
        return "an empty fill"
    in_seg = pos & np.uint64(SEG - 1)
    if np.any(in_seg + n > SEG):
        return "a fill across a segment boundary"
    return np.concatenate([np.flatnonzero(in_seg == 0), [st.size]]).astype(np.int64)


def segments_of(stream):
    """Entries of the segment index less one: ceil(groups / 1024)."""
    return (groups(stream) + SEG - 1) // SEG


# ---- building blocks --------------------------------------------------------------------------------------------------------
def ordinary(rng, n):
    """n ordinary words: random literals (never all zeros or all ones), every third to sixth word a fill of 1 to 9 groups, the
    kinds in turn and never two fills side by side; the first three words and the last are literals."""
    st = sw.literals(rng, n)
    at = np.cumsum(rng.integers(3, 7, n // 3 + 1))
    at = at[at < n - 1]
    st[at] = np.where(np.arange(at.size) % 2 == 0, FILL0, FILL1).astype(np.uint32) | rng.integers(1, 10, at.size).astype(np.uint32)
    return st


def _lit(rng):
    return np.uint32(sw.literals(rng, 1)[0])


def segment_words(w, rng, n_groups=SEG):
    """w words of exactly n_groups groups, none empty: literals only where w == n_groups, else literals around one fill (two of
    different kinds, apart, from four words on)."""
    assert 1 <= w <= n_groups <= SEG, (w, n_groups)
    st = sw.literals(rng, w)
    if w == n_groups:
        return st
    kinds = (FILL0, FILL1) if rng.integers(0, 2) else (FILL1, FILL0)
    if w >= 4 and n_groups - w >= 1:
        rest = n_groups - (w - 2)                               # groups of the two fills together
        a = int(rng.integers(0, w - 2))
        b = int(rng.integers(a + 2, w))
        first = int(rng.integers(1, rest))
        st[a], st[b] = kinds[0] | first, kinds[1] | (rest - first)
    else:
        st[int(rng.integers(0, w))] = kinds[0] | (n_groups - (w - 1))
    return st


_SEGMENT_CYCLE = (1, 7, SEG, 2, 129, 16, 1, 1, 640, 33, 5, SEG, 3, 300)


def split_words(total, shift=0):
    """Words per segment, 1 to 1024 each, that add up to `total`."""
    out, k = [], shift
    while total:
        w = min(_SEGMENT_CYCLE[k % len(_SEGMENT_CYCLE)], total)
        out.append(w)
        total -= w
        k += 1
    return out


def segments(counts, rng):
    """Whole segments of the given word counts, back to back."""
    return np.concatenate([segment_words(w, rng) for w in counts]) if counts else np.zeros(0, np.uint32)


# ---- predecessor pairs ------------------------------------------------------------------------------------------------------
PAIR_KINDS = ("same kind", "different kinds", "empty predecessor", "literal predecessor", "aligned second")


def pair_probes(rng):
    """Word i on every edge of WALK_EDGES (and word 1: its predecessor is the stream's first word, which has none) is a fill of
    ones of 5 groups; the word in front of it is in turn a fill of ones (unmerged, dropped), a fill of zeros, an empty fill of
    ones, a literal, and a fill of ones that ends on a multiple of 1024 groups (the checker does not count word i, the merger
    drops it).  The words around the pair are literals; the probes of an edge differ in word i - 1 alone.
    facts: i, unmerged (word i counts as unmerged), dropped (word i), prev_dropped."""
    out = []
    for edge, i in (("second word of the stream", 1), ) + WALK_EDGES:
        while True:
            base = ordinary(rng, i + 1 + TAIL)
            base[max(i - 2, 0)] = base[i + 1] = _lit(rng)
            before = groups(base[: i - 1])
            if i == 1 or 0 < before % SEG < SEG - 3:         # word i - 1 and word i start inside a segment
                break
        aligned = SEG - before % SEG
        for kind, prev, facts in (("same kind", FILL1 | 3, (True, True, False)), ("different kinds", FILL0 | 3, (False, False, False)),
                                  ("empty predecessor", FILL1, (False, False, True)), ("literal predecessor", _lit(rng), (False, False, False)),
                                  ("aligned second", FILL1 | aligned, (False, True, False))):
            st = base.copy()
            st[i - 1], st[i] = prev, FILL1 | 5
            out.append(Probe(f"pair at the {edge} (word {i}), {kind}", st, dict(i=i, unmerged=facts[0], dropped=facts[1], prev_dropped=facts[2])))
    return out


# ---- positions --------------------------------------------------------------------------------------------------------------
POSITION_Q = (0, 1, SEG - 1)


def position_probes(rng):
    """Word i on every edge is a fill at in-segment position q = 0, 1, 1023 that ends exactly AT the segment's end (1024 - q
    groups: no crossing, the stream has a segment index) or one group behind it (1025 - q: a crossing, no index); and a fill of
    2048 groups from a segment start.  Everything else is whole segments of 1 to 1024 words (segment_words), so the one fill
    decides, and a wrong wave sum or tile base moves q.  facts: i, q, count, crossing."""
    out = []
    for e, (edge, i) in enumerate(WALK_EDGES):
        for q in POSITION_Q:
            lead = 0 if q == 0 else 1 if q == 1 else 9               # words of the q groups in front of the fill
            for count in (SEG - q, SEG + 1 - q, 2 * SEG):
                if count == 2 * SEG and q:
                    continue
                over = (q + count) % SEG                               # groups the fill takes of the segment behind its own
                st = np.concatenate([segments(split_words(i - lead, e + q), rng),
                                     segment_words(lead - 1, rng, q - 1) if lead > 1 else np.zeros(0, np.uint32),
                                     [_lit(rng)] if lead else np.zeros(0, np.uint32),          # (literals around the fill)
                                     [(FILL1 if (e + q) & 1 else FILL0) | count],
                                     np.concatenate([[_lit(rng)], segment_words(4, rng, SEG - over - 1)]) if over else np.zeros(0, np.uint32),
                                     segments(split_words(TAIL, e), rng)]).astype(np.uint32)
                out.append(Probe(f"fill of {count} groups at the {edge} (word {i}), {q} groups into its segment", st,
                                 dict(i=i, q=q, count=count, crossing=q + count > SEG)))
    return out


# ---- stream ends ------------------------------------------------------------------------------------------------------------
END_KINDS = (("empty fill", FILL1), ("literal 0", 0), ("literal of ones", M31), ("fill", FILL0 | 11))


def end_probes(rng):
    """Streams of END_WORDS words: ordinary words, the last one an empty fill, a literal 0, a literal 0x7FFFFFFF and a fill in
    turn.  facts: c_words, last."""
    out = []
    for c in END_WORDS:
        for kind, last in END_KINDS:
            st = np.concatenate([ordinary(rng, c - 1), [last]]).astype(np.uint32)
            out.append(Probe(f"{c} words, the last one {'an' if kind[0] == 'e' else 'a'} {kind}", st, dict(c_words=c, last=last)))
    return out


# ---- segmented streams (the index) ------------------------------------------------------------------------------------------
def _edge_segment_counts():
    """Words per segment such that a segment starts on every edge of WALK_EDGES; one-word and 1024-word segments among them."""
    counts, at = [], 0
    for i in sorted({i for _, i in WALK_EDGES} | {j + 1 for _, j in WALK_EDGES}):   # (a one-word segment ON every edge)
        while at < i:
            w = min(SEG, i - at)
            counts.append(w)
            at += w
    return counts + [1, 5, SEG, 2]


def index_probes(rng):
    """Segmented streams.  "segments on every edge": a segment starts on every edge of WALK_EDGES and holds one word, full
    segments of 1024 literals among the others; once with whole segments (G a multiple of 1024), once with a short last one.
    Then, per edge, a pair that differs in words i and i + 1: the segment on the edge starts with a fill of one group and a
    fill of the other kind (accepted) or with an EMPTY fill and that fill one group longer (the same groups, refused).  The
    1025 - q refusals are position_probes().  facts: starts (word indices that must be in the index, None where refused),
    refused."""
    counts = _edge_segment_counts()
    edges = sorted(i for _, i in WALK_EDGES)
    out = []
    whole = segments(counts, rng)
    out.append(Probe("segments on every edge, whole segments", whole, dict(starts=edges, refused=False)))
    ragged = np.concatenate([whole, segment_words(3, rng, 100)])
    out.append(Probe("segments on every edge, a last segment of 100 groups", ragged, dict(starts=edges, refused=False)))
    for e, (edge, i) in enumerate(WALK_EDGES):
        a, b = (FILL0, FILL1) if e & 1 else (FILL1, FILL0)
        head = segments(split_words(i, e), rng)
        tail = segments(split_words(TAIL, e + 1), rng)
        rest = sw.literals(rng, 20)                                  # the segment on the edge: 2 fills, 20 literals
        for refused in (False, True):
            seg = np.concatenate([[a | (0 if refused else 1), b | (SEG - 20 - (0 if refused else 1))], rest]).astype(np.uint32)
            out.append(Probe(f"segment at the {edge} (word {i}) starts with {'an empty fill' if refused else 'a fill of one group'}",
                             np.concatenate([head, seg, tail]), dict(starts=None if refused else [i], refused=refused, i=i)))
    return out


# ---- merge runs -------------------------------------------------------------------------------------------------------------
RUN_START = 3 * PER_THREAD + 5   # word index of a run's first dropped word: inside a thread


def _droppable(rng, n, kind):
    return (np.uint32(kind) | rng.integers(1, 4, n).astype(np.uint32)).astype(np.uint32)


def run_probes(rng):
    """A kept fill of zeros inside a thread, behind it a run of RUN_LENGTHS fills of zeros (all dropped) that ends inside a
    thread, a kept fill of ones, ordinary words: from 31 words on whole threads keep nothing, from 4096 whole waves, the longest
    whole tiles.  Then streams of empty fills alone (nothing is kept, no groups), and a kept fill followed by dropped and empty
    words up to the stream's end (its count runs to the stream's total).
    facts: head (index of the kept fill), run (dropped words behind it), head_count (its merged count)."""
    out = []
    for n in RUN_LENGTHS:
        front = ordinary(rng, RUN_START - 1)
        run = _droppable(rng, n, FILL0)
        st = np.concatenate([front, [FILL0 | 2], run, [FILL1 | 3], ordinary(rng, TAIL)]).astype(np.uint32)
        assert (RUN_START - 1) % PER_THREAD and (RUN_START + n) % PER_THREAD
        out.append(Probe(f"run of {n} dropped fills", st, dict(head=RUN_START - 1, run=n, head_count=2 + int((run & COUNT_MASK).sum()))))
    for n in (1, PER_THREAD, TILE + 7):
        st = np.where(np.arange(n) % 3 == 0, FILL0, FILL1).astype(np.uint32)
        out.append(Probe(f"{n} empty fills and nothing else", st, dict(head=None, run=n, head_count=None)))
    for n in (3, 20, TILE + 50):
        run = np.concatenate([_droppable(rng, n, FILL1), np.where(np.arange(n // 2 + 1) % 2 == 0, FILL0, FILL1)]).astype(np.uint32)
        st = np.concatenate([ordinary(rng, RUN_START - 1), [FILL1 | 4], run]).astype(np.uint32)
        out.append(Probe(f"a kept fill, {n} dropped and {n // 2 + 1} empty words up to the end", st,
                         dict(head=RUN_START - 1, run=run.size, head_count=4 + int((run & COUNT_MASK).sum()))))
    # "adjacent" is said of the INPUT: a fill behind an empty fill is kept, whatever stands in front of the empty one
    st = np.concatenate([ordinary(rng, RUN_START - 1), [FILL1 | 4, FILL1 | 2, FILL1, FILL1 | 3, FILL0, FILL1 | 1], ordinary(rng, TAIL)]).astype(np.uint32)
    out.append(Probe("fills of one kind with empty fills between them", st, dict(head=RUN_START - 1, run=1, head_count=6)))
    return out


# ---- more than one round of the merge scan ----------------------------------------------------------------------------------
def _scan_stream(n_tiles, run, rng):
    """n_tiles tiles of ordinary words drawn, in an order without a short period, from a pool of 13 random tiles that hold 0 to
    36 pairs of fills of one kind (so the tiles' kept counts differ, neighbours' too); run (first tile, last tile, kind,
    count): a kept fill inside a thread of the first tile, dropped fills up to inside a thread of the last tile, a kept fill of
    the other kind."""
    pool = []
    for k in range(13):
        tile = ordinary(rng, TILE)
        for j in range(3 * k):                                        # 3 k pairs: the second fill of each is dropped
            at = 64 + 100 * j
            tile[at - 1: at + 3] = [_lit(rng), FILL1 | (j % 5 + 1), FILL1 | 2, _lit(rng)]
        tile[-1] = tile[0] = _lit(rng)
        pool.append(tile)
    order = (np.arange(n_tiles) ** 2 + np.arange(n_tiles) // 3) % 13
    st = np.stack(pool)[order].reshape(-1)
    facts = dict(tiles=n_tiles, run=None)
    if run is not None:
        t0, t1, kind, count = run
        lo, hi = t0 * TILE + RUN_START - 1, t1 * TILE + 9 * PER_THREAD + 3
        st[lo - 1] = _lit(rng)
        st[lo: hi] = kind | count
        st[hi] = (kind ^ KIND) | 3
        st[hi + 1] = _lit(rng)
        facts["run"] = (lo, hi)
    return st, facts


# name -> (tiles, the run: first tile, last tile, kind, groups per fill); the totals stay far below 2^29 groups
SCAN_ROUND_STREAMS = {
    "1023 tiles": (SCAN_TILES - 1, None),
    "1024 tiles": (SCAN_TILES, None),
    "1025 tiles, a run from tile 1000 into the last one": (SCAN_TILES + 1, (1000, SCAN_TILES, FILL0, 1)),
    "2048 tiles, a run from tile 3 into the last one": (2 * SCAN_TILES, (3, 2 * SCAN_TILES - 1, FILL1, 2)),
    "2049 tiles, a run from tile 1000 into tile 1030": (2 * SCAN_TILES + 1, (1000, 1030, FILL0, 1)),
    "2049 tiles, a run from tile 3 into tile 2048: a round that keeps nothing": (2 * SCAN_TILES + 1, (3, 2 * SCAN_TILES, FILL1, 2)),
}


def scan_round_stream(name, seed=77):
    """Probe of SCAN_ROUND_STREAMS[name]; facts: tiles, run (first, end: word indices of the kept fill and of the kept fill of
    the other kind behind the run)."""
    n_tiles, run = SCAN_ROUND_STREAMS[name]
    st, facts = _scan_stream(n_tiles, run, np.random.default_rng(seed))
    return Probe(name, st, facts)


# ---- the 2^29 rule ----------------------------------------------------------------------------------------------------------
def _approach(rng, target):
    """Ordinary words, then large fills of alternating kind, then a literal: the next word starts at group `target`."""
    front = ordinary(rng, 30)
    left = target - groups(front) - 1
    big = []
    assert left >= 5
    while left:
        n = 1 << 28 if left >= (1 << 28) + 5 else left            # (never a last fill of under 5 groups)
        big.append((FILL0 if len(big) & 1 else FILL1) | n)
        left -= n
    return np.concatenate([front, np.array(big, np.uint32), [_lit(rng)]]).astype(np.uint32)


def block_probes(rng):
    """Around B = k 2^29 groups, k of BLOCK_MULTIPLES (9: beyond 2^32).  Fills of one kind, side by side, in front of B and
    behind it; the position is brought there by fills of 2^28 groups of alternating kind.
    facts: at (index of the first fill of the group), dropped (per fill of the group), starts (their group positions)."""
    out = []
    cases = (("a pair that ends at group B - 1", -12, (5, 7), (False, True)),
             ("a pair that ends at group B", -11, (5, 7), (False, False)),
             ("a pair that starts at group B", 0, (5, 7), (False, True)),
             ("a pair that starts at group B - 1", -1, (5, 7), (False, False)),
             ("a chain A, B, C: B starts at B, C merges into it", -3, (3, 4, 6), (False, False, True)),
             ("a pair across B - 2^28", -(1 << 28) - 3, (5, 7), (False, True)))
    for k in BLOCK_MULTIPLES:
        for j, (name, start, counts, drops) in enumerate(cases):
            kind = FILL1 if (j + k) & 1 else FILL0
            head = _approach(rng, k * BLOCK + start)
            st = np.concatenate([head, [kind | c for c in counts], ordinary(rng, TAIL)]).astype(np.uint32)
            starts = [k * BLOCK + start + sum(counts[:m]) for m in range(len(counts))]
            out.append(Probe(f"{name}, B = {k} x 2^29", st, dict(at=head.size, dropped=drops, starts=starts, k=k)))
    return out


# ---- all of the small ones --------------------------------------------------------------------------------------------------
def small_probes(seed=2024):
    """Every probe of at most a few tiles: {family: [Probe]}."""
    rng = np.random.default_rng(seed)
    return {"pairs": pair_probes(rng), "positions": position_probes(rng), "ends": end_probes(rng), "index": index_probes(rng),
            "runs": run_probes(rng), "blocks": block_probes(rng)}
