"""numpy references for the grouped sum (wah_group_sum_indexed_device: include/wah.h): per group the set bits of a conjunction
of bitmaps (COUNT(*)), the bits it shares with every slice of bit-sliced attributes, and the attributes' sums.  No GPU, no
library: tests/test_group_reference.py proves these against each other and against the CPU oracle, tests/test_gpu_group_sum.py
holds the kernels against them.  The builders are those of tests/_select.py and tests/_masked.py.

Three levels: on the BITMAPS (ref_group: what the call must give for compress() of them), on the STREAMS (stream_group: all
expanded to their 31-bit groups, for the short and possibly hand-built streams used here, with the pad rule -- the 31 G - 32 n
bits of the last group that lie behind the bitmap are never counted, whichever stream sets them), and on the VALUES (value_model:
keys, values and a filter as arrays, the sums as a database would give them).  Everything is returned as Python ints: a sum of a
64-bit attribute does not fit 64 bits."""
import itertools

import numpy as np

from tests import _masked as msk
from tests import _select as sel

MAX_FILTERS, MAX_ROWS, MAX_ATTRS = 64, 8, 64  # WAH_GROUP_MAX_*


# ---- the items and the chunk (gpu-wah_amd/csrc/wah_select.hip: ChunkCursor, chunked_count_grid) --------------------------------
def chunk_of(n_groups, n_operands, n_segments):
    """Operands that share one conjunction image: the masked count's rule with the groups in the masks' place."""
    return msk.chunk_of(n_groups, n_operands, n_segments)


def items_of(n_groups, n_operands, n_segments):
    """The (group, chunk, segment) items of a call, in the kernel's order."""
    chunk = chunk_of(n_groups, n_operands, n_segments)
    n_chunks = (n_operands + chunk - 1) // chunk
    return [(g, c, s) for g in range(n_groups) for c in range(n_chunks) for s in range(n_segments)]


def runs_of(n_groups, n_operands, n_segments):
    """The contiguous runs of items the wavefronts of the launch take: (items per wavefront, wavefronts that get any)."""
    chunk = chunk_of(n_groups, n_operands, n_segments)
    n_items = n_groups * ((n_operands + chunk - 1) // chunk) * n_segments
    n_waves = min((n_items + 3) // 4, 256 * 4) * 4
    per = (n_items + n_waves - 1) // n_waves
    return per, (n_items + per - 1) // per


# ---- the fold ------------------------------------------------------------------------------------------------------------------
def fold(counts, attr_bits):
    """Per attribute the sum of its slices' counts, slice i of an attribute of b slices weighing 2^(b - 1 - i)."""
    assert sum(attr_bits) == len(counts)
    sums, at = [], 0
    for b in attr_bits:
        sums.append(sum(int(c) << (b - 1 - i) for i, c in enumerate(counts[at: at + b])))
        at += b
    return sums


def split128(value):
    """A sum as the call stores it: (low, high) 64-bit words."""
    assert 0 <= value < 1 << 128
    return value & ((1 << 64) - 1), value >> 64


# ---- on the bitmaps ------------------------------------------------------------------------------------------------------------
def _popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)).sum(dtype=np.int64))


def ref_group(filter_words, group_words, slice_words, attr_bits, n):
    """filter_words: F bitmaps (possibly none); group_words[g]: the R bitmaps of group g; slice_words: K bitmaps, the attributes'
    slices back to back.  Returns (rows [G], counts [G][K], sums [G][A]) over the first n words."""
    rows, counts, sums = [], [], []
    for own in group_words:
        both = np.full(n, 0xFFFFFFFF, np.uint32)
        for w in list(filter_words) + list(own):
            both = both & np.ascontiguousarray(w, dtype=np.uint32)[:n]
        rows.append(_popcount(both))
        counts.append([_popcount(both & np.ascontiguousarray(w, dtype=np.uint32)[:n]) for w in slice_words])
        sums.append(fold(counts[-1], attr_bits))
    return rows, counts, sums


# ---- on the streams ------------------------------------------------------------------------------------------------------------
def stream_group(filter_streams, group_streams, slice_streams, attr_bits, n):
    """The same from streams of bitmaps of n words: group by group, the last group without its pad bits."""
    g = sel.groups_of(n)
    keep = np.full(g, sel.M31, np.uint32)
    if g:
        keep[-1] = sel.M31 >> sel.pad_bits(n)

    def expanded(st):
        e = msk.groups_of_stream(st)
        assert e.size == g, "a stream does not make up the bitmap's groups"
        return e

    slices = [expanded(st) for st in slice_streams]
    rows, counts, sums = [], [], []
    for own in group_streams:
        both = keep.copy()
        for st in list(filter_streams) + list(own):
            both &= expanded(st)
        rows.append(_popcount(both))
        counts.append([_popcount(both & s) for s in slices])
        sums.append(fold(counts[-1], attr_bits))
    return rows, counts, sums


# ---- on the values -------------------------------------------------------------------------------------------------------------
def value_model(keys, n_values, attributes, chosen):
    """keys: one integer array per grouping attribute, n_values their value counts; attributes: (values, exists or None) pairs;
    chosen: the filter, a bool array.  Returns (rows, sums, counts): rows a nested list shaped by n_values, sums / counts one such
    list per attribute (Python ints; COUNT(value) is the rows where the attribute exists)."""
    shape = tuple(int(v) for v in n_values)
    rows = np.zeros(shape, dtype=object)
    sums = [np.zeros(shape, dtype=object) for _ in attributes]
    counts = [np.zeros(shape, dtype=object) for _ in attributes]
    key_rows = np.stack([np.asarray(k) for k in keys], axis=1)
    for group in itertools.product(*[range(v) for v in shape]):
        mine = np.asarray(chosen, dtype=bool) & np.all(key_rows == np.array(group), axis=1)
        rows[group] = int(mine.sum())
        for t, (values, exists) in enumerate(attributes):
            have = mine if exists is None else mine & np.asarray(exists, dtype=bool)
            sums[t][group] = sum(int(v) for v in np.asarray(values)[have])
            counts[t][group] = int(have.sum())
    return rows.tolist(), [s.tolist() for s in sums], [c.tolist() for c in counts]


def slices_of(values, n_bits, n_words, exists=None):
    """The bit-sliced index of a value column as bitmaps: n_bits slices, most significant first, then the existence bitmap if
    there is one (rows outside it are stored as 0)."""
    values = np.asarray(values, dtype=np.uint64)
    have = np.ones(values.size, bool) if exists is None else np.asarray(exists, dtype=bool)
    out = [sel.bitmap_of(np.flatnonzero(((values >> np.uint64(n_bits - 1 - i)) & np.uint64(1)).astype(bool) & have), n_words) for i in range(n_bits)]
    if exists is not None:
        out.append(sel.bitmap_of(np.flatnonzero(have), n_words))
    return out


def key_bitmaps(keys, n_values, n_words):
    """The equality-encoded index of a key column as bitmaps: one per value."""
    return [sel.bitmap_of(np.flatnonzero(np.asarray(keys) == v), n_words) for v in range(n_values)]


# ---- hand-built segments -------------------------------------------------------------------------------------------------------
def fill_segment(ones, groups=sel.SEG_GROUPS):
    """One segment that is one fill word."""
    return np.array([sel.FILL | (sel.ONE if ones else 0) | groups], np.uint32)


def literal_segment(rng, groups=sel.SEG_GROUPS):
    """One segment of random literals, none of them 0 or all ones."""
    return rng.integers(1, sel.M31, groups, dtype=np.uint64).astype(np.uint32)


def mixed_segment(rng):
    """One segment of fills and literals in turn: a one-fill of 3 groups, a literal, a zero-fill of 2, a literal, ... and a
    closing fill over what is left."""
    words, at, k = [], 0, 0
    while at + 7 <= sel.SEG_GROUPS:
        words += [sel.FILL | sel.ONE | 3, int(rng.integers(1, sel.M31)), sel.FILL | 2, int(rng.integers(1, sel.M31))]
        at += 7
        k += 1
    if at < sel.SEG_GROUPS:
        words.append(sel.FILL | (sel.ONE if k % 2 else 0) | (sel.SEG_GROUPS - at))
    return np.array(words, np.uint32)


def segment_kinds(rng):
    """name -> one whole segment (1024 groups) of every kind the kernel tells apart, as a stream: the two fills that need no
    image, literals, fills and literals in turn, and one run of ones (tests/_masked.run_operand) that begins or ends at an edge
    of the image's steps (63 / 64 / 65) or at its end (1023 / 1024)."""
    kinds = {"zero fill": fill_segment(False), "one fill": fill_segment(True), "literals": literal_segment(rng), "mixed": mixed_segment(rng)}
    for a in msk.RUN_EDGES:
        if a < sel.SEG_GROUPS:
            kinds[f"ones up to group {a}"] = msk.run_operand(0, a)
            kinds[f"ones from group {a}"] = msk.run_operand(a, sel.SEG_GROUPS - a)
        else:
            kinds["ones in the last group"] = msk.run_operand(a - 1, 1)
            kinds["ones behind the first group"] = msk.run_operand(1, a - 1)
    return kinds


def partial_kinds(rng, groups):
    """The same for a bitmap's last segment of fewer groups (at least 3): the two fills, literals, and a one-fill, a literal and
    a zero-fill in turn.  The fills and the last literal may set pad bits: the pad rule drops them."""
    assert 3 <= groups < sel.SEG_GROUPS
    return {"zero fill": fill_segment(False, groups), "one fill": fill_segment(True, groups), "literals": literal_segment(rng, groups),
            "mixed": np.array([sel.FILL | sel.ONE | 1, int(rng.integers(1, sel.M31)), sel.FILL | (groups - 2)], np.uint32),
            "ones at the end": np.array([sel.FILL | (groups - 1), sel.FILL | sel.ONE | 1], np.uint32)}


def kind_streams(rng, n):
    """One indexed stream per segment kind for a bitmap of n words: stream k holds kind k + s (in turn) in segment s, so that
    every kind meets every other in some segment when two streams are ANDed.  Returns (names, streams, indexes)."""
    full = segment_kinds(rng)
    whole, rest = divmod(sel.groups_of(n), sel.SEG_GROUPS)
    part = list(partial_kinds(rng, rest).values()) if rest else []
    names, kinds = list(full), list(full.values())
    streams, indexes = [], []
    for k in range(len(kinds)):
        segs = [kinds[(k + s) % len(kinds)] for s in range(whole)] + ([part[k % len(part)]] if rest else [])
        streams.append(np.concatenate(segs))
        indexes.append(np.concatenate([[0], np.cumsum([len(x) for x in segs])]).astype(np.int64))
    return names, streams, indexes


def bitmap_of_stream(stream, n):
    """The first n words of the bitmap a stream decodes to (its pad bits dropped)."""
    return sel.pack(msk.groups_of_stream(stream))[:n]
