"""numpy references and stream builders for the count / positions calls (wah_count_list_indexed_device,
wah_positions_indexed_device: include/wah.h).  No GPU, no library: tests/test_select_reference.py proves these against the CPU
oracle, tests/test_gpu_select.py holds the kernels against them.

Two levels of reference: on the BITMAP (ref_count, ref_positions: what the calls must give for compress() of it), and on the
STREAM (stream_count, stream_positions: a walk over the words of a possibly hand-built stream, with the pad rule -- the 31 G -
32 n bits of the last group that lie behind the bitmap are never counted or listed, whatever the stream holds there)."""
import numpy as np

M31 = 0x7FFFFFFF
FILL, ONE, MASK = 0x80000000, 0x40000000, 0x3FFFFFFF

# the kernels' constants (gpu-wah_amd/csrc/wah_select.hip, wah_segdecode.hpp): every one is a place where the code does
# something else on the other side
STEP_GROUPS = 64                  # groups a wavefront handles per step of the emit kernel
SEG_GROUPS = 1024                 # groups per segment: one wavefront each
SEG_WORDS = 992                   # bitmap words per segment
SEG_BITS = SEG_GROUPS * 31        # 31744
BATCH_WORDS = 128                 # stream words per load batch, two per lane
STAGE_SLOTS = STEP_GROUPS * 31    # 1984: LDS slots of the emit kernel's staging, the set bits of one full step
RANK_CHUNK = 4096                 # entries per workgroup of the rank scan: more than this many segments + 1 is a second level,
                                  # more than RANK_CHUNK ** 2 a third


def groups_of(n_words):
    return (32 * n_words + 30) // 31


def segments_of(n_words):
    return (groups_of(n_words) + SEG_GROUPS - 1) // SEG_GROUPS


def pad_bits(n_words):
    return 31 * groups_of(n_words) - 32 * n_words


# ---- on the bitmap ------------------------------------------------------------------------------------------------------------
def ref_count(words, n):
    w = np.ascontiguousarray(words, dtype=np.uint32)[:n]
    return int(np.unpackbits(w.view(np.uint8)).sum(dtype=np.int64))


def ref_positions(words, n):
    w = np.ascontiguousarray(words, dtype=np.uint32)[:n]
    return np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")).astype(np.int64)


# ---- on the stream ------------------------------------------------------------------------------------------------------------
def _walk(stream):
    w = np.ascontiguousarray(stream, dtype=np.uint32).astype(np.int64)
    fill = (w & FILL) != 0
    n = np.where(fill, w & MASK, 1)
    start = np.cumsum(n) - n
    return w, fill, n, start


def stream_positions(stream, n_words):
    """Positions of the set bits of the bitmap of n_words words the stream decodes to, ascending: group g, bit j is position
    31 g + j, and positions at or behind 32 n_words (the pad bits) do not exist."""
    w, fill, n, start = _walk(stream)
    lit = ~fill
    lw, ls = w[lit], start[lit]
    rows, cols = np.nonzero(((lw[:, None] >> np.arange(31)) & 1).astype(np.uint8))
    parts = [ls[rows] * 31 + cols]
    ones = fill & ((w & ONE) != 0)
    for s, k in zip(start[ones].tolist(), n[ones].tolist()):
        parts.append(np.arange(31 * s, 31 * (s + k), dtype=np.int64))
    pos = np.sort(np.concatenate(parts).astype(np.int64))
    return pos[pos < 32 * n_words]


def stream_count(stream, n_words):
    """The same number by arithmetic on the words: a literal's popcount, 31 per group of a one-fill, less what the LAST word
    holds in the pad bits."""
    w, fill, n, _ = _walk(stream)
    if w.size == 0:
        return 0
    ones = fill & ((w & ONE) != 0)
    lit_bits = np.unpackbits((w[~fill] & M31).astype(np.uint32).view(np.uint8)).sum(dtype=np.int64)
    total = int(lit_bits) + 31 * int(n[ones].sum())
    pad = pad_bits(n_words)
    last = int(w[-1])
    if last & FILL:
        total -= pad if (last & ONE) and (last & MASK) else 0
    else:
        total -= bin(last & M31 & ~(M31 >> pad)).count("1")
    return total


def index_of(stream):
    """The segment index of a stream whose words never cross a multiple of 1024 groups: the word every segment starts at,
    then the stream's length."""
    _, _, n, start = _walk(stream)
    assert np.all(start % SEG_GROUPS + n <= SEG_GROUPS), "a word crosses a segment edge"
    return np.concatenate([np.flatnonzero(start % SEG_GROUPS == 0), [len(stream)]]).astype(np.int64)


# ---- builders -----------------------------------------------------------------------------------------------------------------
def pack(groups):
    """31-bit groups -> the bitmap's words (bit j of group g is bit 31 g + j), the last word zero padded."""
    g = np.ascontiguousarray(groups, dtype=np.uint32)
    assert not np.any(g >> 31)
    bits = ((g[:, None] >> np.arange(31, dtype=np.uint32)) & 1).astype(np.uint8).reshape(-1)
    bits = np.concatenate([bits, np.zeros((-bits.size) % 32, np.uint8)])
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def bitmap_of(positions, n_words):
    bits = np.zeros(32 * n_words, np.uint8)
    bits[np.asarray(positions, dtype=np.int64)] = 1
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def segment_of_words(words, rng, fill_bit=0):
    """One segment (992 words) that compresses to exactly `words` stream words: words - 1 literals, then one fill."""
    lit = rng.integers(1, M31, words - 1, dtype=np.uint64).astype(np.uint32)
    return pack(np.concatenate([lit, np.full(SEG_GROUPS - (words - 1), M31 if fill_bit else 0, np.uint32)]))


def segment_of_bits(k):
    """One segment whose first k bits are set and no other: k = STAGE_SLOTS fills the first step and the staging exactly."""
    return bitmap_of(np.arange(k), SEG_WORDS)


# the set-bit counts of a segment at which the emit kernel's staging and steps switch
SEGMENT_BIT_EDGES = (0, 1, STAGE_SLOTS - 1, STAGE_SLOTS, STAGE_SLOTS + 1, SEG_BITS - 1, SEG_BITS)
# ... and the stream words of a segment around a load batch and around the tests of seg_load_words (128, 512 words)
SEGMENT_WORD_EDGES = (1, 2, BATCH_WORDS - 1, BATCH_WORDS, BATCH_WORDS + 1, 4 * BATCH_WORDS, 4 * BATCH_WORDS + 1, SEG_GROUPS - 1, SEG_GROUPS)


def edge_bits(n_words):
    """A bit on each side of every segment edge and of every step edge of the first segment, inside the bitmap."""
    edges = [SEG_BITS * s for s in range(1, segments_of(n_words) + 1)] + [31 * STEP_GROUPS * s for s in range(1, 16)]
    pos = sorted({p for e in edges for p in (e - 1, e) if 0 <= p < 32 * n_words})
    return bitmap_of(pos, n_words)


def bitmaps(oracle, n):
    """name -> bitmap of n words: every kind the count and the positions are held against."""
    out = {"zeros": np.zeros(n, np.uint32), "ones": np.full(n, 0xFFFFFFFF, np.uint32),
           "uniform 0.3": oracle.gen_uniform(n, 11, 0.3), "uniform 0.9": oracle.gen_uniform(n, 12, 0.9),
           "uniform 2^-10": oracle.gen_uniform(n, 13, 2.0 ** -10), "uniform 2^-13": oracle.gen_uniform(n, 14, 2.0 ** -13),
           "clustered": oracle.gen_clustered(n, 15, 700),
           "first bit": bitmap_of([0], n), "last bit": bitmap_of([32 * n - 1], n), "edges": edge_bits(n)}
    return {k: np.ascontiguousarray(v, dtype=np.uint32) for k, v in out.items()}


def pad_streams():
    """Hand-built streams that SET pad bits: (what, n_words, stream, set bits).  compress() never emits these."""
    out = [("one-fill over both groups of one word", 1, [0xC0000002], 32),
           ("last literal all ones: 1 bit real, 30 pad", 1, [M31, M31], 32),
           ("last literal with pad bits only", 1, [0x12345678, M31 - 1], bin(0x12345678).count("1")),
           ("n = 30: one pad bit, set in a literal", 30, [0xC000001E, M31], 960),
           ("n = 30: one pad bit under a one-fill", 30, [0x8000001E, 0xC0000001], 30),
           ("n = 31: no pad bit", 31, [0xC0000020], 992),
           ("n = 993: a last segment of two groups under a one-fill", 993, [0xC0000400, 0xC0000002], 32 * 993),
           ("n = 993: zeros, then a last literal of pad bits and one real bit", 993, [0x80000400, 0x80000001, M31], 1)]
    return [(what, n, np.array(st, np.uint32), bits) for what, n, st, bits in out]


def long_stream(n_segments, marked):
    """A bitmap of n_segments whole segments, too long to exist decoded: every segment one zero-fill, except the `marked`
    ones (segment -> bit inside its first group), which are a literal and a fill.  Returns (n_words, stream, index, positions)."""
    marked = dict(sorted(marked.items()))
    seg = np.array(list(marked), dtype=np.int64)
    words_in = np.ones(n_segments, np.int64)
    words_in[seg] = 2
    index = np.concatenate([[0], np.cumsum(words_in)]).astype(np.int64)
    stream = np.full(int(index[-1]), FILL | SEG_GROUPS, np.uint32)
    stream[index[seg]] = (1 << np.array(list(marked.values()), dtype=np.int64)).astype(np.uint32)
    stream[index[seg] + 1] = FILL | (SEG_GROUPS - 1)
    positions = seg * SEG_BITS + np.array(list(marked.values()), dtype=np.int64)
    return n_segments * SEG_WORDS, stream, index, positions
