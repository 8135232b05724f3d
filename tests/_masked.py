"""numpy references for the masked count (wah_count_masked_indexed_device: include/wah.h): the set bits a mask shares with an
operand.  No GPU, no library: tests/test_masked_reference.py proves these against the CPU oracle, tests/test_gpu_count_masked.py
holds the kernel against them.  The builders are those of tests/_select.py.

Two levels, as there: on the BITMAPS (ref_counts: what the call must give for compress() of them), and on the STREAMS
(stream_counts: both expanded to their 31-bit groups, for the short and possibly hand-built streams used here, with the pad
rule -- the 31 G - 32 n bits of the last group that lie behind the bitmap are never counted, whichever stream sets them)."""
import numpy as np

from tests import _select as sel

# the kernel's constants (gpu-wah_amd/csrc/wah_select.hip: count_masked_kernel) beside those of tests/_select.py
GRID_WAVES = 256 * 4 * 4          # wavefronts of a full grid: more (mask, operand, segment) triples than this is a run of several
RUN_EDGES = (63, 64, 65, 1023, 1024)  # group positions around a step of the mask image and around its end
ITEMS_PER_WAVE = 8                # the launcher lets operands share a mask image in chunks while this many items per wavefront remain


def chunk_of(n_masks, n_operands, n_segments):
    """Operands that share one mask image (chunked_count_grid): 64, halved while a full grid would get fewer than eight
    (mask, chunk, segment) items per wavefront."""
    chunk = 64
    while chunk > 1 and n_masks * ((n_operands + chunk - 1) // chunk) * n_segments < ITEMS_PER_WAVE * GRID_WAVES:
        chunk //= 2
    return chunk


def _popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)).sum(dtype=np.int64))


def ref_counts(mask_words, op_words, n):
    """The popcount of the AND of the first n words of two bitmaps."""
    a = np.ascontiguousarray(mask_words, dtype=np.uint32)[:n]
    b = np.ascontiguousarray(op_words, dtype=np.uint32)[:n]
    return _popcount(a & b)


def groups_of_stream(stream):
    """A stream's 31-bit groups, one entry each: a literal is itself, a fill its value repeated."""
    w = np.ascontiguousarray(stream, dtype=np.uint32).astype(np.int64)
    fill = (w & sel.FILL) != 0
    value = np.where(fill, np.where((w & sel.ONE) != 0, sel.M31, 0), w & sel.M31)
    return np.repeat(value, np.where(fill, w & sel.MASK, 1)).astype(np.uint32)


def stream_counts(mask_stream, op_stream, n):
    """The same number from two streams of a bitmap of n words: group by group, the last group without its pad bits."""
    a, b = groups_of_stream(mask_stream), groups_of_stream(op_stream)
    g = sel.groups_of(n)
    assert a.size == g and b.size == g, "a stream does not make up the bitmap's groups"
    both = a & b
    if g:
        both[-1] &= sel.M31 >> sel.pad_bits(n)
    return _popcount(both)


def run_operand(a, b):
    """One segment by hand: a zero-fill of a groups, a one-fill of b groups, a zero-fill over the rest (parts of no group are
    left out: a stream holds no empty fill)."""
    parts = [(sel.FILL, a), (sel.FILL | sel.ONE, b), (sel.FILL, sel.SEG_GROUPS - a - b)]
    return np.array([kind | k for kind, k in parts if k], dtype=np.uint32)


def alternating_mask(rng):
    """One segment by hand: one-fills of one group and random literals in turn, 1024 words."""
    st = rng.integers(1, sel.M31, sel.SEG_GROUPS, dtype=np.uint64).astype(np.uint32)
    st[0::2] = sel.FILL | sel.ONE | 1
    return st
