"""The reference and the inputs of the fetch call's tests (wah_fetch_indexed_device: include/wah.h).  No GPU, no library:
tests/test_fetch_reference.py proves these against the CPU oracle and against plain indexing, tests/test_gpu_fetch.py holds
the kernels against them.

ref_fetch answers from the STREAMS: position p is looked up as group p // 31, bit p % 31 of the stream's words -- never as
word p // 32, bit p % 32 of a decoded bitmap, which is what the tests compare it WITH.  items_of restates how the check pass
cuts a list of rows into items."""
import os
import re

import numpy as np

from tests import _select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_SOURCE = os.path.join(ROOT, "gpu-wah_amd", "csrc", "wah_bitop_list.hip")

BITS, FIRST = 0, 1  # WAH_FETCH_BITS, WAH_FETCH_FIRST
U64_MAX = (1 << 64) - 1
ITEM_ROWS = 64                 # listed rows of an item at the most: one per lane
SEG_WORDS = _select.SEG_WORDS  # 992
SEG_BITS = _select.SEG_BITS    # 31744 positions a segment


def grid_waves():
    """The wavefronts of the items pass at the most, read from the kernel source: one item more than this and a wavefront's
    stride loop takes a second turn."""
    with open(KERNEL_SOURCE) as f:
        m = re.search(r"constexpr u32 kFetchGridWaves = (\d+);", f.read())
    assert m, "kFetchGridWaves is no longer a plain constant of wah_bitop_list.hip"
    return int(m.group(1))


def bits_at(stream, rows):
    """Bit rows[i] of the bitmap the stream encodes, by a walk over its words: 0 / 1 as uint8."""
    w, fill, n, start = _select._walk(stream)
    p = np.asarray(rows, dtype=np.int64)
    group, bit = p // 31, p % 31
    at = np.searchsorted(start, group, side="right") - 1
    assert np.all(at >= 0) and np.all(group < start[at] + n[at]), "a row behind the stream's groups"
    word = w[at]
    return np.where(fill[at], (word & _select.ONE) != 0, (word >> bit) & 1 != 0).astype(np.uint8)


def ref_fetch(streams, rows, mode):
    """What the call gives for a table of `streams` (one whole stream per table row) and the listed rows, as Python ints in a
    list: BITS the value whose bit k - 1 - j is the row's bit in stream j, FIRST the lowest j that has the bit, U64_MAX if none."""
    k = len(streams)
    assert k >= 1 and (mode == FIRST or k <= 64)
    rows = np.asarray(rows, dtype=np.int64)
    out = [0 if mode == BITS else U64_MAX] * rows.size
    for j, st in enumerate(streams):
        for i in np.flatnonzero(bits_at(st, rows)):
            if mode == BITS:
                out[i] |= 1 << (k - 1 - j)
            elif out[i] == U64_MAX:
                out[i] = j
    return out


def as_u64(t):
    """An int64 result tensor / array as Python ints in 0 .. 2^64 - 1."""
    return [int(v) & U64_MAX for v in (t.tolist() if hasattr(t, "tolist") else t)]


def segments(n_words):
    return _select.segments_of(n_words)


def items_of(rows, n_words):
    """The items of a non-descending list: [(index of the head, listed rows)].  Row i is a head when i % 64 == 0 or its segment,
    (p // 31) // 1024, differs from row i - 1's."""
    rows = np.asarray(rows, dtype=np.int64)
    assert np.all(rows[1:] >= rows[:-1]) and (rows.size == 0 or (rows[0] >= 0 and rows[-1] < 32 * n_words))
    seg = (rows // 31) // _select.SEG_GROUPS
    head = np.arange(rows.size) % ITEM_ROWS == 0
    head[1:] |= seg[1:] != seg[:-1]
    at = np.flatnonzero(head)
    return list(zip(at.tolist(), np.diff(np.concatenate([at, [rows.size]])).tolist()))


def item_bound(n_rows, n_words):
    """What the scratch has room for: ceil(n_rows / 64) + min(n_rows, S)."""
    return -(-n_rows // ITEM_ROWS) + min(n_rows, segments(n_words))


def one_hot(keys, n_values, n_words):
    """The decoded bitmaps [n_values, n_words] of an equality-encoded key column (keys < 0: in no bitmap)."""
    keys = np.asarray(keys, dtype=np.int64)
    bits = np.zeros((n_values, 32 * n_words), bool)
    have = np.flatnonzero(keys >= 0)
    bits[keys[have], have] = True
    return np.stack([np.packbits(b, bitorder="little").view("<u4").astype(np.uint32) for b in bits])
