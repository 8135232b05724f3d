"""The reference and the kernel's rules of the range call's tests (wah_values_indexed_device: include/wah.h).  No GPU, no library:
tests/test_values_reference.py proves these against the CPU oracle and against plain indexing, tests/test_gpu_values.py holds
the kernel against them.

The reference is tests/_fetch.py's: ref_values(streams, first, n, mode) IS ref_fetch(streams, arange(first, first + n), mode),
which reads the streams by group and bit.  values_of gives the same numbers as one uint64 array, vectorised over the rows (the
same bits_at, the fold in numpy instead of a Python loop per set bit) -- proven equal to ref_values, and what the GPU tests of
whole bitmaps compare with.

The rest restates what values_items_kernel (gpu-wah_amd/csrc/wah_values.hip) does, rule by rule -- which table rows make which
half, which segments a window touches, which rows of a segment an item stores, which bytes of d_out it owns -- and `model` puts a
result together from exactly these rules, byte by byte, counting the writes.  Every rule can be swapped for a WRONG one with one
error (WRONG), to prove that the cases of the tests tell them apart."""
import os
import re

import numpy as np

from tests import _fetch, _select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_SOURCE = os.path.join(ROOT, "gpu-wah_amd", "csrc", "wah_values.hip")

BITS, FIRST = _fetch.BITS, _fetch.FIRST
U64_MAX = _fetch.U64_MAX
SEG_WORDS, SEG_BITS, SEG_GROUPS = _select.SEG_WORDS, _select.SEG_BITS, _select.SEG_GROUPS
POISON = 0xA5  # every byte of an output nobody wrote

WRONG = ("half from the wrong end", "last segment dropped on a seam", "word 32 addressing", "first takes the last")


def grid_items():
    """The workgroups of the launch at the most, read from the kernel source: one item more than this and a workgroup's stride loop
    takes a second turn."""
    with open(KERNEL_SOURCE) as f:
        m = re.search(r"constexpr u32 kValuesGridItems = (\d+);", f.read())
    assert m, "kValuesGridItems is no longer a plain constant of wah_values.hip"
    return int(m.group(1))


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def ref_values(streams, first, n, mode):
    """What the call gives for the window [first, first + n): Python ints in a list."""
    return _fetch.ref_fetch(streams, np.arange(first, first + n, dtype=np.int64), mode)


def fold(bits, mode):
    """The values of rows whose bit in table row j is bits[j] (one 0 / 1 array per table row): uint64."""
    k = len(bits)
    assert k >= 1 and (mode == FIRST or k <= 64)
    n = len(bits[0])
    out = np.zeros(n, np.uint64) if mode == BITS else np.full(n, U64_MAX, np.uint64)
    for j in range(k - 1, -1, -1):  # (FIRST: the lowest j is written last)
        if mode == BITS:
            out |= np.asarray(bits[j]).astype(np.uint64) << np.uint64(k - 1 - j)
        else:
            out[np.asarray(bits[j]).astype(bool)] = j
    return out


def values_of(streams, first, n, mode):
    """ref_values as a uint64 array."""
    rows = np.arange(first, first + n, dtype=np.int64)
    return fold([_fetch.bits_at(st, rows) if n else np.zeros(0, np.uint8) for st in streams], mode)


# ---- the kernel's rules -------------------------------------------------------------------------------------------------------------
def halves(mode, k):
    """Items per segment: a bit-sliced attribute of more than 32 table rows is stored in two halves of 4 bytes."""
    return 2 if mode == BITS and k > 32 else 1


def half_rows(mode, k, half, wrong=None):
    """The table rows an item walks.  FIRST: all.  BITS: row 0 is the MOST significant, so the low half (significance 0 .. 31) is the
    LAST min(32, k) table rows and the high half the rows in front of them."""
    if mode == FIRST:
        return range(k)
    low = min(32, k)
    if wrong == "half from the wrong end":
        return range(low) if half == 0 else range(32, k)
    return range(k - low, k) if half == 0 else range(k - 32)


def window_segments(first, n, wrong=None):
    """The segments a window overlaps: those of its first and of its last row, and every one between."""
    if n == 0:
        return range(0)
    last = first + n - 1
    if wrong == "last segment dropped on a seam":
        last = max(last - 1, first)  # (a last row that is a segment's first: that segment is not seen)
    return range(first // SEG_BITS, last // SEG_BITS + 1)


def item_rows(segment, first, n):
    """The rows of the bitmap an item of `segment` stores: the segment's, clipped to the window."""
    return range(max(first, segment * SEG_BITS), min(first + n, (segment + 1) * SEG_BITS))


def items(mode, k, first, n, wrong=None):
    """The launch's items in order: (segment, half)."""
    return [(s, h) for s in window_segments(first, n, wrong) for h in range(halves(mode, k))]


def item_bytes(mode, k, segment, half, first, n):
    """The bytes of d_out an item owns: per stored row the whole 8-byte element, or the 4-byte half (little endian: the low half
    first).  [(first byte, byte count)] per row, in row order."""
    width = 8 // halves(mode, k)
    return [(8 * (r - first) + width * half, width) for r in item_rows(segment, first, n)]


def writes_of(mode, k, first, n, wrong=None):
    """How often the launch's items write every byte of d_out[0 .. n): uint8 [8 n] (item_bytes, vectorised over an item's rows)."""
    writes = np.zeros(8 * n, np.uint8)
    width = 8 // halves(mode, k)
    for segment, half in items(mode, k, first, n, wrong):
        rows = item_rows(segment, first, n)
        at = 8 * (np.arange(rows.start, rows.stop, dtype=np.int64) - first) + width * half
        assert at.size == 0 or (at[0] >= 0 and at[-1] + width <= 8 * n), "a byte outside d_out[0 .. n)"
        for b in range(width):
            writes[at + b] += 1
    return writes


def groups_of_stream(stream):
    """The stream's 31-bit groups, expanded (a test's bitmaps: a few thousand groups)."""
    w, fill, n, _ = _select._walk(stream)
    value = np.where(fill, np.where((w & _select.ONE) != 0, _select.M31, 0), w & _select.M31)
    return np.repeat(value, n).astype(np.int64)


def _bit(groups, p, wrong=None):
    """Row p of a segment-cut stream: bit p % 31 of group p // 31."""
    if wrong == "word 32 addressing":
        return (groups[p // 32] >> (p % 32)) & 1 if p // 32 < groups.size else 0
    return (groups[p // 31] >> (p % 31)) & 1


def model(streams, first, n, mode, wrong=None):
    """The output as the kernel's rules give it: (uint64 [n], writes per byte uint8 [8 n]).  Every item puts the value of its half
    together from its table rows and stores its bytes into a poisoned buffer."""
    k = len(streams)
    groups = [groups_of_stream(st) for st in streams]
    out = np.full(8 * n, POISON, np.uint8)
    writes = np.zeros(8 * n, np.uint8)
    for segment, half in items(mode, k, first, n, wrong):
        rows = half_rows(mode, k, half, wrong)
        for (at, width), p in zip(item_bytes(mode, k, segment, half, first, n), item_rows(segment, first, n)):
            if mode == BITS:
                v = 0
                for j in rows:
                    v |= int(_bit(groups[j], p, wrong)) << ((k - 1 - j) & 31)
            else:
                v = 0xFFFFFFFF
                for j in rows:
                    if _bit(groups[j], p, wrong):
                        v = j if wrong == "first takes the last" else min(v, j)
                if v == 0xFFFFFFFF:
                    v = U64_MAX
            out[at: at + width] = np.frombuffer(int(v).to_bytes(8, "little")[:width], np.uint8)
            writes[at: at + width] += 1
    return out.view("<u8").astype(np.uint64), writes


# ---- the shapes of the GPU tests ----------------------------------------------------------------------------------------------------
SIZES = (1, 31, SEG_WORDS, SEG_WORDS + 1, 2 * SEG_WORDS, 3 * SEG_WORDS - 5)
BITS_WIDTHS = (1, 2, 31, 32, 33, 63, 64)
FIRST_COLUMNS = (1, 63, 64, 65, 129)


def windows(n_words):
    """(first, n) windows of a bitmap of n_words words: the whole bitmap, no row, one row, 30 / 31 / 32 rows around a group's
    neighbourhood, windows that begin and end on, one before and one behind a group edge (multiples of 31), a word edge (multiples
    of 32) and a segment seam, a window wholly inside the second segment, and the last row."""
    n_bits = 32 * n_words
    out = {(0, n_bits), (0, 0), (n_bits, 0), (n_bits - 1, 1), (0, 1)}
    for e in (31, 62, 32, 64, 31 * 32, SEG_BITS, 2 * SEG_BITS):
        for a in (e - 1, e, e + 1):
            for b in (e - 1, e, e + 1):
                out |= {(a, 0), (a, 1), (a, 30), (a, 31), (a, 32), (max(a - 700, 0), 700 + b - a), (a, SEG_BITS + b - a), (3, b - 3)}
    out |= {(SEG_BITS + 100, 5000), (SEG_BITS, SEG_BITS), (SEG_BITS + 1, SEG_BITS - 2)}
    return sorted((a, n) for a, n in out if a >= 0 and n >= 0 and a + n <= n_bits)
