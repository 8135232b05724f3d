"""Reference and input builders for wah_from_positions_device (include/wah.h): compressed bitmaps from sorted lists of row
numbers.  No GPU, no library: tests/test_rows_reference.py proves the builders against the CPU oracle,
tests/test_gpu_from_positions.py holds the kernels against the reference.

The reference goes the long way round on purpose: every list becomes its decoded bitmap (_select.bitmap_of), the oracle
compresses it, and _select.index_of reads the segment index off the words."""
import numpy as np

from tests import _select

SEG_GROUPS, SEG_WORDS, SEG_BITS = _select.SEG_GROUPS, _select.SEG_WORDS, _select.SEG_BITS
WAVE = 64            # rows a wavefront classifies in registers, one per lane; one more goes through the LDS image
RANK_CHUNK = 4096    # entries per workgroup of the index's prefix sum

EMPTY, REGISTERS, IMAGE = "no row", "registers", "image"


def route_of(rows_in_segment):
    return EMPTY if rows_in_segment == 0 else REGISTERS if rows_in_segment <= WAVE else IMAGE


def max_words(n_words, n_lists, n_rows):
    g = _select.groups_of(n_words)
    return min(n_lists * g, n_lists * _select.segments_of(n_words) + 2 * n_rows)


def reference(oracle, lists, n_words):
    """(stream, index) of the call: the lists' compress() streams back to back, and n_lists * S + 1 index entries counted from
    the first word of the whole."""
    segments = _select.segments_of(n_words)
    streams, index, at = [], [], 0
    for rows in lists:
        st = np.ascontiguousarray(oracle.compress(_select.bitmap_of(rows, n_words)), dtype=np.uint32)
        own = _select.index_of(st)
        assert own.size == segments + 1, (own.size, segments)
        index.append(own[:-1] + at)
        streams.append(st)
        at += st.size
    index.append(np.array([at], np.int64))
    return np.concatenate(streams), np.concatenate(index).astype(np.int64)


def segment_words(stream_index):
    return np.diff(stream_index)


def rows_per_segment(rows, n_words):
    return np.bincount(np.asarray(rows, np.int64) // SEG_BITS, minlength=_select.segments_of(n_words))[: _select.segments_of(n_words)]


def flatten(lists):
    """(rows, ends) as the call takes them."""
    rows = np.concatenate([np.asarray(r, np.int64).reshape(-1) for r in lists] + [np.empty(0, np.int64)])
    ends = np.cumsum([len(r) for r in lists]).astype(np.int64)
    return rows, ends


# ---- builders: (name, n_words, rows, claimed words of every segment) ----------------------------------------------------------
def _run(first_group, groups):
    return np.arange(31 * first_group, 31 * (first_group + groups), dtype=np.int64)


def spread(k):
    """k rows of one segment in k different groups with a gap between any two, the first one in group 0: k literals, k - 1
    gaps and the gap behind the last one."""
    assert k <= 65
    return np.arange(k, dtype=np.int64) * 487 + 3


def switch_cases():
    out = []
    one = SEG_WORDS
    for k in (0, 1, 2, 63, 64, 65):
        out.append((f"{k} rows in one segment", one, spread(k), [2 * k if k else 1]))
    out.append(("31743 rows: all but one", one, np.delete(np.arange(SEG_BITS, dtype=np.int64), 5000), [3]))
    out.append(("31744 rows: the whole segment", one, np.arange(SEG_BITS, dtype=np.int64), [1]))
    for groups in (1, 2, 3):
        k = 31 * groups
        out.append((f"run of {k} alone", one, _run(10, groups), [3]))
        out.append((f"run of {k} touching a literal behind it", one, np.concatenate([_run(10, groups), [31 * (10 + groups) + 4]]), [4]))
        out.append((f"run of {k} touching a literal in front of it", one, np.concatenate([[31 * 9 + 30], _run(10, groups)]), [4]))
        out.append((f"run of {k} at the first group", one, _run(0, groups), [2]))
        out.append((f"run of {k} at the last group", one, _run(SEG_GROUPS - groups, groups), [2]))
    # (a group-aligned run of 31 rows is one group: it cannot straddle a segment edge; the run of 31 below is not aligned)
    out.append(("run of 62 across a segment edge", 2 * one, _run(SEG_GROUPS - 1, 2), [2, 2]))
    out.append(("run of 93 across a segment edge", 2 * one, _run(SEG_GROUPS - 1, 3), [2, 2]))
    out.append(("run of 93 across a segment edge, two groups in front", 2 * one, _run(SEG_GROUPS - 2, 3), [2, 2]))
    out.append(("31 rows across a segment edge, not group aligned", 2 * one, np.arange(SEG_BITS - 15, SEG_BITS + 16, dtype=np.int64), [2, 2]))
    out.append(("the last real bit of a ragged bitmap", 993, np.array([32 * 993 - 1], np.int64), [1, 2]))
    out.append(("the last real bit of a one-word bitmap", 1, np.array([31], np.int64), [2]))
    out.append(("64 rows in 64 neighbouring groups", one, np.array([31 * g + g % 31 for g in range(64)], np.int64), [65]))
    out.append(("64 rows in 3 groups: two all ones that touch, and two bits", one, np.concatenate([_run(5, 2), [31 * 7 + 3, 31 * 7 + 30]]), [4]))
    out.append(("64 rows in 3 groups: all ones, two bits, all ones", one, np.concatenate([_run(5, 1), [31 * 6, 31 * 6 + 9], _run(7, 1)]), [5]))
    out.append(("one bit in every second group, gaps at both ends", one, np.array([31 * g + 7 for g in range(1, SEG_GROUPS - 1, 2)], np.int64), [SEG_GROUPS - 1]))
    out.append(("one bit in every second group from the first", one, np.array([31 * g for g in range(0, SEG_GROUPS, 2)], np.int64), [SEG_GROUPS]))
    out.append(("all literals", 2 * one, np.array([31 * g + g % 31 for g in range(2 * SEG_GROUPS)], np.int64), [SEG_GROUPS, SEG_GROUPS]))
    out.append(("fills across the steps of the image", one, np.concatenate([_run(3, 200), [31 * 300 + 1], _run(640, 384)]), [6]))
    return [(name, n, np.asarray(rows, np.int64), list(words)) for name, n, rows, words in out]


def switch_cases_by_length():
    """n_words -> the rows of all switch cases of that length, in order: the lists of ONE call."""
    out = {}
    for _, n, rows, _ in switch_cases():
        out.setdefault(n, []).append(rows)
    return out


# the two inputs that meet the size bound with equality: by its second term (S + 2 rows) and by its first (n_lists * G)
BOUND_MET_BY_ROWS = "one bit in every second group, gaps at both ends"
BOUND_MET_BY_GROUPS = "all literals"


def parity_lists(oracle, n_words):
    """The set bits of the ten bitmaps of _select.bitmaps as ten lists."""
    return [_select.ref_positions(b, n_words) for b in _select.bitmaps(oracle, n_words).values()]


def many_lists(n_lists):
    """List c: one row, at position c mod 31744."""
    return [np.array([c % SEG_BITS], np.int64) for c in range(n_lists)]


def one_row_words(p, n_words):
    """Words of the bitmap whose only set bit is p: the literal, a gap on either side of it unless it sits in the first or the
    last group of its segment, and one zero-fill for every other segment."""
    groups, segments = _select.groups_of(n_words), _select.segments_of(n_words)
    g = p // 31
    in_segment = min(groups - SEG_GROUPS * (g // SEG_GROUPS), SEG_GROUPS)
    return 1 + (g % SEG_GROUPS > 0) + (g % SEG_GROUPS < in_segment - 1) + segments - 1


MANY_LISTS = ((4095, SEG_WORDS), (4096, SEG_WORDS), (4097, SEG_WORDS), (1366, 3 * SEG_WORDS))
