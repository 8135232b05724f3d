"""CPU tests of the partition-total call's boundary (include/wah.h: wah_bsi_total_parts_indexed_device): the three symbols are declared,
mirrored and exported, the scratch is the builder's layout plus twenty-four bytes per segment, every refusal the host can see comes
back with its code and its own text, in the groups and the order of the partitioned running sum -- WAH_CUMSUM_EXCLUSIVE among the
unknown flag bits -- before any HIP call, so without a device, and the partitioned running sum's refusals are what they were."""
import importlib
import os
import re

import pytest

from tests import _total_parts as tp, test_bsi_cumsum_abi as plain, test_bsi_cumsum_parts_abi as parts

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
EXISTS, EXCLUSIVE, ALL_ROWS = 1, 2, 4
NAMES = ("wah_bsi_total_parts_scratch_bytes", "wah_bsi_total_parts_indexed_device", "wah_bsi_total_parts_status")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 992
PREFIX = "partition totals: "


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.build()
    return pkg.lib()


def test_symbols_are_declared_mirrored_and_exported(lib):
    pkg = importlib.import_module("gpu-wah_amd")
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    for name, n_args in zip(NAMES, (3, 16, 5)):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name) and len(pkg.ABI_SYMBOLS[name][1]) == n_args, name
    # the argument list of the partitioned running sum
    for mine, theirs in zip(NAMES, parts.NAMES):
        assert pkg.ABI_SYMBOLS[mine] == pkg.ABI_SYMBOLS[theirs], mine
    assert callable(pkg.bsi_total_parts_device)
    for name in ("total_column_by", "partition_sizes", "mean_column_by", "rows_of_partitions_where"):
        assert callable(getattr(pkg.columns, name)), name
    # the two running sums' "Not here" lists no longer name the totals, they point here
    assert "Not here: partition totals" not in header and header.count("wah_bsi_total_parts_indexed_device, below") == 2


def _round256(x):
    return (x + 255) & ~255


def test_scratch_is_the_builders_layout_and_the_records(lib):
    """include/wah.h states the formula: wah_bsi_build_scratch_bytes(n_words, rows_out) + 24 bytes per segment rounded up to 256.
    The edges: 10, 11, 21 and 22 segments, where the records pass 256 and 512 bytes, one slice and sixty-four, the largest bitmap."""
    assert tp.RECORD_BYTES == 24
    big = SEG * ((1 << 40) // SEG // 66)
    for n in (SEG, 3 * SEG, 10 * SEG, 11 * SEG, 21 * SEG, 22 * SEG, SEG << 10, big):
        for k in (1, 7, 32, 33, 64):
            for flags in (0, EXISTS, ALL_ROWS, EXISTS | ALL_ROWS):
                rows_out = k + (0 if flags & ALL_ROWS else 1)
                want = lib.wah_bsi_build_scratch_bytes(n, rows_out) + _round256(24 * (n // SEG))
                assert lib.wah_bsi_total_parts_scratch_bytes(n, k, flags) == want and want % 256 == 0 and want > 0, (n, k, flags)
    assert lib.wah_bsi_total_parts_scratch_bytes(10 * SEG, 1, 0) - lib.wah_bsi_build_scratch_bytes(10 * SEG, 2) == 256
    assert lib.wah_bsi_total_parts_scratch_bytes(11 * SEG, 1, 0) - lib.wah_bsi_build_scratch_bytes(11 * SEG, 2) == 512
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    assert re.search(r"wah_bsi_total_parts_scratch_bytes\(n_words, n_slices_out, flags\) = wah_bsi_build_scratch_bytes\(n_words, rows_out\) \+ 24", header)


# pointers that are never followed: every call below is refused on the host
FILT, VAL, OUT, COUNT, OFFS, SCRATCH, STARTS = plain.FILT, plain.VAL, plain.OUT, plain.COUNT, plain.OFFS, plain.SCRATCH, parts.STARTS


def _call(lib, n_words=SEG, n_rows=SEG * 32, n_filters=2, filters=FILT, kv=20, val=VAL, starts=STARTS, k_out=40, flags=0, out=OUT, cap=1 << 20,
          count=COUNT, offs=OFFS, scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bsi_total_parts_scratch_bytes(n_words, k_out, flags)
    return lib.wah_bsi_total_parts_indexed_device(n_words, n_rows, n_filters, filters, kv, val, starts, k_out, flags, out, cap, count, offs, scratch,
                                                  scratch_bytes, None)


# the partitioned running sum's refusals, every one, and WAH_CUMSUM_EXCLUSIVE alone and beside every legal flag
REFUSED = parts.REFUSED + (dict(flags=EXCLUSIVE), dict(flags=EXCLUSIVE | EXISTS), dict(flags=EXCLUSIVE | ALL_ROWS), dict(flags=EXCLUSIVE | EXISTS | ALL_ROWS))
LEGAL = tuple(kw for kw in parts.LEGAL if not kw.get("flags", 0) & EXCLUSIVE) + (dict(flags=EXISTS | ALL_ROWS),)


def test_host_visible_refusals(lib):
    assert len(LEGAL) == len(parts.LEGAL) - 1  # (two with EXCLUSIVE left, one came)
    for kw in REFUSED:
        assert _call(lib, scratch_bytes=1 << 62, **kw) == WAH_ERR_ARG, kw
        assert lib.wah_last_error().decode().startswith(PREFIX), kw
        # the argument checks come first: a bad argument AND too small a scratch is a bad argument
        assert _call(lib, scratch_bytes=0, **kw) == WAH_ERR_ARG, kw
    assert lib.wah_bsi_total_parts_status(None, SEG, 17, 0, None) == WAH_ERR_ARG


def test_each_legal_extreme_reaches_the_scratch_check(lib):
    for kw in LEGAL:
        need = lib.wah_bsi_total_parts_scratch_bytes(kw.get("n_words", SEG), kw.get("k_out", 40), kw.get("flags", 0))
        assert _call(lib, scratch_bytes=need - 1, **kw) == WAH_ERR_WORKSPACE, kw
        assert lib.wah_last_error().decode() == PREFIX + "scratch too small", kw
        assert _call(lib, scratch_bytes=0, **kw) == WAH_ERR_WORKSPACE, kw


def test_the_refusals_texts(lib):
    def text(**kw):
        assert _call(lib, scratch_bytes=1 << 62, **kw) == WAH_ERR_ARG
        return lib.wah_last_error().decode()

    for kw in (dict(kv=33), dict(k_out=0), dict(k_out=65), dict(flags=8), dict(flags=EXCLUSIVE), dict(flags=EXCLUSIVE | ALL_ROWS), dict(n_filters=65)):
        assert text(**kw) == PREFIX + ("a value of at most 32 slices, a result of 1 to 64, no flag besides WAH_BSI_EXISTS and WAH_CUMSUM_ALL_ROWS, "
                                       "at most 64 filter rows"), kw
    for kw in (dict(scratch=None), dict(out=OUT + 2), dict(offs=None), dict(val=None), dict(kv=0), dict(filters=None), dict(starts=None),
               dict(starts=STARTS + 4)):
        assert text(**kw).startswith(PREFIX + "null or misaligned scratch or output, a value table that does not go with n_slices_val"), kw
        assert text(**kw).endswith("or a null or misaligned starts row"), kw
    for kw in (dict(n_words=0, n_rows=0), dict(n_words=SEG + 1), dict(n_words=1 << 40, n_rows=0), dict(n_rows=SEG * 32 + 1)):
        assert text(**kw) == PREFIX + "slices of a multiple of 992 words, all slices of the result together fewer than 2^40 words, at most 32 n_words rows", kw


def test_the_stated_order_of_the_refusals(lib):
    """include/wah.h: the partitioned running sum's order, WAH_CUMSUM_EXCLUSIVE in the first group."""
    def text(**kw):
        kw.setdefault("scratch_bytes", 1 << 62)
        assert _call(lib, **kw) in (WAH_ERR_ARG, WAH_ERR_WORKSPACE)
        return lib.wah_last_error().decode()

    first, second, third, size = text(kv=33), text(starts=None), text(n_words=SEG + 1), text(scratch_bytes=0)
    assert len({first, second, third, size}) == 4
    assert text(kv=33, starts=None, n_words=SEG + 1, scratch_bytes=0) == first
    assert text(flags=EXCLUSIVE, starts=None, n_words=SEG + 1, scratch_bytes=0) == first
    assert text(flags=8, starts=STARTS + 4) == first
    assert text(n_filters=65, n_rows=1 << 62) == first
    assert text(val=None) == second and text(filters=None, n_words=1 << 40) == second
    assert text(starts=None, n_words=SEG + 1, scratch_bytes=0) == second
    assert text(starts=STARTS + 4, n_rows=1 << 62) == second
    assert text(n_words=SEG + 1, scratch_bytes=0) == third
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE


def test_the_partitioned_running_sums_refusals_are_unaffected(lib):
    """The partitioned running sum, called: its codes, its texts (none carries this call's prefix) and its order; it still takes
    WAH_CUMSUM_EXCLUSIVE."""
    parts.test_host_visible_refusals(lib)
    parts.test_each_legal_extreme_reaches_the_scratch_check(lib)
    parts.test_the_refusals_texts(lib)
    parts.test_the_stated_order_of_the_refusals(lib)
    assert parts._call(lib, kv=33, scratch_bytes=1 << 62) == WAH_ERR_ARG and not lib.wah_last_error().decode().startswith(PREFIX)
    assert parts._call(lib, flags=EXCLUSIVE, scratch_bytes=0) == WAH_ERR_WORKSPACE
