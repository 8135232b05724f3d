"""CPU tests of the running-sum call's boundary (include/wah.h: wah_bsi_cumsum_indexed_device): the three symbols are declared,
mirrored and exported, the scratch is the builder's layout plus eight bytes per segment, and every refusal the host can see comes
back with its code and its text, in the order the header states, before any HIP call -- so without a device."""
import importlib
import os
import re

import pytest

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
EXISTS, EXCLUSIVE, ALL_ROWS = 1, 2, 4
NAMES = ("wah_bsi_cumsum_scratch_bytes", "wah_bsi_cumsum_indexed_device", "wah_bsi_cumsum_status")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 992


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.build()
    return pkg.lib()


def test_symbols_are_declared_mirrored_and_exported(lib):
    pkg = importlib.import_module("gpu-wah_amd")
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define WAH_CUMSUM_EXCLUSIVE 2u", header) and re.search(r"#define WAH_CUMSUM_ALL_ROWS 4u", header)
    assert (pkg.CUMSUM_EXCLUSIVE, pkg.CUMSUM_ALL_ROWS, pkg.BSI_EXISTS) == (EXCLUSIVE, ALL_ROWS, EXISTS)
    assert len({EXISTS, EXCLUSIVE, ALL_ROWS}) == 3
    assert callable(pkg.bsi_cumsum_device)
    for name in ("cumsum_column", "row_numbers_where"):
        assert callable(getattr(pkg.columns, name)), name


def _round256(x):
    return (x + 255) & ~255


def test_scratch_is_the_builders_layout_and_the_totals(lib):
    """include/wah.h states the formula: wah_bsi_build_scratch_bytes(n_words, rows_out) + 8 bytes per segment rounded up to 256,
    rows_out = n_slices_out and one more row unless WAH_CUMSUM_ALL_ROWS.  The edges: 32 and 33 segments, where the totals pass 256
    bytes, one slice and sixty-four, the largest bitmap."""
    big = SEG * ((1 << 40) // SEG // 66)
    for n in (SEG, 3 * SEG, 32 * SEG, 33 * SEG, SEG << 10, big):
        for k in (1, 7, 32, 33, 64):
            for flags in range(8):
                rows_out = k + (0 if flags & ALL_ROWS else 1)
                want = lib.wah_bsi_build_scratch_bytes(n, rows_out) + _round256(8 * (n // SEG))
                assert lib.wah_bsi_cumsum_scratch_bytes(n, k, flags) == want and want % 256 == 0 and want > 0, (n, k, flags)
    assert lib.wah_bsi_cumsum_scratch_bytes(32 * SEG, 1, 0) - lib.wah_bsi_build_scratch_bytes(32 * SEG, 2) == 256
    assert lib.wah_bsi_cumsum_scratch_bytes(33 * SEG, 1, 0) - lib.wah_bsi_build_scratch_bytes(33 * SEG, 2) == 512


# pointers that are never followed: every call below is refused on the host
FILT, VAL, OUT, COUNT, OFFS, SCRATCH = 0x20000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000


def _call(lib, n_words=SEG, n_rows=SEG * 32, n_filters=2, filters=FILT, kv=20, val=VAL, k_out=40, flags=0, out=OUT, cap=1 << 20, count=COUNT,
          offs=OFFS, scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bsi_cumsum_scratch_bytes(n_words, k_out, flags)
    return lib.wah_bsi_cumsum_indexed_device(n_words, n_rows, n_filters, filters, kv, val, k_out, flags, out, cap, count, offs, scratch,
                                             scratch_bytes, None)


BIG = SEG * ((1 << 40) // SEG)  # the largest multiple of 992 below 2^40

REFUSED = (
    # (1) widths, flags and the filter count
    dict(kv=33), dict(kv=1 << 32), dict(k_out=0), dict(k_out=65), dict(k_out=1 << 32), dict(flags=8), dict(flags=8 | EXISTS), dict(flags=1 << 31),
    dict(n_filters=65), dict(n_filters=1 << 32),
    # (2) pointers and alignment, and a value table that does not go with n_slices_val and the flags
    dict(scratch=None), dict(scratch=SCRATCH + 128), dict(scratch=SCRATCH + 8), dict(out=None), dict(out=OUT + 2), dict(count=None),
    dict(count=COUNT + 4), dict(offs=None), dict(offs=OFFS + 4), dict(val=None), dict(val=VAL + 4), dict(kv=0), dict(kv=0, flags=EXISTS, val=None),
    dict(kv=0, flags=ALL_ROWS | EXCLUSIVE), dict(filters=None), dict(filters=FILT + 4), dict(n_filters=0, filters=FILT + 4),
    # (3) the sizes
    dict(n_words=0, n_rows=0), dict(n_words=SEG + 1), dict(n_words=31, n_rows=0), dict(n_words=BIG + SEG, n_rows=0), dict(n_words=1 << 40, n_rows=0),
    dict(n_words=BIG // 32 + SEG - (BIG // 32) % SEG, k_out=32, n_rows=0), dict(n_words=BIG // 32 + SEG - (BIG // 32) % SEG, k_out=33, flags=ALL_ROWS, n_rows=0),
    dict(n_rows=SEG * 32 + 1), dict(n_rows=1 << 62),
)

LEGAL = (
    dict(), dict(flags=EXISTS), dict(flags=EXCLUSIVE), dict(flags=ALL_ROWS), dict(flags=EXISTS | EXCLUSIVE | ALL_ROWS), dict(kv=1), dict(kv=32, k_out=64),
    dict(k_out=1), dict(kv=0, val=None), dict(kv=0, flags=EXISTS), dict(n_filters=0, filters=None), dict(n_filters=0), dict(n_filters=64), dict(n_rows=0),
    dict(n_rows=SEG * 32 - 1), dict(cap=0), dict(n_words=3 * SEG, n_rows=3 * SEG * 32), dict(n_words=BIG, k_out=1, flags=ALL_ROWS, n_rows=0),
    dict(n_words=BIG // 32 + SEG - (BIG // 32) % SEG, k_out=31, flags=ALL_ROWS, n_rows=0),
)


def test_host_visible_refusals(lib):
    for kw in REFUSED:
        assert _call(lib, scratch_bytes=1 << 62, **kw) == WAH_ERR_ARG, kw
        assert lib.wah_last_error(), kw
        # the argument checks come first: a bad argument AND too small a scratch is a bad argument
        assert _call(lib, scratch_bytes=0, **kw) == WAH_ERR_ARG, kw
    assert lib.wah_bsi_cumsum_status(None, SEG, 17, 0, None) == WAH_ERR_ARG


def test_each_legal_extreme_reaches_the_scratch_check(lib):
    for kw in LEGAL:
        need = lib.wah_bsi_cumsum_scratch_bytes(kw.get("n_words", SEG), kw.get("k_out", 40), kw.get("flags", 0))
        assert _call(lib, scratch_bytes=need - 1, **kw) == WAH_ERR_WORKSPACE, kw
        assert lib.wah_last_error().decode() == "scratch too small", kw
        assert _call(lib, scratch_bytes=0, **kw) == WAH_ERR_WORKSPACE, kw


def test_the_refusals_texts(lib):
    def text(**kw):
        assert _call(lib, scratch_bytes=1 << 62, **kw) == WAH_ERR_ARG
        return lib.wah_last_error().decode()

    for kw in (dict(kv=33), dict(k_out=0), dict(k_out=65), dict(flags=8), dict(n_filters=65)):
        assert text(**kw).startswith("a value of at most 32 slices, a result of 1 to 64, no flag besides WAH_BSI_EXISTS"), kw
        assert "at most 64 filter rows" in text(**kw), kw
    for kw in (dict(scratch=None), dict(out=OUT + 2), dict(offs=None), dict(val=None), dict(kv=0), dict(filters=None)):
        assert text(**kw).startswith("null or misaligned scratch or output, a value table that does not go with n_slices_val"), kw
    for kw in (dict(n_words=0, n_rows=0), dict(n_words=SEG + 1), dict(n_words=1 << 40, n_rows=0), dict(n_rows=SEG * 32 + 1)):
        assert text(**kw) == "slices of a multiple of 992 words, all slices of the result together fewer than 2^40 words, at most 32 n_words rows", kw


def test_the_stated_order_of_the_refusals(lib):
    """include/wah.h: (1) widths, flags and the filter count, (2) scratch, output, value table and filter table, (3) the sizes, then
    the scratch's size.  The text of wah_last_error names the first one that fails."""
    def text(**kw):
        kw.setdefault("scratch_bytes", 1 << 62)
        assert _call(lib, **kw) in (WAH_ERR_ARG, WAH_ERR_WORKSPACE)
        return lib.wah_last_error().decode()

    first, second, third, size = text(kv=33), text(val=None), text(n_words=SEG + 1), text(scratch_bytes=0)
    assert len({first, second, third, size}) == 4
    assert text(kv=33, val=None, n_words=SEG + 1, scratch_bytes=0) == first
    assert text(flags=8, scratch=None) == first
    assert text(k_out=65, filters=None) == first
    assert text(n_filters=65, n_rows=1 << 62) == first
    assert text(val=None, n_words=SEG + 1, scratch_bytes=0) == second
    assert text(scratch=SCRATCH + 8, n_words=0) == second
    assert text(offs=None, n_rows=1 << 62) == second
    assert text(filters=None, n_words=1 << 40) == second
    assert text(n_words=SEG + 1, scratch_bytes=0) == third
    assert text(n_rows=SEG * 32 + 1, scratch_bytes=0) == third
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
