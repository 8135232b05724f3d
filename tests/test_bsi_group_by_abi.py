"""CPU tests of the group-by call's boundary (include/wah.h: wah_bsi_group_by_indexed_device): the three symbols are declared,
mirrored and exported, the scratch is the control words, and every refusal the host can see comes back with its code, in the
order the header states, before any HIP call -- so without a device."""
import importlib
import os
import re

import pytest

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
EXISTS, ACCUMULATE = 1, 2
MAX_BUCKETS, MAX_FILTERS = 1 << 30, 64
NAMES = ("wah_bsi_group_by_scratch_bytes", "wah_bsi_group_by_indexed_device", "wah_bsi_group_by_status")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    assert re.search(r"#define WAH_GROUP_BY_ACCUMULATE 2u", header) and re.search(r"#define WAH_GROUP_BY_MAX_BUCKETS \(1u << 30\)", header)
    assert (pkg.GROUP_BY_ACCUMULATE, pkg.GROUP_BY_MAX_BUCKETS, pkg.BSI_EXISTS, pkg.GROUP_MAX_FILTERS) == (ACCUMULATE, MAX_BUCKETS, EXISTS, MAX_FILTERS)
    assert callable(pkg.bsi_group_by_device)
    for name in ("group_by_column", "group_by_joined", "count_distinct_where"):
        assert callable(getattr(pkg.columns, name)), name


def test_scratch_is_the_control_words(lib):
    """include/wah.h states the formula: 1024 bytes for every n_words -- a multiple of 256, never 0."""
    for n in (0, 1, 31, 992, 992 * 3 + 5, 1 << 23, (1 << 40) - 1):
        assert lib.wah_bsi_group_by_scratch_bytes(n) == 1024


# pointers that are never followed: every call below is refused on the host
FILTERS, KEY, VAL, MAP, COUNTS, SUMS, SCRATCH = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000


def _call(lib, n_words=992, n_rows=992 * 32, n_filters=2, filters=FILTERS, ks=20, key=KEY, vs=17, val=VAL, lookup=MAP, n_keys=1000, n_buckets=256,
          flags=0, counts=COUNTS, sums=SUMS, scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bsi_group_by_scratch_bytes(n_words)
    return lib.wah_bsi_group_by_indexed_device(n_words, n_rows, n_filters, filters, ks, key, vs, val, lookup, n_keys, n_buckets, flags, counts, sums,
                                               scratch, scratch_bytes, None)


COUNT_ONLY = dict(vs=0, val=None, sums=None)
NO_MAP = dict(lookup=None, n_keys=0)

REFUSED = (
    # (1) widths, flags, the number of filters
    dict(ks=0), dict(ks=33), dict(ks=1 << 32), dict(vs=33), dict(vs=1 << 32), dict(flags=4), dict(flags=4 | EXISTS), dict(flags=1 << 31),
    dict(n_filters=MAX_FILTERS + 1), dict(n_filters=1 << 32),
    # (2) the tables and the scratch
    dict(key=None), dict(key=KEY + 4), dict(scratch=None), dict(scratch=SCRATCH + 128), dict(scratch=SCRATCH + 8), dict(val=None), dict(val=VAL + 4),
    dict(vs=0), dict(vs=0, sums=None), dict(filters=None), dict(filters=FILTERS + 4),
    # (3) the map
    dict(lookup=None), dict(n_keys=0), dict(lookup=MAP + 2), dict(lookup=MAP + 1), dict(n_keys=(1 << 32) + 1),
    # (4) the buckets and the outputs
    dict(n_buckets=0), dict(n_buckets=MAX_BUCKETS + 1), dict(counts=None), dict(counts=COUNTS + 4), dict(sums=None), dict(sums=SUMS + 4),
    dict(vs=0, val=None),
    # (5) the bitmap
    dict(n_words=1 << 40, n_rows=0), dict(n_rows=992 * 32 + 1), dict(n_words=0, n_rows=1),
)

LEGAL = (
    dict(), dict(flags=EXISTS | ACCUMULATE), dict(ks=1), dict(ks=32, vs=32), dict(vs=1), COUNT_ONLY, dict(COUNT_ONLY, **NO_MAP), NO_MAP,
    dict(n_filters=0, filters=None), dict(n_filters=0), dict(n_filters=MAX_FILTERS), dict(lookup=MAP + 4, n_keys=1), dict(n_keys=1 << 32),
    dict(n_buckets=1), dict(n_buckets=MAX_BUCKETS), dict(n_rows=0), dict(n_rows=992 * 32 - 1), dict(n_words=0, n_rows=0),
    dict(n_words=(1 << 40) - 1, n_rows=32 * ((1 << 40) - 1)),
)


def test_host_visible_refusals(lib):
    for kw in REFUSED:
        assert _call(lib, **kw) == WAH_ERR_ARG, kw
        assert lib.wah_last_error(), kw
        # the argument checks come first: a bad argument AND too small a scratch is a bad argument
        assert _call(lib, scratch_bytes=0, **kw) == WAH_ERR_ARG, kw
    assert lib.wah_bsi_group_by_status(None, None) == WAH_ERR_ARG


def test_each_legal_extreme_reaches_the_scratch_check(lib):
    for kw in LEGAL:
        need = lib.wah_bsi_group_by_scratch_bytes(kw.get("n_words", 992))
        assert _call(lib, scratch_bytes=need - 1, **kw) == WAH_ERR_WORKSPACE, kw
        assert _call(lib, scratch_bytes=0, **kw) == WAH_ERR_WORKSPACE, kw


def test_the_stated_order_of_the_refusals(lib):
    """include/wah.h: (1) widths, flags and the number of filters, (2) tables and scratch, (3) the map, (4) buckets and outputs, (5)
    the bitmap's length and rows, then the scratch's size.  The text of wah_last_error names the first one that fails."""
    def text(**kw):
        assert _call(lib, **kw) in (WAH_ERR_ARG, WAH_ERR_WORKSPACE)
        return lib.wah_last_error().decode()

    first, second, third, fourth, fifth, size = (text(ks=0), text(key=None), text(lookup=MAP + 2), text(n_buckets=0), text(n_words=1 << 40, n_rows=0),
                                                 text(scratch_bytes=0))
    assert len({first, second, third, fourth, fifth, size}) == 6
    assert text(ks=0, key=None, lookup=MAP + 2, n_buckets=0, n_rows=1 << 62, scratch_bytes=0) == first
    assert text(flags=4, scratch=None) == first
    assert text(n_filters=MAX_FILTERS + 1, filters=None) == first
    assert text(vs=33, val=None) == first
    assert text(key=None, lookup=MAP + 2, n_buckets=0, n_rows=1 << 62, scratch_bytes=0) == second
    assert text(val=None, n_keys=0) == second
    assert text(filters=None, counts=None) == second
    assert text(scratch=SCRATCH + 8, n_keys=(1 << 32) + 1) == second
    assert text(lookup=MAP + 2, n_buckets=0, n_rows=1 << 62, scratch_bytes=0) == third
    assert text(lookup=None, counts=None) == third
    assert text(n_keys=(1 << 32) + 1, n_words=1 << 40) == third
    assert text(n_buckets=0, n_rows=1 << 62, scratch_bytes=0) == fourth
    assert text(sums=None, n_words=1 << 40) == fourth
    assert text(counts=COUNTS + 4, n_rows=992 * 32 + 1) == fourth
    assert text(n_rows=992 * 32 + 1, scratch_bytes=0) == fifth
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
