"""CPU tests of the boundary of wah_group_sum_indexed_device (include/wah.h): the symbol exists in the header, in
api.ABI_SYMBOLS and in the library; every argument error the host can see comes back before any HIP call is made, argument
checks first (no GPU here: made-up non-null integers stand in for device pointers, nothing follows them); the scratch is the
count calls', unchanged; and the Python front ends are exported."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wah_group_sum_indexed_device"
WAH_ERR_ARG, WAH_ERR_WORKSPACE = -1, -2
MAX_PAIRS = 1 << 24  # WAH_BITOP_LIST_MAX_OPERANDS


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("gpu-wah_amd")
    p.build()
    return p


def test_symbol_in_header_binding_and_library(pkg):
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    declared = set(re.findall(r"\b(wah_[a-z_0-9]+)\s*\(", header))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path()], text=True)
    assert NAME in declared
    assert NAME in pkg.ABI_SYMBOLS and len(pkg.ABI_SYMBOLS[NAME][1]) == 16
    assert re.search(rf"\bT {NAME}\b", exported)
    assert hasattr(pkg.lib(), NAME)
    for limit, value in (("WAH_GROUP_MAX_FILTERS", 64), ("WAH_GROUP_MAX_ROWS", 8), ("WAH_GROUP_MAX_ATTRS", 64)):
        assert re.search(rf"#define\s+{limit}\s+{value}u\b", header), limit
    assert "one scratch serves all four calls" in header


def _widths(bits):
    return None if bits is None else (ctypes.c_uint8 * max(len(bits), 1))(*bits)


def _group(lib, n_words=992 * 4, n_filters=1, filters=0x4000, n_groups=2, rows_per_group=1, groups=0x8000, n_operands=3, table=0x10000,
           bits=(2, 1), n_attrs=None, rows=0x20000, counts=0x28000, sums=0x30000, scratch=0x100000, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_select_scratch_bytes(min(n_words, (1 << 40) - 1), max(n_operands, 1))
    widths = _widths(bits)
    if n_attrs is None:
        n_attrs = len(bits)
    return lib.wah_group_sum_indexed_device(n_words, n_filters, filters, n_groups, rows_per_group, groups, n_operands, table, n_attrs,
                                            widths, rows, counts, sums, scratch, scratch_bytes, None)


BAD_ARGUMENTS = [
    dict(scratch=None), dict(scratch=0x100000 + 128),                    # null scratch, not 256-byte aligned
    dict(filters=None), dict(filters=0x4004),                            # a null filter table with a filter, a misaligned one
    dict(n_filters=0, filters=0x4004),                                   # misaligned even when it is not read
    dict(n_filters=65),
    dict(groups=None), dict(groups=0x8004), dict(table=None), dict(table=0x10004),
    dict(rows=None), dict(rows=0x20004), dict(counts=None), dict(counts=0x28004), dict(sums=None), dict(sums=0x30004),
    dict(rows_per_group=0), dict(rows_per_group=9), dict(rows_per_group=1 << 63),
    dict(n_groups=0), dict(n_operands=0, bits=(), n_attrs=1), dict(n_operands=0),
    dict(n_groups=MAX_PAIRS // 3 + 1), dict(n_groups=MAX_PAIRS + 1, n_operands=1, bits=(1,)),   # G * K above 2^24
    dict(n_groups=MAX_PAIRS // 8 + 1, rows_per_group=8, n_operands=1, bits=(1,)),               # G * R above 2^24
    dict(n_groups=(1 << 63) + 1, rows_per_group=2, n_operands=1, bits=(1,)),                    # ... and wrapping round 2^64
    dict(n_groups=1 << 62, n_operands=4, bits=(4,)),
    dict(n_attrs=0), dict(n_attrs=65, n_operands=65, bits=(1,) * 65), dict(bits=None, n_attrs=2),
    dict(bits=(0, 3)), dict(bits=(3, 0)), dict(n_operands=65, bits=(65,)), dict(n_operands=255, bits=(255,)),
    dict(bits=(2, 2)), dict(bits=(1, 1)), dict(bits=(4,)), dict(n_operands=4, bits=(2, 1)),    # widths that do not add up
    dict(n_words=1 << 40), dict(n_words=(1 << 64) - 1),
]


def test_argument_errors_come_back_before_any_hip_call(pkg):
    lib = pkg.lib()
    need = lib.wah_select_scratch_bytes(992 * 4, 3)
    for bad in BAD_ARGUMENTS:
        assert _group(lib, **bad) == WAH_ERR_ARG, bad
        assert ctypes.c_char_p(lib.wah_last_error()).value, bad
        # the argument checks come first: a bad argument with too small a scratch is an argument error
        assert _group(lib, scratch_bytes=0, **bad) == WAH_ERR_ARG, bad
    assert _group(lib, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
    assert _group(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE


def test_the_limits_themselves_pass_the_argument_checks(pkg):
    """At every limit the arguments pass, and the next check (the scratch) is reached."""
    lib = pkg.lib()
    for good in (dict(n_filters=0, filters=None), dict(n_filters=64), dict(rows_per_group=8), dict(n_groups=MAX_PAIRS // 8, rows_per_group=8, n_operands=1, bits=(1,)),
                 dict(n_groups=MAX_PAIRS, n_operands=1, bits=(1,)), dict(),
                 dict(n_groups=4096, n_operands=4096, bits=(64,) * 64), dict(n_operands=64, bits=(64,)), dict(n_operands=64, bits=(1,) * 64),
                 dict(n_operands=1, bits=(1,)), dict(n_words=0), dict(n_words=(1 << 40) - 1)):
        assert _group(lib, scratch_bytes=0, **good) == WAH_ERR_WORKSPACE, good


def test_scratch_is_the_count_calls_unchanged(pkg):
    """wah_select_scratch_bytes serves the new call as it is: the same for every table size, and what it was."""
    lib = pkg.lib()
    for n_words in (0, 1, 991, 992, 993, 992 * 37 + 5, 992 * 4096, 268435200, (1 << 40) - 1):
        got = lib.wah_select_scratch_bytes(n_words, 1)
        segments = ((32 * n_words + 30) // 31 + 1023) // 1024
        n0 = segments + 1
        n1 = (n0 + 4095) // 4096
        n2 = (n1 + 4095) // 4096
        r256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
        assert got == 1024 + r256(8 * n0) + r256(8 * n1) + r256(8 * n2), n_words
        for k in (3, 64, 4097, 1 << 24):
            assert lib.wah_select_scratch_bytes(n_words, k) == got, (n_words, k)
        # exactly enough for the new call, whatever the tables' sizes
        assert _group(lib, n_words=n_words, n_filters=7, n_groups=11, rows_per_group=3, scratch_bytes=got - 1) == WAH_ERR_WORKSPACE
        assert _group(lib, n_words=n_words, n_filters=7, n_groups=11, rows_per_group=3, scratch_bytes=0) == WAH_ERR_WORKSPACE


def test_python_front_ends_are_exported(pkg):
    assert callable(pkg.group_sum_device)
    assert callable(pkg.columns.aggregate_columns) and callable(pkg.columns.extremes_by)
    assert "wah_group_sum_indexed_device" in pkg.group_sum_device.__doc__
    assert "wah_group_sum_indexed_device" in pkg.columns.aggregate_columns.__doc__
    assert "G x 2 calls" in pkg.columns.extremes_by.__doc__ and "host read" in pkg.columns.extremes_by.__doc__
    assert "AVG" in pkg.columns.aggregate_columns.__doc__
    assert (pkg.api.GROUP_MAX_FILTERS, pkg.api.GROUP_MAX_ROWS, pkg.api.GROUP_MAX_ATTRS) == (64, 8, 64)
