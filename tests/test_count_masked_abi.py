"""CPU tests of the boundary of wah_count_masked_indexed_device (include/wah.h): the symbol exists in the header, in
api.ABI_SYMBOLS and in the library; every argument error the host can see comes back before any HIP call is made, argument
checks first (no GPU here: made-up non-null integers stand in for device pointers, nothing follows them); the scratch is the
count call's, unchanged; and the Python front ends are exported."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wah_count_masked_indexed_device"
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
    assert NAME in pkg.ABI_SYMBOLS and len(pkg.ABI_SYMBOLS[NAME][1]) == 9
    assert re.search(rf"\bT {NAME}\b", exported)
    assert hasattr(pkg.lib(), NAME)
    assert re.search(r"#define\s+WAH_BITOP_LIST_MAX_OPERANDS\s+\(1u << 24\)", header)


def _masked(lib, n_words=992 * 4, n_masks=2, masks=0x8000, n_operands=3, table=0x10000, counts=0x20000, scratch=0x100000, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_select_scratch_bytes(min(n_words, (1 << 40) - 1), max(n_operands, 1))
    return lib.wah_count_masked_indexed_device(n_words, n_masks, masks, n_operands, table, counts, scratch, scratch_bytes, None)


def test_argument_errors_come_back_before_any_hip_call(pkg):
    lib = pkg.lib()
    assert _masked(lib, n_masks=0) == WAH_ERR_ARG
    assert _masked(lib, n_operands=0) == WAH_ERR_ARG
    assert _masked(lib, scratch=None) == WAH_ERR_ARG                      # null scratch
    assert _masked(lib, scratch=0x100000 + 128) == WAH_ERR_ARG            # not 256-byte aligned
    assert _masked(lib, masks=None) == WAH_ERR_ARG                        # null mask table
    assert _masked(lib, masks=0x8004) == WAH_ERR_ARG                      # mask table not 8-byte aligned
    assert _masked(lib, table=None) == WAH_ERR_ARG                        # null operand table
    assert _masked(lib, table=0x10004) == WAH_ERR_ARG                     # operand table not 8-byte aligned
    assert _masked(lib, counts=None) == WAH_ERR_ARG
    assert _masked(lib, counts=0x20004) == WAH_ERR_ARG
    assert _masked(lib, n_words=1 << 40) == WAH_ERR_ARG
    assert ctypes.c_char_p(lib.wah_last_error()).value
    need = lib.wah_select_scratch_bytes(992 * 4, 3)
    assert _masked(lib, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
    assert _masked(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
    # the argument checks come first: a bad argument with too small a scratch is an argument error
    for bad in (dict(n_masks=0), dict(n_operands=0), dict(masks=None), dict(table=None), dict(counts=None), dict(n_words=1 << 40),
                dict(n_masks=MAX_PAIRS, n_operands=2)):
        assert _masked(lib, scratch_bytes=0, **bad) == WAH_ERR_ARG, bad


def test_more_than_2_to_the_24_pairs_are_refused(pkg):
    """The limit is on n_masks * n_operands; at the limit the arguments pass, and the next check (the scratch) is reached."""
    lib = pkg.lib()
    for m, k in ((1, MAX_PAIRS + 1), (MAX_PAIRS + 1, 1), (2, MAX_PAIRS // 2 + 1), (4097, 4096), (1 << 12, (1 << 12) + 1),
                 (1 << 32, 1 << 32), (1 << 40, 1 << 24), ((1 << 64) - 1, (1 << 64) - 1), ((1 << 63) + 1, 2)):
        assert _masked(lib, n_masks=m, n_operands=k) == WAH_ERR_ARG, (m, k)
        assert _masked(lib, n_masks=m, n_operands=k, scratch_bytes=0) == WAH_ERR_ARG, (m, k)
    for m, k in ((1, MAX_PAIRS), (MAX_PAIRS, 1), (4096, 4096), (2, MAX_PAIRS // 2), (3, 130)):
        assert _masked(lib, n_masks=m, n_operands=k, scratch_bytes=0) == WAH_ERR_WORKSPACE, (m, k)


def test_scratch_is_the_count_calls_unchanged(pkg):
    """wah_select_scratch_bytes serves the new call as it is: the same for every n_operands, and what it was."""
    lib = pkg.lib()
    for n_words in (0, 1, 991, 992, 993, 992 * 37 + 5, 992 * 4096, 268435200, (1 << 40) - 1):
        got = lib.wah_select_scratch_bytes(n_words, 1)
        segments = ((32 * n_words + 30) // 31 + 1023) // 1024
        n0 = segments + 1
        n1 = (n0 + 4095) // 4096
        n2 = (n1 + 4095) // 4096
        r256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
        assert got == 1024 + r256(8 * n0) + r256(8 * n1) + r256(8 * n2), n_words
        for k in (2, 64, 4097, 1 << 24):
            assert lib.wah_select_scratch_bytes(n_words, k) == got, (n_words, k)
        # exactly enough for the new call, whatever the tables' sizes
        assert _masked(lib, n_words=n_words, n_masks=7, n_operands=11, scratch_bytes=got - 1) == WAH_ERR_WORKSPACE


def test_python_front_ends_are_exported(pkg):
    assert callable(pkg.count_masked_device)
    assert callable(pkg.columns.count_columns_where) and callable(pkg.columns.crosstab_columns)
    assert "wah_count_masked_indexed_device" in pkg.count_masked_device.__doc__
