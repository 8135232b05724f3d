"""CPU tests of wah_bitop_clauses_indexed_device's boundary (include/wah.h): the three symbols exist in the header, in
api.ABI_SYMBOLS and in the library; the scratch size is what the header says it is; every argument error the host can see
comes back before any HIP call is made (no GPU here: made-up non-null integers stand in for device pointers, nothing follows
them); and the Python front ends are exported."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wah_bitop_clauses_scratch_bytes", "wah_bitop_clauses_indexed_device", "wah_bitop_clauses_status")
WAH_ERR_ARG, WAH_ERR_WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("gpu-wah_amd")
    p.build()
    return p


def test_symbols_in_header_binding_and_library(pkg):
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    declared = set(re.findall(r"\b(wah_[a-z_0-9]+)\s*\(", header))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path()], text=True)
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.ABI_SYMBOLS, name
        assert re.search(rf"\bT {name}\b", exported), name
        assert hasattr(pkg.lib(), name)
    assert re.search(r"#define\s+WAH_CLAUSE_NEGATE\s+\(1ull << 63\)", header)
    assert pkg.CLAUSE_NEGATE == -(1 << 63)  # bit 63 as the int64 a clause table holds


@pytest.mark.parametrize("n_words", [0, 1, 991, 992, 992 * 37 + 5, 268435200, (1 << 33) + 7])
def test_scratch_equals_the_indexed_scratch_whatever_the_counts(pkg, n_words):
    """include/wah.h: the scratch EQUALS wah_bitop_indexed_scratch_bytes(n_words) for every n_operands and n_clauses."""
    lib = pkg.lib()
    want = lib.wah_bitop_indexed_scratch_bytes(n_words)
    for k, c in ((1, 1), (2, 1), (8, 8), (9, 3), (300, 12), (65536, 130), (1 << 24, 1 << 24)):
        got = lib.wah_bitop_clauses_scratch_bytes(n_words, k, c)
        assert got == want and got % 256 == 0 and got > 0, (n_words, k, c)


def _call(lib, n_words=992 * 4, n_clauses=2, ends=0x8000, n_operands=3, table=0x10000, out=0x20000, cap=1 << 20, out_words=0x30000,
          out_offsets=0x40000, scratch=0x100000, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bitop_clauses_scratch_bytes(min(n_words, (1 << 40) - 1), max(n_operands, 1), max(n_clauses, 1))
    return lib.wah_bitop_clauses_indexed_device(n_words, n_clauses, ends, n_operands, table, out, cap, out_words, out_offsets, scratch,
                                                scratch_bytes, None)


def test_argument_errors_come_back_before_any_hip_call(pkg):
    lib = pkg.lib()
    assert _call(lib, n_clauses=0) == WAH_ERR_ARG
    assert _call(lib, n_clauses=4) == WAH_ERR_ARG                       # more clauses than operands: one would be empty
    assert _call(lib, n_operands=0, n_clauses=1) == WAH_ERR_ARG
    assert _call(lib, n_operands=0, n_clauses=0) == WAH_ERR_ARG
    assert _call(lib, n_operands=(1 << 24) + 1) == WAH_ERR_ARG          # above WAH_BITOP_LIST_MAX_OPERANDS
    assert _call(lib, scratch=None) == WAH_ERR_ARG                      # null scratch
    assert _call(lib, scratch=0x100000 + 128) == WAH_ERR_ARG            # not 256-byte aligned
    assert _call(lib, table=None) == WAH_ERR_ARG                        # null operand table
    assert _call(lib, table=0x10004) == WAH_ERR_ARG                     # operand table not 8-byte aligned
    assert _call(lib, ends=None) == WAH_ERR_ARG                         # null clause table
    assert _call(lib, ends=0x8004) == WAH_ERR_ARG                       # clause table not 8-byte aligned
    assert _call(lib, n_words=1 << 40) == WAH_ERR_ARG
    assert _call(lib, out_words=None) == WAH_ERR_ARG
    assert _call(lib, out=None) == WAH_ERR_ARG
    assert ctypes.c_char_p(lib.wah_last_error()).value
    need = lib.wah_bitop_clauses_scratch_bytes(992 * 4, 3, 2)
    assert _call(lib, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
    # the argument checks come first: a bad count with too small a scratch is an argument error
    assert _call(lib, n_clauses=0, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, n_clauses=4, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, ends=None, scratch_bytes=0) == WAH_ERR_ARG
    assert lib.wah_bitop_clauses_status(None, 992, 1, 1, None) == WAH_ERR_ARG


def test_python_front_ends_are_exported(pkg):
    for name in ("bitop_clauses_indexed_device", "bitop_clause_table"):
        assert callable(getattr(pkg, name))
    assert callable(pkg.columns.filter_columns)
    assert "raw pointers" in pkg.bitop_clause_table.__doc__.lower()
