"""CPU tests of wah_bitop_list_indexed_device's boundary (include/wah.h): the three symbols exist in the header, in
api.ABI_SYMBOLS and in the library; the operand struct is 24 bytes; the scratch size is what the header says it is; and every
argument error the host can see comes back before any HIP call is made (no GPU here: made-up non-null integers stand in for
device pointers, nothing follows them)."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wah_bitop_list_scratch_bytes", "wah_bitop_list_indexed_device", "wah_bitop_list_status")
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


def test_operand_struct_is_24_bytes_without_padding(pkg):
    assert ctypes.sizeof(pkg.BitopOperand) == 24
    assert [f[0] for f in pkg.BitopOperand._fields_] == ["d_stream", "stream_words", "d_offsets"]
    assert (pkg.BitopOperand.d_stream.offset, pkg.BitopOperand.stream_words.offset, pkg.BitopOperand.d_offsets.offset) == (0, 8, 16)
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    assert re.search(r"#define\s+WAH_BITOP_LIST_MAX_OPERANDS\s+\(1u << 24\)", header)  # the stated bound: at least 65 536


@pytest.mark.parametrize("n_words", [0, 1, 991, 992, 992 * 37 + 5, 268435200, (1 << 33) + 7])
def test_scratch_equals_the_indexed_scratch_whatever_the_operand_count(pkg, n_words):
    """include/wah.h: the scratch EQUALS wah_bitop_indexed_scratch_bytes(n_words) for every n_operands."""
    lib = pkg.lib()
    want = lib.wah_bitop_indexed_scratch_bytes(n_words)
    for k in (1, 2, 8, 9, 300, 65536, 1 << 24):
        got = lib.wah_bitop_list_scratch_bytes(n_words, k)
        assert got == want and got % 256 == 0 and got > 0, (n_words, k)


def _call(lib, op=1, n_words=992 * 4, n_operands=3, table=0x10000, out=0x20000, cap=1 << 20, out_words=0x30000, out_offsets=0x40000,
          scratch=0x100000, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bitop_list_scratch_bytes(min(n_words, (1 << 40) - 1), max(n_operands, 1))
    return lib.wah_bitop_list_indexed_device(op, n_words, n_operands, table, out, cap, out_words, out_offsets, scratch, scratch_bytes, None)


def test_argument_errors_come_back_before_any_hip_call(pkg):
    lib = pkg.lib()
    for bad_op in (-1, 4, 17):
        assert _call(lib, op=bad_op) == WAH_ERR_ARG
    assert _call(lib, n_operands=0) == WAH_ERR_ARG
    assert _call(lib, n_operands=(1 << 24) + 1) == WAH_ERR_ARG          # above WAH_BITOP_LIST_MAX_OPERANDS
    assert _call(lib, scratch=None) == WAH_ERR_ARG                      # null scratch
    assert _call(lib, scratch=0x100000 + 128) == WAH_ERR_ARG            # not 256-byte aligned
    assert _call(lib, table=None) == WAH_ERR_ARG                        # null table
    assert _call(lib, table=0x10004) == WAH_ERR_ARG                     # table not 8-byte aligned
    assert _call(lib, n_words=1 << 40) == WAH_ERR_ARG
    assert _call(lib, out_words=None) == WAH_ERR_ARG
    assert _call(lib, out=None) == WAH_ERR_ARG
    assert ctypes.c_char_p(lib.wah_last_error()).value
    need = lib.wah_bitop_list_scratch_bytes(992 * 4, 3)
    assert _call(lib, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
    # the argument checks come first: a bad operation with too small a scratch is an argument error
    assert _call(lib, op=9, scratch_bytes=0) == WAH_ERR_ARG
    assert lib.wah_bitop_list_status(None, 992, 1, None) == WAH_ERR_ARG


def test_python_front_ends_are_exported(pkg):
    for name in ("bitop_list_indexed_device", "bitop_operand_table"):
        assert callable(getattr(pkg, name))
    for name in ("column_operand_table", "combine_columns"):
        assert callable(getattr(pkg.columns, name))
    assert "raw pointers" in pkg.bitop_operand_table.__doc__.lower()
