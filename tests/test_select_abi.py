"""CPU tests of the boundary of wah_count_list_indexed_device / wah_positions_indexed_device (include/wah.h): the four symbols
exist in the header, in api.ABI_SYMBOLS and in the library; the scratch size is what the header says it is; every argument
error the host can see comes back before any HIP call is made (no GPU here: made-up non-null integers stand in for device
pointers, nothing follows them); and the Python front ends are exported."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wah_select_scratch_bytes", "wah_count_list_indexed_device", "wah_positions_indexed_device", "wah_select_status")
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


def test_scratch_size(pkg):
    """A multiple of 256, never 0, monotone in n_words, the same for every n_operands, and with room for the control words and
    one uint64 per segment + 1."""
    lib = pkg.lib()
    sizes = []
    for n_words in (0, 1, 991, 992, 993, 992 * 37 + 5, 992 * 4095, 992 * 4096, 268435200, (1 << 33) + 7, (1 << 40) - 1):
        got = lib.wah_select_scratch_bytes(n_words, 1)
        segments = ((32 * n_words + 30) // 31 + 1023) // 1024
        assert got > 0 and got % 256 == 0 and got >= 1024 + 8 * (segments + 1), n_words
        assert got <= 1024 + 8 * (segments + 1) + (segments // 4096 + 1) * 8 + (segments // (4096 * 4096) + 1) * 8 + 3 * 256, n_words
        for k in (2, 64, 4097, 1 << 24):
            assert lib.wah_select_scratch_bytes(n_words, k) == got, (n_words, k)
        sizes.append(got)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]


def _count(lib, n_words=992 * 4, n_operands=3, table=0x10000, counts=0x20000, scratch=0x100000, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_select_scratch_bytes(min(n_words, (1 << 40) - 1), max(n_operands, 1))
    return lib.wah_count_list_indexed_device(n_words, n_operands, table, counts, scratch, scratch_bytes, None)


def _positions(lib, n_words=992 * 4, stream=0x10000, stream_words=100, offsets=0x18000, first=0, out=0x20000, cap=10, info=0x30000,
               scratch=0x100000, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_select_scratch_bytes(min(n_words, (1 << 40) - 1), 1)
    return lib.wah_positions_indexed_device(n_words, stream, stream_words, offsets, first, out, cap, info, scratch, scratch_bytes, None)


def test_count_argument_errors_come_back_before_any_hip_call(pkg):
    lib = pkg.lib()
    assert _count(lib, n_operands=0) == WAH_ERR_ARG
    assert _count(lib, n_operands=(1 << 24) + 1) == WAH_ERR_ARG          # above WAH_BITOP_LIST_MAX_OPERANDS
    assert _count(lib, scratch=None) == WAH_ERR_ARG                      # null scratch
    assert _count(lib, scratch=0x100000 + 128) == WAH_ERR_ARG            # not 256-byte aligned
    assert _count(lib, table=None) == WAH_ERR_ARG                        # null operand table
    assert _count(lib, table=0x10004) == WAH_ERR_ARG                     # operand table not 8-byte aligned
    assert _count(lib, counts=None) == WAH_ERR_ARG
    assert _count(lib, n_words=1 << 40) == WAH_ERR_ARG
    assert ctypes.c_char_p(lib.wah_last_error()).value
    need = lib.wah_select_scratch_bytes(992 * 4, 3)
    assert _count(lib, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
    assert _count(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
    # the argument checks come first: a bad argument with too small a scratch is an argument error
    assert _count(lib, n_operands=0, scratch_bytes=0) == WAH_ERR_ARG
    assert _count(lib, table=None, scratch_bytes=0) == WAH_ERR_ARG
    assert _count(lib, counts=None, scratch_bytes=0) == WAH_ERR_ARG
    assert _count(lib, n_words=1 << 40, scratch_bytes=0) == WAH_ERR_ARG


def test_positions_argument_errors_come_back_before_any_hip_call(pkg):
    lib = pkg.lib()
    assert _positions(lib, scratch=None) == WAH_ERR_ARG
    assert _positions(lib, scratch=0x100000 + 64) == WAH_ERR_ARG
    assert _positions(lib, info=None) == WAH_ERR_ARG
    assert _positions(lib, out=None) == WAH_ERR_ARG                      # a capacity without an output
    assert _positions(lib, out=None, cap=0, info=None) == WAH_ERR_ARG    # (a null output is allowed with no capacity, a null info never)
    assert _positions(lib, n_words=1 << 40) == WAH_ERR_ARG
    assert ctypes.c_char_p(lib.wah_last_error()).value
    need = lib.wah_select_scratch_bytes(992 * 4, 1)
    assert _positions(lib, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
    assert _positions(lib, out=None, cap=0, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE  # (accepted as arguments: the next check)
    assert _positions(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _positions(lib, info=None, scratch_bytes=0) == WAH_ERR_ARG
    assert _positions(lib, out=None, scratch_bytes=0) == WAH_ERR_ARG
    assert _positions(lib, n_words=1 << 40, scratch_bytes=0) == WAH_ERR_ARG
    assert lib.wah_select_status(None, None) == WAH_ERR_ARG


def test_python_front_ends_are_exported(pkg):
    for name in ("count_device", "positions_device"):
        assert callable(getattr(pkg, name))
    assert callable(pkg.columns.count_columns) and callable(pkg.columns.select_rows)
    assert "two calls" in pkg.positions_device.__doc__.lower()
