"""CPU tests of the range call's boundary (include/wah.h: wah_values_indexed_device): the three symbols are declared and exported,
the scratch is the control words -- a multiple of 256, never 0, whatever the sizes --, and every refusal the host can see comes
back with its code before any HIP call, the argument checks first and in the header's order -- so without a device (made-up
non-null integers stand in for device pointers, nothing follows them)."""
import importlib
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
BITS, FIRST = 0, 1
MAX_OPERANDS = 1 << 24  # WAH_BITOP_LIST_MAX_OPERANDS
NAMES = ("wah_values_scratch_bytes", "wah_values_indexed_device", "wah_values_status")


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.build()
    return pkg.lib()


def test_symbols_are_declared_and_exported(lib):
    pkg = importlib.import_module("gpu-wah_amd")
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    declared = set(re.findall(r"\b(wah_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    assert len(re.findall(r"#define WAH_FETCH_[A-Z]+ ", header)) == 2  # the two modes of the list call: no new ones
    assert "wah_values_indexed_device" in header.split("decoding the slices is the better")[1].split("*/")[0]  # the fetch contract points here
    assert list(inspect.signature(pkg.values_device).parameters) == ["table", "n_words", "mode", "first_row", "n_rows", "scratch", "out", "check"]
    assert list(inspect.signature(pkg.columns.values_of_column).parameters) == ["wah", "bsi", "first", "n_rows"]
    assert list(inspect.signature(pkg.columns.keys_of_column).parameters) == ["wah", "index", "first", "n_rows"]
    assert list(inspect.signature(pkg.columns.reorder_rows).parameters) == ["wah", "index", "order", "n_rows"]
    assert list(inspect.signature(pkg.columns._values_of_column_torch).parameters) == ["wah", "bsi", "first", "n_rows"]


def test_scratch_is_the_control_words(lib):
    sizes = {lib.wah_values_scratch_bytes(n, k) for n in (0, 1, 31, 992, 993, 1 << 23, (1 << 40) - 1, 1 << 40, (1 << 64) - 1)
             for k in (0, 1, 32, 33, 64, 65, MAX_OPERANDS, (1 << 64) - 1)}
    assert len(sizes) == 1  # the items are known to the host: nothing is listed on the device
    size = sizes.pop()
    assert size >= 1024 and size % 256 == 0
    assert size <= lib.wah_fetch_scratch_bytes(992, 1)


# pointers that are never followed: every call below is refused on the host
TABLE, OUT, SCRATCH = 0x10000, 0x30000, 0x50000


def _call(lib, mode=BITS, n_words=992, n_operands=20, table=TABLE, first_row=0, n_rows=100, out=OUT, scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_values_scratch_bytes(n_words, n_operands)
    return lib.wah_values_indexed_device(mode, n_words, n_operands, table, first_row, n_rows, out, scratch, scratch_bytes, None)


def test_host_visible_refusals(lib):
    for mode in (2, 3, 1 << 31):
        assert _call(lib, mode=mode) == WAH_ERR_ARG, mode
    for mode, counts in ((BITS, (0, 65, MAX_OPERANDS, 1 << 32)), (FIRST, (0, MAX_OPERANDS + 1, 1 << 32, (1 << 64) - 1))):
        for n_operands in counts:
            assert _call(lib, mode=mode, n_operands=n_operands) == WAH_ERR_ARG, (mode, n_operands)
    assert _call(lib, n_words=1 << 40) == WAH_ERR_ARG and _call(lib, n_words=(1 << 64) - 1, n_rows=0) == WAH_ERR_ARG
    # a window that leaves 32 n_words, overflow of first_row + n_rows included
    n_bits = 32 * 992
    for first_row, n_rows in ((0, n_bits + 1), (n_bits, 1), (n_bits + 1, 0), (1, n_bits), (n_bits - 1, 2), ((1 << 64) - 1, 1), ((1 << 64) - 1, 2),
                              (1, (1 << 64) - 1), (1 << 63, 1 << 63), ((1 << 64) - 50, 100)):
        assert _call(lib, first_row=first_row, n_rows=n_rows) == WAH_ERR_ARG, (first_row, n_rows)
    assert _call(lib, n_words=0, n_rows=1) == WAH_ERR_ARG
    for name, bad in (("table", None), ("table", TABLE + 4), ("out", None), ("out", OUT + 4), ("out", OUT + 1), ("scratch", None),
                      ("scratch", SCRATCH + 128), ("scratch", SCRATCH + 8)):
        assert _call(lib, **{name: bad}) == WAH_ERR_ARG, (name, bad)
    assert lib.wah_last_error()
    assert lib.wah_values_status(None, None) == WAH_ERR_ARG


def test_the_argument_checks_come_first_and_in_order(lib):
    """A bad argument AND too small a scratch is a bad argument; the text names the first check that fails."""
    for bad in (dict(mode=2), dict(n_operands=0), dict(n_operands=65), dict(mode=FIRST, n_operands=MAX_OPERANDS + 1), dict(n_words=1 << 40),
                dict(n_rows=32 * 992 + 1), dict(first_row=(1 << 64) - 1, n_rows=2), dict(out=None), dict(out=OUT + 4), dict(table=None),
                dict(scratch=SCRATCH + 8)):
        assert _call(lib, scratch_bytes=0, **bad) == WAH_ERR_ARG, bad

    def text(**bad):
        assert _call(lib, **bad) == WAH_ERR_ARG
        return lib.wah_last_error().decode()

    assert "mode" in text(mode=7, n_operands=0, n_words=1 << 40, n_rows=1 << 50, table=None)
    assert "table rows" in text(n_operands=0, n_words=1 << 40, n_rows=1 << 50, table=None)
    assert "2^40" in text(n_words=1 << 40, n_rows=(1 << 64) - 1, table=None)
    assert "window" in text(n_rows=32 * 992 + 1, table=None, out=None)
    assert "null or misaligned" in text(table=None)
    for mode, n_operands in ((BITS, 1), (BITS, 64), (FIRST, 65), (FIRST, MAX_OPERANDS)):
        for first_row, n_rows in ((0, 1), (5, 100), (0, 32 * 992)):
            need = lib.wah_values_scratch_bytes(992, n_operands)
            assert _call(lib, mode=mode, n_operands=n_operands, first_row=first_row, n_rows=n_rows, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
            assert _call(lib, mode=mode, n_operands=n_operands, first_row=first_row, n_rows=n_rows, scratch_bytes=0) == WAH_ERR_WORKSPACE


def test_no_row_at_all(lib):
    """n_rows == 0: d_out may be null but not misaligned; the window, the table and the scratch are judged as ever."""
    n_bits = 32 * 992
    for first_row in (0, 5, n_bits):
        assert _call(lib, first_row=first_row, n_rows=0, out=None, scratch_bytes=0) == WAH_ERR_WORKSPACE  # (past every argument check)
    assert _call(lib, n_words=0, first_row=0, n_rows=0, out=None, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, first_row=n_bits + 1, n_rows=0, out=None) == WAH_ERR_ARG
    for name, bad in (("table", None), ("table", TABLE + 4), ("out", OUT + 4), ("scratch", None), ("scratch", SCRATCH + 128)):
        assert _call(lib, n_rows=0, **{name: bad}) == WAH_ERR_ARG, (name, bad)
    assert _call(lib, n_rows=0, mode=2, out=None) == WAH_ERR_ARG and _call(lib, n_rows=0, n_operands=65, out=None) == WAH_ERR_ARG


def test_python_front_ends_refuse_before_the_library():
    import torch

    pkg = importlib.import_module("gpu-wah_amd")
    table = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(pkg.WahError):
        pkg.values_device(table, 992, pkg.FETCH_BITS)  # a table on the CPU
    index = (torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), 992)
    for first, n_rows in ((-1, 5), (0, 32 * 992 + 1), (32 * 992, 1), (5, -1)):
        with pytest.raises(ValueError):
            pkg.columns.keys_of_column(pkg, index, first, n_rows)
        with pytest.raises(ValueError):
            pkg.columns.values_of_column(pkg, index + (3, False), first, n_rows)
    with pytest.raises(ValueError):
        pkg.columns.reorder_rows(pkg, index[:2], torch.zeros(3, dtype=torch.int64), 5)  # neither kind of index
    with pytest.raises(ValueError):
        pkg.columns.reorder_rows(pkg, index, torch.zeros(3, dtype=torch.int32), 5)  # an order of another type
    with pytest.raises(ValueError):
        pkg.columns.reorder_rows(pkg, index, torch.tensor([0, 5]), 5)  # an entry at n_rows
