"""CPU tests of the boundary of wah_update_indexed_device (include/wah.h): the four symbols exist in the header, in
api.ABI_SYMBOLS and in the library; both size helpers are what the header says they are; every argument error the host can see
comes back before any HIP call is made, argument checks before the scratch's size (no GPU here: made-up non-null integers stand in
for device pointers, nothing follows them); the Python front ends have the signatures the documents state and refuse what does
not fit before anything touches a device."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess

import pytest
import torch

from tests import _update as up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wah_update_max_words", "wah_update_scratch_bytes", "wah_update_indexed_device", "wah_update_status")
WAH_ERR_ARG, WAH_ERR_WORKSPACE = -1, -2
MAX_COLUMNS = 1 << 24  # WAH_BITOP_LIST_MAX_OPERANDS
SIZES = (1, 30, 31, 991, 992, 993, 992 * 4095, 992 * 4096, (1 << 40) - 1)


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("gpu-wah_amd")
    p.build()
    return p


def test_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    declared = set(re.findall(r"\b(wah_[a-z_0-9]+)\s*\(", header))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path()], text=True)
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.ABI_SYMBOLS, name
        assert re.search(rf"\bT {name}\b", exported), name
        assert hasattr(pkg.lib(), name)


def test_max_words_is_the_smaller_of_the_two_bounds(pkg):
    lib = pkg.lib()
    for n_words in SIZES:
        for n_columns in (1, 3, 4097, MAX_COLUMNS):
            for mask_words in (0, 1, 1000, (1 << 64) - 1):
                for source_words in (0, 1, 10 ** 9, (1 << 64) - 1):
                    got = lib.wah_update_max_words(n_words, n_columns, mask_words, source_words)
                    assert got == up.max_words(n_words, n_columns, mask_words, source_words), (n_words, n_columns, mask_words, source_words)
    assert lib.wah_update_max_words((1 << 40) - 1, MAX_COLUMNS, (1 << 64) - 1, (1 << 64) - 1) == (1 << 64) - 1  # saturating
    # by hand: 2 columns of 1024 groups; 5 source words, a mask of 7 words: 5 + 2 * (7 + 3)
    assert lib.wah_update_max_words(992, 2, 7, 5) == 25
    assert lib.wah_update_max_words(992, 2, 7, 1 << 20) == 2 * 1024 and lib.wah_update_max_words(992, 2, 1 << 20, 5) == 2 * 1024
    assert lib.wah_update_max_words(992, 1, 0, 0) == 3


def test_scratch_size(pkg):
    """The control words (1 KiB) and one uint64 per 4096 entries for each of the two upper levels of the prefix sum over the
    n_columns * S + 1 index entries, every part rounded up to 256 bytes: no ranks, no starts -- the from-positions call's scratch."""
    lib = pkg.lib()
    for n_words in SIZES:
        for n_columns in (1, 2, 3, 4095, 4096, 4097, 1 << 20):
            got = lib.wah_update_scratch_bytes(n_words, n_columns)
            assert got == up.scratch_bytes(n_words, n_columns) == lib.wah_from_positions_scratch_bytes(n_words, n_columns), (n_words, n_columns)
            assert got > 0 and got % 256 == 0
    # by hand: four segments, three columns: 13 index entries, one entry on either level
    assert lib.wah_update_scratch_bytes(992 * 4, 3) == 1024 + 256 + 256 == 1536
    assert lib.wah_update_scratch_bytes(1, 1) == 1536
    # the level-1 area passes 256 bytes at 32 x 4096 + 1 index entries
    assert lib.wah_update_scratch_bytes(992 * 4096, 32) == 1024 + 512 + 256


def _call(lib, n_words=992 * 4, n_rows=1000, mask=0x8000, n_columns=3, else_=0x20000, then=0x28000, out=0x30000, cap=1000,
          out_words=0x40000, out_offsets=0x50000, scratch=0x100000, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_update_scratch_bytes(max(min(n_words, (1 << 40) - 1), 1), min(max(n_columns, 1), MAX_COLUMNS))
    return lib.wah_update_indexed_device(n_words, n_rows, mask, n_columns, else_, then, out, cap, out_words, out_offsets, scratch, scratch_bytes, None)


BAD_ARGUMENTS = (
    dict(n_columns=0), dict(n_columns=MAX_COLUMNS + 1),
    dict(n_columns=1 << 21, n_words=992 * 1024, n_rows=0),  # n_columns * S = 2^31
    dict(n_columns=2, n_words=992 << 30, n_rows=0),         # n_columns * S = 2^31 with two columns
    dict(n_words=0), dict(n_words=1 << 40),
    dict(n_rows=32 * 992 * 4 + 1), dict(n_words=1, n_rows=33), dict(n_rows=(1 << 64) - 1),
    dict(mask=None), dict(mask=0x8004),
    dict(else_=None), dict(else_=0x20004),
    dict(then=None), dict(then=0x28004),
    dict(out_offsets=None), dict(out_offsets=0x50004),
    dict(out_words=None), dict(out_words=0x40004),
    dict(out=None), dict(out=0x30002),
    dict(scratch=None), dict(scratch=0x100000 + 128),
)


@pytest.mark.parametrize("bad", BAD_ARGUMENTS, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_ARGUMENTS])
def test_argument_errors_come_back_before_any_hip_call(pkg, bad):
    lib = pkg.lib()
    assert _call(lib, **bad) == WAH_ERR_ARG
    assert ctypes.c_char_p(lib.wah_last_error()).value
    # the argument checks come first: a bad argument with too small a scratch is an argument error
    assert _call(lib, scratch_bytes=0, **bad) == WAH_ERR_ARG


def test_the_order_of_two_refusals(pkg):
    """Counts before rows before the index's size before pointers, and all of them before the scratch's size: the text names the
    first."""
    lib = pkg.lib()

    def text(**bad):
        assert _call(lib, **bad) == WAH_ERR_ARG
        return ctypes.c_char_p(lib.wah_last_error()).value.decode()

    assert "columns" in text(n_columns=0, n_rows=1 << 50)
    assert "words" in text(n_words=0, n_rows=1)
    assert "rows" in text(n_rows=1 << 50, mask=None)
    assert "rows" in text(n_columns=2, n_words=992 << 30, n_rows=(1 << 64) - 1)
    assert "2^31" in text(n_columns=2, n_words=992 << 30, n_rows=0, scratch=None)
    assert "scratch" in text(scratch=None, mask=None)
    assert "mask" in text(mask=None, out=None)
    assert "then" in text(then=0x28004, out=None)
    assert "output" in text(out_words=0x40004)


def test_workspace_errors_and_the_edges_that_are_accepted_as_arguments(pkg):
    lib = pkg.lib()
    need = lib.wah_update_scratch_bytes(992 * 4, 3)
    assert _call(lib, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
    # accepted as arguments (the next check refuses them for their scratch): the most columns, the longest bitmap, every row, no
    # row at all, one index entry fewer than 2^31
    assert _call(lib, n_columns=MAX_COLUMNS, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_columns=1, n_words=(1 << 40) - 1, n_rows=32 * ((1 << 40) - 1), scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_rows=32 * 992 * 4, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_rows=0, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_columns=(1 << 21) - 1, n_words=992 * 1024, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_update_status(None, None) == WAH_ERR_ARG


def test_python_front_ends(pkg):
    def names(fn):
        return list(inspect.signature(fn).parameters)

    assert names(pkg.update_max_words) == ["n_words", "n_columns", "mask_words", "source_words"]
    assert names(pkg.update_operand_table) == ["entries", "device"]
    assert names(pkg.update_device) == ["mask", "else_table", "then_table", "n_words", "n_rows", "mask_words", "source_words", "scratch", "out",
                                        "out_offsets", "check"]
    parameters = inspect.signature(pkg.update_device).parameters
    assert parameters["check"].default is True and parameters["mask_words"].default is None and parameters["source_words"].default is None
    c = pkg.columns
    assert names(c.update_rows) == ["wah", "index", "mask", "n_rows", "source", "reuse"]
    assert names(c.set_values_where) == ["wah", "bsi", "mask", "n_rows", "value", "reuse"]
    assert names(c.set_keys_where) == ["wah", "index", "mask", "n_rows", "key", "reuse"]
    assert names(c.choose_columns) == ["wah", "mask", "bsi_then", "bsi_else", "n_rows", "n_bits", "reuse"]
    assert names(c.greatest_columns) == names(c.least_columns) == ["wah", "bsi_a", "bsi_b", "n_rows"]
    assert "wah_update_indexed_device" in pkg.update_device.__doc__
    assert pkg.update_max_words(992, 3, 10, 100) == up.max_words(992, 3, 10, 100) == 139
    assert names(pkg.bitop_operand_table) == ["operands", "device"]  # (stays as it is)


def test_the_front_ends_refuse_what_does_not_fit(pkg):
    """... before anything touches a device: host tensors stand in for the streams and indexes."""
    c = pkg.columns
    st = torch.zeros(4, dtype=torch.int32)
    index = (st, torch.zeros(6, dtype=torch.int64), 992)          # five columns
    bsi = (st, torch.zeros(5, dtype=torch.int64), 992, 4, False)  # four slices
    bsi_e = (st, torch.zeros(6, dtype=torch.int64), 992, 4, True)
    mask = (st, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        c.update_rows(pkg, index, mask, 10, bsi)                  # two kinds
    with pytest.raises(ValueError):
        c.update_rows(pkg, bsi, mask, 10, bsi_e)                  # has_exists differs
    with pytest.raises(ValueError):
        c.update_rows(pkg, index, mask, 10, (st, torch.zeros(11, dtype=torch.int64), 2 * 992))  # another column length
    with pytest.raises(ValueError):
        c.update_rows(pkg, index, mask, 32 * 992 + 1, index)      # more rows than the columns hold
    with pytest.raises(ValueError):
        c.update_rows(pkg, index, mask, -1, index)
    with pytest.raises(ValueError):
        c.update_rows(pkg, index, mask + (992,), 10, index)       # a mask is a pair
    for value in (-1, 16, 1 << 40):
        with pytest.raises(ValueError):
            c.set_values_where(pkg, bsi, mask, 10, value)
    with pytest.raises(ValueError, match="existence"):
        c.set_values_where(pkg, bsi, mask, 10, None)              # NULL needs an existence slice
    for key in (-1, 5):
        with pytest.raises(ValueError):
            c.set_keys_where(pkg, index, mask, 10, key)
    with pytest.raises(ValueError):
        c.set_keys_where(pkg, bsi, mask, 10, 0)                   # not an equality-encoded index
    with pytest.raises(ValueError):
        c.choose_columns(pkg, mask, bsi, bsi_e, 10, n_bits=3)     # narrower than either
    with pytest.raises(ValueError):
        c.choose_columns(pkg, mask, bsi, (st, torch.zeros(9, dtype=torch.int64), 2 * 992, 4, False), 10)
    for fn in (c.greatest_columns, c.least_columns):
        with pytest.raises(ValueError, match="existence"):
            fn(pkg, bsi, bsi_e, 10)
