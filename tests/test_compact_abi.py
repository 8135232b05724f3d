"""CPU tests of the boundary of wah_compact_indexed_device (include/wah.h): the four symbols and the flag exist in the header, in
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

from tests import _compact as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wah_compact_max_words", "wah_compact_scratch_bytes", "wah_compact_indexed_device", "wah_compact_status")
WAH_ERR_ARG, WAH_ERR_WORKSPACE = -1, -2
MAX_COLUMNS = 1 << 24  # WAH_BITOP_LIST_MAX_OPERANDS
SIZES = (1, 30, 31, 991, 992, 993, 992 * 4095, 992 * 4096, (1 << 40) - 1)


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("gpu-wah_amd")
    p.build()
    return p


def test_symbols_and_define(pkg):
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    declared = set(re.findall(r"\b(wah_[a-z_0-9]+)\s*\(", header))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path()], text=True)
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.ABI_SYMBOLS, name
        assert re.search(rf"\bT {name}\b", exported), name
        assert hasattr(pkg.lib(), name)
    assert re.search(r"#define WAH_COMPACT_DELETE 1u", header)
    assert pkg.COMPACT_DELETE == 1


def test_max_words_is_the_smaller_of_the_two_bounds(pkg):
    lib = pkg.lib()
    for n_words in SIZES:
        for n_columns in (1, 3, 4097, MAX_COLUMNS):
            for source_words in (0, 1, 1000, 10 ** 9, (1 << 64) - 1):
                assert lib.wah_compact_max_words(n_words, n_columns, source_words) == cp.max_words(n_words, n_columns, source_words), (n_words, n_columns, source_words)
    assert lib.wah_compact_max_words((1 << 40) - 1, MAX_COLUMNS, (1 << 64) - 1) == (1 << 64) - 1  # saturating
    assert lib.wah_compact_max_words(992, 2, 5) == 2 * 2 + 10 and lib.wah_compact_max_words(992, 2, 1 << 20) == 2 * 1024


def test_scratch_size(pkg):
    """The control words (1 KiB), S_src + 1 running ranks, and one uint64 per 4096 entries for each of the two upper levels of the
    two prefix sums -- over the n_columns * S_out + 1 index entries and over the ranks --, every part rounded up to 256 bytes: a
    multiple of 256, never 0."""
    lib = pkg.lib()
    for n_words in SIZES:
        for n_words_out in (1, 992, 993, 992 * 4096):
            for n_columns in (1, 2, 4095, 4096, 4097, 1 << 20):
                got = lib.wah_compact_scratch_bytes(n_words, n_words_out, n_columns)
                assert got == cp.scratch_bytes(n_words, n_words_out, n_columns), (n_words, n_words_out, n_columns)
                assert got > 0 and got % 256 == 0
    # by hand: the smallest call -- control words, two ranks in 256 bytes, four levels of 256 bytes each
    assert lib.wah_compact_scratch_bytes(1, 1, 1) == 1024 + 256 + 4 * 256 == 2304
    # by hand: 4096 source segments are 4097 ranks (32 776 bytes -> 32 768 + 256) and TWO level-1 entries; 4 columns of 1024 output
    # segments are 4097 index entries, two level-1 entries as well: still 256 bytes per level
    assert lib.wah_compact_scratch_bytes(992 * 4096, 992 * 1024, 4) == 1024 + 33024 + 4 * 256 == 35072
    # the level-1 area passes 256 bytes at 32 x 4096 + 1 entries
    assert lib.wah_compact_scratch_bytes(992, 992 * 4096, 32) == 1024 + 256 + (512 + 256) + (256 + 256)


def _call(lib, n_words=992 * 4, n_rows=1000, flags=0, mask=0x8000, n_columns=3, table=0x20000, n_words_out=992, out=0x30000, cap=1000,
          out_words=0x40000, out_offsets=0x50000, out_rows=0x60000, scratch=0x100000, scratch_bytes=None):
    if scratch_bytes is None:
        clip = lambda v: max(min(v, (1 << 40) - 1), 1)  # noqa: E731
        scratch_bytes = lib.wah_compact_scratch_bytes(clip(n_words), clip(n_words_out), min(max(n_columns, 1), MAX_COLUMNS))
    return lib.wah_compact_indexed_device(n_words, n_rows, flags, mask, n_columns, table, n_words_out, out, cap, out_words, out_offsets, out_rows,
                                          scratch, scratch_bytes, None)


BAD_ARGUMENTS = (
    dict(n_columns=0), dict(n_columns=MAX_COLUMNS + 1),
    dict(n_columns=1 << 21, n_words_out=992 * 1024),  # n_columns * S_out = 2^31
    dict(n_columns=2, n_words_out=992 << 30),         # n_columns * S_out = 2^31 with two columns
    dict(n_words=0), dict(n_words=1 << 40), dict(n_words_out=0), dict(n_words_out=1 << 40),
    dict(n_rows=32 * 992 * 4 + 1), dict(n_words=1, n_rows=33), dict(n_rows=(1 << 64) - 1),
    dict(flags=2), dict(flags=3), dict(flags=1 << 31),
    dict(mask=None), dict(mask=0x8004),
    dict(table=None), dict(table=0x20004),
    dict(out_offsets=None), dict(out_offsets=0x50004),
    dict(out_words=None), dict(out_words=0x40004),
    dict(out_rows=None), dict(out_rows=0x60004),
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
    """Counts before rows before flags before pointers, and all of them before the scratch's size: the text names the first."""
    lib = pkg.lib()

    def text(**bad):
        assert _call(lib, **bad) == WAH_ERR_ARG
        return ctypes.c_char_p(lib.wah_last_error()).value.decode()

    assert "columns" in text(n_columns=0, n_rows=1 << 50)
    assert "rows" in text(n_rows=1 << 50, flags=2)
    assert "flag" in text(flags=2, mask=None)
    assert "2^31" in text(n_columns=2, n_words_out=992 << 30, scratch=None)
    assert "scratch" in text(scratch=None, mask=None)
    assert "mask" in text(mask=None, out=None)
    assert "output" in text(out_rows=0x60004)


def test_workspace_errors_and_the_edges_that_are_accepted_as_arguments(pkg):
    lib = pkg.lib()
    need = lib.wah_compact_scratch_bytes(992 * 4, 992, 3)
    assert _call(lib, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
    # accepted as arguments (the next check refuses them for their scratch): the most columns, the longest bitmaps, every row of
    # the source, no row at all, the flag, one index entry fewer than 2^31
    assert _call(lib, n_columns=MAX_COLUMNS, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_words=(1 << 40) - 1, n_rows=32 * ((1 << 40) - 1), scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_columns=1, n_words_out=(1 << 40) - 1, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_rows=32 * 992 * 4, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_rows=0, flags=1, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_columns=(1 << 21) - 1, n_words_out=992 * 1024, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_compact_status(None, None) == WAH_ERR_ARG


def test_python_front_ends(pkg):
    def names(fn):
        return list(inspect.signature(fn).parameters)

    assert names(pkg.compact_max_words) == ["n_words_out", "n_columns", "source_words"]
    assert names(pkg.compact_device) == ["mask", "table", "n_words", "n_rows", "n_words_out", "delete", "source_words", "scratch", "out",
                                         "out_offsets", "out_rows", "check"]
    parameters = inspect.signature(pkg.compact_device).parameters
    assert parameters["check"].default is True and parameters["delete"].default is False
    for fn in (pkg.columns.keep_rows, pkg.columns.delete_rows):
        assert names(fn) == ["wah", "index", "mask", "n_rows", "n_rows_out", "reuse"]
        assert inspect.signature(fn).parameters["n_rows_out"].default is None
    assert "wah_compact_indexed_device" in pkg.compact_device.__doc__
    assert "SYNCHRONISES" in pkg.columns.keep_rows.__doc__ and "keep_rows" in pkg.columns.delete_rows.__doc__
    assert pkg.compact_max_words(992, 3, 10) == cp.max_words(992, 3, 10)


def test_keep_rows_refuses_what_does_not_fit(pkg):
    """... before anything touches a device: host tensors stand in for the streams and indexes."""
    st = torch.zeros(4, dtype=torch.int32)
    index = (st, torch.zeros(6, dtype=torch.int64), 992)
    mask = (st, torch.zeros(2, dtype=torch.int64))
    for fn in (pkg.columns.keep_rows, pkg.columns.delete_rows):
        with pytest.raises(ValueError):
            fn(pkg, index[:2], mask, 10)                  # neither kind of tuple
        with pytest.raises(ValueError):
            fn(pkg, index, mask, 32 * 992 + 1)            # more rows than the columns hold
        with pytest.raises(ValueError):
            fn(pkg, index, mask, -1)
        with pytest.raises(ValueError):
            fn(pkg, index, mask + (992,), 10)             # a mask is a pair
        with pytest.raises(ValueError):
            fn(pkg, index, mask, 10, n_rows_out=-1)
        with pytest.raises(ValueError, match="n_rows_out"):
            fn(pkg, index, mask, 10, check=False)         # the exact size needs the count read back
