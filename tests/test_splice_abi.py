"""CPU tests of the boundary of wah_splice_indexed_device (include/wah.h): the four symbols, the piece struct and its bound exist in
the header, in api.ABI_SYMBOLS and in the library; both size helpers are what the header says they are; every argument error the
host can see comes back before any HIP call is made (no GPU here: made-up non-null integers stand in for device pointers, nothing
follows them); the Python front ends have the signatures the documents state, and append_rows refuses what does not match."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess

import pytest
import torch

from tests import _splice as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wah_splice_max_words", "wah_splice_scratch_bytes", "wah_splice_indexed_device", "wah_splice_status")
WAH_ERR_ARG, WAH_ERR_WORKSPACE = -1, -2
MAX_COLUMNS = 1 << 24  # WAH_BITOP_LIST_MAX_OPERANDS
SIZES = (1, 30, 31, 991, 992, 993, 992 * 4096, (1 << 40) - 1)


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("gpu-wah_amd")
    p.build()
    return p


def test_symbols_struct_and_define(pkg):
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    declared = set(re.findall(r"\b(wah_[a-z_0-9]+)\s*\(", header))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path()], text=True)
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.ABI_SYMBOLS, name
        assert re.search(rf"\bT {name}\b", exported), name
        assert hasattr(pkg.lib(), name)
    m = re.search(r"typedef struct \{([^}]*)\} wah_splice_piece;", header)
    fields = re.findall(r"uint64_t (\w+);", m.group(1)) if m else []
    assert fields == ["n_words", "first_row", "n_rows"]
    assert ctypes.sizeof(type("Piece", (ctypes.Structure,), {"_fields_": [(f, ctypes.c_uint64) for f in fields]})) == 24
    assert re.search(r"#define WAH_SPLICE_MAX_PIECES \(1u << 16\)", header)
    assert pkg.SPLICE_MAX_PIECES == sp.MAX_PIECES == 1 << 16


def test_max_words_is_the_smaller_of_the_two_bounds(pkg):
    lib = pkg.lib()
    for n_words in SIZES:
        for n_columns in (1, 3, 4097, MAX_COLUMNS):
            for n_pieces in (1, 2, 1 << 16):
                for source_words in (0, 1, 1000, 10 ** 9, (1 << 64) - 1):
                    want = sp.max_words(n_words, n_columns, n_pieces, source_words)
                    assert lib.wah_splice_max_words(n_words, n_columns, n_pieces, source_words) == want, (n_words, n_columns, n_pieces, source_words)
    assert lib.wah_splice_max_words((1 << 40) - 1, MAX_COLUMNS, 1, (1 << 64) - 1) == (1 << 64) - 1  # saturating


def test_scratch_size(pkg):
    """The control words (1 KiB), n_pieces + 1 running starts, and one uint64 per 4096 entries for each of the two upper levels of
    the prefix sum over the n_columns * S + 1 index entries, every part rounded up to 256 bytes: a multiple of 256, never 0."""
    lib = pkg.lib()
    for n_words in SIZES:
        for n_columns in (1, 2, 4095, 4096, 4097, 1 << 20):
            for n_pieces in (1, 31, 32, 1 << 16):
                got = lib.wah_splice_scratch_bytes(n_words, n_columns, n_pieces)
                assert got == sp.scratch_bytes(n_words, n_columns, n_pieces), (n_words, n_columns, n_pieces)
                assert got > 0 and got % 256 == 0


def _call(lib, n_words=992 * 4, n_columns=3, n_pieces=2, pieces=0x10000, table=0x20000, out=0x30000, cap=1000, out_words=0x40000,
          out_offsets=0x50000, scratch=0x100000, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_splice_scratch_bytes(max(min(n_words, (1 << 40) - 1), 1), min(max(n_columns, 1), MAX_COLUMNS),
                                                     min(max(n_pieces, 1), 1 << 16))
    return lib.wah_splice_indexed_device(n_words, n_columns, n_pieces, pieces, table, out, cap, out_words, out_offsets, scratch, scratch_bytes, None)


BAD_ARGUMENTS = (
    dict(n_columns=0), dict(n_columns=MAX_COLUMNS + 1),
    dict(n_pieces=0), dict(n_pieces=(1 << 16) + 1),
    dict(n_pieces=1 << 16, n_columns=257),                # n_pieces * n_columns > 2^24
    dict(n_columns=1 << 21, n_pieces=1, n_words=992 * 1024),  # n_columns * S = 2^31
    dict(n_columns=2, n_pieces=1, n_words=992 << 30),     # n_columns * S = 2^31 with two columns
    dict(n_words=0), dict(n_words=1 << 40),
    dict(pieces=None), dict(pieces=0x10004),
    dict(table=None), dict(table=0x20004),
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


def test_workspace_errors_and_the_edges_that_are_accepted_as_arguments(pkg):
    lib = pkg.lib()
    need = lib.wah_splice_scratch_bytes(992 * 4, 3, 2)
    assert _call(lib, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
    # accepted as arguments (the next check refuses them for their scratch): the most columns, the most pieces, the most table
    # entries, the longest bitmap, one index entry fewer than 2^31
    assert _call(lib, n_columns=MAX_COLUMNS, n_pieces=1, n_words=992, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_columns=1, n_pieces=1 << 16, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_columns=256, n_pieces=1 << 16, n_words=1, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_columns=1, n_words=(1 << 40) - 1, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_columns=(1 << 21) - 1, n_pieces=1, n_words=992 * 1024, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_splice_status(None, None) == WAH_ERR_ARG


def test_python_front_ends(pkg):
    def names(fn):
        return list(inspect.signature(fn).parameters)

    assert names(pkg.splice_pieces) == ["pieces", "device"]
    assert names(pkg.splice_max_words) == ["n_words_out", "n_columns", "n_pieces", "source_words"]
    assert names(pkg.splice_device) == ["pieces", "table", "n_columns", "n_words_out", "source_words", "scratch", "out", "out_offsets", "check"]
    assert inspect.signature(pkg.splice_device).parameters["check"].default is True
    assert names(pkg.columns.splice_columns) == ["wah", "parts", "n_words_per_column", "reuse"]
    assert names(pkg.columns.append_rows) == ["wah", "index", "rows", "batch", "batch_rows"]
    assert names(pkg.columns.slice_rows) == ["wah", "index", "first", "n_rows"]
    assert "wah_splice_indexed_device" in pkg.splice_device.__doc__
    assert pkg.splice_max_words(992, 3, 2, 10) == sp.max_words(992, 3, 2, 10)


def test_append_rows_refuses_what_does_not_match(pkg):
    """... before anything touches a device: host tensors stand in for the streams and indexes."""
    st = torch.zeros(4, dtype=torch.int32)

    def index(columns, segments=1):
        return torch.zeros(columns * segments + 1, dtype=torch.int64)

    keys = (st, index(5), 992)
    bsi = (st, index(5), 992, 4, True)
    with pytest.raises(ValueError):
        pkg.columns.append_rows(pkg, keys, 10, bsi, 10)  # a bit-sliced batch for an equality-encoded index
    with pytest.raises(ValueError):
        pkg.columns.append_rows(pkg, bsi, 10, keys, 10)
    with pytest.raises(ValueError, match="column count"):
        pkg.columns.append_rows(pkg, keys, 10, (st, index(5, 2), 992), 10)  # eleven entries: ten columns of one segment
    with pytest.raises(ValueError, match="column count"):
        pkg.columns.append_rows(pkg, keys, 10, (st, index(6), 992), 10)
    with pytest.raises(ValueError, match="n_bits or has_exists"):
        pkg.columns.append_rows(pkg, bsi, 10, (st, index(5), 992, 5, False), 10)   # 4 bits + existence against 5 bits: five columns each
    with pytest.raises(ValueError, match="n_bits or has_exists"):
        pkg.columns.append_rows(pkg, (st, index(5), 992, 5, False), 10, (st, index(5), 992, 4, True), 10)
    with pytest.raises(ValueError):
        pkg.columns.append_rows(pkg, (st, index(5)), 10, (st, index(5)), 10)          # neither kind of tuple
    with pytest.raises(ValueError):
        pkg.columns.slice_rows(pkg, (st, index(5)), 0, 10)
