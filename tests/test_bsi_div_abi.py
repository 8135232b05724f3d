"""CPU tests of the column division call's boundary (include/wah.h: wah_bsi_div_indexed_device): the three symbols are declared,
listed and exported, the scratch is the formula the header states (the builder's for n_slices_out + 1 rows, and 4 KiB per segment
for each slice of B's image and of the two remainder buffers), and every refusal the host can see comes back with its code, in
the order the header states, before any HIP call -- so without a device: made-up non-null integers stand in for device pointers,
nothing follows them."""
import importlib
import inspect
import os
import re
import subprocess

import pytest

from tests import _div

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
EXISTS_A, EXISTS_B = 1, 2
QUOTIENT, REMAINDER = 0, 1
SEG = 992
SYMBOLS = ("wah_bsi_div_scratch_bytes", "wah_bsi_div_indexed_device", "wah_bsi_div_status")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wah.h")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("gpu-wah_amd")
    p.build()
    return p


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _round256(x):
    return (x + 255) // 256 * 256


def test_symbols_are_declared_listed_and_exported(pkg, lib):
    with open(HEADER) as f:
        header = f.read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path()], text=True)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
        assert re.search(rf"\bT {name}\b", exported), name
    assert "XA, XB, B0, B1, A2, A1, A0" in header
    assert re.search(r"#define\s+WAH_DIV_QUOTIENT\s+0\b", header) and re.search(r"#define\s+WAH_DIV_REMAINDER\s+1\b", header)
    assert (pkg.DIV_QUOTIENT, pkg.DIV_REMAINDER) == (QUOTIENT, REMAINDER)
    assert list(inspect.signature(pkg.bsi_div_row_order).parameters) == ["ka", "kb", "exists_a", "exists_b"]
    assert list(inspect.signature(pkg.bsi_div_device).parameters) == [
        "table", "n_bits_a", "n_bits_b", "n_bits_out", "n_words", "remainder", "exists_a", "exists_b", "scratch", "out", "out_offsets", "check"]
    for front in (pkg.columns.divide_columns, pkg.columns.modulo_columns):
        assert list(inspect.signature(front).parameters) == ["wah", "bsi_a", "bsi_b", "n_bits", "table", "reuse"]
    assert list(inspect.signature(pkg.columns.divide_column_by).parameters) == ["wah", "bsi", "c", "remainder", "n_bits"]


def test_scratch_is_the_documented_formula(lib):
    """The builder's scratch for rows_out = n_slices_out + 1 rows WHATEVER the flags -- the control words (1 KiB), the result's slice
    matrix and the compress workspace, every part rounded up to 256 bytes -- and behind it the working area: per segment 4 KiB for
    each slice of B's image and of the two remainder buffers of n_slices_b + 1 slices."""
    for n_words in (SEG, SEG * 3, SEG * 4096):
        for kb in (1, 8, 40, 64):
            for n_out in (1, 2, 21, 63, 64):
                for flags in (0, EXISTS_A, EXISTS_B, EXISTS_A | EXISTS_B):
                    rows_out = n_out + 1
                    build = 1024 + _round256(4 * rows_out * n_words) + _round256(lib.wah_compress_workspace_bytes(rows_out * n_words))
                    want = build + 4096 * (n_words // SEG) * (3 * kb + 2)
                    got = lib.wah_bsi_div_scratch_bytes(n_words, kb, n_out, flags)
                    assert got == want == lib.wah_bsi_build_scratch_bytes(n_words, rows_out) + 4096 * (n_words // SEG) * (3 * kb + 2), (n_words, kb, n_out, flags)
                    assert got == lib.wah_bsi_arith_scratch_bytes(n_words, n_out, EXISTS_A) + 4096 * (n_words // SEG) * (3 * kb + 2)
                    assert build % 256 == 0  # the working area's 16-byte accesses are aligned


# pointers that are never followed: every call below is refused on the host
TABLE, OUT, COUNT, OFFSETS, SCRATCH = 0x10000, 0x30000, 0x40000, 0x60000, 0x100000


def _call(lib, what=QUOTIENT, n_words=SEG * 4, ka=20, kb=13, n_out=20, table=TABLE, flags=0, out=OUT, count=COUNT, offsets=OFFSETS,
          scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = 1 << 62  # enough for anything: what is refused is refused for its arguments
    return lib.wah_bsi_div_indexed_device(what, n_words, ka, kb, n_out, table, flags, out, 1 << 20, count, offsets, scratch, scratch_bytes, None)


BAD_ARGUMENTS = (
    dict(what=2), dict(what=-1), dict(what=1 << 20),
    dict(ka=0), dict(ka=65), dict(ka=1 << 32), dict(kb=0), dict(kb=65), dict(kb=1 << 32), dict(n_out=0), dict(n_out=65), dict(n_out=1 << 32),
    dict(flags=4), dict(flags=7), dict(flags=1 << 31),
    dict(n_words=0), dict(n_words=SEG + 1), dict(n_words=SEG - 1), dict(n_words=1),
    dict(n_words=SEG << 31, n_out=1),                     # a multiple of 992 at or above 2^40 words in ONE slice
    dict(n_words=SEG << 26, n_out=16),                    # 17 rows of 992 * 2^26 words: 16864 * 2^26 >= 2^40
    dict(n_words=SEG << 25, n_out=64),                    # 65 rows of 992 * 2^25 words: 64480 * 2^25 >= 2^40, WITHOUT a flag
    dict(table=None), dict(table=TABLE + 4), dict(table=TABLE + 1),
    dict(scratch=None), dict(scratch=SCRATCH + 128), dict(scratch=SCRATCH + 8),
    dict(out=None), dict(out=OUT + 2),
    dict(count=None), dict(count=COUNT + 4),
    dict(offsets=None), dict(offsets=OFFSETS + 4),
)


@pytest.mark.parametrize("what", [QUOTIENT, REMAINDER])
@pytest.mark.parametrize("bad", BAD_ARGUMENTS, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_ARGUMENTS])
def test_argument_errors_come_back_before_any_hip_call(lib, bad, what):
    args = dict(what=what)
    args.update(bad)
    assert _call(lib, **args) == WAH_ERR_ARG
    assert lib.wah_last_error()
    # the argument checks come first: a bad argument AND too small a scratch is a bad argument
    assert _call(lib, scratch_bytes=0, **args) == WAH_ERR_ARG


def _message(lib):
    text = lib.wah_last_error()
    return text.decode() if isinstance(text, bytes) else str(text)


def test_the_order_of_the_refusals(lib):
    """An unknown `what`, then the slice counts and the flags, then n_words, then the table and the scratch, then the output
    triple, then the scratch's size: of two things wrong the earlier one is named."""
    steps = (dict(what=2), dict(ka=65), dict(n_words=SEG + 1), dict(table=None), dict(out=None))
    messages = []
    for bad in steps:
        assert _call(lib, **bad) == WAH_ERR_ARG
        messages.append(_message(lib))
    assert len(set(messages)) == len(steps), messages
    for i, first in enumerate(steps):
        for later in steps[i + 1:]:
            both = dict(first)
            both.update(later)
            assert _call(lib, scratch_bytes=0, **both) == WAH_ERR_ARG and _message(lib) == messages[i], (first, later)
    assert _call(lib, what=2, ka=0, kb=0, n_out=0, flags=8) == WAH_ERR_ARG and _message(lib) == messages[0]
    assert _call(lib, scratch=None) == WAH_ERR_ARG and _message(lib) == messages[3]  # (the scratch pointer is judged with the table)
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE and _message(lib) not in messages


def test_the_existence_row_counts_whatever_the_flags(lib):
    """rows_out = n_slices_out + 1: 64 slices of 992 * 2^24 words and the existence row reach 2^40 words where the 64 slices alone
    do not -- the multiplication call, whose result has no such row without a flag, accepts these arguments."""
    n_words = ((1 << 40) // 65 // SEG + 1) * SEG
    assert 64 * n_words < (1 << 40) <= 65 * n_words
    assert _call(lib, n_words=n_words, ka=64, kb=64, n_out=64, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, n_words=n_words, ka=64, kb=64, n_out=63, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_bsi_mul_indexed_device(n_words, 64, 64, 64, TABLE, 0, OUT, 1 << 20, COUNT, OFFSETS, SCRATCH, 0, None) == WAH_ERR_WORKSPACE
    assert lib.wah_bsi_mul_indexed_device(n_words, 64, 64, 64, TABLE, EXISTS_A, OUT, 1 << 20, COUNT, OFFSETS, SCRATCH, 0, None) == WAH_ERR_ARG
    assert lib.wah_bsi_arith_indexed_device(0, n_words, 64, 64, 64, TABLE, 0, OUT, 1 << 20, COUNT, OFFSETS, SCRATCH, 0, None) == WAH_ERR_WORKSPACE


def test_workspace_errors_and_the_edges_that_are_accepted_as_arguments(lib):
    for what in (QUOTIENT, REMAINDER):
        for ka, kb, n_out, flags in ((1, 1, 1, 0), (20, 13, 20, EXISTS_A), (13, 20, 8, EXISTS_B), (64, 64, 64, EXISTS_A | EXISTS_B), (1, 64, 1, 0),
                                     (64, 1, 64, 0), (5, 3, 12, 0)):
            need = lib.wah_bsi_div_scratch_bytes(SEG * 4, kb, n_out, flags)
            assert _call(lib, what=what, ka=ka, kb=kb, n_out=n_out, flags=flags, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
            assert _call(lib, what=what, ka=ka, kb=kb, n_out=n_out, flags=flags, scratch_bytes=0) == WAH_ERR_WORKSPACE
    # the builder's scratch does not suffice: the working area lies behind it; nor does that of a narrower B
    assert _call(lib, scratch_bytes=lib.wah_bsi_build_scratch_bytes(SEG * 4, 21)) == WAH_ERR_WORKSPACE
    assert _call(lib, kb=13, scratch_bytes=lib.wah_bsi_div_scratch_bytes(SEG * 4, 12, 20, 0)) == WAH_ERR_WORKSPACE
    # the flags change nothing: the existence row is there without them
    assert len({lib.wah_bsi_div_scratch_bytes(SEG * 4, 13, 20, flags) for flags in (0, EXISTS_A, EXISTS_B, EXISTS_A | EXISTS_B)}) == 1
    # the most words: one segment fewer than 2^40 over two rows, and over seventeen
    most = ((1 << 40) - 1) // 2 // SEG * SEG
    assert _call(lib, n_words=most, n_out=1, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_words=((1 << 40) - 1) // 17 // SEG * SEG, n_out=16, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_bsi_div_status(None, SEG, 13, 20, 0, None) == WAH_ERR_ARG


def test_row_order_is_the_tests_own(pkg):
    for ka, kb, _ in _div.WIDTHS:
        for have_a, have_b in _div.EXISTENCE:
            assert pkg.bsi_div_row_order(ka, kb, have_a, have_b) == _div.row_order(ka, kb, have_a, have_b), (ka, kb, have_a, have_b)
    assert pkg.bsi_div_row_order(3, 2, True, True) == [("a", 3), ("b", 2), ("b", 1), ("b", 0), ("a", 0), ("a", 1), ("a", 2)]


def test_python_front_end_refuses_before_the_library(pkg):
    for front in (pkg.columns.divide_columns, pkg.columns.modulo_columns):
        with pytest.raises(ValueError):
            front(pkg, (None, None, SEG, 3, False), (None, None, SEG * 2, 3, False))
        with pytest.raises(ValueError):
            front(pkg, (None, None, SEG, 3, False), (None, None, SEG, 3, False), n_bits=65)
        with pytest.raises(ValueError):
            front(pkg, (None, None, SEG, 3, False), (None, None, SEG, 3, False), n_bits=0)
    for c in (0, -1, 1 << 63):
        with pytest.raises(ValueError):
            pkg.columns.divide_column_by(pkg, (None, None, SEG, 3, False), c)
