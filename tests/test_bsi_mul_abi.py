"""CPU tests of the column multiplication call's boundary (include/wah.h: wah_bsi_mul_indexed_device): the three symbols are
declared, listed and exported, the scratch is the formula the header states (the arithmetic call's, and 4 KiB per segment for each
slice of A and of the result), and every refusal the host can see comes back with its code before any HIP call -- so without a
device: made-up non-null integers stand in for device pointers, nothing follows them."""
import importlib
import inspect
import os
import re
import subprocess

import pytest

from tests import _mul

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
EXISTS_A, EXISTS_B = 1, 2
SEG = 992
SYMBOLS = ("wah_bsi_mul_scratch_bytes", "wah_bsi_mul_indexed_device", "wah_bsi_mul_status")
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
    assert "XA, XB, A0, A1, A2, B0, B1" in header
    assert callable(pkg.bsi_mul_row_order)
    assert list(inspect.signature(pkg.bsi_mul_device).parameters) == [
        "table", "n_bits_a", "n_bits_b", "n_bits_out", "n_words", "exists_a", "exists_b", "scratch", "out", "out_offsets", "check"]
    assert list(inspect.signature(pkg.columns.multiply_columns).parameters) == ["wah", "bsi_a", "bsi_b", "n_bits", "table", "reuse"]
    assert list(inspect.signature(pkg.columns.sum_product_where).parameters) == ["wah", "bsi_a", "bsi_b", "mask_stream", "mask_offsets"]


def test_scratch_is_the_documented_formula(lib):
    """The arithmetic call's scratch for rows_out = n_slices_out + (any existence flag ? 1 : 0) rows -- the control words (1 KiB),
    the result's slice matrix and the compress workspace, every part rounded up to 256 bytes -- and behind it the working area:
    per segment 4 KiB for each slice of A and of the result."""
    for n_words in (SEG, SEG * 3, SEG * 4096):
        for ka in (1, 8, 40, 64):
            for n_out in (1, 2, 21, 63, 64):
                for flags in (0, EXISTS_A, EXISTS_B, EXISTS_A | EXISTS_B):
                    rows_out = n_out + (1 if flags else 0)
                    build = 1024 + _round256(4 * rows_out * n_words) + _round256(lib.wah_compress_workspace_bytes(rows_out * n_words))
                    want = build + 4096 * (n_words // SEG) * (ka + n_out)
                    got = lib.wah_bsi_mul_scratch_bytes(n_words, ka, n_out, flags)
                    assert got == want == lib.wah_bsi_arith_scratch_bytes(n_words, n_out, flags) + 4096 * (n_words // SEG) * (ka + n_out), (n_words, ka, n_out, flags)
                    assert build % 256 == 0  # the working area's 16-byte accesses are aligned


# pointers that are never followed: every call below is refused on the host
TABLE, OUT, COUNT, OFFSETS, SCRATCH = 0x10000, 0x30000, 0x40000, 0x60000, 0x100000


def _call(lib, n_words=SEG * 4, ka=20, kb=13, n_out=33, table=TABLE, flags=0, out=OUT, count=COUNT, offsets=OFFSETS, scratch=SCRATCH,
          scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = 1 << 62  # enough for anything: what is refused is refused for its arguments
    return lib.wah_bsi_mul_indexed_device(n_words, ka, kb, n_out, table, flags, out, 1 << 20, count, offsets, scratch, scratch_bytes, None)


BAD_ARGUMENTS = (
    dict(ka=0), dict(ka=65), dict(ka=1 << 32), dict(kb=0), dict(kb=65), dict(kb=1 << 32), dict(n_out=0), dict(n_out=65), dict(n_out=1 << 32),
    dict(flags=4), dict(flags=7), dict(flags=1 << 31),
    dict(n_words=0), dict(n_words=SEG + 1), dict(n_words=SEG - 1), dict(n_words=1),
    dict(n_words=SEG << 31, n_out=1),                     # a multiple of 992 at or above 2^40 words in ONE slice
    dict(n_words=SEG << 26, n_out=17),                    # 17 slices of 992 * 2^26 words: 16864 * 2^26 >= 2^40
    dict(n_words=SEG << 25, n_out=64, flags=EXISTS_B),    # 65 rows of 992 * 2^25 words: 64480 * 2^25 >= 2^40
    dict(table=None), dict(table=TABLE + 4), dict(table=TABLE + 1),
    dict(scratch=None), dict(scratch=SCRATCH + 128), dict(scratch=SCRATCH + 8),
    dict(out=None), dict(out=OUT + 2),
    dict(count=None), dict(count=COUNT + 4),
    dict(offsets=None), dict(offsets=OFFSETS + 4),
)


@pytest.mark.parametrize("bad", BAD_ARGUMENTS, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_ARGUMENTS])
def test_argument_errors_come_back_before_any_hip_call(lib, bad):
    assert _call(lib, **bad) == WAH_ERR_ARG
    assert lib.wah_last_error()
    # the argument checks come first: a bad argument AND too small a scratch is a bad argument
    assert _call(lib, scratch_bytes=0, **bad) == WAH_ERR_ARG


def test_workspace_errors_and_the_edges_that_are_accepted_as_arguments(lib):
    for ka, kb, n_out, flags in ((1, 1, 2, 0), (1, 1, 1, 0), (20, 13, 33, EXISTS_A), (13, 20, 8, EXISTS_B), (64, 64, 64, EXISTS_A | EXISTS_B),
                                 (1, 64, 1, 0), (5, 3, 12, 0)):
        need = lib.wah_bsi_mul_scratch_bytes(SEG * 4, ka, n_out, flags)
        assert _call(lib, ka=ka, kb=kb, n_out=n_out, flags=flags, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
        assert _call(lib, ka=ka, kb=kb, n_out=n_out, flags=flags, scratch_bytes=0) == WAH_ERR_WORKSPACE
    # the arithmetic call's scratch does not suffice: the working area lies behind it; nor does that of a narrower A
    assert _call(lib, scratch_bytes=lib.wah_bsi_arith_scratch_bytes(SEG * 4, 33, 0)) == WAH_ERR_WORKSPACE
    assert _call(lib, ka=20, scratch_bytes=lib.wah_bsi_mul_scratch_bytes(SEG * 4, 19, 33, 0)) == WAH_ERR_WORKSPACE
    # with an existence flag the result has one row more: what suffices without does not suffice with one
    plain, flagged = lib.wah_bsi_mul_scratch_bytes(SEG * 4, 20, 33, 0), lib.wah_bsi_mul_scratch_bytes(SEG * 4, 20, 33, EXISTS_A)
    assert plain < flagged and _call(lib, flags=EXISTS_A, scratch_bytes=plain) == WAH_ERR_WORKSPACE
    # the most words: one segment fewer than 2^40, in one row and over sixteen
    most = ((1 << 40) - 1) // SEG * SEG
    assert _call(lib, n_words=most, n_out=1, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_words=most // 16 // SEG * SEG, n_out=16, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_bsi_mul_status(None, SEG, 20, 33, 0, None) == WAH_ERR_ARG


def test_row_order_is_the_tests_own(pkg):
    for ka, kb, _ in _mul.WIDTHS:
        for have_a, have_b in _mul.EXISTENCE:
            assert pkg.bsi_mul_row_order(ka, kb, have_a, have_b) == _mul.row_order(ka, kb, have_a, have_b), (ka, kb, have_a, have_b)
    assert pkg.bsi_mul_row_order(3, 2, True, True) == [("a", 3), ("b", 2), ("a", 2), ("a", 1), ("a", 0), ("b", 1), ("b", 0)]


def test_python_front_end_refuses_before_the_library(pkg):
    with pytest.raises(ValueError):
        pkg.columns.multiply_columns(pkg, (None, None, SEG, 3, False), (None, None, SEG * 2, 3, False))
    with pytest.raises(ValueError):
        pkg.columns.multiply_columns(pkg, (None, None, SEG, 3, False), (None, None, SEG, 3, False), n_bits=65)
    with pytest.raises(ValueError):
        pkg.columns.sum_product_where(pkg, (None, None, SEG, 33, False), (None, None, SEG, 32, False), None, None)
