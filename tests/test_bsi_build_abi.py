"""CPU tests of the boundary of wah_bsi_build_device (include/wah.h): the three symbols exist in the header, in api.ABI_SYMBOLS
and in the library; the scratch size is the formula the header states; every argument error the host can see comes back before
any HIP call is made (no GPU here: made-up non-null integers stand in for device pointers, nothing follows them); and the Python
front ends are exported."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wah_bsi_build_scratch_bytes", "wah_bsi_build_device", "wah_bsi_build_status")
WAH_ERR_ARG, WAH_ERR_WORKSPACE = -1, -2
SEG = 992


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("gpu-wah_amd")
    p.build()
    return p


def _round256(x):
    return (x + 255) // 256 * 256


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
    """The control words (1 KiB), the slice matrix of 4 * n_slices * n_words bytes and the compress workspace of a bitmap of
    n_slices * n_words words, every part rounded up to 256 bytes."""
    lib = pkg.lib()
    for n_words in (SEG, SEG * 3, SEG * 4096):
        for n_slices in (1, 2, 21, 64, 65):
            want = 1024 + _round256(4 * n_slices * n_words) + _round256(lib.wah_compress_workspace_bytes(n_slices * n_words))
            got = lib.wah_bsi_build_scratch_bytes(n_words, n_slices)
            assert got == want, (n_words, n_slices)
            assert got % 256 == 0 and got > 4 * n_slices * n_words


def _call(lib, n_words=SEG * 4, n_bits=20, values=0x20000, n_rows=100, exists=0x60000, out=0x30000, cap=1000, out_words=0x40000,
          out_offsets=0x50000, scratch=0x100000, scratch_bytes=None):
    if scratch_bytes is None:
        slices = min(max(n_bits, 1), 64) + (1 if exists else 0)
        scratch_bytes = lib.wah_bsi_build_scratch_bytes(max(min(n_words, (1 << 40) // slices - 1), 1), slices)
    return lib.wah_bsi_build_device(n_words, n_bits, values, n_rows, exists, out, cap, out_words, out_offsets, scratch, scratch_bytes, None)


BAD_ARGUMENTS = (
    dict(n_bits=0), dict(n_bits=65), dict(n_bits=1 << 32),
    dict(n_words=0), dict(n_words=SEG + 1), dict(n_words=SEG - 1), dict(n_words=1),
    dict(n_words=SEG << 31, n_bits=1, exists=None),      # a multiple of 992 at or above 2^40 words in ONE slice
    dict(n_words=SEG << 26, n_bits=17, exists=None),     # 17 slices of 992 * 2^26 words: 16864 * 2^26 >= 2^40
    dict(n_words=SEG << 25, n_bits=64),                  # 65 slices of 992 * 2^25 words: 64480 * 2^25 >= 2^40
    dict(n_rows=32 * SEG * 4 + 1),
    dict(values=None),                                   # null values with n_rows > 0
    dict(values=0x20004),
    dict(out=None), dict(out=0x30002),
    dict(out_words=None), dict(out_words=0x40004),
    dict(out_offsets=None), dict(out_offsets=0x50004),
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
    need = lib.wah_bsi_build_scratch_bytes(SEG * 4, 21)
    assert _call(lib, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
    # without existence bytes the scratch is one slice smaller: what suffices there does not suffice with them
    plain = lib.wah_bsi_build_scratch_bytes(SEG * 4, 20)
    assert plain < need and _call(lib, scratch_bytes=plain) == WAH_ERR_WORKSPACE
    assert _call(lib, exists=None, scratch_bytes=plain - 1) == WAH_ERR_WORKSPACE
    # accepted as arguments (the next check refuses them for their scratch): 1 and 64 bits, 64 bits and existence bytes; no rows
    # and no value pointer; a full column; existence bytes at any address; the most words: one segment fewer than 2^40
    for n_bits in (1, 64):
        assert _call(lib, n_bits=n_bits, scratch_bytes=0) == WAH_ERR_WORKSPACE
        assert _call(lib, n_bits=n_bits, exists=None, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, values=None, n_rows=0, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_rows=32 * SEG * 4, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, exists=0x60003, scratch_bytes=0) == WAH_ERR_WORKSPACE
    most = ((1 << 40) - 1) // SEG * SEG
    assert _call(lib, n_words=most, n_bits=1, exists=None, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_words=most // 16 // SEG * SEG, n_bits=16, exists=None, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_bsi_build_status(None, SEG, 1, None) == WAH_ERR_ARG


def test_python_front_ends_are_exported(pkg):
    assert callable(pkg.bsi_build_device) and "wah_bsi_build_device" in pkg.bsi_build_device.__doc__
    assert list(inspect.signature(pkg.bsi_build_device).parameters) == ["values", "n_bits", "n_words", "exists", "scratch", "out", "out_offsets", "check"]
    from_values = inspect.signature(pkg.columns.bsi_from_values).parameters
    assert list(from_values) == ["wah", "values", "n_bits", "n_words_per_column", "exists", "check"] and from_values["check"].default is True
    assert list(inspect.signature(pkg.columns._bsi_from_values_torch).parameters) == ["wah", "values", "n_bits", "n_words_per_column", "exists"]
