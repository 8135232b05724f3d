"""CPU tests of the column-to-column comparison call's boundary (include/wah.h: wah_bsi_compare_indexed_device): the three symbols
are declared, listed and exported, the scratch is the other indexed calls', and every refusal the host can see comes back with its
code before any HIP call -- so without a device."""
import importlib
import os

import pytest

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
EXISTS_A, EXISTS_B = 1, 2
SYMBOLS = ("wah_bsi_compare_scratch_bytes", "wah_bsi_compare_indexed_device", "wah_bsi_compare_status")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wah.h")


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.build()
    return pkg.lib()


def test_symbols_are_declared_listed_and_exported(lib):
    pkg = importlib.import_module("gpu-wah_amd")
    with open(HEADER) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    for text in ("#define WAH_BSI_EXISTS_A 1u", "#define WAH_BSI_EXISTS_B 2u", "#define WAH_CMP_LT 0", "#define WAH_CMP_LE 1",
                 "#define WAH_CMP_GT 2", "#define WAH_CMP_GE 3", "#define WAH_CMP_EQ 4", "#define WAH_CMP_NE 5"):
        assert text in header, text
    assert pkg.CMP_OPS == {"<": 0, "<=": 1, ">": 2, ">=": 3, "==": 4, "!=": 5}
    assert (pkg.BSI_EXISTS_A, pkg.BSI_EXISTS_B) == (EXISTS_A, EXISTS_B)
    assert callable(pkg.bsi_compare_device) and callable(pkg.bsi_compare_row_order)
    assert callable(pkg.columns.compare_columns)


@pytest.mark.parametrize("ka,kb", ((1, 1), (20, 13), (1, 64), (64, 64)))
def test_scratch_is_the_indexed_calls(lib, ka, kb):
    for n in (0, 1, 31, 992, 992 * 3 + 5, 1 << 23):
        assert lib.wah_bsi_compare_scratch_bytes(n, ka, kb) == lib.wah_bitop_indexed_scratch_bytes(n) > 0


# pointers that are never followed: every call below is refused on the host
TABLE, OUT, COUNT, SCRATCH = 0x10000, 0x30000, 0x40000, 0x50000


def _call(lib, op=2, n_words=992, ka=20, kb=13, table=TABLE, flags=0, out=OUT, count=COUNT, scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bsi_compare_scratch_bytes(n_words, ka, kb)
    return lib.wah_bsi_compare_indexed_device(op, n_words, ka, kb, table, flags, out, 1 << 20, count, None, scratch, scratch_bytes, None)


def test_host_visible_refusals(lib):
    for op in (-1, 6, 1 << 20):
        assert _call(lib, op=op) == WAH_ERR_ARG, op
    for k in (0, 65, 1 << 32):
        assert _call(lib, ka=k) == WAH_ERR_ARG, k
        assert _call(lib, kb=k) == WAH_ERR_ARG, k
    for flags in (4, 7, 1 << 31):
        assert _call(lib, flags=flags) == WAH_ERR_ARG, flags
    for name, bad in (("table", None), ("table", TABLE + 4), ("table", TABLE + 1), ("scratch", None), ("scratch", SCRATCH + 128),
                      ("scratch", SCRATCH + 8), ("count", None), ("out", None)):
        assert _call(lib, **{name: bad}) == WAH_ERR_ARG, (name, bad)
    assert _call(lib, n_words=1 << 40) == WAH_ERR_ARG
    assert lib.wah_last_error()
    # the argument checks come first: a bad argument AND too small a scratch is a bad argument
    assert _call(lib, op=6, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, ka=0, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, flags=4 | EXISTS_A, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, count=None, scratch_bytes=0) == WAH_ERR_ARG
    for op in range(6):
        for ka, kb, flags in ((1, 1, 0), (20, 13, EXISTS_A), (13, 20, EXISTS_B), (64, 64, EXISTS_A | EXISTS_B)):
            need = lib.wah_bsi_compare_scratch_bytes(992, ka, kb)
            assert _call(lib, op=op, ka=ka, kb=kb, flags=flags, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
            assert _call(lib, op=op, ka=ka, kb=kb, flags=flags, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_bsi_compare_status(None, 992, 20, 13, None) == WAH_ERR_ARG


def test_python_front_end_refuses_before_the_library():
    pkg = importlib.import_module("gpu-wah_amd")
    with pytest.raises(pkg.WahError):
        pkg.bsi_compare_device([], 3, 3, "=<", 0)  # the operator is looked at first
    with pytest.raises(ValueError):
        pkg.columns.compare_columns(pkg, (None, None, 992, 3, False), "<>", (None, None, 992, 3, False))
    with pytest.raises(ValueError):
        pkg.columns.compare_columns(pkg, (None, None, 992, 3, False), "<", (None, None, 1984, 3, False))
