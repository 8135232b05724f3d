"""CPU tests of the membership call's boundary (include/wah.h: wah_bsi_member_indexed_device): the three symbols are declared,
mirrored and exported, the scratch is the other indexed calls', and every refusal the host can see comes back with its code, in
the order the header states, before any HIP call -- so without a device."""
import importlib
import os
import re

import numpy as np
import pytest

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
EXISTS, NEGATE, BITSET = 1, 2, 4
NAMES = ("wah_bsi_member_scratch_bytes", "wah_bsi_member_indexed_device", "wah_bsi_member_status")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.build()
    return pkg.lib()


def test_symbols_are_declared_mirrored_and_exported(lib):
    pkg = importlib.import_module("gpu-wah_amd")
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define WAH_MEMBER_NEGATE 2u", header) and re.search(r"#define WAH_MEMBER_BITSET 4u", header)
    assert (pkg.MEMBER_NEGATE, pkg.MEMBER_BITSET, pkg.BSI_EXISTS) == (NEGATE, BITSET, EXISTS)
    assert callable(pkg.bsi_member_device) and callable(pkg.member_set)
    for name in ("isin_column", "semi_join_rows", "semi_join_values"):
        assert callable(getattr(pkg.columns, name)), name


@pytest.mark.parametrize("n_slices", (1, 20, 32, 33, 64))
def test_scratch_is_the_indexed_calls(lib, n_slices):
    for n in (0, 1, 31, 992, 992 * 3 + 5, 1 << 23):
        assert lib.wah_bsi_member_scratch_bytes(n, n_slices) == lib.wah_bitop_indexed_scratch_bytes(n) > 0


# pointers that are never followed: every call below is refused on the host
TABLE, SET, COUNT, OUT, WORDS, SCRATCH = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000


def _call(lib, n_words=992, n_slices=20, table=TABLE, members=SET, capacity=100, count=None, flags=0, out=OUT, words=WORDS, scratch=SCRATCH,
          scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bsi_member_scratch_bytes(n_words, n_slices)
    return lib.wah_bsi_member_indexed_device(n_words, n_slices, table, members, capacity, count, flags, out, 1 << 20, words, None, scratch,
                                             scratch_bytes, None)


def test_host_visible_refusals(lib):
    for n_slices in (0, 65, 1 << 32):
        assert _call(lib, n_slices=n_slices) == WAH_ERR_ARG, n_slices
    for flags in (8, 8 | EXISTS, 16, 1 << 31):
        assert _call(lib, flags=flags) == WAH_ERR_ARG, flags
    for name, bad in (("table", None), ("table", TABLE + 4), ("scratch", None), ("scratch", SCRATCH + 128), ("scratch", SCRATCH + 8),
                      ("members", None), ("members", SET + 4), ("members", SET + 1), ("count", COUNT + 4), ("count", COUNT + 1),
                      ("capacity", 1 << 40), ("words", None), ("out", None)):
        assert _call(lib, **{name: bad}) == WAH_ERR_ARG, (name, bad)
    # a bit array: aligned to its words, and no count
    assert _call(lib, flags=BITSET, members=SET + 2) == WAH_ERR_ARG
    assert _call(lib, flags=BITSET, count=COUNT) == WAH_ERR_ARG
    assert _call(lib, flags=BITSET | NEGATE | EXISTS, capacity=1 << 40) == WAH_ERR_ARG
    assert _call(lib, flags=BITSET, members=None, capacity=1) == WAH_ERR_ARG
    assert _call(lib, n_words=1 << 40) == WAH_ERR_ARG
    assert lib.wah_last_error()
    # the argument checks come first: a bad argument AND too small a scratch is a bad argument
    assert _call(lib, n_slices=0, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, flags=8, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, members=SET + 4, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, out=None, scratch_bytes=0) == WAH_ERR_ARG
    # what is legal reaches the scratch check: every flag, a count, an empty set without a pointer, a 4-byte aligned bit array
    legal = (dict(), dict(flags=EXISTS | NEGATE), dict(count=COUNT), dict(members=None, capacity=0), dict(flags=BITSET, members=SET + 4),
             dict(flags=BITSET | NEGATE | EXISTS, capacity=(1 << 40) - 1), dict(flags=BITSET, members=None, capacity=0), dict(n_slices=64, flags=EXISTS),
             dict(n_slices=1), dict(n_slices=33, capacity=(1 << 40) - 1))
    for kw in legal:
        need = lib.wah_bsi_member_scratch_bytes(992, kw.get("n_slices", 20))
        assert _call(lib, scratch_bytes=need - 1, **kw) == WAH_ERR_WORKSPACE, kw
        assert _call(lib, scratch_bytes=0, **kw) == WAH_ERR_WORKSPACE, kw
    assert lib.wah_bsi_member_status(None, 992, 20, None) == WAH_ERR_ARG


def test_the_stated_order_of_the_refusals(lib):
    """include/wah.h: slices and flags, then table and scratch, then the set, then the output, then the scratch's size.  The text
    of wah_last_error names the first one that fails."""
    def text(**kw):
        assert _call(lib, **kw) in (WAH_ERR_ARG, WAH_ERR_WORKSPACE)
        return lib.wah_last_error().decode()

    slices, table, members, output, size = (text(n_slices=0), text(table=None), text(members=SET + 4), text(out=None), text(scratch_bytes=0))
    assert len({slices, table, members, output, size}) == 5
    assert text(n_slices=0, table=None, members=SET + 4, out=None, scratch_bytes=0) == slices
    assert text(flags=8, scratch=None) == slices
    assert text(table=None, members=SET + 4, out=None, scratch_bytes=0) == table
    assert text(scratch=SCRATCH + 8, capacity=1 << 40) == table
    assert text(members=SET + 4, out=None, scratch_bytes=0) == members
    assert text(flags=BITSET, count=COUNT, n_words=1 << 40) == members
    assert text(words=None, scratch_bytes=0) == output
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE


def test_member_set_sorts_unsigned_and_keeps_bit_patterns():
    pkg = importlib.import_module("gpu-wah_amd")
    t = pkg.member_set([5, (1 << 64) - 1, 1 << 63, 0, 5], "cpu")
    assert t.tolist() == [0, 5, 5, -(1 << 63), -1]
    t = pkg.member_set(np.array([1 << 63, 3, (1 << 64) - 1, 3], dtype=np.uint64), "cpu")
    assert t.numpy().view(np.uint64).tolist() == [3, 3, 1 << 63, (1 << 64) - 1]
    assert pkg.member_set([], "cpu").numel() == 0
    for bad in ([-1], [1 << 64]):
        with pytest.raises(pkg.WahError):
            pkg.member_set(bad, "cpu")
    with pytest.raises(pkg.WahError):
        pkg.member_set(np.array([1, 2], dtype=np.int64), "cpu")
