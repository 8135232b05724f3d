"""CPU tests of the fetch call's boundary (include/wah.h: wah_fetch_indexed_device): the three symbols are exported, the scratch
is a multiple of 256, never 0 and monotone in n_rows, and every refusal the host can see comes back with its code before any
HIP call, the argument checks first -- so without a device."""
import importlib

import pytest

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
BITS, FIRST = 0, 1
MAX_OPERANDS = 1 << 24  # WAH_BITOP_LIST_MAX_OPERANDS


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.build()
    return pkg.lib()


def test_symbols_are_exported(lib):
    pkg = importlib.import_module("gpu-wah_amd")
    for name in ("wah_fetch_scratch_bytes", "wah_fetch_indexed_device", "wah_fetch_status"):
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    assert callable(pkg.fetch_device) and (pkg.FETCH_BITS, pkg.FETCH_FIRST) == (BITS, FIRST)
    for name in ("values_at_rows", "keys_at_rows", "select_values", "top_rows"):
        assert callable(getattr(pkg.columns, name)), name


@pytest.mark.parametrize("n_words", (1, 31, 992, 992 * 3 + 5, 1 << 23, (1 << 40) - 1))
def test_scratch_is_aligned_and_monotone(lib, n_words):
    counts = (0, 1, 63, 64, 65, 100, 10_000, 1 << 20, 1 << 30, (1 << 40) - 1, 1 << 40, (1 << 64) - 1)
    sizes = [lib.wah_fetch_scratch_bytes(n_words, r) for r in counts]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    segments = ((32 * n_words + 30) // 31 + 1023) // 1024
    for r, s in zip(counts[:10], sizes):
        assert s >= 1024 + 8 * (-(-r // 64) + min(r, segments))  # the control words and the item list
    assert lib.wah_fetch_scratch_bytes(n_words, 100) <= 1024 + 8 * 102 + 255  # ... and no more: it goes with the list
    assert lib.wah_fetch_scratch_bytes(0, 0) > 0


# pointers that are never followed: every call below is refused on the host
TABLE, ROWS, OUT, SCRATCH = 0x10000, 0x20000, 0x30000, 0x50000


def _call(lib, mode=BITS, n_words=992, n_operands=20, table=TABLE, rows=ROWS, n_rows=100, out=OUT, scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_fetch_scratch_bytes(n_words, n_rows)
    return lib.wah_fetch_indexed_device(mode, n_words, n_operands, table, rows, n_rows, out, scratch, scratch_bytes, None)


def test_host_visible_refusals(lib):
    for mode in (2, 3, 1 << 31):
        assert _call(lib, mode=mode) == WAH_ERR_ARG, mode
    for mode, counts in ((BITS, (0, 65, MAX_OPERANDS, 1 << 32)), (FIRST, (0, MAX_OPERANDS + 1, 1 << 32, (1 << 64) - 1))):
        for n_operands in counts:
            assert _call(lib, mode=mode, n_operands=n_operands) == WAH_ERR_ARG, (mode, n_operands)
    assert _call(lib, n_words=0, n_rows=1) == WAH_ERR_ARG
    assert _call(lib, n_words=1 << 40) == WAH_ERR_ARG
    assert _call(lib, n_rows=1 << 40) == WAH_ERR_ARG
    assert _call(lib, n_rows=(1 << 64) - 1) == WAH_ERR_ARG
    for name, bad in (("table", None), ("table", TABLE + 4), ("rows", None), ("rows", ROWS + 4), ("rows", ROWS + 1), ("out", None),
                      ("out", OUT + 4), ("scratch", None), ("scratch", SCRATCH + 128), ("scratch", SCRATCH + 8)):
        assert _call(lib, **{name: bad}) == WAH_ERR_ARG, (name, bad)
    # no listed row: rows and out may be null, but not misaligned; table and scratch are still needed
    for name, bad in (("table", None), ("rows", ROWS + 4), ("out", OUT + 4), ("scratch", None), ("scratch", SCRATCH + 128)):
        assert _call(lib, n_rows=0, **{name: bad}) == WAH_ERR_ARG, (name, bad)
    assert lib.wah_last_error()
    # the argument checks come first: a bad argument AND too small a scratch is a bad argument
    for bad in (dict(mode=2), dict(n_operands=0), dict(n_operands=65), dict(mode=FIRST, n_operands=MAX_OPERANDS + 1), dict(n_words=0),
                dict(n_words=1 << 40), dict(n_rows=1 << 40), dict(rows=None), dict(out=OUT + 4), dict(table=None)):
        assert _call(lib, scratch_bytes=0, **bad) == WAH_ERR_ARG, bad
    for mode, n_operands in ((BITS, 1), (BITS, 64), (FIRST, 65), (FIRST, MAX_OPERANDS)):
        for n_rows in (1, 100, 10_000):
            need = lib.wah_fetch_scratch_bytes(992, n_rows)
            assert _call(lib, mode=mode, n_operands=n_operands, n_rows=n_rows, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
            assert _call(lib, mode=mode, n_operands=n_operands, n_rows=n_rows, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert _call(lib, n_rows=0, rows=None, out=None, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_fetch_status(None, None) == WAH_ERR_ARG


def test_python_front_end_refuses_before_the_library():
    import torch

    pkg = importlib.import_module("gpu-wah_amd")
    with pytest.raises(pkg.WahError):
        pkg.fetch_device(torch.zeros((2, 3), dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 992, pkg.FETCH_BITS)  # a table on the CPU
