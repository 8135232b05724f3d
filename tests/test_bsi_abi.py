"""CPU tests of the bit-sliced range call's boundary (include/wah.h: wah_bsi_range_indexed_device): the three symbols are
exported, the scratch is the other indexed calls', and every refusal the host can see comes back with its code before any HIP
call -- so without a device."""
import ctypes
import importlib

import pytest

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
EXISTS = 1


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.build()
    return pkg.lib()


def test_symbols_are_exported(lib):
    pkg = importlib.import_module("gpu-wah_amd")
    for name in ("wah_bsi_range_scratch_bytes", "wah_bsi_range_indexed_device", "wah_bsi_range_status"):
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    assert callable(pkg.bsi_range_device) and pkg.BSI_MAX_SLICES == 64 and pkg.BSI_EXISTS == EXISTS
    for name in ("bsi_from_values", "range_column", "compare_column", "sum_column_where"):
        assert callable(getattr(pkg.columns, name)), name


@pytest.mark.parametrize("n_slices", (1, 20, 64))
def test_scratch_is_the_indexed_calls(lib, n_slices):
    for n in (0, 1, 31, 992, 992 * 3 + 5, 1 << 23):
        assert lib.wah_bsi_range_scratch_bytes(n, n_slices) == lib.wah_bitop_indexed_scratch_bytes(n) > 0


# pointers that are never followed: every call below is refused on the host
TABLE, BOUNDS, OUT, COUNT, SCRATCH = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


def _call(lib, n_words=992, n_slices=20, table=TABLE, bounds=BOUNDS, flags=0, out=OUT, count=COUNT, scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bsi_range_scratch_bytes(n_words, n_slices)
    return lib.wah_bsi_range_indexed_device(n_words, n_slices, table, bounds, flags, out, 1 << 20, count, None, scratch, scratch_bytes, None)


def test_host_visible_refusals(lib):
    for n_slices in (0, 65, 1 << 32):
        assert _call(lib, n_slices=n_slices) == WAH_ERR_ARG, n_slices
    for flags in (2, 3, 1 << 31):
        assert _call(lib, flags=flags) == WAH_ERR_ARG, flags
    for name, bad in (("table", None), ("table", TABLE + 4), ("bounds", None), ("bounds", BOUNDS + 4), ("bounds", BOUNDS + 1),
                      ("scratch", None), ("scratch", SCRATCH + 128), ("scratch", SCRATCH + 8), ("count", None), ("out", None)):
        assert _call(lib, **{name: bad}) == WAH_ERR_ARG, (name, bad)
    assert _call(lib, n_words=1 << 40) == WAH_ERR_ARG
    assert lib.wah_last_error()
    # the argument checks come first: a bad argument AND too small a scratch is a bad argument
    assert _call(lib, n_slices=0, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, flags=2 | EXISTS, scratch_bytes=0) == WAH_ERR_ARG
    for n_slices, flags in ((1, 0), (20, EXISTS), (64, EXISTS)):
        need = lib.wah_bsi_range_scratch_bytes(992, n_slices)
        assert _call(lib, n_slices=n_slices, flags=flags, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
        assert _call(lib, n_slices=n_slices, flags=flags, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_bsi_range_status(None, 992, 20, None) == WAH_ERR_ARG


def test_python_front_end_refuses_bad_bounds():
    pkg = importlib.import_module("gpu-wah_amd")
    for lo, hi in ((-1, 5), (0, 1 << 64)):
        with pytest.raises(pkg.WahError):
            pkg.bsi_bounds(lo, hi, "cpu")
    t = pkg.bsi_bounds(1 << 63, (1 << 64) - 1, "cpu")
    assert t.tolist() == [-(1 << 63), -1]
    assert ctypes.c_uint64(t[1].item()).value == (1 << 64) - 1
