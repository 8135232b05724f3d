"""CPU tests of the order-statistics call's boundary (include/wah.h: wah_bsi_kth_indexed_device): the three symbols are
exported, the scratch is a multiple of 256 and never 0, and every refusal the host can see comes back with its code before any
HIP call, the argument checks first -- so without a device."""
import ctypes
import importlib

import pytest

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2


@pytest.fixture(scope="module")
def lib():
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.build()
    return pkg.lib()


def test_symbols_are_exported(lib):
    pkg = importlib.import_module("gpu-wah_amd")
    for name in ("wah_bsi_kth_scratch_bytes", "wah_bsi_kth_indexed_device", "wah_bsi_kth_status"):
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    assert callable(pkg.bsi_kth_device) and callable(pkg.bsi_kth_query)
    assert (pkg.BSI_KTH_ASCENDING, pkg.BSI_KTH_DESCENDING, pkg.BSI_KTH_QUANTILE, pkg.BSI_KTH_MAX_FILTERS) == (0, 1, 2, 64)
    for name in ("kth_column_where", "quantile_column_where", "min_column_where", "max_column_where", "median_column_where", "top_rows"):
        assert callable(getattr(pkg.columns, name)), name


@pytest.mark.parametrize("n_slices", (1, 3, 4, 5, 20, 63, 64))
def test_scratch_is_small_and_aligned(lib, n_slices):
    sizes = {lib.wah_bsi_kth_scratch_bytes(n, n_slices) for n in (0, 1, 31, 992, 992 * 3 + 5, 1 << 23, (1 << 40) - 1)}
    assert len(sizes) == 1  # nothing in it goes with n_words
    size = sizes.pop()
    assert size > 0 and size % 256 == 0 and size <= lib.wah_bsi_kth_scratch_bytes(0, 64) < 1 << 20


# pointers that are never followed: every call below is refused on the host
TABLE, QUERY, RESULT, SCRATCH = 0x10000, 0x20000, 0x30000, 0x50000


def _call(lib, n_words=992, n_filters=1, n_slices=20, table=TABLE, query=QUERY, result=RESULT, scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bsi_kth_scratch_bytes(n_words, n_slices)
    return lib.wah_bsi_kth_indexed_device(n_words, n_filters, n_slices, table, query, result, scratch, scratch_bytes, None)


def test_host_visible_refusals(lib):
    for n_slices in (0, 65, 1 << 32):
        assert _call(lib, n_slices=n_slices) == WAH_ERR_ARG, n_slices
    for n_filters in (65, 1 << 32, (1 << 64) - 1):
        assert _call(lib, n_filters=n_filters) == WAH_ERR_ARG, n_filters
    for name, bad in (("table", None), ("table", TABLE + 4), ("query", None), ("query", QUERY + 4), ("query", QUERY + 1),
                      ("result", None), ("result", RESULT + 4), ("scratch", None), ("scratch", SCRATCH + 128), ("scratch", SCRATCH + 8)):
        assert _call(lib, **{name: bad}) == WAH_ERR_ARG, (name, bad)
    assert _call(lib, n_words=1 << 40) == WAH_ERR_ARG
    assert lib.wah_last_error()
    # the argument checks come first: a bad argument AND too small a scratch is a bad argument
    assert _call(lib, n_slices=0, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, n_filters=65, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, query=None, scratch_bytes=0) == WAH_ERR_ARG
    assert _call(lib, n_words=1 << 40, scratch_bytes=0) == WAH_ERR_ARG
    for n_filters, n_slices in ((0, 1), (1, 20), (64, 64)):
        need = lib.wah_bsi_kth_scratch_bytes(992, n_slices)
        assert _call(lib, n_filters=n_filters, n_slices=n_slices, scratch_bytes=need - 1) == WAH_ERR_WORKSPACE
        assert _call(lib, n_filters=n_filters, n_slices=n_slices, scratch_bytes=0) == WAH_ERR_WORKSPACE
    assert lib.wah_bsi_kth_status(None, None) == WAH_ERR_ARG


def test_python_front_end_refuses_bad_query_words():
    pkg = importlib.import_module("gpu-wah_amd")
    for triple in ((-1, 0, 1), (0, 1 << 64, 1), (2, 1, -5)):
        with pytest.raises(pkg.WahError):
            pkg.bsi_kth_query(*triple, device="cpu")
    t = pkg.bsi_kth_query(2, (1 << 64) - 1, 1 << 63, device="cpu")
    assert t.tolist() == [2, -1, -(1 << 63)]
    assert ctypes.c_uint64(t[1].item()).value == (1 << 64) - 1
    with pytest.raises(ValueError):
        pkg.columns.quantile_column_where(pkg, None, 3, 2)
    with pytest.raises(ValueError):
        pkg.columns.quantile_column_where(pkg, None, 0, 0)
