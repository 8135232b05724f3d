"""CPU tests of the boundary of wah_bsi_kth_grouped_indexed_device (include/wah.h): the three symbols are declared, listed in
api.ABI_SYMBOLS and exported; the scratch is a multiple of 256, never 0, follows the formula the header states and does not go with
n_words; every refusal the host can see comes back with its code before any HIP call, the argument checks first (no GPU here:
made-up non-null integers stand in for device pointers, nothing follows them); the Python front ends refuse what they can see."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wah_bsi_kth_grouped_scratch_bytes", "wah_bsi_kth_grouped_indexed_device", "wah_bsi_kth_grouped_status")
WAH_ERR_ARG, WAH_ERR_WORKSPACE = -1, -2
MAX_LANES = 4096      # WAH_BSI_KTH_GROUPED_MAX_LANES
MAX_ROWS = 1 << 24    # WAH_BITOP_LIST_MAX_OPERANDS


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("gpu-wah_amd")
    p.build()
    return p


def test_symbols_in_header_binding_and_library(pkg):
    header = open(os.path.join(ROOT, "include", "wah.h")).read()
    declared = set(re.findall(r"\b(wah_[a-z_0-9]+)\s*\(", header))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path()], text=True)
    for name, n_args in zip(NAMES, (4, 14, 2)):
        assert name in declared, name
        assert name in pkg.ABI_SYMBOLS and len(pkg.ABI_SYMBOLS[name][1]) == n_args, name
        assert re.search(rf"\bT {name}\b", exported), name
        assert hasattr(pkg.lib(), name), name
    assert re.search(r"#define\s+WAH_BSI_KTH_GROUPED_MAX_LANES\s+4096u\b", header)
    assert pkg.BSI_KTH_GROUPED_MAX_LANES == MAX_LANES
    assert "by the items of lane 0 in the LAST pass" in header  # where the contract is weaker than the ungrouped call's
    assert callable(pkg.bsi_kth_grouped_device) and callable(pkg.bsi_kth_queries) and callable(pkg.columns.quantiles_by)
    assert "wah_bsi_kth_grouped_indexed_device" in pkg.bsi_kth_grouped_device.__doc__
    assert "extremes_by" in pkg.columns.quantiles_by.__doc__
    # extremes_by is not touched
    assert "G x 2 calls" in pkg.columns.extremes_by.__doc__ and "no new kernel" in pkg.columns.extremes_by.__doc__


def _r256(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("n_slices", (1, 4, 5, 20, 63, 64))
@pytest.mark.parametrize("n_groups,n_queries", ((1, 1), (3, 3), (6, 2), (64, 2), (70, 1), (1, 4096), (4096, 1), (64, 64)))
def test_scratch_follows_the_stated_formula(pkg, n_slices, n_groups, n_queries):
    lib = pkg.lib()
    sizes = {lib.wah_bsi_kth_grouped_scratch_bytes(n, n_slices, n_groups, n_queries) for n in (0, 1, 31, 992, 992 * 3 + 5, 1 << 23, (1 << 40) - 1)}
    assert len(sizes) == 1  # nothing in it goes with n_words
    size = sizes.pop()
    lanes, passes = n_groups * n_queries, (n_slices + 3) // 4
    assert size == 1024 + _r256(lanes * 128) + _r256(passes * lanes * 128)
    assert size > 0 and size % 256 == 0
    assert size <= lib.wah_bsi_kth_grouped_scratch_bytes(0, 64, 64, 64) < 16 << 20


def test_scratch_of_a_call_that_is_refused_anyway_is_never_zero(pkg):
    lib = pkg.lib()
    for args in ((0, 1, 1), (65, 1, 1), (20, 0, 1), (20, 1, 0), (20, 4097, 1), (20, 1 << 40, 1 << 40), (20, (1 << 64) - 1, 3)):
        size = lib.wah_bsi_kth_grouped_scratch_bytes(992, *args)
        assert size > 0 and size % 256 == 0, args


# pointers that are never followed: every call below is refused on the host
FILTERS, GROUPS, SLICES, QUERIES, RESULTS, SCRATCH = 0x4000, 0x8000, 0x10000, 0x20000, 0x30000, 0x100000


def _call(lib, n_words=992 * 4, n_filters=1, filters=FILTERS, n_groups=3, rows_per_group=1, groups=GROUPS, n_slices=20, slices=SLICES,
          n_queries=2, queries=QUERIES, results=RESULTS, scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bsi_kth_grouped_scratch_bytes(n_words, n_slices, n_groups, n_queries)
    return lib.wah_bsi_kth_grouped_indexed_device(n_words, n_filters, filters, n_groups, rows_per_group, groups, n_slices, slices,
                                                  n_queries, queries, results, scratch, scratch_bytes, None)


BAD_ARGUMENTS = [
    dict(n_slices=0), dict(n_slices=65), dict(n_slices=1 << 32),
    dict(n_filters=65), dict(n_filters=1 << 32), dict(n_filters=(1 << 64) - 1),
    dict(filters=None), dict(filters=FILTERS + 4), dict(n_filters=0, filters=FILTERS + 4),      # null with a filter; misaligned even unread
    dict(groups=None), dict(groups=GROUPS + 4), dict(slices=None), dict(slices=SLICES + 4),
    dict(queries=None), dict(queries=QUERIES + 4), dict(queries=QUERIES + 1), dict(results=None), dict(results=RESULTS + 4),
    dict(scratch=None), dict(scratch=SCRATCH + 128), dict(scratch=SCRATCH + 8),
    dict(rows_per_group=0), dict(rows_per_group=9), dict(rows_per_group=1 << 63),
    dict(n_groups=0), dict(n_queries=0),
    dict(n_groups=MAX_LANES + 1, n_queries=1), dict(n_groups=1, n_queries=MAX_LANES + 1), dict(n_groups=MAX_LANES // 2 + 1, n_queries=2),
    dict(n_groups=65, n_queries=64), dict(n_groups=1 << 32, n_queries=1 << 32), dict(n_groups=(1 << 63) + 1, n_queries=2),   # ... wrapping round 2^64
    dict(n_groups=1 << 62, rows_per_group=4, n_queries=1),
    dict(n_words=1 << 40), dict(n_words=(1 << 64) - 1),
]


def test_argument_errors_come_back_before_any_hip_call(pkg):
    lib = pkg.lib()
    for bad in BAD_ARGUMENTS:
        assert _call(lib, **bad) == WAH_ERR_ARG, bad
        assert ctypes.c_char_p(lib.wah_last_error()).value, bad
        # the argument checks come first: a bad argument with too small a scratch is an argument error
        assert _call(lib, scratch_bytes=0, **bad) == WAH_ERR_ARG, bad
    assert lib.wah_bsi_kth_grouped_status(None, None) == WAH_ERR_ARG


def test_the_limits_themselves_reach_the_workspace_check(pkg):
    lib = pkg.lib()
    for good in (dict(), dict(n_filters=0, filters=None), dict(n_filters=64), dict(rows_per_group=8), dict(n_slices=1), dict(n_slices=64),
                 dict(n_groups=MAX_LANES, n_queries=1), dict(n_groups=1, n_queries=MAX_LANES), dict(n_groups=64, n_queries=64),
                 dict(n_groups=MAX_LANES, rows_per_group=8, n_queries=1), dict(n_groups=1, n_queries=1), dict(n_words=0),
                 dict(n_words=(1 << 40) - 1)):
        need = lib.wah_bsi_kth_grouped_scratch_bytes(good.get("n_words", 992 * 4), good.get("n_slices", 20), good.get("n_groups", 3),
                                                     good.get("n_queries", 2))
        assert _call(lib, scratch_bytes=need - 1, **good) == WAH_ERR_WORKSPACE, good
        assert _call(lib, scratch_bytes=0, **good) == WAH_ERR_WORKSPACE, good
    assert MAX_LANES * 8 <= MAX_ROWS  # the group-row bound cannot be reached below the lane bound: it is stated for the interface's sake


def test_python_front_ends_refuse_what_they_can_see(pkg):
    import torch

    for rows in ([(-1, 0, 1)], [(0, 1 << 64, 1)], [(2, 1, 2), (2, 1, -5)], []):
        with pytest.raises(pkg.WahError):
            pkg.bsi_kth_queries(rows, device="cpu")
    t = pkg.bsi_kth_queries([(2, (1 << 64) - 1, 1 << 63), (0, 5, 1)], device="cpu")
    assert t.dtype == torch.int64 and t.tolist() == [[2, -1, -(1 << 63)], [0, 5, 1]]
    out = torch.zeros((2, 3), dtype=torch.int64)
    assert pkg.bsi_kth_queries([(1, 2, 3), (2, 1, 2)], out=out) is out and out.tolist() == [[1, 2, 3], [2, 1, 2]]
    with pytest.raises(pkg.WahError):
        pkg.bsi_kth_queries([(1, 2, 3)], out=out)  # another number of rows
    # tables of the wrong shape: refused before anything is enqueued (CPU tensors are no tables)
    good = torch.zeros((3, 3), dtype=torch.int64)
    for filters, groups, slices in ((None, good, good), (None, good[:, :2], good), (None, good.to(torch.int32), good), (good, good, good)):
        with pytest.raises(pkg.WahError):
            pkg.bsi_kth_grouped_device(filters, groups, slices, [(0, 0, 1)], 992)
    for bad in (["mean"], [(1, 2, 3, 4)], [(3, 2)], [(0, 0)], [(1,)], []):
        with pytest.raises(ValueError):
            pkg.columns._quantile_queries(pkg, bad)
    assert pkg.columns._quantile_queries(pkg, ["min", "max", "median", (99, 100), (1, 7, 1)]) == [(2, 0, 1), (2, 1, 1), (2, 1, 2), (2, 99, 100), (1, 7, 1)]
