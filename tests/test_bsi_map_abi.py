"""CPU tests of the map call's boundary (include/wah.h: wah_bsi_map_indexed_device): the three symbols are declared, mirrored and
exported, the scratch is the builder's layout, and every refusal the host can see comes back with its code, in the order the header
states, before any HIP call -- so without a device."""
import importlib
import os
import re

import pytest

WAH_OK, WAH_ERR_ARG, WAH_ERR_WORKSPACE = 0, -1, -2
EXISTS, PARTIAL = 1, 2
NAMES = ("wah_bsi_map_scratch_bytes", "wah_bsi_map_indexed_device", "wah_bsi_map_status")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 992


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
    assert re.search(r"#define WAH_MAP_PARTIAL 2u", header) and re.search(r"#define WAH_MAP_NULL 0xFFFFFFFFu", header)
    assert "2^32 - 1" in header[header.index("WAH_MAP_NULL"):]  # the reserved value is named
    assert (pkg.MAP_PARTIAL, pkg.MAP_NULL, pkg.BSI_EXISTS, pkg.columns.MAP_NULL) == (PARTIAL, 0xFFFFFFFF, EXISTS, 0xFFFFFFFF)
    assert callable(pkg.bsi_map_device)
    for name in ("map_column", "join_column", "apply_column"):
        assert callable(getattr(pkg.columns, name)), name


def test_scratch_is_the_builders_layout(lib):
    """include/wah.h states the formula: wah_bsi_build_scratch_bytes(n_words, rows_out), rows_out = n_slices_out and one more row with
    either flag."""
    for n in (SEG, 3 * SEG, SEG << 10):
        for k in (1, 7, 32):
            for flags in (0, EXISTS, PARTIAL, EXISTS | PARTIAL):
                want = lib.wah_bsi_build_scratch_bytes(n, k + (1 if flags else 0))
                assert lib.wah_bsi_map_scratch_bytes(n, k, flags) == want and want % 256 == 0 and want > 0, (n, k, flags)


# pointers that are never followed: every call below is refused on the host
KEY, MAP, OUT, COUNT, OFFS, SCRATCH = 0x20000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000


def _call(lib, n_words=SEG, n_rows=SEG * 32, ks=20, key=KEY, lookup=MAP, n_keys=1000, k_out=17, flags=0, out=OUT, cap=1 << 20, count=COUNT,
          offs=OFFS, scratch=SCRATCH, scratch_bytes=None):
    if scratch_bytes is None:
        scratch_bytes = lib.wah_bsi_map_scratch_bytes(n_words, k_out, flags)
    return lib.wah_bsi_map_indexed_device(n_words, n_rows, ks, key, lookup, n_keys, k_out, flags, out, cap, count, offs, scratch, scratch_bytes, None)


BIG = SEG * ((1 << 40) // SEG)  # the largest multiple of 992 below 2^40

REFUSED = (
    # (1) widths and flags
    dict(ks=0), dict(ks=33), dict(ks=1 << 32), dict(k_out=0), dict(k_out=33), dict(k_out=1 << 32), dict(flags=4), dict(flags=4 | EXISTS), dict(flags=1 << 31),
    # (2) pointers and alignment
    dict(key=None), dict(key=KEY + 4), dict(scratch=None), dict(scratch=SCRATCH + 128), dict(scratch=SCRATCH + 8), dict(out=None), dict(out=OUT + 2),
    dict(count=None), dict(count=COUNT + 4), dict(offs=None), dict(offs=OFFS + 4),
    # (3) the map
    dict(lookup=None), dict(lookup=MAP + 2), dict(lookup=MAP + 1), dict(n_keys=0), dict(n_keys=(1 << 32) + 1),
    # (4) the sizes
    dict(n_words=0, n_rows=0), dict(n_words=SEG + 1), dict(n_words=31, n_rows=0), dict(n_words=BIG + SEG, n_rows=0), dict(n_words=1 << 40, n_rows=0),
    dict(n_words=BIG // 16 + SEG - (BIG // 16) % SEG, k_out=17, n_rows=0), dict(n_rows=SEG * 32 + 1), dict(n_rows=1 << 62),
)

LEGAL = (
    dict(), dict(flags=EXISTS), dict(flags=PARTIAL), dict(flags=EXISTS | PARTIAL), dict(ks=1), dict(ks=32, k_out=32), dict(k_out=1),
    dict(lookup=MAP + 4, n_keys=1), dict(n_keys=1 << 32), dict(n_rows=0), dict(n_rows=SEG * 32 - 1), dict(cap=0), dict(n_words=3 * SEG, n_rows=3 * SEG * 32),
    dict(n_words=BIG, k_out=1, n_rows=0),
)


def test_host_visible_refusals(lib):
    for kw in REFUSED:
        assert _call(lib, scratch_bytes=1 << 62, **kw) == WAH_ERR_ARG, kw
        assert lib.wah_last_error(), kw
        # the argument checks come first: a bad argument AND too small a scratch is a bad argument
        assert _call(lib, scratch_bytes=0, **kw) == WAH_ERR_ARG, kw
    assert lib.wah_bsi_map_status(None, SEG, 17, 0, None) == WAH_ERR_ARG


def test_each_legal_extreme_reaches_the_scratch_check(lib):
    for kw in LEGAL:
        need = lib.wah_bsi_map_scratch_bytes(kw.get("n_words", SEG), kw.get("k_out", 17), kw.get("flags", 0))
        assert _call(lib, scratch_bytes=need - 1, **kw) == WAH_ERR_WORKSPACE, kw
        assert _call(lib, scratch_bytes=0, **kw) == WAH_ERR_WORKSPACE, kw


def test_the_stated_order_of_the_refusals(lib):
    """include/wah.h: (1) widths and flags, (2) key table, scratch and output, (3) the map and n_keys, (4) the sizes, then the
    scratch's size.  The text of wah_last_error names the first one that fails."""
    def text(**kw):
        kw.setdefault("scratch_bytes", 1 << 62)
        assert _call(lib, **kw) in (WAH_ERR_ARG, WAH_ERR_WORKSPACE)
        return lib.wah_last_error().decode()

    first, second, third, fourth, size = text(ks=0), text(key=None), text(lookup=MAP + 2), text(n_words=SEG + 1), text(scratch_bytes=0)
    assert len({first, second, third, fourth, size}) == 5
    assert text(ks=0, key=None, lookup=MAP + 2, n_words=SEG + 1, scratch_bytes=0) == first
    assert text(flags=4, scratch=None) == first
    assert text(k_out=33, n_keys=0) == first
    assert text(key=None, lookup=MAP + 2, n_words=SEG + 1, scratch_bytes=0) == second
    assert text(scratch=SCRATCH + 8, n_keys=(1 << 32) + 1) == second
    assert text(offs=None, n_rows=1 << 62) == second
    assert text(lookup=MAP + 2, n_words=SEG + 1, scratch_bytes=0) == third
    assert text(lookup=None, n_rows=1 << 62) == third
    assert text(n_keys=0, n_words=1 << 40) == third
    assert text(n_words=SEG + 1, scratch_bytes=0) == fourth
    assert text(n_rows=SEG * 32 + 1, scratch_bytes=0) == fourth
    assert _call(lib, scratch_bytes=0) == WAH_ERR_WORKSPACE
