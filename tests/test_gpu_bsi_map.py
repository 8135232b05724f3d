"""GPU tests of wah_bsi_map_indexed_device: a bit-sliced key pushed through a lookup table, the looked-up value as a new bit-sliced
attribute in one call (include/wah.h), and its front ends in api.py and columns.py.  Everything is exact: the result's words, their
count and its whole segment index against the CPU oracle's compress() and an indexed compress of the slice matrix that numpy builds
FROM THE VALUES and the lookup (tests/_map.py); tests/test_map_reference.py proves the model against a restatement of the kernel's
steps and that every named case can fail.  Outputs are poisoned and have a guard word behind them.

The named cases run at 992, 2 * 992 and 3 * 992 words -- one, two and three segments: the segment number in the address of a matrix
row, the half block's 32 words in front of the next segment's first -- over the widths, row counts, key counts and modes of
tests/_map.py; 513 segments are one more than the grid has workgroups; the bitmap of more than 2^32 rows comes from tests/_long.py."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _foreign as fg, _long as lg, _map as mp
from tests.test_gpu_bsi_arith import Expected, _dev, _dev_values, _host, _same

pytestmark = pytest.mark.gpu

WAH_ERR_STREAM = -6
SEG = 992
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


@pytest.fixture(scope="module")
def expected(wah):
    return Expected(wah)


@pytest.fixture(scope="module")
def cases():
    return mp.named_cases()


def _dev_lookup(lookup):
    import torch

    return torch.from_numpy(np.ascontiguousarray(lookup, dtype=np.uint32).view(np.int32)).cuda()


def _dev_bool(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _key(wah, case):
    """The key as the index holds it: bsi_from_values over all 32 n rows (a row outside the existence bitmap is stored as 0)."""
    return wah.columns.bsi_from_values(wah, _dev_values(case["keys"]), case["ks"], n_words_per_column=case["n"], exists=_dev_bool(case["exists"]))


def _rows_out(case):
    return case["k_out"] + (1 if mp.has_exists_row(case) else 0)


def _call(wah, case, table, check=True, scratch=None):
    """The call into poisoned outputs with a guard behind each; returns what bsi_map_device returns."""
    import torch

    n, rows_out = case["n"], _rows_out(case)
    cap, entries = wah.max_compressed_words(rows_out * n), rows_out * (n // SEG) + 1
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    offs = torch.full((entries + 1,), -1, dtype=torch.int64, device="cuda")
    got = wah.bsi_map_device(table, n, case["n_rows"], _dev_lookup(case["lookup"]), case["k_out"], exists=case["exists"] is not None,
                             partial=case["partial"], scratch=scratch, out=buf[:cap], out_offsets=offs[:entries], check=check)
    torch.cuda.synchronize()
    assert int(buf[cap].item()) == GUARD and int(offs[entries].item()) == -1, "guard"
    return got


def _run(wah, oracle, expected, case, what, table=None):
    want, refused = mp.expected(case)
    assert not refused, what
    key = None
    if table is None:
        key = _key(wah, case)  # (kept until the call is done: a table holds raw pointers)
        table = wah.columns._slice_table(key)
    got, offs = _call(wah, case, table)
    del key
    _same(expected, oracle, got, offs, want, what)


# ---- 1: the named cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mp.named_cases()))
def test_named_case_vs_value_model(wah, oracle, expected, cases, name):
    _run(wah, oracle, expected, cases[name], name)


def test_one_segment_more_than_the_grid(wah, oracle, expected):
    """513 segments, a 1-slice key and a 2-bit result: the first workgroup takes a second segment."""
    n = (mp.GRID_ITEMS + 1) * SEG
    rng = np.random.default_rng(513)
    keys = (rng.random(32 * n) < 0.5).astype(np.uint64)
    keys[-mp.SEG_BITS:] = np.where(rng.random(mp.SEG_BITS) < 0.9, 1, 0)  # the last segment differs from the first
    case = dict(n=n, n_rows=32 * n - 3, ks=1, keys=keys, exists=None, lookup=np.array([2, 1], np.uint32), k_out=2, partial=False)
    _run(wah, oracle, expected, case, "513 segments")


def test_a_bitmap_of_more_than_2_32_rows(wah, oracle):
    """135 400 segments (4.298e9 rows), a 1-slice key that is 1, then 0 in its constant segments and random in the named live ones,
    the lookup [1, 0] and a 1-bit result without an existence row: NOT key in front of n_rows = 2^32 + 5, zeros behind -- row
    numbers, word offsets of the matrix and the selection clip pass 2^32.  Expected from tests/_long.py's run model."""
    import torch

    a = lg.A_SEGMENTS
    n = a * SEG
    n_rows = 2**32 + 5
    assert n_rows // lg.SEG_BITS in lg.A_NAMED and n_rows < 32 * n
    key = lg.column(a, lg.A_NAMED, 1, 77, ([0, 70_000], [1, 0]))[0]
    want = lg.bitop("and", [lg.invert(key), lg.below(a, n_rows)])
    assert 2**30 < want.count() < lg.invert(key).count()  # (the ones of the key's second run in front of n_rows; the clip matters)
    want_stream, want_index = want.expected_stream_index(oracle)
    stream, index = key.stream_index(oracle)
    d_stream, d_index = _dev(stream), torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).cuda()
    table = wah.bitop_operand_table([(d_stream, d_index)])
    cap = want_stream.size + 64
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    offs = torch.full((a + 2,), -1, dtype=torch.int64, device="cuda")
    got, got_offs = wah.bsi_map_device(table, n, n_rows, _dev_lookup(np.array([1, 0], np.uint32)), 1, out=buf[:cap], out_offsets=offs[: a + 1])
    assert int(buf[cap].item()) == GUARD and int(offs[a + 1].item()) == -1
    assert got.numel() == want_stream.size
    assert torch.equal(got_offs, torch.from_numpy(want_index).cuda())
    assert torch.equal(got, _dev(want_stream))


# ---- 2: foreign streams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", (0, 5))
def test_the_key_in_every_reencoding(wah, oracle, expected, first):
    """The key's slices and its existence row written in every way of tests/_foreign.py that compress() never emits, the ways rotating
    over the thirteen table rows: the result is the canonical one."""
    n, ks, k_out = 2 * SEG, 12, 17
    rng = np.random.default_rng(12)
    rows = 32 * n
    keys = _bsi.make_values("clustered", rng, rows, ks)
    exists = np.repeat(rng.random(rows // 992 + 1) < 0.8, 992)[:rows]  # runs: the existence row has fills too
    lookup = mp.make_lookup(rng, 1 << ks, k_out, "nulls")
    case = dict(n=n, n_rows=rows - 100, ks=ks, keys=keys, exists=exists, lookup=lookup, k_out=k_out, partial=True)
    matrix = _bsi.build_slices(keys, ks, exists, zero_missing=True)
    foreign = fg.rows_foreign(matrix, n, np.random.default_rng(3), first=first)
    assert {way for way, _ in foreign} == set(fg.WAYS[1:]) and len(foreign) == ks + 1
    operands = []
    for way, stream in foreign:
        assert np.array_equal(oracle.decompress(stream)[:n], matrix[len(operands)]), way
        d = _dev(stream)
        offs, _ = wah.build_index_device(d)
        operands.append((d, offs))
    _run(wah, oracle, expected, case, ("foreign", first), table=wah.bitop_operand_table(operands))


# ---- 3: what only the device sees -----------------------------------------------------------------------------------------------------
def _status(wah, case, table=None):
    """Enqueue only; the verdict comes from the status call."""
    import torch

    flags = (wah.BSI_EXISTS if case["exists"] is not None else 0) | (wah.MAP_PARTIAL if case["partial"] else 0)
    sc = torch.empty(int(wah.lib().wah_bsi_map_scratch_bytes(case["n"], case["k_out"], flags)), dtype=torch.uint8, device="cuda")
    key = None
    if table is None:
        key = _key(wah, case)  # (kept until the status is read: a table holds raw pointers)
        table = wah.columns._slice_table(key)
    _call(wah, case, table, check=False, scratch=sc)
    rc = int(wah.lib().wah_bsi_map_status(sc.data_ptr(), case["n"], case["k_out"], flags, None))
    del key
    return rc


def test_refusals_come_from_the_status_call(wah, oracle, expected):
    refused, fine = mp.refused_cases()
    for name, case in refused.items():
        assert _status(wah, case) == WAH_ERR_STREAM, name
    with pytest.raises(wah.WahError):
        case = refused["a NULL entry"]
        key = _key(wah, case)
        _call(wah, case, wah.columns._slice_table(key))
    for name, case in fine.items():
        assert _status(wah, case) == 0, name
        _run(wah, oracle, expected, case, name)


def test_a_bad_key_operand_is_refused(wah):
    case = mp.make_case(2 * SEG, 12, 17, None, True, True, seed=9)
    key = _key(wah, case)
    table = wah.columns._slice_table(key)
    assert _status(wah, case, table) == 0
    for r, col in ((0, 2), (5, 2), (11, 0), (12, 2), (12, 0)):  # a slice or the existence row without an index, or without a stream
        bad = table.clone()
        bad[r, col] = 0
        assert _status(wah, case, bad) == WAH_ERR_STREAM, (r, col)
    # a fill of the existence row one group shorter: the segment's groups do not add up
    exists = np.repeat(np.random.default_rng(2).random(32 * case["n"] // 992) < 0.7, 992)
    case = dict(case, exists=exists)
    key = _key(wah, case)
    table = wah.columns._slice_table(key)
    assert _status(wah, case, table) == 0
    segs = case["n"] // SEG
    first, last = int(key[1][12 * segs].item()), int(key[1][13 * segs].item())
    words = _host(key[0]).copy()
    fills = first + np.flatnonzero((words[first:last] >> 31 == 1) & ((words[first:last] & 0x3FFFFFFF) >= 2))
    assert fills.size
    words[int(fills[0])] -= 1
    broken = (_dev(words), key[1], *key[2:])
    assert _status(wah, case, wah.columns._slice_table(broken)) == WAH_ERR_STREAM


def test_front_end_refuses_bad_arguments(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    lookup = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(wah.WahError):
        wah.bsi_map_device([(stream, offs)] * 33, SEG, 0, lookup, 8)
    with pytest.raises(wah.WahError):
        wah.bsi_map_device([(stream, offs)] * 3, SEG, 0, lookup, 33)
    with pytest.raises(wah.WahError):
        wah.bsi_map_device([(stream, offs)] * 3, SEG + 1, 0, lookup, 8)
    with pytest.raises(wah.WahError):
        wah.bsi_map_device([(stream, offs)] * 3, SEG, 0, lookup[:0], 8)
    wide = (stream, offs, SEG, 33, False)
    with pytest.raises(ValueError):
        wah.columns.map_column(wah, wide, 0, lookup)
    with pytest.raises(ValueError):
        wah.columns.map_column(wah, (stream, offs, SEG, 8, False), 0, lookup, n_bits=33)
    with pytest.raises(ValueError):
        wah.columns.apply_column(wah, (stream, offs, SEG, 25, False), 0, lambda x: x)


# ---- 4: the front ends ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star(wah):
    """A fact table of 2 * 992 * 32 - 50 rows with a 12-bit foreign key (an existence bitmap; some keys behind the dimension's 3000
    rows), a 9-bit quantity and a 7-bit tier, and a dimension with a 7-bit price and a filter."""
    n, fk_bits = 2 * SEG, 12
    rows = 32 * n - 50
    rng = np.random.default_rng(2024)
    fk = np.where(rng.random(rows) < 0.95, rng.integers(0, 3000, rows), rng.integers(3000, 4096, rows)).astype(np.uint64)
    fk_exists = rng.random(rows) < 0.9
    qty, tier = _bsi.uniform_values(rng, rows, 9), _bsi.uniform_values(rng, rows, 7)
    price = rng.integers(0, 128, 3000).astype(np.int64)
    keep = rng.random(3000) < 0.8

    def build(values, bits, exists=None):
        return wah.columns.bsi_from_values(wah, _dev_values(values), bits, n_words_per_column=n, exists=_dev_bool(exists))

    return dict(n=n, rows=rows, fk=fk, fk_exists=fk_exists, qty=qty, tier=tier, price=price, keep=keep, d_fk=build(fk, fk_bits, fk_exists),
                d_qty=build(qty, 9), d_tier=build(tier, 7))


def _joined(s):
    """numpy: (d.price of every fact row, whether the row has one)."""
    inside = s["fk"] < 3000
    at = np.minimum(s["fk"], 2999).astype(np.int64)
    has = s["fk_exists"] & inside & s["keep"][at]
    return np.where(has, s["price"][at], 0).astype(np.uint64), has


def _padded(a, n, dtype):
    out = np.zeros(32 * n, dtype)
    out[: a.size] = a
    return out


def test_join_column_and_what_takes_its_result(wah, oracle, expected, star):
    import torch

    s = star
    n, rows = s["n"], s["rows"]
    want, has = _joined(s)
    joined = wah.columns.join_column(wah, s["d_fk"], rows, torch.from_numpy(s["price"]).cuda(), torch.from_numpy(s["keep"]).cuda())
    assert joined[2:] == (n, 7, True) and has.any() and not has.all()
    _same(expected, oracle, joined[0], joined[1], _bsi.build_slices(_padded(want, n, np.uint64), 7, _padded(has, n, bool)), "join_column")
    values, have = wah.columns.values_of_column(wah, joined, 0, rows)
    assert np.array_equal(have.cpu().numpy(), has) and np.array_equal(values.cpu().numpy().view(np.uint64), want)
    # WHERE d.price > f.tier
    greater, _ = wah.columns.compare_columns(wah, joined, ">", s["d_tier"])
    bitmap = _padded((want > s["tier"]) & has, n, bool)
    assert bitmap.any() and np.array_equal(_host(greater), oracle.compress(_bsi.pack_bits(bitmap)))
    # SUM(f.qty * d.price) row by row
    product = wah.columns.multiply_columns(wah, s["d_qty"], joined)
    values, have = wah.columns.values_of_column(wah, product, 0, rows)
    assert np.array_equal(have.cpu().numpy(), has) and np.array_equal(values.cpu().numpy().view(np.uint64), np.where(has, s["qty"] * want, 0))
    # GROUP BY d.price
    grouped = wah.columns.group_by_column(wah, joined, rows)
    assert np.array_equal(grouped["rows"].cpu().numpy(), np.bincount(want[has].astype(np.int64), minlength=128))


def test_apply_column(wah, oracle, expected, star):
    s = star
    n, rows = s["n"], s["rows"]
    tens = wah.columns.apply_column(wah, s["d_qty"], rows, lambda x: x // 10)
    assert tens[2:] == (n, 6, True)  # 511 // 10 = 51: six bits
    values, have = wah.columns.values_of_column(wah, tens, 0, rows)
    assert bool(have.all()) and np.array_equal(values.cpu().numpy().view(np.uint64), s["qty"] // np.uint64(10))
    values, have = wah.columns.values_of_column(wah, tens, rows, 50)
    assert not bool(have.any()) and not bool(values.any())  # rows behind n_rows have no value
    # a CASE with a NULL branch over a key with an existence bitmap
    banded = wah.columns.apply_column(wah, s["d_fk"], rows, lambda x: (x % 7 != 0) * (x >> 5) - (x % 7 == 0) * 1)
    want_has = s["fk_exists"] & (s["fk"] % np.uint64(7) != 0)
    assert banded[2:] == (n, 7, True) and not want_has.all()
    values, have = wah.columns.values_of_column(wah, banded, 0, rows)
    assert np.array_equal(have.cpu().numpy(), want_has)
    assert np.array_equal(values.cpu().numpy().view(np.uint64), np.where(want_has, s["fk"] >> np.uint64(5), 0))
    _same(expected, oracle, banded[0], banded[1],
          _bsi.build_slices(_padded(np.where(want_has, s["fk"] >> np.uint64(5), 0).astype(np.uint64), n, np.uint64), 7, _padded(want_has, n, bool)), "apply_column")


# ---- 5: a chain with nothing read back, and the same as one captured graph -----------------------------------------------------------------
def _chain_want(s, lookup, lo, hi):
    v = lookup[s["qty"].astype(np.int64)]
    return int(((v >= lo) & (v <= hi)).sum())


def test_chain_without_a_read_back_and_its_graph_replay(wah, star):
    """bsi_from_values -> map_column -> range_column -> count_columns, every call with check=False into tensors made beforehand: the
    statuses are read once at the end.  Then the three calls as ONE captured graph, replayed after the lookup was rewritten in place
    (capture as the arithmetic call's test: side stream, warm-up outside, check=False; one chain of launches, no parallel branches)."""
    import torch

    s = star
    n, rows, k_out, lo, hi = s["n"], s["rows"], 10, 100, 700
    rng = np.random.default_rng(31)
    lookups = [rng.integers(0, 1 << k_out, 512).astype(np.uint32) for _ in range(3)]
    lookup = _dev_lookup(lookups[0])
    lib = wah.lib()
    sc_map = torch.empty(int(lib.wah_bsi_map_scratch_bytes(n, k_out, 0)), dtype=torch.uint8, device="cuda")
    sc_range = torch.empty(int(lib.wah_bsi_range_scratch_bytes(n, k_out)), dtype=torch.uint8, device="cuda")
    sc_count = torch.empty(int(lib.wah_select_scratch_bytes(n, 1)), dtype=torch.uint8, device="cuda")
    out_map = torch.empty(wah.max_compressed_words(k_out * n), dtype=torch.int32, device="cuda")
    offs_map = torch.zeros(k_out * (n // SEG) + 1, dtype=torch.int64, device="cuda")
    out_range = torch.empty(wah.max_compressed_words(n), dtype=torch.int32, device="cuda")
    offs_range = torch.zeros((wah.max_compressed_words(n) + 1023) // 1024 + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    key = wah.columns.bsi_from_values(wah, _dev_values(s["qty"]), 9, n_words_per_column=n, check=False)

    def statuses():
        return (int(lib.wah_bsi_map_status(sc_map.data_ptr(), n, k_out, 0, None)), int(lib.wah_bsi_range_status(sc_range.data_ptr(), n, k_out, None)),
                int(lib.wah_select_status(sc_count.data_ptr(), None)))

    # the front ends (they build their tables on the device); this is the warm-up outside the capture, too
    mapped = wah.columns.map_column(wah, key, rows, lookup, n_bits=k_out, scratch=sc_map, out=out_map, out_offsets=offs_map, check=False)
    assert mapped[2:] == (n, k_out, False) and mapped[0].data_ptr() == out_map.data_ptr()
    hit, _, hit_offs = wah.columns.range_column(wah, mapped, lo, hi, scratch=sc_range, out=out_range, out_offsets=offs_range, check=False)
    wah.columns.count_columns(wah, hit, hit_offs, n, [0], scratch=sc_count, counts=counts, check=False)
    assert statuses() == (0, 0, 0)
    assert int(counts.item()) == _chain_want(s, lookups[0], lo, hi) > 0
    # the same three calls over tables made beforehand: inside a capture nothing is copied from the host
    key_table = wah.columns._slice_table(key)
    range_table = wah.columns.column_operand_table(out_map, offs_map, n, list(range(k_out)))
    count_table = wah.bitop_operand_table([(out_range, offs_range)])
    bounds = wah.bsi_bounds(lo, hi, torch.device("cuda:0"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            wah.bsi_map_device(key_table, n, rows, lookup, k_out, scratch=sc_map, out=out_map, out_offsets=offs_map, check=False)
            wah.bsi_range_device(range_table, bounds, n, scratch=sc_range, out=out_range, out_offsets=offs_range, check=False)
            wah.count_device(count_table, n, scratch=sc_count, counts=counts, check=False)
    seen = set()
    for other in lookups[1:] + lookups[:1]:
        lookup.copy_(_dev_lookup(other))  # rewritten in place: the captured calls hold its address
        counts.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert statuses() == (0, 0, 0)
        assert int(counts.item()) == _chain_want(s, other, lo, hi)
        seen.add(int(counts.item()))
    assert len(seen) == 3  # different answers from one captured chain
