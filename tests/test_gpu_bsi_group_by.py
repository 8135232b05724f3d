"""GPU tests of wah_bsi_group_by_indexed_device: COUNT and SUM per value of a bit-sliced key in one call (include/wah.h), and its
front ends in api.py and columns.py.  Everything is integer-exact against the numpy model that answers FROM THE VALUES
(tests/_groupby.py: expected).  tests/test_groupby_reference.py proves that model against the restatement of the kernel's steps
on the CPU, and that the named cases can fail.

Shapes are the smallest at which the kernel can still go wrong: 1, 31, 992 and 992 * 3 + 5 words (a ragged last segment, more than
one item), key widths 1 .. 32 and value widths 0 .. 32, bucket counts on both sides of the switch between the LDS and the global
route, one item more than the capped grid, and one bitmap of more than 2^32 rows."""
import importlib

import numpy as np
import pytest

from tests import _bsi, _foreign as fg, _groupby as gb, _long as lg

pytestmark = pytest.mark.gpu

WAH_ERR_STREAM = -6
SEG = 992
POISON = 0x5A5A5A5A5A5A5A5A
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


@pytest.fixture(scope="module")
def cases():
    return gb.named_cases()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    """An int64 device tensor as Python ints of its bit patterns."""
    return [int(v) & M64 for v in t.reshape(-1).tolist()]


class Streams:
    """One indexed compressor of n_words, reused for every row of the tables."""

    made = {}

    def __init__(self, wah, n_words):
        self.comp = wah.DeviceCompressor(n_words, indexed=True)

    @classmethod
    def get(cls, wah, n_words):
        if n_words not in cls.made:
            cls.made[n_words] = cls(wah, n_words)
        return cls.made[n_words]

    def of(self, words):
        self.comp.run(_dev(words))
        return self.comp.result().clone(), self.comp.seg_offsets.clone()


def _tables(wah, case):
    """The case's three tables on the device (and the streams they point into, which have to stay alive)."""
    st = Streams.get(wah, case["n"])
    key = [st.of(row) for row in _bsi.build_slices(case["keys"], case["ks"], case["exists"])]
    val = [st.of(row) for row in _bsi.build_slices(case["vals"], case["vs"])] if case["vs"] else None
    fil = [st.of(_bsi.pack_bits(f)) for f in case["filters"]]
    bt = wah.bitop_operand_table
    return dict(alive=(key, val, fil), key=bt(key), val=bt(val) if val else None, filters=bt(fil) if fil else None)


def _run(wah, case, tables, check=True, scratch=None):
    """One call with poisoned outputs and a guard word behind each; returns (counts, sums) as Python ints, the sums whole."""
    import torch

    nb, pre = case["n_buckets"], case["prefill"]
    counts = torch.full((nb + 2,), POISON, dtype=torch.int64, device="cuda")
    sums = torch.full((2 * (nb + 1) + 1,), POISON, dtype=torch.int64, device="cuda") if case["vs"] else None
    if pre is not None:
        counts[: nb + 1] = _dev64(np.array(pre[0], dtype=np.uint64))
        if sums is not None:
            sums[: 2 * (nb + 1)] = _dev64(np.array([[s & M64, s >> 64] for s in pre[1]], dtype=np.uint64).reshape(-1))
    lookup = None if case["lookup"] is None else _dev(case["lookup"])
    got_counts, got_sums = wah.bsi_group_by_device(
        tables["key"], case["n"], case["n_rows"], nb, value_table=tables["val"], filters=tables["filters"], exists=case["exists"] is not None,
        lookup=lookup, accumulate=pre is not None, counts=counts[: nb + 1], sums=None if sums is None else sums[: 2 * (nb + 1)].view(nb + 1, 2),
        check=check, scratch=scratch)
    if not check:
        return None
    assert int(counts[-1].item()) == POISON and (sums is None or int(sums[-1].item()) == POISON), "the guard words"
    assert got_counts.data_ptr() == counts.data_ptr()
    whole = None
    if got_sums is not None:
        words = _u64(got_sums)
        whole = [words[2 * i] + (words[2 * i + 1] << 64) for i in range(nb + 1)]
    return _u64(got_counts), whole


def _check(wah, case, what, tables=None):
    got = _run(wah, case, tables or _tables(wah, case))
    want = gb.expected(case)
    assert got[0] == want[0], (what, "counts")
    assert got[1] == want[1], (what, "sums")


# ---- 1: the named cases: sizes, widths, filters, n_rows, bucket counts, key patterns, maps, the carry -------------------------------
GROUPS = ("widths", "size 1:", "size 31:", "size 992:", f"size {gb.BIG}:", "n_rows", "buckets", "pattern", "map", "carry")


@pytest.mark.parametrize("group", GROUPS)
def test_named_cases(wah, cases, group):
    mine = {name: case for name, case in cases.items() if name.startswith(group)}
    assert mine and sum(len([n for n in cases if n.startswith(g)]) for g in GROUPS) == len(cases)
    for name, case in mine.items():
        _check(wah, case, name)


def test_empty_bitmap(wah):
    """n_words == 0: all zeros, or under ACCUMULATE nothing added."""
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    for vs in (0, 5):
        for nb in (3, gb.LDS_BUCKETS):
            val = [(stream, offs)] * vs if vs else None
            counts = torch.full((nb + 1,), 9, dtype=torch.int64, device="cuda")
            sums = torch.full((nb + 1, 2), 9, dtype=torch.int64, device="cuda") if vs else None
            wah.bsi_group_by_device([(stream, offs)] * 4, 0, 0, nb, value_table=val, exists=True, accumulate=True, counts=counts, sums=sums)
            assert bool((counts == 9).all()) and (sums is None or bool((sums == 9).all()))
            wah.bsi_group_by_device([(stream, offs)] * 4, 0, 0, nb, value_table=val, exists=True, counts=counts, sums=sums)
            assert bool((counts == 0).all()) and (sums is None or bool((sums == 0).all()))


# ---- 2: ACCUMULATE: two calls equal one call over both ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [256, 1 << 12])
def test_two_accumulated_calls_equal_one(wah, nb):
    """A table's rows split by a bitmap and its complement: the two partitions land in one histogram, which is the unfiltered one."""
    case = gb.make_case(SEG + 5, 12, 32, 0, True, n_buckets=nb, seed=21)
    tables = _tables(wah, case)
    whole = _run(wah, case, tables)
    assert whole == gb.expected(case)
    part = np.random.default_rng(22).random(32 * case["n"]) < 0.4
    st = Streams.get(wah, case["n"])
    halves = [st.of(_bsi.pack_bits(p)) for p in (part, ~part)]
    counts, sums = wah.bsi_group_by_device(tables["key"], case["n"], case["n_rows"], nb, value_table=tables["val"], filters=[halves[0]], exists=True)
    first = _u64(counts)
    wah.bsi_group_by_device(tables["key"], case["n"], case["n_rows"], nb, value_table=tables["val"], filters=[halves[1]], exists=True, accumulate=True,
                            counts=counts, sums=sums)
    words = _u64(sums)
    assert _u64(counts) == whole[0] and first != whole[0]
    assert [words[2 * i] + (words[2 * i + 1] << 64) for i in range(nb + 1)] == whole[1]


# ---- 3: one item more than the capped grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vs", [0, 1])
def test_one_item_more_than_the_grid(wah, vs):
    """GRID workgroups stride over the items: count only, GRID * 992 + 1 words are GRID + 1 segments, and workgroup 0 takes the ragged
    last segment as its second item; with a value attribute (two items a segment) GRID / 2 * 992 + 1 words are GRID + 2 items.  A
    workgroup's second item must not see the first one's rows, selection or LDS buckets."""
    n = (gb.GRID_ITEMS // (2 if vs else 1)) * SEG + 1
    rng = np.random.default_rng(31 + vs)
    rows = 32 * n
    case = dict(n=n, n_rows=rows - 3, ks=2, vs=vs, keys=rng.integers(0, 4, rows, dtype=np.uint64), exists=None,
                vals=rng.integers(0, 2, rows, dtype=np.uint64) if vs else None, filters=[], lookup=None, n_buckets=3, prefill=None)
    case["keys"][-32:] = 3  # the ragged last segment holds bucket "other" only
    want = gb.expected(case)
    assert want[0][3] >= 29 and min(want[0]) > 0
    _check(wah, case, ("grid", vs))
    _check(wah, dict(case, n_buckets=gb.LDS_BUCKETS), ("grid, global route", vs))


# ---- 4: more than 2^32 rows ------------------------------------------------------------------------------------------------------------
def test_more_than_2_32_rows(wah, oracle):
    """A 2-slice key of 135 400 segments (rows 2^31 and 2^32 exist) whose constant segments hold 2 and whose few live segments hold
    random keys: bucket 2 counts more than 2^32 rows; n_rows above 2^32 cuts the tail; the key's low slice as the value attribute."""
    import torch

    segs = lg.A_SEGMENTS
    n = segs * lg.SEG_WORDS
    column = lg.column(segs, lg.A_NAMED, 2, 77, 2)
    stream, index = lg.expected_streams(oracle, column)
    d_stream, d_index = _dev(stream), _dev64(index)
    key = wah.columns.column_operand_table(d_stream, d_index, n, [0, 1])
    val = wah.columns.column_operand_table(d_stream, d_index, n, [1])
    scratch = torch.empty(int(wah.lib().wah_bsi_group_by_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
    for n_rows in (32 * n, 2**32 + 12345):
        assert n_rows > 2**32
        by_value = lg.value_counts(column, None if n_rows == 32 * n else lg.below(segs, n_rows))
        if n_rows == 32 * n:
            assert sum(by_value.values()) == segs * lg.SEG_BITS  # (32 n rows are exactly the segments' rows)
        want = [by_value.get(v, 0) for v in range(4)]
        assert sum(want) == n_rows and min(want) > 0 and (want[2] > 2**32 or n_rows < 32 * n)
        for nb in (4, 3, gb.LDS_BUCKETS):
            counts, sums = wah.bsi_group_by_device(key, n, n_rows, nb, value_table=val, scratch=scratch)
            folded = want[:nb] + [0] * (nb - 4) + [sum(want[nb:])]
            assert _u64(counts) == folded, (n_rows, nb)
            words = _u64(sums)
            low = [c * (b & 1) for b, c in enumerate(want)]
            assert words[0::2] == low[:nb] + [0] * (nb - 4) + [sum(low[nb:])] and not any(words[1::2]), (n_rows, nb)
        counts, sums = wah.bsi_group_by_device(key, n, n_rows, 4, scratch=scratch)
        assert _u64(counts) == want + [0] and sums is None


# ---- 5: foreign re-encodings of every table's rows ----------------------------------------------------------------------------------------
def test_foreign_streams(wah, oracle):
    """Every way of tests/_foreign.py in every row in turn -- key slices, the existence row, value slices, a filter -- indexed with
    wah_build_index_device."""
    n, ks, vs = SEG * 2 + 30, 3, 2
    rng = np.random.default_rng(61)
    case = gb.make_case(n, ks, vs, 1, True, n_buckets=6, seed=61)
    case["keys"] = _bsi.make_values("clustered", rng, 32 * n, ks)
    case["vals"] = _bsi.make_values("clustered", rng, 32 * n, vs)
    case["exists"][-4000:] = True  # (the one-fill pad ways need a bitmap that ends in ones)
    matrix = np.concatenate([_bsi.build_slices(case["keys"], ks, case["exists"]), _bsi.build_slices(case["vals"], vs), [_bsi.pack_bits(case["filters"][0])]])
    ways = fg.ways_for(n)
    assert fg.pad_bits(n) and len(ways) == len(fg.WAYS) + len(fg.PAD_WAYS) and matrix.shape[0] == ks + 1 + vs + 1
    want = gb.expected(case)
    assert sum(want[0]) > 0 and sum(want[1]) > 0
    seen = set()
    for first in range(len(ways)):
        made = fg.rows_foreign(matrix, n, np.random.default_rng(first), ways, first)
        seen |= {way for way, _ in made}
        pairs = []
        for way, st in made:
            assert np.array_equal(oracle.decompress(st)[:n], matrix[len(pairs)]), way
            d = _dev(st)
            offs, groups = wah.build_index_device(d)
            assert groups == fg.n_groups(n)
            pairs.append((d, offs))
        bt = wah.bitop_operand_table
        tables = dict(key=bt(pairs[: ks + 1]), val=bt(pairs[ks + 1: ks + 1 + vs]), filters=bt(pairs[ks + 1 + vs:]))
        for nb in (6, gb.LDS_BUCKETS):
            c = dict(case, n_buckets=nb)
            assert _run(wah, c, tables) == gb.expected(c), (first, nb)
    assert seen >= set(fg.WAYS) | {"pad: literal"}


# ---- 6: refusals only the device sees ------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_status_call(wah):
    import torch

    n, ks, vs = SEG * 2, 12, 17
    rng = np.random.default_rng(41)
    case = gb.make_case(n, ks, vs, 2, True, n_buckets=300, seed=41)
    case["keys"] = _bsi.make_values("clustered", rng, 32 * n, ks)  # fills in every slice
    tables = _tables(wah, case)
    key, val, fil = tables["alive"]
    sc = torch.empty(int(wah.lib().wah_bsi_group_by_scratch_bytes(n)), dtype=torch.uint8, device="cuda")

    def status(t, **kw):
        _run(wah, dict(case, **kw), t, check=False, scratch=sc)
        return int(wah.lib().wah_bsi_group_by_status(sc.data_ptr(), None))

    assert status(tables) == 0 and status(tables, n_buckets=1 << 12) == 0 and status(tables, n_rows=0) == 0
    # a broken stream: a fill one group short
    words = _host(key[3][0]).copy()
    fills = np.flatnonzero((words >> 31 == 1) & ((words & 0x3FFFFFFF) >= 2))
    assert fills.size, "a clustered slice has fills"
    words[int(fills[fills.size // 2])] -= 1
    broken = (_dev(words), key[3][1])
    bt = wah.bitop_operand_table
    for name, rows, at in (("key", key, 0), ("key", key, ks - 1), ("key", key, ks), ("val", val, 0), ("val", val, vs - 1), ("filters", fil, 0), ("filters", fil, 1)):
        bad = list(rows)
        bad[at] = broken
        bad_tables = dict(tables, **{name: bt(bad)})
        for kw in (dict(), dict(n_buckets=1 << 12), dict(n_rows=0)):  # the verdict depends neither on the route nor on which rows are selected
            assert status(bad_tables, **kw) == WAH_ERR_STREAM, (name, at, kw)
    with pytest.raises(wah.WahError):
        _run(wah, case, bad_tables)
    for name in ("key", "val", "filters"):
        t = tables[name].clone()
        t[-1, 2] = 0  # a row without an index
        assert status(dict(tables, **{name: t})) == WAH_ERR_STREAM, name
    assert status(tables) == 0


def test_front_end_refuses_bad_arguments(wah):
    import torch

    stream = torch.zeros(1, dtype=torch.int32, device="cuda")
    offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    row = [(stream, offs)]
    for bad in (lambda: wah.bsi_group_by_device(row * 33, 0, 0, 4),
                lambda: wah.bsi_group_by_device(row, 0, 0, 4, exists=True),
                lambda: wah.bsi_group_by_device(row, 0, 0, 0),
                lambda: wah.bsi_group_by_device(row, 0, 0, (1 << 30) + 1),
                lambda: wah.bsi_group_by_device(row, 0, 1, 4),
                lambda: wah.bsi_group_by_device(row, 0, 0, 4, value_table=row * 33),
                lambda: wah.bsi_group_by_device(row, 0, 0, 4, lookup=torch.zeros(4, dtype=torch.int64, device="cuda")),
                lambda: wah.bsi_group_by_device(row, 0, 0, 4, lookup=torch.zeros(0, dtype=torch.int32, device="cuda")),
                lambda: wah.bsi_group_by_device(row, 0, 0, 4, accumulate=True),
                lambda: wah.bsi_group_by_device(row, 0, 0, 4, sums=torch.zeros((5, 2), dtype=torch.int64, device="cuda")),
                lambda: wah.bsi_group_by_device(row, 0, 0, 4, counts=torch.zeros(4, dtype=torch.int64, device="cuda"))):
        with pytest.raises(wah.WahError):
            bad()


# ---- 7: the front ends --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star(wah):
    """A fact table of 2 * 31 744 - 100 rows with a 13-bit foreign key (NULLs: an existence bitmap) into a dimension table of 5000
    rows (keys beyond them dangle), a 40-bit attribute, a 20-bit attribute with NULLs and a filter attribute."""
    import torch

    n = SEG * 2
    n_rows = 32 * n - 100
    rng = np.random.default_rng(10)
    fk = rng.integers(0, 8192, n_rows).astype(np.uint64)
    fk_exists = rng.random(n_rows) < 0.9
    wide = rng.integers(0, 1 << 40, n_rows).astype(np.uint64)
    x = rng.integers(0, 1 << 20, n_rows).astype(np.uint64)
    x_exists = rng.random(n_rows) < 0.8
    flag = rng.integers(0, 100, n_rows).astype(np.uint64)
    dim_rows = 5000
    year = rng.integers(0, 7, dim_rows)
    keep = rng.random(dim_rows) < 0.6
    cuda = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    c = wah.columns
    return dict(n=n, n_rows=n_rows, fk=fk, fk_exists=fk_exists, wide=wide, x=x, x_exists=x_exists, flag=flag, year=year, keep=keep,
                bsi_fk=c.bsi_from_values(wah, _dev64(fk), 13, exists=cuda(fk_exists)),
                bsi_wide=c.bsi_from_values(wah, _dev64(wide), 40),
                bsi_x=c.bsi_from_values(wah, _dev64(x), 20, exists=cuda(x_exists)),
                bsi_flag=c.bsi_from_values(wah, _dev64(flag), 7))


def _grouped(buckets, n_buckets, weights=None):
    """Python ints per bucket, and those of the rows at or above n_buckets."""
    out = [0] * (n_buckets + 1)
    for b, w in zip(buckets.tolist(), [1] * buckets.size if weights is None else weights.tolist()):
        out[min(b, n_buckets)] += int(w)
    return out


def test_group_by_column_and_count_distinct(wah, star):
    """`SELECT fk, COUNT(*), SUM(wide), SUM(x), COUNT(x) WHERE flag <= 59 GROUP BY fk` -- a 40-slice attribute, one with NULLs --
    with the filter made by range_column and nothing of it read back in between; then COUNT(DISTINCT fk)."""
    c = wah.columns
    fk, have = star["fk"], star["fk_exists"]
    where = c.range_column(wah, star["bsi_flag"], 0, 59, check=False)[::2]  # (out, count, out_offsets) -> (out, out_offsets)
    sel = have & (star["flag"] <= 59)
    res = c.group_by_column(wah, star["bsi_fk"], star["n_rows"], attributes=[star["bsi_wide"], star["bsi_x"]], where=where)
    b = fk[sel].astype(np.int64)
    assert res["rows"].tolist() == _grouped(b, 8192)[:-1] and res["other"]["rows"] == 0 and sum(res["rows"].tolist()) == int(sel.sum()) > 0
    assert res["sums"][0].tolist() == _grouped(b, 8192, star["wide"][sel])[:-1] and max(res["sums"][0].tolist()) > 1 << 40
    xe = star["x_exists"][sel]
    assert res["sums"][1].tolist() == _grouped(b[xe], 8192, star["x"][sel][xe])[:-1]
    assert res["counts"][1].tolist() == _grouped(b[xe], 8192)[:-1] and res["counts"][0].tolist() == res["rows"].tolist()
    assert res["other"] == {"rows": 0, "sums": [0, 0], "counts": [0, 0]}
    # fewer buckets than keys: the rest is "other"; a lookup given as a list
    few = c.group_by_column(wah, star["bsi_fk"], star["n_rows"], attributes=[star["bsi_x"]], n_buckets=100)
    b = fk[have].astype(np.int64)
    want = _grouped(b, 100)
    assert few["rows"].tolist() == want[:-1] and few["other"]["rows"] == want[-1] > 0
    xe = star["x_exists"][have]
    assert few["other"]["sums"] == [_grouped(b[xe], 100, star["x"][have][xe])[-1]] and few["other"]["counts"] == [_grouped(b[xe], 100)[-1]]
    folded = c.group_by_column(wah, star["bsi_fk"], star["n_rows"], lookup=[3, 0, c.GROUP_BY_DROP, 3, 1])
    want = [int((have & (fk == 1)).sum()), int((have & (fk == 4)).sum()), 0, int((have & ((fk == 0) | (fk == 3))).sum())]
    assert folded["rows"].tolist() == want and folded["other"]["rows"] == int(have.sum()) - sum(want) and folded["sums"] == []
    assert int(c.count_distinct_where(wah, star["bsi_fk"], star["n_rows"]).item()) == np.unique(fk[have]).size
    assert int(c.count_distinct_where(wah, star["bsi_fk"], star["n_rows"], where=where).item()) == np.unique(fk[sel]).size
    with pytest.raises(ValueError):
        c.group_by_column(wah, star["bsi_wide"], star["n_rows"])


def test_group_by_joined(wah, star):
    """`SELECT d.year, COUNT(*), SUM(f.x) FROM f JOIN d ON f.fk = d.rowid WHERE d.keep GROUP BY d.year`."""
    import torch

    c = wah.columns
    fk, have, year, keep = star["fk"].astype(np.int64), star["fk_exists"], star["year"], star["keep"]
    for dim_keep in (None, keep):
        res = c.group_by_joined(wah, star["bsi_fk"], star["n_rows"], torch.from_numpy(year).cuda(),
                                dim_keep=None if dim_keep is None else torch.from_numpy(dim_keep).cuda(), attributes=[star["bsi_x"]])
        inside = have & (fk < year.size)
        if dim_keep is not None:
            inside &= dim_keep[np.minimum(fk, year.size - 1)]
        b = year[fk[inside]]
        assert res["rows"].tolist() == _grouped(b, 7)[:-1] and res["other"]["rows"] == int(have.sum() - inside.sum()) > 0
        xe = star["x_exists"][inside]
        assert res["sums"][0].tolist() == _grouped(b[xe], 7, star["x"][inside][xe])[:-1]
        assert res["counts"][0].tolist() == _grouped(b[xe], 7)[:-1]


# ---- 8: one captured graph replayed after the map was overwritten in place ----------------------------------------------------------------
def test_graph_replay_answers_the_new_map(wah, star):
    import torch

    n, n_rows, nb = star["n"], star["n_rows"], 16
    fk, have = star["fk"].astype(np.int64), star["fk_exists"]
    key = wah.columns.column_operand_table(star["bsi_fk"][0], star["bsi_fk"][1], n, list(range(14)))
    val = wah.columns.column_operand_table(star["bsi_flag"][0], star["bsi_flag"][1], n, list(range(7)))
    lookup = torch.zeros(6000, dtype=torch.int32, device="cuda")
    counts = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
    sums = torch.zeros((nb + 1, 2), dtype=torch.int64, device="cuda")
    sc = torch.empty(int(wah.lib().wah_bsi_group_by_scratch_bytes(n)), dtype=torch.uint8, device="cuda")

    def call():
        wah.bsi_group_by_device(key, n, n_rows, nb, value_table=val, exists=True, lookup=lookup, scratch=sc, counts=counts, sums=sums, check=False)

    def query(seed):
        table = np.random.default_rng(seed).integers(0, nb + 4, 6000).astype(np.uint32)
        table[::7] = gb.DROP
        lookup.copy_(_dev(table))
        case = dict(n=n, n_rows=n_rows, keys=np.r_[star["fk"], np.zeros(100, np.uint64)], exists=np.r_[have, np.zeros(100, bool)],
                    vals=np.r_[star["flag"], np.zeros(100, np.uint64)], vs=7, filters=[], lookup=table, n_buckets=nb, prefill=None)
        return gb.expected(case)

    want = query(1)
    call()
    assert int(wah.lib().wah_bsi_group_by_status(sc.data_ptr(), None)) == 0
    assert _u64(counts) == want[0] and _u64(sums)[0::2] == want[1]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            call()
    seen = set()
    for seed in (2, 3, 1):
        want = query(seed)
        counts.fill_(-1)
        sums.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(wah.lib().wah_bsi_group_by_status(sc.data_ptr(), None)) == 0
        assert _u64(counts) == want[0] and _u64(sums)[0::2] == want[1] and not any(_u64(sums)[1::2]), seed
        seen.add(tuple(want[0]))
    assert len(seen) == 3
