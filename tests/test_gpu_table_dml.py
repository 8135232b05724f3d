"""GPU tests of a table's second life: an index built once and then changed only by columns.delete_rows / keep_rows /
update_rows / reorder_rows / append_rows / slice_rows under masks made on the device from the device table, and after every
mutation (a) every index word for word against a from-scratch build of the model at the state's column length, (b) the first
battery of tests/_table.py and (c) the second one of tests/_table_dml.py: membership, grouping by a bit-sliced key, mapped
attributes, division, running and partitioned totals, the setters, whole-column read-back, and all of those fed into the older
calls.  Every comparison is exact.  tests/test_table_dml_reference.py proves on the CPU that the lives reach the seams they name
and that the second battery bites.  Outputs are filled with 0x5A5A5A5A, have 64 entries of guard behind them and a scratch of
0xA5 bytes, as in tests/test_gpu_table_life.py, whose helpers this file uses."""
import numpy as np
import pytest

from tests import _table as T, _table_dml as D
from tests.test_gpu_table_life import (KEYS, SEG_WORDS, WAH_ERR_STREAM, WAH_OK, Buffers, _dev, _np, assert_same_index, assert_state, build,
                                       computed, queries, wah)  # noqa: F401  (wah: the module's fixture)

pytestmark = pytest.mark.gpu

SECTIONS = "ABCDEFGHI"
BY_SECTION = {"A": ("c in ", "c not in "), "B": ("group by b", "group by a"), "C": ("values of mp", "values of k"),
              "D": ("values of q", "values of r", "values of d / 1000", "c != q", "c == q", "sum q"),
              "E": ("cumsum a where W", "row numbers where W"),
              "F": ("partition starts", "cumsum a by k", "total a", "row numbers by k", "partition sizes", "mean a by k", "rows of partitions", "streak lengths",
                    "count distinct"),
              "G": ("values of a set", "a set to 7", "min of a set", "count g with key 0", "values of CASE", "sum of CASE", "values of greatest",
                    "values of least", "greatest(b, k) >"),
              "H": ("read c", "read g"),
              "I": ("rows with the running sum", "kth q", "median q", "group by g, h", "running sum <= total", "quantiles of the running sum")}


def section_of(name):
    found = [s for s, prefixes in BY_SECTION.items() if name.startswith(prefixes)]
    assert len(found) == 1, name
    return found[0]


def zero_bitmap(n):
    """The indexed bitmap of n words without a set bit: one zero fill of 1024 groups per segment."""
    import torch

    segs = n // SEG_WORDS
    return (torch.full((segs,), -(1 << 31) + 1024, dtype=torch.int32, device="cuda:0"), torch.arange(segs + 1, dtype=torch.int64, device="cuda:0"))


def mask_of(wah, t, name, bufs=None):
    """A predicate of D.predicate as a (stream, seg_offsets) pair, made on the device from the device table."""
    C = wah.columns
    n = t["g"][2]
    segs = n // SEG_WORDS
    bufs = Buffers() if bufs is None else bufs

    def bitmap(scratch_bytes):
        return dict(scratch=Buffers.scratch(scratch_bytes), out=bufs.words(wah.max_compressed_words(n)), out_offsets=bufs.longs(segs + 1))

    def negation(pair):
        return C.filter_columns(wah, [(pair[0], pair[1], [0], True)], n, **bitmap(wah.lib().wah_bitop_clauses_scratch_bytes(n, 1, 1)))

    if name in ("W", "NOT W"):
        lo, hi = T.bounds()
        in_range = C.range_column(wah, t["a"], lo, hi, **bitmap(wah.lib().wah_bsi_range_scratch_bytes(n, T.BITS["a"])))
        preds = [(t["g"][0], t["g"][1], list(T.W_G), False), (t["h"][0], t["h"][1], list(T.W_NOT_H), True), (in_range[0], in_range[1], [0], False)]
        got = C.filter_columns(wah, preds, n, **bitmap(wah.lib().wah_bitop_clauses_scratch_bytes(n, 4, 3)))
        got = negation(got) if name == "NOT W" else got
    elif name == "c top":
        got = C.compare_column(wah, t["c"], "==", D.C_TOP, **bitmap(wah.lib().wah_bsi_range_scratch_bytes(n, T.BITS["c"])))
    elif name == "a absent":  # the clause negation of a's existence column
        got = C.filter_columns(wah, [(t["a"][0], t["a"][1], [T.BITS["a"]], True)], n, **bitmap(wah.lib().wah_bitop_clauses_scratch_bytes(n, 1, 1)))
    elif name == "all":
        got = negation(zero_bitmap(n))
    elif name == "none":
        got = zero_bitmap(n)
    else:
        raise ValueError(name)
    assert bufs.kept()
    return got[0], got[1]


def _compacted(wah, fn, index, mask, n_rows, n_rows_out):
    """keep_rows / delete_rows into guarded buffers of the documented sizes; returns (index, rows tensor)."""
    n = index[2]
    k = wah.columns._index_columns(index[1], n)
    n_out = T.n_words_of(n_rows if n_rows_out is None else n_rows_out)
    bufs = Buffers()
    reuse = dict(scratch=Buffers.scratch(wah.lib().wah_compact_scratch_bytes(n, n_out, k)), out=bufs.words(k * wah.max_compressed_words(n_out)),
                 out_offsets=bufs.longs(k * (n_out // SEG_WORDS) + 1), out_rows=bufs.longs(1))
    got = fn(wah, index, mask, n_rows, n_rows_out=n_rows_out, **reuse)
    assert bufs.kept()
    return got


def mutate(wah, table, before, after):
    """The whole table through the mutation that made state `after`: all five indexes under the same mask or order."""
    import torch

    C = wah.columns
    step = after.mutation
    kind = step[0]
    if kind == "append":
        batch = build(wah, T.batch_of(after.batch))
        return {key: C.append_rows(wah, ix, before.rows, batch[key], step[1]) for key, ix in table.items()}
    if kind == "trim":
        return {key: C.slice_rows(wah, ix, step[1], before.rows - step[1] - step[2]) for key, ix in table.items()}
    if kind in ("delete", "keep"):
        mask = mask_of(wah, table, step[1])
        fn = C.delete_rows if kind == "delete" else C.keep_rows
        got = {key: _compacted(wah, fn, ix, mask, before.rows, None if step[2] == "exact" else before.rows) for key, ix in table.items()}
        assert {int(rows.item()) for _, rows in got.values()} == {after.rows}
        return {key: ix for key, (ix, _) in got.items()}
    if kind == "update":
        mask = mask_of(wah, table, step[1])
        source = build(wah, T.batch_of((before.ids + step[2]) % T.N), n_words=before.n_words)
        bufs = Buffers()
        out = {}
        for key, ix in table.items():
            n = ix[2]
            k = C._index_columns(ix[1], n)
            out[key] = C.update_rows(wah, ix, mask, before.rows, source[key], scratch=Buffers.scratch(wah.lib().wah_update_scratch_bytes(n, k)),
                                     out=bufs.words(k * wah.max_compressed_words(n)), out_offsets=bufs.longs(k * (n // SEG_WORDS) + 1))
        assert bufs.kept()
        return out
    if kind == "cluster":
        if step[1] == "g":
            key = C.keys_of_column(wah, table["g"], 0, before.rows)
        else:
            key = C.values_of_column(wah, C.map_column(wah, table["b"], before.rows, _dev(D.k_lookup()), n_bits=D.K_BITS), 0, before.rows)[0]
        order = torch.argsort(key, stable=True)
        return {name: C.reorder_rows(wah, ix, order, before.rows) for name, ix in table.items()}
    raise ValueError(kind)


def assert_indexes(wah, table, state, what):
    fresh = build(wah, T.batch_of(state.ids), n_words=state.n_words)
    for name in fresh:
        assert_same_index(table[name], fresh[name], (what, name))


def walk(wah, states):
    """(i, table) for every state of a life: built once from the first state, then only mutated."""
    table = build(wah, T.batch_of(states[0].ids))
    yield 0, table
    for i in range(1, len(states)):
        table = mutate(wah, table, states[i - 1], states[i])
        yield i, table


# ---- the second battery on the device ---------------------------------------------------------------------------------------------
def queries_dml(wah, t, rows, sections=SECTIONS):
    """The battery of D.battery_dml on the device table t of `rows` rows: the same names, the same types; sections: the letters
    of the sections whose answers are wanted (the attributes they share are computed in any case)."""
    import torch

    C, lib = wah.columns, wah.lib()
    n = t["g"][2]
    assert all(ix[2] == n for ix in t.values())
    segs = n // SEG_WORDS
    gs, go, _ = t["g"]
    hs, ho, _ = t["h"]
    all_g, all_h = list(range(T.N_G)), list(range(T.N_H))
    bufs = Buffers()
    w, not_w = mask_of(wah, t, "W", bufs), mask_of(wah, t, "NOT W", bufs)
    ka, kb, kc = T.BITS["a"], T.BITS["b"], T.BITS["c"]

    def attribute(fn, rows_out, scratch_bytes, *args, **kw):
        """A call that leaves a bit-sliced attribute of rows_out slices, into guarded buffers of exactly the documented sizes."""
        got = fn(wah, *args, scratch=Buffers.scratch(scratch_bytes), out=bufs.words(wah.max_compressed_words(rows_out * n)),
                 out_offsets=bufs.longs(rows_out * segs + 1), **kw)
        assert bufs.kept(), fn.__name__
        return got

    def read(bsi):
        values, have = C.values_of_column(wah, bsi)
        return _np(values), (None if have is None else _np(have))

    def listed(pair):
        return _np(wah.positions_device(pair[0], pair[-1], n)[0])

    sum_bits = ka + int(rows).bit_length()
    count_bits = max(int(rows).bit_length(), 1)
    ex, excl, every_row = wah.BSI_EXISTS, wah.CUMSUM_EXCLUSIVE, wah.CUMSUM_ALL_ROWS
    comp = computed(wah, t)
    d = comp["d"]
    mp = attribute(C.map_column, D.MP_BITS + 1, lib.wah_bsi_map_scratch_bytes(n, D.MP_BITS, wah.MAP_PARTIAL), t["b"], rows, _dev(D.mp_lookup()),
                   n_bits=D.MP_BITS, partial=True)
    k = attribute(C.map_column, D.K_BITS, lib.wah_bsi_map_scratch_bytes(n, D.K_BITS, 0), t["b"], rows, _dev(D.k_lookup()), n_bits=D.K_BITS)
    assert mp[2:] == (n, D.MP_BITS, True) and k[2:] == (n, D.K_BITS, False)
    q = attribute(C.divide_columns, kc + 1, lib.wah_bsi_div_scratch_bytes(n, kb, kc, wah.BSI_EXISTS_A), t["c"], t["b"])
    r = attribute(C.modulo_columns, kb + 1, lib.wah_bsi_div_scratch_bytes(n, kb, kb, wah.BSI_EXISTS_A), t["c"], t["b"])
    assert q[2:] == (n, kc, True) and r[2:] == (n, kb, True)
    cs = attribute(C.cumsum_column, sum_bits + 1, lib.wah_bsi_cumsum_scratch_bytes(n, sum_bits, ex), t["a"], rows, where=w)
    assert cs[2:] == (n, sum_bits, True)
    if rows:
        starts = C.partition_starts(wah, k, rows, out=bufs.words(wah.max_compressed_words(n)), out_offsets=bufs.longs(segs + 1))
    else:  # no row, no partition: the front end refuses 0 rows, and the battery goes on without a start
        with pytest.raises(ValueError):
            C.partition_starts(wah, k, rows)
        starts = zero_bitmap(n)
    cs_by = attribute(C.cumsum_column_by, sum_bits + 1, lib.wah_bsi_cumsum_parts_scratch_bytes(n, sum_bits, ex), t["a"], rows, starts, where=w)
    total_by = attribute(C.total_column_by, sum_bits + 1, lib.wah_bsi_total_parts_scratch_bytes(n, sum_bits, ex), t["a"], rows, starts, where=w)
    out = {}
    if "A" in sections:
        for label, members in D.MEMBER_SETS:
            out[f"c in {label}"] = listed(C.isin_column(wah, t["c"], list(members), out=bufs.words(wah.max_compressed_words(n)), out_offsets=bufs.longs(segs + 1)))
            out[f"c not in {label}"] = listed(C.isin_column(wah, t["c"], list(members), negate=True))
    if "B" in sections:
        for prefix, got in (("group by b where W", C.group_by_column(wah, t["b"], rows, attributes=[t["a"], d], where=w)),
                            ("group by a >> 8", C.group_by_column(wah, t["a"], rows, attributes=[t["a"], d], lookup=_dev(D.a_lookup()), n_buckets=D.A_BUCKETS))):
            out[f"{prefix}: rows"] = _np(got["rows"])
            out[f"{prefix}: other"] = (got["other"]["rows"], list(got["other"]["sums"]), list(got["other"]["counts"]))
            for i, name in enumerate(("a", "d")):
                out[f"{prefix}: sum {name}"], out[f"{prefix}: count {name}"] = got["sums"][i], _np(got["counts"][i])
    if "C" in sections:
        out["values of mp"], out["values of k"] = read(mp), read(k)
    if "D" in sections:
        out["values of q"], out["values of r"] = read(q), read(r)
        out["values of d / 1000"] = read(C.divide_column_by(wah, d, 1000))
        back = C.add_columns(wah, C.multiply_columns(wah, q, t["b"]), r)
        assert back[3:] == (kc + kb + 1, True)
        out["c != q * b + r"] = listed(C.compare_columns(wah, t["c"], "!=", back))
        out["c == q * b + r"] = listed(C.compare_columns(wah, t["c"], "==", back))
        out["sum q where W"] = C.sum_column_where(wah, q, *w)
    if "E" in sections:
        out["cumsum a where W"] = read(cs)
        out["cumsum a where W, exclusive, all rows"] = read(attribute(C.cumsum_column, D.CS_BITS, lib.wah_bsi_cumsum_scratch_bytes(n, D.CS_BITS, ex | excl | every_row),
                                                                      t["a"], rows, where=w, exclusive=True, all_rows=True, n_bits=D.CS_BITS))
        out["row numbers where W"] = read(attribute(C.row_numbers_where, count_bits + 1, lib.wah_bsi_cumsum_scratch_bytes(n, count_bits, 0), w, n, rows))
        out["row numbers where W, exclusive, all rows"] = read(attribute(C.row_numbers_where, count_bits, lib.wah_bsi_cumsum_scratch_bytes(n, count_bits, excl | every_row),
                                                                         w, n, rows, exclusive=True, all_rows=True))
    if "F" in sections:
        out["partition starts"] = listed(starts)
        out["cumsum a by k where W"], out["total a by k where W"] = read(cs_by), read(total_by)
        out["total a by k where W, all rows"] = read(attribute(C.total_column_by, sum_bits, lib.wah_bsi_total_parts_scratch_bytes(n, sum_bits, ex | every_row),
                                                               t["a"], rows, starts, where=w, all_rows=True))
        out["total a"] = read(C.total_column_by(wah, t["a"], rows, None))
        out["row numbers by k"] = read(attribute(C.row_numbers_by, count_bits + 1, lib.wah_bsi_cumsum_parts_scratch_bytes(n, count_bits, 0), starts, n, rows))
        out["partition sizes where W, all rows"] = read(attribute(C.partition_sizes, count_bits, lib.wah_bsi_total_parts_scratch_bytes(n, count_bits, every_row),
                                                                  starts, n, rows, where=w, all_rows=True))
        out["mean a by k"] = read(C.mean_column_by(wah, t["a"], rows, starts))
        out["rows of partitions of k where sum a > bound, W"] = listed(C.rows_of_partitions_where(wah, t["a"], rows, starts, ">", D.PARTITION_BOUND, where=w))
        out["streak lengths of W"] = read(C.streak_lengths(wah, w, n, rows))
        out["count distinct k"] = int(C.count_distinct_where(wah, k, rows).item())
    if "G" in sections:
        updated = dict(scratch=Buffers.scratch(lib.wah_update_scratch_bytes(n, ka + 1)), out=bufs.words((ka + 1) * wah.max_compressed_words(n)),
                       out_offsets=bufs.longs((ka + 1) * segs + 1))
        a7 = C.set_values_where(wah, t["a"], w, rows, 7, **updated)
        out["values of a set to 7 where W"] = read(a7)
        out["a set to 7 where W == 7"] = listed(C.compare_column(wah, a7, "==", 7))
        a_null = C.set_values_where(wah, t["a"], not_w, rows, None)
        out["values of a set to NULL where NOT W"] = read(a_null)
        out["min of a set to NULL where NOT W"] = tuple(C.min_column_where(wah, a_null))
        g0 = C.set_keys_where(wah, t["g"], w, rows, 0)
        out["count g with key 0 set where W"] = _np(C.count_columns(wah, g0[0], g0[1], n, all_g))
        chosen = C.choose_columns(wah, w, comp["s"], t["c"], rows)
        assert chosen[2:] == (n, kc, True)
        out["values of CASE WHEN W THEN s ELSE c"] = read(chosen)
        out["sum of CASE WHEN W THEN s ELSE c where W"] = C.sum_column_where(wah, chosen, *w)
        most, least = C.greatest_columns(wah, t["b"], k, rows), C.least_columns(wah, t["b"], k, rows)
        out["values of greatest(b, k)"], out["values of least(b, k)"] = read(most), read(least)
        out["greatest(b, k) > least(b, k)"] = listed(C.compare_columns(wah, most, ">", least))
        assert bufs.kept()
    if "H" in sections:
        for first, count in D.read_windows({"n_words": n, "rows": rows}):
            values, have = C.values_of_column(wah, t["c"], first, count)
            out[f"read c [{first}, +{count})"] = (_np(values), _np(have))
            out[f"read g [{first}, +{count})"] = _np(C.keys_of_column(wah, t["g"], first, count))
    if "I" in sections:
        out["rows with the running sum in a range"] = listed(C.range_column(wah, cs, *D.RANGE_ON_SUM))
        out["kth q where W"], out["median q where W"] = tuple(C.kth_column_where(wah, q, D.KTH, w)), tuple(C.median_column_where(wah, q, w))
        got = C.aggregate_columns(wah, [(gs, go, all_g), (hs, ho, all_h)], [mp], n)
        out["group by g, h: rows"], out["group by g, h: sum mp"], out["group by g, h: count mp"] = _np(got["rows"]), got["sums"][0], _np(got["counts"][0])
        out["running sum <= total, by k"] = listed(C.compare_columns(wah, cs_by, "<=", total_by))
        got = C.quantiles_by(wah, [(gs, go, all_g)], cs_by, n, list(T.QUANTILES), where=w)
        out["quantiles of the running sum by g: values"] = got["values"]
        for part in ("totals", "less", "equal"):
            out[f"quantiles of the running sum by g: {part}"] = _np(got[part])
    assert bufs.kept()
    return out


# ---- the lives -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.LIVES))
def test_life(wah, name):
    """The table is made once, from the life's first state, and then only mutated; after every mutation every index is the
    from-scratch index of the model AT THE STATE'S COLUMN LENGTH -- stream length, words, every offset, the tuple's tail -- and
    the whole first battery answers as the model does, the empty table and the table in columns longer than it needs included."""
    states = D.run(name)
    for i, table in walk(wah, states):
        assert_state(wah, table, states[i], (name, i, states[i].mutation))


@pytest.mark.parametrize("sections", ["ABCD", "EFG", "HI"])
@pytest.mark.parametrize("name", list(D.LIVES))
def test_life_dml(wah, name, sections):
    """The same walk, the second battery at every state (a third of its sections per case, so that each case stays short)."""
    states = D.run(name)
    for i, table in walk(wah, states):
        want = {key: v for key, v in D.battery_dml(D.columns(states[i])).items() if section_of(key) in sections}
        got = queries_dml(wah, table, states[i].rows, sections)
        assert D.differing(got, want) == [], (name, i, states[i].mutation)


def test_the_exclusive_row_number_is_where_keep_rows_puts_a_row(wah):
    """In every keep_where and delete_where step of `purge`: the exclusive row number over all rows, taken under the step's
    selection, is at every kept row the row it is moved to, and the count keep_rows / delete_rows returns is the inclusive row
    number of the table's last row."""
    import torch

    C = wah.columns
    states = D.run("purge")
    steps = 0
    for i, table in walk(wah, states[:-1]):
        before, after = states[i], states[i + 1]
        if after.mutation[0] not in ("delete", "keep"):
            continue
        steps += 1
        n = before.n_words
        mask = mask_of(wah, table, after.mutation[1])
        selection = mask if after.mutation[0] == "keep" else C.filter_columns(wah, [(mask[0], mask[1], [0], True)], n)
        model = D.predicate(D.columns(before), after.mutation[1])[: before.rows]
        kept = np.flatnonzero(model if after.mutation[0] == "keep" else ~model)
        rn = C.row_numbers_where(wah, selection, n, before.rows, exclusive=True, all_rows=True)
        values, have = C.values_at_rows(wah, rn, _dev(kept))
        assert have is None and np.array_equal(_np(values), np.arange(kept.size)), (i, after.mutation)
        fn = C.keep_rows if after.mutation[0] == "keep" else C.delete_rows
        _, count = fn(wah, table["b"], mask, before.rows, n_rows_out=before.rows)
        last = C.row_numbers_where(wah, selection, n, before.rows, all_rows=True)
        assert int(count.item()) == kept.size == after.rows
        if before.rows:
            assert int(C.values_at_rows(wah, last, torch.tensor([before.rows - 1], dtype=torch.int64, device="cuda:0"))[0].item()) == kept.size
    assert steps == 6


def test_derived_attributes_commute_with_dml(wah):
    """q = c / b, mp = map(b) and the running sum of a under W, computed from the first state and carried through a delete_where and
    an update_from as 5-tuples like any other index: q and mp are then, word for word, the q and mp of the mutated base; the
    running sum does not commute -- a carried row keeps the sum it had, an updated row takes the source table's -- and is held
    against the model."""
    C = wah.columns
    states = D.run(D.CARRIED)
    sum_bits = T.BITS["a"] + int(states[0].rows).bit_length()

    def derived(t, rows):
        w = mask_of(wah, t, "W")
        return {"q": C.divide_columns(wah, t["c"], t["b"]), "mp": C.map_column(wah, t["b"], rows, _dev(D.mp_lookup()), n_bits=D.MP_BITS, partial=True),
                "cs": C.cumsum_column(wah, t["a"], rows, where=w, n_bits=sum_bits)}

    def model_cs(state):
        return D.battery_dml(D.columns(state))["cumsum a where W"]

    base = {key: ix for key, ix in build(wah, T.batch_of(states[0].ids)).items()}
    carried = derived(base, states[0].rows)
    want_cs = model_cs(states[0])
    for i in (1, 2):
        before, after = states[i - 1], states[i]
        kind, pred = after.mutation[:2]
        mask = mask_of(wah, base, pred)
        selected = D.predicate(D.columns(before), pred)[: before.rows]
        if kind == "delete":
            base = {key: C.delete_rows(wah, ix, mask, before.rows)[0] for key, ix in base.items()}
            carried = {key: C.delete_rows(wah, ix, mask, before.rows)[0] for key, ix in carried.items()}
            want_cs = tuple(D._padded(x[: before.rows][~selected], 32 * after.n_words, x.dtype) for x in want_cs)
        else:
            shifted = D.State((before.ids + after.mutation[2]) % T.N, None, n_words=before.n_words)
            source = build(wah, T.batch_of(shifted.ids), n_words=before.n_words)
            source_derived = derived(source, before.rows)
            base = {key: C.update_rows(wah, ix, mask, before.rows, source[key]) for key, ix in base.items()}
            carried = {key: C.update_rows(wah, ix, mask, before.rows, source_derived[key]) for key, ix in carried.items()}
            chosen = D._padded(selected, 32 * after.n_words, bool)
            want_cs = tuple(np.where(chosen, x, y) for x, y in zip(model_cs(shifted), want_cs))
        assert_indexes(wah, base, after, ("carried", i))
        fresh = derived(base, after.rows)
        for key in ("q", "mp"):
            assert_same_index(carried[key], fresh[key], ("carried", i, key))
        values, have = C.values_of_column(wah, carried["cs"])
        assert carried["cs"][2:] == (after.n_words, sum_bits, True)
        assert np.array_equal(_np(values), want_cs[0]) and np.array_equal(_np(have), want_cs[1]), i
        if kind == "update":  # (it does not commute: the source's sums are those of another table)
            assert not np.array_equal(_np(C.values_of_column(wah, fresh["cs"])[0]), want_cs[0])


# ---- a chain with nothing read back --------------------------------------------------------------------------------------------------
def _chain_table(wah, ids):
    u = T.universe()
    C = wah.columns
    return {"g": C.index_from_keys(wah, _dev(u["g"][ids]), T.N_G), "h": C.index_from_keys(wah, _dev(u["h"][ids]), T.N_H),
            "a": C.bsi_from_values(wah, _dev(u["a"][ids]), T.BITS["a"], exists=_dev(u["ea"][ids])), "b": C.bsi_from_values(wah, _dev(u["b"][ids]), T.BITS["b"])}


def test_a_dml_chain_with_nothing_read_back(wah):
    """clause -> row numbers -> keep_rows of b and a under a bound -> map -> partition starts -> running sum per partition -> range ->
    masked count, every stage with check=False and every output passed on as the whole sentinel-filled, guarded buffer it came in: a
    stream whose length is a capacity, a compacted index whose rows end somewhere in front of the bound.  The statuses are read
    after the last stage is enqueued, and the answers are those of the check=True chain and of the model."""
    import torch

    C, lib = wah.columns, wah.lib()
    ids = np.arange(T.CHAIN_ROWS)
    rows = int(ids.size)
    t = _chain_table(wah, ids)
    n = T.n_words_of(rows)
    segs = n // SEG_WORDS
    ka, kb, kk = T.BITS["a"], T.BITS["b"], D.K_BITS
    sum_bits, count_bits = ka + rows.bit_length(), rows.bit_length()
    lookup = _dev(D.k_lookup()).to(torch.int32)
    want = D.chain_answers(ids, ids)
    kept_rows = want["kept"]
    column = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    slices = torch.arange(kk, dtype=torch.int64, device="cuda:0")

    def chain(check):
        bufs, sc = Buffers(), {}

        def attribute(name, rows_out, scratch_bytes, columns=1):
            sc[name] = Buffers.scratch(scratch_bytes)
            return dict(check=check, scratch=sc[name], out=bufs.words(columns * wah.max_compressed_words(rows_out * n)), out_offsets=bufs.longs(columns * rows_out * segs + 1))

        preds = [(t["g"][0], t["g"][1], list(D.CHAIN_NOT_G), True), (t["h"][0], t["h"][1], list(D.CHAIN_NOT_H), True)]
        f = C.filter_columns(wah, preds, n, **attribute("clause", 1, lib.wah_bitop_clauses_scratch_bytes(n, 4, 2)))
        f = (f[0], f[-1])
        assert f[0].numel() == wah.max_compressed_words(n) or check  # the whole buffer
        rn = C.row_numbers_where(wah, f, n, rows, exclusive=True, all_rows=True,
                                 **attribute("rn", count_bits, lib.wah_bsi_cumsum_scratch_bytes(n, count_bits, wah.CUMSUM_EXCLUSIVE | wah.CUMSUM_ALL_ROWS)))
        kept, counts = {}, {}
        for name, bits in (("b", kb), ("a", ka + 1)):
            reuse = attribute("keep " + name, 1, lib.wah_compact_scratch_bytes(n, n, bits), columns=bits)
            kept[name], counts[name] = C.keep_rows(wah, t[name], f, rows, n_rows_out=rows, out_rows=bufs.longs(1), **reuse)
        k = C.map_column(wah, kept["b"], rows, lookup, n_bits=kk, **attribute("map", kk, lib.wah_bsi_map_scratch_bytes(n, kk, 0)))
        shift = attribute("shift", 1, lib.wah_splice_scratch_bytes(n, kk, 2), columns=kk)
        del shift["check"]
        starts = C.partition_starts(wah, k, rows, shift=shift, **attribute("starts", 1, lib.wah_bsi_compare_scratch_bytes(n, kk, kk)))
        cs = C.cumsum_column_by(wah, kept["a"], rows, starts, **attribute("sum", sum_bits + 1, lib.wah_bsi_cumsum_parts_scratch_bytes(n, sum_bits, wah.BSI_EXISTS)))
        r = C.range_column(wah, cs, *D.CHAIN_RANGE, **attribute("range", 1, lib.wah_bsi_range_scratch_bytes(n, sum_bits)))
        sc["inner"] = Buffers.scratch(lib.wah_bitop_clauses_scratch_bytes(n, 1, 1))
        sc["count"] = Buffers.scratch(lib.wah_select_scratch_bytes(n, kk))
        got = C.count_columns_where(wah, [(r[0], r[-1], column, False)], k[0], k[1], n, slices, check=check, scratch=sc["count"],
                                    counts=bufs.longs(kk).view(1, kk), filter=dict(scratch=sc["inner"]))
        # every stage is enqueued: now the statuses
        flags_rn = wah.CUMSUM_EXCLUSIVE | wah.CUMSUM_ALL_ROWS
        status = {"clause": lib.wah_bitop_clauses_status(sc["clause"].data_ptr(), n, 4, 2, None),
                  "rn": lib.wah_bsi_cumsum_status(sc["rn"].data_ptr(), n, count_bits, flags_rn, None),
                  "keep b": lib.wah_compact_status(sc["keep b"].data_ptr(), None), "keep a": lib.wah_compact_status(sc["keep a"].data_ptr(), None),
                  "map": lib.wah_bsi_map_status(sc["map"].data_ptr(), n, kk, 0, None), "shift": lib.wah_splice_status(sc["shift"].data_ptr(), None),
                  "starts": lib.wah_bsi_compare_status(sc["starts"].data_ptr(), n, kk, kk, None),
                  "sum": lib.wah_bsi_cumsum_parts_status(sc["sum"].data_ptr(), n, sum_bits, wah.BSI_EXISTS, None),
                  "range": lib.wah_bsi_range_status(sc["range"].data_ptr(), n, sum_bits, None),
                  "inner": lib.wah_bitop_clauses_status(sc["inner"].data_ptr(), n, 1, 1, None), "count": lib.wah_select_status(sc["count"].data_ptr(), None)}
        assert all(rc == WAH_OK for rc in status.values()), status
        assert bufs.kept()
        assert int(counts["a"].item()) == int(counts["b"].item()) == kept_rows.size
        ranks, _ = C.values_at_rows(wah, (rn[0], rn[1], n, count_bits, False), _dev(kept_rows))
        return {"clause": wah.positions_device(f[0], f[1], n)[1], "kept": _np(ranks), "counts": _np(got), "hit": _np(wah.positions_device(r[0], r[-1], n)[0])}

    want = dict(want, kept=np.arange(kept_rows.size))  # the exclusive row number of a kept row is where it goes
    loose, checked = chain(False), chain(True)
    assert want["counts"].min() > 0 and want["clause"] > kept_rows.size and D.differing(loose, want) == [] and D.differing(checked, want) == []


def test_the_dml_chain_replays_as_one_graph(wah):
    """The same chain from the device calls -- bsi_build twice, bitop_clauses, bsi_cumsum, compact twice, bsi_map, splice,
    bsi_compare, bsi_cumsum_parts, bsi_range, count_masked --, captured ONCE (side stream, warm-up outside, check=False; one chain
    of launches, no parallel branches) over fixed scratch, out, out_offsets and tables made before the capture from the fixed
    buffers' addresses, and replayed after the value tensors were overwritten in place with three other stretches of the universe,
    one of them constant.  Every output is refilled with 0x5A5A5A5A before each replay; after each one the statuses, the guards,
    the kept rows' count and the counts are checked."""
    import torch

    C, lib = wah.columns, wah.lib()
    stretches = T.chain_stretches()
    key_ids = stretches[0]
    rows = T.CHAIN_ROWS
    n = T.n_words_of(rows)
    segs = n // SEG_WORDS
    ka, kb, kk = T.BITS["a"], T.BITS["b"], D.K_BITS
    sum_bits, count_bits = ka + rows.bit_length(), rows.bit_length()
    rn_flags = wah.CUMSUM_EXCLUSIVE | wah.CUMSUM_ALL_ROWS
    u = T.universe()
    d_a, d_b, d_ea = (_dev(u[name][key_ids].copy()) for name in ("a", "b", "ea"))
    g = C.index_from_keys(wah, _dev(u["g"][key_ids]), T.N_G)
    h = C.index_from_keys(wah, _dev(u["h"][key_ids]), T.N_H)
    lookup = _dev(D.k_lookup()).to(torch.int32)
    bufs = Buffers()
    widths = {"a": ka + 1, "b": kb, "f": 1, "rn": count_bits, "kept a": ka + 1, "kept b": kb, "k": kk, "shifted": kk, "starts": 1, "cs": sum_bits + 1, "r": 1}
    out = {name: bufs.words(wah.max_compressed_words(width * n) if name not in ("kept a", "kept b", "shifted") else width * wah.max_compressed_words(n))
           for name, width in widths.items()}
    offs = {name: bufs.longs(width * segs + 1) for name, width in widths.items()}
    kept_rows = {"a": bufs.longs(1), "b": bufs.longs(1)}
    counts = bufs.longs(kk).view(1, kk)
    sc = {"a": lib.wah_bsi_build_scratch_bytes(n, ka + 1), "b": lib.wah_bsi_build_scratch_bytes(n, kb), "f": lib.wah_bitop_clauses_scratch_bytes(n, 4, 2),
          "rn": lib.wah_bsi_cumsum_scratch_bytes(n, count_bits, rn_flags), "kept a": lib.wah_compact_scratch_bytes(n, n, ka + 1),
          "kept b": lib.wah_compact_scratch_bytes(n, n, kb), "k": lib.wah_bsi_map_scratch_bytes(n, kk, 0), "shifted": lib.wah_splice_scratch_bytes(n, kk, 2),
          "starts": lib.wah_bsi_compare_scratch_bytes(n, kk, kk), "cs": lib.wah_bsi_cumsum_parts_scratch_bytes(n, sum_bits, wah.BSI_EXISTS),
          "r": lib.wah_bsi_range_scratch_bytes(n, sum_bits), "c": lib.wah_select_scratch_bytes(n, kk)}
    sc = {name: Buffers.scratch(size) for name, size in sc.items()}

    # the tables, from the fixed buffers' addresses: a stream's length is its buffer's capacity
    def table(name, columns):
        return C.column_operand_table(out[name], offs[name], n, list(columns))

    clause_table = torch.cat([C.column_operand_table(g[0], g[1], n, list(D.CHAIN_NOT_G)), C.column_operand_table(h[0], h[1], n, list(D.CHAIN_NOT_H))])
    clause_ends = torch.tensor([len(D.CHAIN_NOT_G) | wah.CLAUSE_NEGATE, (len(D.CHAIN_NOT_G) + len(D.CHAIN_NOT_H)) | wah.CLAUSE_NEGATE], dtype=torch.int64, device="cuda:0")
    f_table = table("f", [0])
    a_table, b_table = table("a", range(ka + 1)), table("b", range(kb))
    kept_b_table, kept_a_table = table("kept b", range(kb)), table("kept a", range(ka + 1))
    k_table = table("k", range(kk))
    pieces = wah.splice_pieces([(n, 0, 1), (n, 0, rows - 1)], "cuda:0")
    shift_table = torch.cat([k_table, k_table])
    k_bsi, shifted_bsi = (out["k"], offs["k"], n, kk, False), (out["shifted"], offs["shifted"], n, kk, False)
    compare_table = C._two_attribute_table(wah.bsi_compare_row_order(kk, kk, False, False), k_bsi, shifted_bsi)
    starts_table = table("starts", [0])
    range_table = table("cs", range(sum_bits + 1))
    bounds = wah.bsi_bounds(*D.CHAIN_RANGE, "cuda:0")
    r_table = table("r", [0])

    def reuse(name):
        return dict(scratch=sc[name], out=out[name], out_offsets=offs[name], check=False)

    def enqueue():
        wah.bsi_build_device(d_a, ka, n, exists=d_ea, **reuse("a"))
        wah.bsi_build_device(d_b, kb, n, **reuse("b"))
        wah.bitop_clauses_indexed_device((clause_table, clause_ends), n, **reuse("f"))
        wah.bsi_cumsum_device(None, n, rows, 0, count_bits, filters=f_table, exclusive=True, all_rows=True, **reuse("rn"))
        wah.compact_device(f_table, b_table, n, rows, n, out_rows=kept_rows["b"], **reuse("kept b"))
        wah.compact_device(f_table, a_table, n, rows, n, out_rows=kept_rows["a"], **reuse("kept a"))
        wah.bsi_map_device(kept_b_table, n, rows, lookup, kk, **reuse("k"))
        wah.splice_device(pieces, shift_table, kk, n, **reuse("shifted"))
        wah.bsi_compare_device(compare_table, kk, kk, "!=", n, **reuse("starts"))
        wah.bsi_cumsum_parts_device(kept_a_table, n, rows, ka, sum_bits, starts_table, exists=True, **reuse("cs"))
        wah.bsi_range_device(range_table, bounds, n, exists=True, **reuse("r"))
        wah.count_masked_device(r_table, k_table, n, scratch=sc["c"], counts=counts, check=False)

    enqueue()  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            enqueue()
    sizes = set()
    for i in (1, 2, 3, 0):
        ids = stretches[i]
        d_a.copy_(_dev(u["a"][ids]))
        d_b.copy_(_dev(u["b"][ids]))
        d_ea.copy_(_dev(u["ea"][ids]))
        for buf, _, sentinel in bufs.made:
            buf.fill_(sentinel)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        status = [lib.wah_bsi_build_status(sc["a"].data_ptr(), n, ka + 1, None), lib.wah_bsi_build_status(sc["b"].data_ptr(), n, kb, None),
                  lib.wah_bitop_clauses_status(sc["f"].data_ptr(), n, 4, 2, None), lib.wah_bsi_cumsum_status(sc["rn"].data_ptr(), n, count_bits, rn_flags, None),
                  lib.wah_compact_status(sc["kept b"].data_ptr(), None), lib.wah_compact_status(sc["kept a"].data_ptr(), None),
                  lib.wah_bsi_map_status(sc["k"].data_ptr(), n, kk, 0, None), lib.wah_splice_status(sc["shifted"].data_ptr(), None),
                  lib.wah_bsi_compare_status(sc["starts"].data_ptr(), n, kk, kk, None),
                  lib.wah_bsi_cumsum_parts_status(sc["cs"].data_ptr(), n, sum_bits, wah.BSI_EXISTS, None),
                  lib.wah_bsi_range_status(sc["r"].data_ptr(), n, sum_bits, None), lib.wah_select_status(sc["c"].data_ptr(), None)]
        assert status == [WAH_OK] * 12, (i, status)
        assert bufs.kept(), i
        want = D.chain_answers(key_ids, ids)
        assert int(kept_rows["a"].item()) == int(kept_rows["b"].item()) == want["kept"].size, i
        assert np.array_equal(_np(counts).reshape(-1), want["counts"]), (i, _np(counts), want["counts"])
        sizes.add(int(offs["k"][-1].item()))
    assert len(sizes) == 4 and max(sizes) > 20 * min(sizes)  # the constant stretch's k is a few fills


# ---- mismatched column lengths after a bound-sized delete --------------------------------------------------------------------------
def test_a_stale_column_length_is_refused_not_misread(wah):
    """After a bound-sized delete that kept the column length and an exact one that shortened it: an attribute of the old
    length beside one of the new is a ValueError of the front end, before any launch; a mask of the old length under a
    device-tensor column list is WAH_ERR_STREAM from the status; and what a launch would have written into is still the sentinel."""
    import torch

    C = wah.columns
    states = D.run("cluster")
    before = states[3]
    old = build(wah, T.batch_of(before.ids))
    mask = mask_of(wah, old, "W")
    bound = {key: C.delete_rows(wah, ix, mask, before.rows, n_rows_out=before.rows)[0] for key, ix in old.items()}
    exact = {key: C.delete_rows(wah, ix, mask, before.rows)[0] for key, ix in old.items()}
    n_old, n_new = before.n_words, T.n_words_of(states[4].rows)
    assert n_old == 3 * SEG_WORDS and n_new == 2 * SEG_WORDS and bound["a"][2] == n_old and exact["a"][2] == n_new
    bufs = Buffers()
    with pytest.raises(ValueError):
        C.compare_columns(wah, bound["a"], "<", exact["b"], out=bufs.words(wah.max_compressed_words(n_old)), out_offsets=bufs.longs(n_old // SEG_WORDS + 1))
    for fn in (C.add_columns, C.multiply_columns, C.divide_columns, C.modulo_columns):
        with pytest.raises(ValueError):
            fn(wah, exact["a"], bound["b"], out=bufs.words(wah.max_compressed_words(64 * n_old)), out_offsets=bufs.longs(64 * (n_old // SEG_WORDS) + 1))
    with pytest.raises(ValueError):
        C.update_rows(wah, bound["a"], mask, states[4].rows, exact["a"], out=bufs.words(13 * wah.max_compressed_words(n_old)),
                      out_offsets=bufs.longs(13 * (n_old // SEG_WORDS) + 1))
    with pytest.raises(ValueError):
        C.choose_columns(wah, mask, bound["a"], exact["c"], states[4].rows)
    with pytest.raises(ValueError):
        C.group_by_column(wah, bound["b"], states[4].rows, attributes=[exact["a"]])
    assert bufs.untouched()
    # a mask made over the exact-sized table, two segments long, under the bound-sized table's three
    lo, hi = T.bounds()
    bufs = Buffers()
    stale = C.range_column(wah, exact["a"], lo, hi, out_offsets=bufs.longs(n_new // SEG_WORDS + 1))
    gs, go, _ = bound["g"]
    all_g = list(range(T.N_G))
    with pytest.raises(ValueError):
        C.count_columns_where(wah, [(stale[0], stale[1], [0], False)], gs, go, n_old, all_g)
    column = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    counts = bufs.longs(T.N_G).view(1, T.N_G)
    with pytest.raises(wah.WahError, match=r"the filter failed \(code -6\)"):
        C.count_columns_where(wah, [(stale[0], stale[1], column, False)], gs, go, n_old, all_g, counts=counts)
    assert bufs.kept()
    fresh = C.range_column(wah, bound["a"], lo, hi)  # ... and the mask of the table's own length counts
    got = C.count_columns_where(wah, [(fresh[0], fresh[1], column, False)], gs, go, n_old, all_g)
    m = T.columns_of(states[4], n_old)
    in_range = m["ea"] & (m["a"] >= lo) & (m["a"] <= hi)
    assert _np(got).tolist() == [int(np.count_nonzero(in_range & (m["g"] == v))) for v in range(T.N_G)]
