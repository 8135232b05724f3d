"""GPU tests of a table that lives: an index built once and then changed only by columns.append_rows / slice_rows /
splice_columns, every result fed into the next mutation, and after every mutation (a) every index word for word against a
from-scratch build of the model's padded columns and (b) the whole query battery of tests/_table.py, name by name.  Every
comparison is exact.  tests/test_table_reference.py proves on the CPU that the lives reach the seams they name and that the
battery bites.  The arithmetic calls, the WHERE clause's range and filters, the grouped sum and the chains get their outputs
filled with 0x5A5A5A5A, 64 entries of guard behind them and a scratch of 0xA5 bytes, as tests/test_gpu_full_grid.py does."""
import importlib

import numpy as np
import pytest

from tests import _table as T

pytestmark = pytest.mark.gpu

WAH_OK, WAH_ERR_STREAM = 0, -6
SENTINEL, SENTINEL64, GUARD = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A, 64
SEG_WORDS = T.SEG_WORDS
KEYS = (("g", T.N_G), ("h", T.N_H))


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


class Buffers:
    """Outputs filled with the sentinel and followed by GUARD entries of it, scratch filled with 0xA5; kept() after the call."""

    def __init__(self):
        self.made = []

    def words(self, n):
        import torch

        buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
        self.made.append((buf, n, SENTINEL))
        return buf[:n]

    def longs(self, n):
        import torch

        buf = torch.full((n + GUARD,), SENTINEL64, dtype=torch.int64, device="cuda:0")
        self.made.append((buf, n, SENTINEL64))
        return buf[:n]

    @staticmethod
    def scratch(n_bytes):
        import torch

        return torch.full((int(n_bytes),), 0xA5, dtype=torch.uint8, device="cuda:0")

    def kept(self):
        return all(bool((buf[n:] == sentinel).all()) for buf, n, sentinel in self.made)

    def untouched(self):
        return all(bool((buf == sentinel).all()) for buf, _, sentinel in self.made)


# ---- the device table --------------------------------------------------------------------------------------------------------------
def build(wah, cols, n_words=None):
    """The indexes of bare columns (T.batch_of), from scratch: name -> index_from_keys 3-tuple / bsi_from_values 5-tuple."""
    C = wah.columns
    out = {key: C.index_from_keys(wah, _dev(cols[key]), count, n_words_per_column=n_words) for key, count in KEYS}
    for name, bits in T.BITS.items():
        exists = _dev(cols["e" + name]) if T.HAS_EXISTS[name] else None
        out[name] = C.bsi_from_values(wah, _dev(cols[name]), bits, n_words_per_column=n_words, exists=exists)
    return out


def mutate(wah, index, before, after, batch):
    """One index of the table through the mutation that made state `after`; batch: the batch's index of the same kind."""
    C = wah.columns
    step = after.mutation
    if step[0] == "append":
        return C.append_rows(wah, index, before.rows, batch, step[1])
    if step[0] == "drop_front":
        return C.slice_rows(wah, index, step[1], before.rows - step[1])
    if step[0] == "window":
        return C.slice_rows(wah, index, step[1], step[2])
    lo, hi = step[1:]
    return C.splice_columns(wah, [(tuple(index[:3]), 0, lo), (tuple(index[:3]), hi, before.rows - hi)]) + tuple(index[3:])


def assert_same_index(got, want, what):
    """Stream length, words, every index entry and the tuple's tail."""
    assert len(got) == len(want) and tuple(got[2:]) == tuple(want[2:]), what
    assert got[0].numel() == want[0].numel() and bool((got[0] == want[0]).all()), what
    assert got[1].numel() == want[1].numel() and bool((got[1] == want[1]).all()), what


def _arith(wah, fn, a, b, n_bits, mul=False):
    """add / subtract / multiply_columns into guarded buffers of exactly the documented sizes."""
    n = a[2]
    has = bool(a[4] or b[4])
    rows_out = n_bits + (1 if has else 0)
    flags = ((wah.BSI_EXISTS_A if a[4] else 0) | (wah.BSI_EXISTS_B if b[4] else 0))
    if mul:
        if b[3] < a[3]:  # (multiply_columns passes the narrower attribute as A)
            flags = ((wah.BSI_EXISTS_A if b[4] else 0) | (wah.BSI_EXISTS_B if a[4] else 0))
        sc = Buffers.scratch(wah.lib().wah_bsi_mul_scratch_bytes(n, min(a[3], b[3]), n_bits, flags))
    else:
        sc = Buffers.scratch(wah.lib().wah_bsi_arith_scratch_bytes(n, n_bits, flags))
    bufs = Buffers()
    out = bufs.words(wah.max_compressed_words(rows_out * n))
    offs = bufs.longs(rows_out * (n // SEG_WORDS) + 1)
    got = fn(wah, a, b, n_bits=n_bits, scratch=sc, out=out, out_offsets=offs)
    assert bufs.kept() and got[2:] == (n, n_bits, has)
    return got


def computed(wah, t):
    """s = a + b, p = a * b at the default width and at 8 bits, d = c - p."""
    C = wah.columns
    s = _arith(wah, C.add_columns, t["a"], t["b"], T.S_BITS)
    p = _arith(wah, C.multiply_columns, t["a"], t["b"], T.P_BITS, mul=True)
    p8 = _arith(wah, C.multiply_columns, t["a"], t["b"], T.P8_BITS, mul=True)
    d = _arith(wah, C.subtract_columns, t["c"], p, T.D_BITS)
    assert C.add_columns(wah, t["a"], t["b"])[3] == T.S_BITS and C.multiply_columns(wah, t["a"], t["b"])[3] == T.P_BITS  # the default widths
    assert C.subtract_columns(wah, t["c"], p)[3] == T.D_BITS
    return {"s": s, "p": p, "p8": p8, "d": d}


def queries(wah, t, rows):
    """The battery of T.battery on the device table t (name -> index tuple) of `rows` rows: the same names, the same types."""
    import torch

    C = wah.columns
    n = t["g"][2]
    assert all(ix[2] == n for ix in t.values())
    lo, hi = T.bounds()
    gs, go, _ = t["g"]
    hs, ho, _ = t["h"]
    all_g, all_h = list(range(T.N_G)), list(range(T.N_H))
    bufs, segs = Buffers(), n // SEG_WORDS

    def bitmap(scratch_bytes):
        return dict(scratch=Buffers.scratch(scratch_bytes), out=bufs.words(wah.max_compressed_words(n)), out_offsets=bufs.longs(segs + 1))

    in_range = C.range_column(wah, t["a"], lo, hi, **bitmap(wah.lib().wah_bsi_range_scratch_bytes(n, T.BITS["a"])))
    preds = [(gs, go, list(T.W_G), False), (hs, ho, list(T.W_NOT_H), True), (in_range[0], in_range[1], [0], False)]
    w = C.filter_columns(wah, preds, n, **bitmap(wah.lib().wah_bitop_clauses_scratch_bytes(n, 4, 3)))
    negated = [(w[0], w[1], [0], True)]
    not_w = C.filter_columns(wah, negated, n, **bitmap(wah.lib().wah_bitop_clauses_scratch_bytes(n, 1, 1)))
    assert bufs.kept()
    masks = {"W": w, None: None, "NOT W": not_w}
    comp = computed(wah, t)
    out = {}
    # 1
    out["count g"] = _np(C.count_columns(wah, gs, go, n, all_g))
    out["count h"] = _np(C.count_columns(wah, hs, ho, n, all_h))
    out["crosstab g x h"] = _np(C.crosstab_columns(wah, (gs, go, all_g), (hs, ho, all_h), n))
    out["count g where W"] = _np(C.count_columns_where(wah, preds, gs, go, n, all_g))
    out["count h where W"] = _np(C.count_columns_where(wah, preds, hs, ho, n, all_h))
    # 2
    listed, total = C.select_rows(wah, preds, n)
    out["rows W"] = (_np(listed), total)
    for first, limit in T.windows(total):
        got, matching = C.select_rows(wah, preds, n, first=first, limit=limit)
        out[f"rows W [{first}, +{limit})"] = (_np(got), matching)
    got, matching = C.select_rows(wah, negated, n)
    out["rows NOT W"] = (_np(got), matching)
    # 3
    for const in (T.c_constant(), 0, (1 << T.BITS["c"]) - 1):
        for op in T.CMP_OPS:
            out[f"c {op} {const}"] = _np(wah.positions_device(*C.compare_column(wah, t["c"], op, const), n)[0])
    # 4
    for op in ("<", "==", ">="):
        out[f"a {op} b"] = _np(wah.positions_device(*C.compare_columns(wah, t["a"], op, t["b"]), n)[0])
    out["c != p"] = _np(wah.positions_device(*C.compare_columns(wah, t["c"], "!=", comp["p"]), n)[0])
    # 5
    every = torch.arange(32 * n, dtype=torch.int64, device="cuda:0")
    for name in ("s", "p", "p8", "d"):
        values, have = C.values_at_rows(wah, comp[name], every)
        out[f"values of {name}"] = (_np(values), _np(have))
    # 6
    out["sum d where W"] = C.sum_column_where(wah, comp["d"], *w)
    out["sum a * b where W"] = C.sum_product_where(wah, t["a"], t["b"], *w)
    out["sum b where NOT W"] = C.sum_column_where(wah, t["b"], *not_w)
    # 7
    for label, attr, mask in T.STATS:
        bsi, m = t[attr], masks[mask]
        out[f"min {label}"] = tuple(C.min_column_where(wah, bsi, m))
        out[f"max {label}"] = tuple(C.max_column_where(wah, bsi, m))
        out[f"median {label}"] = tuple(C.median_column_where(wah, bsi, m))
        out[f"99/100 {label}"] = tuple(C.quantile_column_where(wah, bsi, 99, 100, m))
        out[f"0th {label}"] = tuple(C.kth_column_where(wah, bsi, 0, m))
        out[f"0th largest {label}"] = tuple(C.kth_column_where(wah, bsi, 0, m, largest=True))
        selected = out[f"min {label}"][1]
        out[f"last {label}"] = tuple(C.kth_column_where(wah, bsi, max(selected - 1, 0), m))
        out[f"one past the last {label}"] = tuple(C.kth_column_where(wah, bsi, selected, m))
    # 8
    for mask in ("W", None):
        for largest in (True, False):
            out[f"top 10 of c, {'largest' if largest else 'smallest'}, {mask}"] = _np(C.top_rows(wah, t["c"], 10, masks[mask], largest=largest))
    more = out["min c where W"][1] + 7
    for largest in (True, False):
        out[f"top of c, more than there are, {'largest' if largest else 'smallest'}"] = _np(C.top_rows(wah, t["c"], more, w, largest=largest))
    # 9
    keys = [(gs, go, all_g), (hs, ho, all_h)]
    attrs = [("a", t["a"]), ("b", t["b"]), ("d", comp["d"])]
    n_groups = T.N_G * T.N_H
    operands = sum(ix[3] + (1 if ix[4] else 0) for _, ix in attrs)
    n_attrs = sum(2 if ix[4] else 1 for _, ix in attrs)
    for mask in ("W", None):
        bufs = Buffers()
        reuse = dict(scratch=Buffers.scratch(wah.lib().wah_select_scratch_bytes(n, operands)), group_rows=bufs.longs(n_groups),
                     counts=bufs.longs(n_groups * operands).view(n_groups, operands), sums=bufs.longs(n_groups * n_attrs * 2).view(n_groups, n_attrs, 2))
        got = C.aggregate_columns(wah, keys, [ix for _, ix in attrs], n, where=masks[mask], **reuse)
        assert bufs.kept()
        out[f"group by g, h: rows, {mask}"] = _np(got["rows"])
        for i, (name, _) in enumerate(attrs):
            out[f"group by g, h: sum {name}, {mask}"] = got["sums"][i]
            out[f"group by g, h: count {name}, {mask}"] = _np(got["counts"][i])
    # 10
    for name, bsi in (("c", t["c"]), ("d", comp["d"])):
        got = C.quantiles_by(wah, [(gs, go, all_g)], bsi, n, list(T.QUANTILES), where=w)
        out[f"quantiles of {name} by g: values"] = got["values"]
        for part in ("totals", "less", "equal"):
            out[f"quantiles of {name} by g: {part}"] = _np(got[part])
        out[f"extremes of {name} by g"] = tuple(C.extremes_by(wah, [(gs, go, all_g)], bsi, n, where=w))
    # 11
    at = T.listed_rows({"n_words": n, "rows": rows})
    out["keys g at listed rows"] = _np(C.keys_at_rows(wah, t["g"], _dev(np.array(at, np.int64))))
    first, limit = T.windows(total)[1]
    picked, fetched, matching = C.select_values(wah, preds, n, [t["a"], comp["d"]], first=first, limit=limit)
    out["select a, d where W"] = (_np(picked), [(_np(v), _np(e)) for v, e in fetched], matching)
    return out


def assert_state(wah, table, state, what):
    m = T.columns_of(state)
    cols = T.batch_of(state.ids)
    fresh = build(wah, cols, n_words=state.n_words)
    for name in fresh:
        assert_same_index(table[name], fresh[name], (what, name))
    got, want = queries(wah, table, state.rows), T.battery(m)
    assert T.differing(got, want) == [], what
    if state.rows == 0:  # the empty index: every count 0, every statistic of c None, those of b 0 with every position counted
        assert not got["count g"].any() and not got["crosstab g x h"].any() and got["rows W"][1] == 0, what
        assert got["min c"] == got["max c where W"] == got["median c"] == (None, 0), what
        assert got["min b"] == got["max b"] == got["median b"] == (0, 32 * SEG_WORDS), what


# ---- a life -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.LIVES))
def test_life(wah, name):
    """The table is made once, from the life's first state, and then only mutated; after every mutation every index is the
    from-scratch index of the model and the whole battery answers as the model does.  The empty states run the battery too:
    every count 0, every statistic of c None, those of b 0 with all 32 * 992 positions counted."""
    states = T.run(name)
    table = build(wah, T.batch_of(states[0].ids))
    assert_state(wah, table, states[0], (name, 0, states[0].mutation))
    for i in range(1, len(states)):
        before, after = states[i - 1], states[i]
        batch = build(wah, T.batch_of(after.batch)) if after.mutation[0] == "append" else None
        table = {key: mutate(wah, ix, before, after, batch and batch[key]) for key, ix in table.items()}
        assert_state(wah, table, after, (name, i, after.mutation))


# ---- computed attributes -------------------------------------------------------------------------------------------------------------
def test_computed_attributes_commute_with_the_rows(wah):
    """Life `derived`: s, p and d computed from the mutated base attributes at every state against the s, p and d of the FIRST
    state carried through the same mutations as 5-tuples -- the same compress() streams, word for word --, then s + p from the
    carried operands against the model: arithmetic on a spliced result of arithmetic."""
    import torch

    C = wah.columns
    states = T.run("derived")
    base = {k: v for k, v in build(wah, T.batch_of(states[0].ids)).items() if k in T.BITS}
    carried = computed(wah, base)
    for i in range(1, len(states)):
        before, after = states[i - 1], states[i]
        batch = batch_computed = None
        if after.mutation[0] == "append":
            batch = {k: v for k, v in build(wah, T.batch_of(after.batch)).items() if k in T.BITS}
            batch_computed = computed(wah, batch)
        base = {k: mutate(wah, ix, before, after, batch and batch[k]) for k, ix in base.items()}
        carried = {k: mutate(wah, ix, before, after, batch_computed and batch_computed[k]) for k, ix in carried.items()}
        fresh = computed(wah, base)
        for k in fresh:
            assert_same_index(carried[k], fresh[k], ("derived", i, after.mutation, k))
        both = C.add_columns(wah, carried["s"], carried["p"])
        assert both[2:] == (after.n_words, T.P_BITS + 1, True)
        values, have = C.values_at_rows(wah, both, torch.arange(32 * after.n_words, dtype=torch.int64, device="cuda:0"))
        want = T.computed(T.columns_of(after))
        assert np.array_equal(_np(have), want["s"][1]) and np.array_equal(_np(values), np.where(want["s"][1], want["s"][0] + want["p"][0], 0)), i


# ---- a chain with nothing read back --------------------------------------------------------------------------------------------------
def _chain_columns(ids):
    u = T.universe()
    return {k: _dev(u[k][ids]) for k in ("g", "h", "a", "b", "ea")}


def test_a_chain_with_nothing_read_back(wah):
    """build -> multiply -> range -> clause -> masked count and grouped sum, every stage with check=False and every output passed
    on as the whole buffer it came in: a stream whose length is a capacity, an index that _index_columns divides by the column
    length.  The statuses are read after the last stage is enqueued (of the stages whose front end takes the scratch; the two
    builders keep theirs), and the answers are those of the check=True chain and of the model."""
    import torch

    C, lib = wah.columns, wah.lib()
    ids = np.arange(T.CHAIN_ROWS)
    d = _chain_columns(ids)
    n = T.n_words_of(ids.size)
    segs = n // SEG_WORDS
    ka, kb, kp = T.BITS["b"], T.BITS["a"], T.P_BITS  # (the narrower attribute is the product's A)
    flags = wah.BSI_EXISTS_B
    all_h = torch.arange(T.N_H, dtype=torch.int64, device="cuda:0")

    def chain(check):
        bufs, sc = Buffers(), {}
        a = C.bsi_from_values(wah, d["a"], T.BITS["a"], exists=d["ea"], check=check)
        b = C.bsi_from_values(wah, d["b"], T.BITS["b"], check=check)
        g = C.index_from_keys(wah, d["g"], T.N_G, check=check)
        h = C.index_from_keys(wah, d["h"], T.N_H, check=check)
        assert a[0].numel() == wah.max_compressed_words(13 * n) or check  # the whole buffer
        sc["mul"] = Buffers.scratch(lib.wah_bsi_mul_scratch_bytes(n, ka, kp, flags))
        p = C.multiply_columns(wah, a, b, check=check, scratch=sc["mul"], out=bufs.words(wah.max_compressed_words((kp + 1) * n)),
                               out_offsets=bufs.longs((kp + 1) * segs + 1))
        sc["range"] = Buffers.scratch(lib.wah_bsi_range_scratch_bytes(n, kp))
        r = C.range_column(wah, p, *T.P_RANGE, check=check, scratch=sc["range"], out=bufs.words(wah.max_compressed_words(n)), out_offsets=bufs.longs(segs + 1))
        sc["clause"] = Buffers.scratch(lib.wah_bitop_clauses_scratch_bytes(n, 3, 2))
        f = C.filter_columns(wah, [(r[0], r[-1], [0], False), (g[0], g[1], list(T.W_G), False)], n, check=check, scratch=sc["clause"],
                             out=bufs.words(wah.max_compressed_words(n)), out_offsets=bufs.longs(segs + 1))
        sc["inner"] = Buffers.scratch(lib.wah_bitop_clauses_scratch_bytes(n, 1, 1))
        sc["count"] = Buffers.scratch(lib.wah_select_scratch_bytes(n, T.N_H))
        counts = C.count_columns_where(wah, [(f[0], f[-1], torch.zeros(1, dtype=torch.int64, device="cuda:0"), False)], h[0], h[1], n, all_h,
                                       check=check, scratch=sc["count"], counts=bufs.longs(T.N_H).view(1, T.N_H), filter=dict(scratch=sc["inner"]))
        sc["sum"] = Buffers.scratch(lib.wah_select_scratch_bytes(n, kp + 1))
        agg = C.aggregate_columns(wah, [(h[0], h[1], all_h)], [p], n, where=(f[0], f[-1]), check=check, scratch=sc["sum"])
        # every stage is enqueued (aggregate_columns read its sums at its end): now the statuses
        status = {"mul": lib.wah_bsi_mul_status(sc["mul"].data_ptr(), n, ka, kp, flags, None),
                  "range": lib.wah_bsi_range_status(sc["range"].data_ptr(), n, kp, None),
                  "clause": lib.wah_bitop_clauses_status(sc["clause"].data_ptr(), n, 3, 2, None),
                  "inner": lib.wah_bitop_clauses_status(sc["inner"].data_ptr(), n, 1, 1, None),
                  "count": lib.wah_select_status(sc["count"].data_ptr(), None), "sum": lib.wah_select_status(sc["sum"].data_ptr(), None)}
        assert all(rc == WAH_OK for rc in status.values()), status
        assert bufs.kept()
        return {"counts": _np(counts), "rows": _np(agg["rows"]), "sum p": agg["sums"][0], "count p": _np(agg["counts"][0])}

    loose, checked, want = chain(False), chain(True), T.chain_answers(ids, ids)
    assert want["counts"].min() > 0 and T.differing(loose, want) == [] and T.differing(checked, want) == []


def test_the_chain_replays_as_one_graph(wah):
    """The same chain from the device calls -- bsi_build twice, bsi_mul, bsi_range, bitop_clauses, count_masked --, captured ONCE
    (as tests/test_gpu_bsi_build.py: side stream, warm-up outside, check=False; one chain of launches, no parallel branches) over
    fixed scratch, out, out_offsets and tables made before the capture from the fixed buffers' addresses, and replayed after the
    value tensors were overwritten in place with three other stretches of the universe, one of them constant: the stream sizes
    change a lot between replays.  Every output is refilled with 0x5A5A5A5A before each replay."""
    import torch

    C, lib = wah.columns, wah.lib()
    stretches = T.chain_stretches()
    key_ids = stretches[0]
    n = T.n_words_of(T.CHAIN_ROWS)
    segs = n // SEG_WORDS
    bits_a, bits_b, kp = T.BITS["a"], T.BITS["b"], T.P_BITS
    flags = wah.BSI_EXISTS_B  # the product's A is b, the narrower attribute, which has no existence bitmap; its B is a
    u = T.universe()
    d_a, d_b, d_ea = (_dev(u[k][key_ids].copy()) for k in ("a", "b", "ea"))
    g = C.index_from_keys(wah, _dev(u["g"][key_ids]), T.N_G)
    h = C.index_from_keys(wah, _dev(u["h"][key_ids]), T.N_H)
    bufs = Buffers()
    out = {"a": bufs.words(wah.max_compressed_words((bits_a + 1) * n)), "b": bufs.words(wah.max_compressed_words(bits_b * n)),
           "p": bufs.words(wah.max_compressed_words((kp + 1) * n)), "r": bufs.words(wah.max_compressed_words(n)), "f": bufs.words(wah.max_compressed_words(n))}
    offs = {"a": bufs.longs((bits_a + 1) * segs + 1), "b": bufs.longs(bits_b * segs + 1), "p": bufs.longs((kp + 1) * segs + 1),
            "r": bufs.longs(segs + 1), "f": bufs.longs(segs + 1)}
    counts = bufs.longs(T.N_H).view(1, T.N_H)
    sc = {"a": Buffers.scratch(lib.wah_bsi_build_scratch_bytes(n, bits_a + 1)), "b": Buffers.scratch(lib.wah_bsi_build_scratch_bytes(n, bits_b)),
          "p": Buffers.scratch(lib.wah_bsi_mul_scratch_bytes(n, bits_b, kp, flags)), "r": Buffers.scratch(lib.wah_bsi_range_scratch_bytes(n, kp)),
          "f": Buffers.scratch(lib.wah_bitop_clauses_scratch_bytes(n, 3, 2)), "c": Buffers.scratch(lib.wah_select_scratch_bytes(n, T.N_H))}
    # the tables, from the fixed buffers' addresses: a stream's length is its buffer's capacity
    bsi_a, bsi_b = (out["a"], offs["a"], n, bits_a, True), (out["b"], offs["b"], n, bits_b, False)
    mul_table = C._two_attribute_table(wah.bsi_mul_row_order(bits_b, bits_a, False, True), bsi_b, bsi_a)
    range_table = C.column_operand_table(out["p"], offs["p"], n, list(range(kp + 1)))
    bounds = wah.bsi_bounds(*T.P_RANGE, "cuda:0")
    clause_table = torch.cat([C.column_operand_table(out["r"], offs["r"], n, [0]), C.column_operand_table(g[0], g[1], n, list(T.W_G))])
    clause_ends = torch.tensor([1, 3], dtype=torch.int64, device="cuda:0")
    mask = C.column_operand_table(out["f"], offs["f"], n, [0])
    h_table = C.column_operand_table(h[0], h[1], n, list(range(T.N_H)))

    def enqueue():
        wah.bsi_build_device(d_a, bits_a, n, exists=d_ea, scratch=sc["a"], out=out["a"], out_offsets=offs["a"], check=False)
        wah.bsi_build_device(d_b, bits_b, n, scratch=sc["b"], out=out["b"], out_offsets=offs["b"], check=False)
        wah.bsi_mul_device(mul_table, bits_b, bits_a, kp, n, exists_a=False, exists_b=True, scratch=sc["p"], out=out["p"], out_offsets=offs["p"], check=False)
        wah.bsi_range_device(range_table, bounds, n, exists=True, scratch=sc["r"], out=out["r"], out_offsets=offs["r"], check=False)
        wah.bitop_clauses_indexed_device((clause_table, clause_ends), n, scratch=sc["f"], out=out["f"], out_offsets=offs["f"], check=False)
        wah.count_masked_device(mask, h_table, n, scratch=sc["c"], counts=counts, check=False)

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
        status = [lib.wah_bsi_build_status(sc["a"].data_ptr(), n, bits_a + 1, None), lib.wah_bsi_build_status(sc["b"].data_ptr(), n, bits_b, None),
                  lib.wah_bsi_mul_status(sc["p"].data_ptr(), n, bits_b, kp, flags, None), lib.wah_bsi_range_status(sc["r"].data_ptr(), n, kp, None),
                  lib.wah_bitop_clauses_status(sc["f"].data_ptr(), n, 3, 2, None), lib.wah_select_status(sc["c"].data_ptr(), None)]
        assert status == [WAH_OK] * 6, (i, status)
        assert bufs.kept(), i
        want = T.chain_answers(key_ids, ids)["counts"]
        assert np.array_equal(_np(counts).reshape(-1), want), (i, _np(counts), want)
        sizes.add(int(offs["p"][-1].item()))
    assert len(sizes) == 4 and max(sizes) > 20 * min(sizes)  # the constant stretch's product is a few fills


# ---- mismatched column lengths -------------------------------------------------------------------------------------------------------
def test_mismatched_column_lengths_are_refused_not_misread(wah):
    """After an append has doubled the column length: an attribute of the old length beside one of the new is a ValueError of the
    front end, before any launch; a filter bitmap of the old length at the new one is an operand whose index ends in front of
    the segments the call reads -- with a Python list of columns the front end refuses it, with a device tensor of columns the
    device does: the entry behind the index is no range inside the stream, which include/wah.h makes WAH_ERR_STREAM of the
    call's status.  Never a count."""
    import torch

    C = wah.columns
    states = T.run("derived")
    old_state, new_state = states[0], states[2]
    assert old_state.n_words == SEG_WORDS and new_state.n_words == 2 * SEG_WORDS
    old = build(wah, T.batch_of(old_state.ids))
    new = build(wah, T.batch_of(new_state.ids))
    n = new_state.n_words
    keys = [(new["g"][0], new["g"][1], list(range(T.N_G)))]
    bufs = Buffers()  # what a launch would have written into: still the sentinel after every refusal
    operands = T.BITS["a"] + 1 + T.BITS["b"]
    with pytest.raises(ValueError):
        C.aggregate_columns(wah, keys, [new["a"], old["b"]], n, group_rows=bufs.longs(T.N_G), counts=bufs.longs(T.N_G * operands).view(T.N_G, operands),
                            sums=bufs.longs(T.N_G * 3 * 2).view(T.N_G, 3, 2))
    with pytest.raises(ValueError):
        C.compare_columns(wah, new["a"], "<", old["b"], out=bufs.words(wah.max_compressed_words(n)), out_offsets=bufs.longs(n // SEG_WORDS + 1))
    for fn, a, b in ((C.add_columns, old["a"], new["b"]), (C.subtract_columns, new["c"], old["a"]), (C.multiply_columns, new["a"], old["b"])):
        with pytest.raises(ValueError):
            fn(wah, a, b, out=bufs.words(wah.max_compressed_words(64 * n)), out_offsets=bufs.longs(64 * (n // SEG_WORDS) + 1))
    assert bufs.untouched()
    with pytest.raises(ValueError):
        C.append_rows(wah, new["g"], new_state.rows, new["a"], 1)      # a 3-tuple and a 5-tuple
    u = T.universe()
    wide = C.bsi_from_values(wah, _dev(u["a"][new_state.ids]), T.BITS["a"] + 1)   # 13 slices: as many columns as a's 12 and its existence bitmap
    assert C._index_columns(wide[1], wide[2]) == C._index_columns(new["a"][1], new["a"][2])
    with pytest.raises(ValueError):
        C.append_rows(wah, new["a"], new_state.rows, wide, 1)         # another n_bits
    # the stale filter: its index, with the guard behind it, is read one entry too far
    lo, hi = T.bounds()
    bufs = Buffers()
    stale = C.range_column(wah, old["a"], lo, hi, out_offsets=bufs.longs(2))
    assert stale[1].numel() == 2 and wah.count_device([stale], SEG_WORDS).item() > 0
    gs, go, _ = new["g"]
    with pytest.raises(ValueError):
        C.count_columns_where(wah, [(stale[0], stale[1], [0], False)], gs, go, n, list(range(T.N_G)))
    column = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    with pytest.raises(wah.WahError, match=r"the filter failed \(code -6\)"):
        C.count_columns_where(wah, [(stale[0], stale[1], column, False)], gs, go, n, list(range(T.N_G)))
    assert bufs.kept()
    fresh = C.range_column(wah, new["a"], lo, hi)  # ... and the filter of the new length counts
    got = C.count_columns_where(wah, [(fresh[0], fresh[1], column, False)], gs, go, n, list(range(T.N_G)))
    m = T.columns_of(new_state)
    in_range = m["ea"] & (m["a"] >= lo) & (m["a"] <= hi)
    assert _np(got).tolist() == [int(np.count_nonzero(in_range & (m["g"] == v))) for v in range(T.N_G)]
