"""A table's second life: DELETE, UPDATE and re-clustering by predicate, and the newer queries.  The model, the lives and the
second battery that tests/test_gpu_table_dml.py holds the device index against after every mutation.  numpy only; the universe,
the padded model and the exact comparison are those of tests/_table.py.  tests/test_table_dml_reference.py proves on the CPU
that the lives reach the sizes they name, that their masks hold every kind of word, that the second battery's answers are not
trivial, and that eight plausible composition errors (WRONG: run(name, wrong), battery_dml(m, wrong)) each change an answer or
a state.

A state is still the int64 array of the universe rows the table holds, in order.  New here: the rows need not ascend (an update
replaces a row by another universe row, a clustering permutes them), and a state carries the column length the library's front
end gives its result, which after a compaction sized by an upper bound is longer than the rows need:
  delete_where(pred, sizing)  without the rows pred selects                       columns.delete_rows
  keep_where(pred, sizing)    the rows pred selects                               columns.keep_rows
      sizing "exact": n_rows_out=None, max(1, ceil(rows / 31744)) segments; "bound": n_rows_out=the rows before, rounded up
  update_from(pred, shift)    a selected row becomes universe row (id + shift) % N  columns.update_rows; the column length stays
  cluster(key)                the rows in the stable order of the key             columns.reorder_rows; the default length
  append(k), trim(f, b)       as in _table.py; trim: without f rows in front and b behind   append_rows, slice_rows
A predicate is a mask over ALL 32 * n_words positions of the padded model; n_rows cuts it off at the table's rows."""
import numpy as np

from tests import _table as T
from tests._table import columns_of, computed, differing, same, universe, where_mask  # noqa: F401  (the shared model)

SEG, N = T.SEG, T.N
C_TOP = (1 << T.BITS["c"]) - 1
DROP = MAP_NULL = 0xFFFFFFFF  # columns.GROUP_BY_DROP, columns.MAP_NULL

LIVES = {
    # three segments to two by an exact delete, a bound-sized delete and keep, the identity, the empty table, one row again
    "purge": [("start", 2 * SEG + 700), ("delete", "a absent", "exact"), ("delete", "c top", "bound"), ("append", 33),
              ("keep", "W", "bound"), ("delete", "none", "exact"), ("delete", "W", "exact"), ("delete", "all", "exact"), ("append", 1)],
    # updates under a mask, its negation, nothing and everything; a delete that lands in one segment; an update, then a window
    "amend": [("start", SEG + 6000), ("update", "W", 50_000), ("update", "NOT W", 20_000), ("update", "none", 1), ("update", "all", 70_000),
              ("delete", "W", "exact"), ("update", "a absent", 3), ("trim", 31, 32)],
    # re-clustered by a key and by a mapped attribute, appended to, compacted with a bound and clustered again
    "cluster": [("start", SEG - 1), ("cluster", "g"), ("append", SEG + 2), ("cluster", "k"), ("delete", "W", "bound"), ("cluster", "g"),
                ("keep", "a absent", "exact")],
}
# the short life that carries derived attributes: a delete that lands in one segment, then an update under a negated mask
CARRIED = (("start", SEG + 6000), ("delete", "a absent", "exact"), ("update", "NOT W", 20_000))
NEGATED = ("NOT W", "a absent", "all")  # the predicates that select positions behind the table
WRONG = ("a bound-sized result takes the exact length", "update takes the source's row by rank, not by number",
         "update leaves the existence bits", "rows behind n_rows survive a delete under a negated mask",
         "division by zero is 0 and exists", "a partition starts only at a selected row",
         "a running sum counts rows without a value", "cluster is not stable")
WRONG_APPLIES = {  # the lives in which the error can show at all
    "a bound-sized result takes the exact length": ("purge", "cluster"),          # a bound-sized step that loses a segment's worth of rows
    "update takes the source's row by rank, not by number": ("amend",),
    "update leaves the existence bits": ("amend",),
    "rows behind n_rows survive a delete under a negated mask": ("purge", "amend", "cluster"),  # a compaction whose selection holds the padding
    "division by zero is 0 and exists": ("purge", "amend", "cluster"),
    "a partition starts only at a selected row": ("purge", "amend", "cluster"),
    "a running sum counts rows without a value": ("purge", "amend", "cluster"),
    "cluster is not stable": ("cluster",),
}


class State(T.State):
    """T.State with the column length the front end gave (None: the default, the rows rounded up to whole segments) and, for
    the one wrong model that needs it, the universe rows the existence bits were left from."""

    def __init__(self, ids, mutation, n_words=None, batch=None, exists_from=None):
        super().__init__(ids, mutation, batch=batch)
        self.given_n_words = n_words
        self.exists_from = exists_from

    @property
    def n_words(self):
        return T.n_words_of(self.rows) if self.given_n_words is None else self.given_n_words


def columns(state):
    """T.columns_of at the state's own column length."""
    m = T.columns_of(state)
    if state.exists_from is not None:  # (only "update leaves the existence bits")
        u, at = T.universe(), np.arange(state.rows)
        raw = {"a": np.zeros_like(m["a"]), "c": np.zeros_like(m["c"])}
        for e, name in (("ea", "a"), ("ec", "c")):
            m[e] = np.zeros_like(m[e])
            m[e][at] = u[e][state.exists_from]
            raw[name][at] = u[name][state.ids]
            m[name] = np.where(m[e], raw[name], 0)
    return m


def predicate(m, name):
    """The mask of a predicate over every position of the padded model."""
    size = 32 * m["n_words"]
    if name == "W":
        return T.where_mask(m)
    if name == "NOT W":
        return ~T.where_mask(m)
    if name == "c top":
        return m["ec"] & (m["c"] == C_TOP)
    if name == "a absent":
        return ~m["ea"]
    if name == "all":
        return np.ones(size, bool)
    if name == "none":
        return np.zeros(size, bool)
    raise ValueError(name)


def cluster_key(m, key):
    """The sort key of a clustering over the table's rows: the key g, or k = b >> 6 as section F maps it."""
    return (m["g"] if key == "g" else m["b"] >> 6)[: m["rows"]]


def run(name, wrong=None):
    """The states of a life (its name, or its steps), the first one included.  wrong: one of WRONG that concerns a mutation."""
    steps = LIVES[name] if isinstance(name, str) else list(name)
    assert steps[0][0] == "start"
    states = [State(np.arange(steps[0][1]), steps[0])]
    cursor = steps[0][1]
    for step in steps[1:]:
        before = states[-1]
        ids, kind = before.ids, step[0]
        m = columns(before)
        exists_from = before.exists_from
        if kind == "append":
            batch = np.arange(cursor, cursor + step[1])
            cursor += step[1]
            if exists_from is not None:
                exists_from = np.concatenate([exists_from, batch])
            states.append(State(np.concatenate([ids, batch]), step, batch=batch, exists_from=exists_from))
        elif kind == "trim":
            first, n = step[1], ids.size - step[1] - step[2]
            assert 0 <= first and n >= 0
            states.append(State(ids[first: first + n], step, exists_from=None if exists_from is None else exists_from[first: first + n]))
        elif kind in ("delete", "keep"):
            mask = predicate(m, step[1])
            selected = mask if kind == "keep" else ~mask
            if wrong == "rows behind n_rows survive a delete under a negated mask":
                padded = np.concatenate([ids, np.full(selected.size - ids.size, -1)])
                after = padded[selected]
            else:
                after = ids[selected[: ids.size]]
            exact = step[2] == "exact" or wrong == "a bound-sized result takes the exact length"
            states.append(State(after, step, n_words=T.n_words_of(max(after.size, 0 if exact else ids.size)),
                                exists_from=None if exists_from is None else exists_from[selected[: ids.size]]))
        elif kind == "update":
            mask = predicate(m, step[1])[: ids.size]
            source = np.where(ids >= 0, (ids + step[2]) % N, -1)
            if wrong == "update takes the source's row by rank, not by number":
                after = ids.copy()
                after[mask] = source[: np.count_nonzero(mask)]
            else:
                after = np.where(mask, source, ids)
            if wrong == "update leaves the existence bits":
                exists_from = ids if exists_from is None else exists_from
            elif exists_from is not None:
                exists_from = np.where(mask, source, exists_from)
            states.append(State(after, step, n_words=before.n_words, exists_from=exists_from))
        elif kind == "cluster":
            key = cluster_key(m, step[1])
            order = np.argsort(key, kind="stable")
            if wrong == "cluster is not stable":  # equal keys in descending row order
                order = np.lexsort((-np.arange(key.size), key))
            states.append(State(ids[order], step, exists_from=None if exists_from is None else exists_from[order]))
        else:
            raise ValueError(kind)
    return states


def masks_used(states):
    """(state before, predicate name) of every mutation that takes a mask."""
    return [(before, after.mutation[1]) for before, after in zip(states, states[1:]) if after.mutation[0] in ("delete", "keep", "update")]


# ---- the second battery ------------------------------------------------------------------------------------------------------------
ABSENT_C = 123_457  # a value of c that no universe row holds (the reference test proves it)
MEMBER_SETS = (("some", (C_TOP, 0, ABSENT_C, 1 << 21, C_TOP)), ("none", ()))
B_BUCKETS = 1 << T.BITS["b"]
A_LOOKUP_SIZE, A_BUCKETS = 4000, 16  # the lookup of the second grouping ends in front of a's largest keys
MP_BITS, K_BITS = 10, 3
CS_BITS = 16  # the width of the exclusive running sum: narrower than the sum, which is stored mod 2^16
RANGE_ON_SUM = (1 << 20, 1 << 22)
PARTITION_BOUND = 3000
KTH = 5


def a_lookup():
    """key a -> v >> 8, every 101st entry dropped; keys at or behind the lookup's end go to "other" too."""
    v = np.arange(A_LOOKUP_SIZE, dtype=np.int64)
    return np.where(v % 101 == 7, DROP, v >> 8)


def mp_lookup():
    """key b -> (37 v + 5) & 1023, every 17th entry without a value."""
    v = np.arange(B_BUCKETS, dtype=np.int64)
    return np.where(v % 17 == 0, MAP_NULL, (37 * v + 5) & 1023)


def k_lookup():
    return np.arange(B_BUCKETS, dtype=np.int64) >> 6


def read_windows(m):
    """(first, n) of section H: the whole column, [31, 33), across row SEG where the table has one, the last row, none."""
    size, rows = 32 * m["n_words"], m["rows"]
    out = [(0, size), (31, 2)]
    if rows > SEG:
        out.append((SEG - 3, 7))
    if rows:
        out.append((rows - 1, 1))
    return out + [(5, 0)]


def _padded(values, size, dtype=np.int64):
    out = np.zeros(size, dtype)
    out[: values.size] = values
    return out


def _parts(starts, vals, selected):
    """Per row of the table: the inclusive and the exclusive running sum of vals over the selected rows of its partition, and
    the partition's total.  starts: bool per row (row 0 needs no bit)."""
    rows = vals.size
    if rows == 0:
        z = np.zeros(0, np.int64)
        return z, z, z
    v = np.where(selected, vals, 0).astype(np.int64)
    begins = starts.copy()
    begins[0] = True
    first = np.flatnonzero(begins)
    pid = np.cumsum(begins) - 1
    cs = np.cumsum(v)
    base = np.concatenate([[0], cs[first[1:] - 1]])
    incl = cs - base[pid]
    return incl, incl - v, np.add.reduceat(v, first)[pid]


def _grouped(bucket, n_buckets, selected, attrs):
    """(rows, [sums], [counts], other) of a GROUP BY: bucket per position (n_buckets: "other"), attrs: (values, have or None)."""
    b = bucket[selected]
    rows = np.bincount(b, minlength=n_buckets + 1)
    sums, counts = [], []
    for values, have in attrs:
        s = np.zeros(n_buckets + 1, np.int64)
        np.add.at(s, b, values[selected])
        sums.append(s)
        counts.append(rows if have is None else np.bincount(bucket[selected & have], minlength=n_buckets + 1))
    other = (int(rows[-1]), [int(s[-1]) for s in sums], [int(c[-1]) for c in counts])
    return (rows[:-1].astype(np.int64), [np.array([int(x) for x in s[:-1]], object) for s in sums],
            [c[:-1].astype(np.int64) for c in counts], other)


def battery_dml(m, wrong=None):
    """name -> answer of the newer queries, on the padded model, with the types of T.battery: row lists and counts int64
    arrays, sums Python ints (object arrays of them), an attribute read at every position (values, have or None)."""
    size, rows = 32 * m["n_words"], m["rows"]
    table = np.arange(size) < rows
    w = T.where_mask(m)
    ea, ec = m["ea"], m["ec"]
    a, b, c, g = m["a"], m["b"], m["c"], m["g"]
    comp = T.computed(m)
    d, d_have = comp["d"]
    out = {}
    # A. membership
    for label, members in MEMBER_SETS:
        inside = np.isin(c, np.array(members, np.int64))
        out[f"c in {label}"] = np.flatnonzero(ec & inside)
        out[f"c not in {label}"] = np.flatnonzero(ec & ~inside)
    # B. GROUP BY a bit-sliced key
    rows_b, sums_b, counts_b, other_b = _grouped(b, B_BUCKETS, table & w, [(a, ea), (d, d_have)])
    out["group by b where W: rows"], out["group by b where W: other"] = rows_b, other_b
    for t, name in enumerate(("a", "d")):
        out[f"group by b where W: sum {name}"], out[f"group by b where W: count {name}"] = sums_b[t], counts_b[t]
    lookup = a_lookup()
    bucket = np.full(size, A_BUCKETS, np.int64)
    inside = a < A_LOOKUP_SIZE
    bucket[inside] = np.minimum(lookup[a[inside]], A_BUCKETS)
    rows_a, sums_a, counts_a, other_a = _grouped(bucket, A_BUCKETS, table & ea, [(a, ea), (d, d_have)])
    out["group by a >> 8: rows"], out["group by a >> 8: other"] = rows_a, other_a
    for t, name in enumerate(("a", "d")):
        out[f"group by a >> 8: sum {name}"], out[f"group by a >> 8: count {name}"] = sums_a[t], counts_a[t]
    # C. mapped attributes
    entry = mp_lookup()[b]
    mp_have = table & (entry != MAP_NULL)
    mp = np.where(mp_have, entry, 0)
    out["values of mp"] = (mp, mp_have)
    k = np.where(table, b >> 6, 0)
    out["values of k"] = (k, None)
    # D. division
    q_have = ec & (b != 0)
    if wrong == "division by zero is 0 and exists":
        q_have = ec
    safe = np.where(b != 0, b, 1)
    q, r = np.where(q_have & (b != 0), c // safe, 0), np.where(q_have & (b != 0), c % safe, 0)
    out["values of q"], out["values of r"] = (q, q_have), (r, q_have)
    out["values of d / 1000"] = (np.where(d_have, d // 1000, 0), d_have)
    back = (q * b + r) & ((1 << 30) - 1)
    out["c != q * b + r"] = np.flatnonzero(q_have & (c != back))
    out["c == q * b + r"] = np.flatnonzero(q_have & (c == back))
    out["sum q where W"] = int(q[w].sum())
    # E. running totals
    counted = table & w  # (W holds a's existence bitmap: the selection under W is W itself)
    cs =_padded(np.cumsum(np.where(counted, a, 0)[:rows]), size)
    cs_bits = T.BITS["a"] + int(rows).bit_length()
    out["cumsum a where W"] = (np.where(counted, cs & ((1 << cs_bits) - 1), 0), counted)
    out["cumsum a where W, exclusive, all rows"] = (np.where(table, (cs - np.where(counted, a, 0)) & ((1 << CS_BITS) - 1), 0), None)
    sel = table & w
    number = _padded(np.cumsum(sel[:rows]), size)
    out["row numbers where W"] = (np.where(sel, number, 0), sel)
    out["row numbers where W, exclusive, all rows"] = (np.where(table, number - sel, 0), None)
    # F. partitions of k
    starts = np.zeros(size, bool)
    if rows > 1:
        starts[1:rows] = k[1:rows] != k[: rows - 1]
    starts[rows:] |= k[rows:] != 0 if rows else False
    out["partition starts"] = np.flatnonzero(starts)
    seen = starts & counted if wrong == "a partition starts only at a selected row" else starts
    incl, _, total = (_padded(x, size) for x in _parts(seen[:rows], a[:rows], counted[:rows]))
    out["cumsum a by k where W"] = (np.where(counted, incl, 0), counted)
    out["total a by k where W"] = (np.where(counted, total, 0), counted)
    out["total a by k where W, all rows"] = (np.where(table, total, 0), None)
    every = table & ea if wrong != "a running sum counts rows without a value" else table
    out["total a"] = (np.where(every, int(a[every].sum()), 0), every)
    numbers = _padded(_parts(starts[:rows], np.ones(rows, np.int64), np.ones(rows, bool))[0], size)
    out["row numbers by k"] = (numbers, table.copy())
    sizes = _padded(_parts(seen[:rows], np.ones(rows, np.int64), sel[:rows])[2], size)
    out["partition sizes where W, all rows"] = (sizes, None)
    seen_every = starts & every if wrong == "a partition starts only at a selected row" else starts
    t_every = _padded(_parts(seen_every[:rows], a[:rows], every[:rows])[2], size)
    n_every = _padded(_parts(seen_every[:rows], np.ones(rows, np.int64), every[:rows])[2], size)
    out["mean a by k"] = (np.where(every, t_every // np.maximum(n_every, 1), 0), every)
    out["rows of partitions of k where sum a > bound, W"] = np.flatnonzero(counted & (total > PARTITION_BOUND))
    streak = _padded(_parts(~sel[:rows], np.ones(rows, np.int64), sel[:rows])[0], size)
    out["streak lengths of W"] = (np.where(sel, streak, 0), sel)
    out["count distinct k"] = int(np.unique(k[:rows]).size)
    # G. setters, each through a later call
    a7, ea7 = np.where(sel, 7, a), ea | sel
    out["values of a set to 7 where W"] = (a7, ea7)
    out["a set to 7 where W == 7"] = np.flatnonzero(ea7 & (a7 == 7))
    not_w = table & ~w
    a_null, ea_null = np.where(not_w, 0, a), ea & ~not_w
    out["values of a set to NULL where NOT W"] = (a_null, ea_null)
    out["min of a set to NULL where NOT W"] = T.rank_of(a_null[ea_null], 0, 1)[:2]
    out["count g with key 0 set where W"] = np.array([np.count_nonzero(np.where(sel, 0, g) == v) for v in range(T.N_G)])
    s, s_have = comp["s"]
    chosen, chosen_have = np.where(sel, s, c), np.where(sel, s_have, ec)
    out["values of CASE WHEN W THEN s ELSE c"] = (chosen, chosen_have)
    out["sum of CASE WHEN W THEN s ELSE c where W"] = int(chosen[w].sum())
    most, least = np.maximum(b, k), np.minimum(b, k)
    out["values of greatest(b, k)"], out["values of least(b, k)"] = (most, None), (least, None)
    out["greatest(b, k) > least(b, k)"] = np.flatnonzero(most > least)
    # H. whole-column read-back
    for first, n in read_windows(m):
        out[f"read c [{first}, +{n})"] = (c[first: first + n], ec[first: first + n])
        out[f"read g [{first}, +{n})"] = g[first: first + n]
    # I. into the older calls
    stored = out["cumsum a where W"][0]
    out["rows with the running sum in a range"] = np.flatnonzero(counted & (stored >= RANGE_ON_SUM[0]) & (stored <= RANGE_ON_SUM[1]))
    under = q[w & q_have]
    out["kth q where W"], out["median q where W"] = T.kth_of(under, KTH), T.rank_of(under, 1, 2)[:2]
    rows_gh = np.zeros((T.N_G, T.N_H), np.int64)
    sums_gh, counts_gh = np.empty((T.N_G, T.N_H), object), np.zeros((T.N_G, T.N_H), np.int64)
    for i in range(T.N_G):
        for j in range(T.N_H):
            grp = (g == i) & (m["h"] == j)
            rows_gh[i, j], sums_gh[i, j], counts_gh[i, j] = np.count_nonzero(grp), int(mp[grp].sum()), np.count_nonzero(grp & mp_have)
    out["group by g, h: rows"], out["group by g, h: sum mp"], out["group by g, h: count mp"] = rows_gh, sums_gh, counts_gh
    out["running sum <= total, by k"] = np.flatnonzero(counted)
    shape = (T.N_G, len(T.QUANTILES))
    values = np.empty(shape, object)
    totals, less, equal = (np.zeros(shape, np.int64) for _ in range(3))
    for i in range(T.N_G):
        v = incl[(g == i) & w & counted]
        for j, query in enumerate(T.QUANTILES):
            values[i, j], totals[i, j], less[i, j], equal[i, j] = T.rank_of(v, *T._QUANTILE.get(query, query))
    out["quantiles of the running sum by g: values"], out["quantiles of the running sum by g: totals"] = values, totals
    out["quantiles of the running sum by g: less"], out["quantiles of the running sum by g: equal"] = less, equal
    return out


# ---- the chain: clause -> row numbers -> keep b and a -> map -> partition starts -> running sum per partition -> range -> masked count
CHAIN_NOT_G, CHAIN_NOT_H = (0, 2, 4), (0,)  # two NOT IN lists: the clause selects every position behind the table too
CHAIN_RANGE = (3000, 9000)


def chain_answers(key_ids, value_ids):
    """The chain's answers for keys g, h of universe rows key_ids and values a, b of rows value_ids, both CHAIN_ROWS long: the
    rows the clause keeps (n_rows cuts the clause off at the table), and of the kept table -- as long as the BOUND says, the rows
    behind the kept ones zeros without a value -- the rows whose running sum of a within their partition of k = b >> 6 lies in
    CHAIN_RANGE, counted per slice of k, most significant first."""
    u = T.universe()
    rows = int(key_ids.size)
    size = 32 * T.n_words_of(rows)
    table = np.arange(size) < rows
    g, h = np.full(size, -1, np.int64), np.full(size, -1, np.int64)
    g[:rows], h[:rows] = u["g"][key_ids], u["h"][key_ids]
    clause = ~np.isin(g, CHAIN_NOT_G) & ~np.isin(h, CHAIN_NOT_H)
    kept = np.flatnonzero(clause & table)
    ea = u["ea"][value_ids][kept]
    a = _padded(np.where(ea, u["a"][value_ids][kept], 0), size)
    have = _padded(ea, size, bool)
    k = _padded(u["b"][value_ids][kept] >> 6, size)
    starts = np.zeros(rows, bool)
    starts[1:] = k[1:rows] != k[: rows - 1]
    running = _padded(_parts(starts, a[:rows], have[:rows])[0], size)
    hit = have & (running >= CHAIN_RANGE[0]) & (running <= CHAIN_RANGE[1])
    return {"clause": int(np.count_nonzero(clause)), "kept": kept, "counts": np.array([np.count_nonzero(hit & (((k >> (K_BITS - 1 - i)) & 1) != 0)) for i in range(K_BITS)]),
            "hit": np.flatnonzero(hit)}
