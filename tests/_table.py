"""A small table that lives: the model, the named lives and the query battery that tests/test_gpu_table_life.py holds the device
index against after every insert, window and delete.  numpy only: no torch, no GPU, no library.  tests/test_table_reference.py
proves on the CPU that the lives reach the sizes they name, that their cuts go through fills, that the battery's answers are not
trivial, and that six plausible composition errors (WRONG: run(name, wrong), battery(m, wrong)) each change an answer.

The universe is ONE seeded table of N rows; a table's state is the int64 array of the universe rows it holds, in order, so a
mutation is a pure function on such arrays and says which front end does it on the device:
  append(k)         the next k universe rows                   columns.append_rows
  drop_front(k)     without its first k rows                   columns.slice_rows
  window(first, n)  rows [first, first + n)                    columns.slice_rows
  delete(lo, hi)    without rows [lo, hi)                      columns.splice_columns with two parts
columns_of() is the padded model: every column 32 * n_words positions long, the table's rows first, and behind them no key (-1),
the value 0 and no existence -- what include/wah.h defines (the pad rule, "zeros behind them" of the splice call).  battery() is
computed on the padded columns, never on the bare rows: a negated predicate and an attribute without an existence bitmap see the
positions behind the table, and so must the reference."""
import functools

import numpy as np

SEG_WORDS = 992
SEG = 32 * SEG_WORDS  # 31 744 rows: 1024 groups of 31 bits, one segment
N = 140_000
N_G, N_H = 5, 3
BITS = {"a": 12, "b": 9, "c": 20}
HAS_EXISTS = {"a": True, "b": False, "c": True}
W_G, W_NOT_H = (1, 3), (0,)
MARGIN = 1700  # rows of a special stretch on either side of the cuts it is there for
CMP_OPS = ("<", "<=", ">", ">=", "==")


def n_words_of(rows):
    """The column length every front end defaults to: the rows rounded up to whole segments, at least one."""
    return max(-(-((rows + 31) // 32) // SEG_WORDS), 1) * SEG_WORDS


# ---- the lives ------------------------------------------------------------------------------------------------------------------
LIVES = {
    # the empty index, the word and group seams, one segment exactly, the step to two segments, three segments
    "grow": [("start", 0), ("append", 1), ("append", 30), ("append", 1), ("append", 1), ("append", SEG - 1 - 33), ("append", 1),
             ("append", 1), ("append", SEG + 4)],
    # a time-partition rollover, and the empty index again at its end
    "roll": [("start", 2 * SEG + 700), ("drop_front", 1), ("append", 32), ("drop_front", 31), ("append", 1), ("drop_front", 32),
             ("append", SEG + 1), ("drop_front", SEG), ("append", 31), ("drop_front", SEG + 1), ("append", SEG), ("window", 5, 0)],
    # deletes from the middle: inside a constant stretch, across a segment seam, from a multiple of 31 to a multiple of 32
    "edit": [("start", SEG + 6000), ("delete", 1000, 1500), ("delete", SEG - 40, SEG + 25), ("delete", 31 * 100, 32 * 110),
             ("window", 977, 34782), ("append", 1)],
    # grow from one row below a segment on: the life that carries computed attributes
    # (and a window at its end: slice_rows of a computed attribute against the computed attribute of the sliced operands)
    "derived": [("start", SEG - 1), ("append", 1), ("append", 1), ("append", SEG + 4), ("window", 31, SEG + 900)],
}
SIZES = {
    "grow": [0, 1, 31, 32, 33, SEG - 1, SEG, SEG + 1, 2 * SEG + 5],
    "roll": [2 * SEG + 700, 2 * SEG + 699, 2 * SEG + 731, 2 * SEG + 700, 2 * SEG + 701, 2 * SEG + 669, 3 * SEG + 670, 2 * SEG + 670,
             2 * SEG + 701, SEG + 700, 2 * SEG + 700, 0],
    "edit": [SEG + 6000, SEG + 5500, SEG + 5435, SEG + 5015, 34782, 34783],
    "derived": [SEG - 1, SEG, SEG + 1, 2 * SEG + 5, SEG + 900],
}
WRONG = ("append at the next word", "window keeps the rows behind it", "b without the padding", "arithmetic keeps stored values",
         "delete takes a row too many at a seam", "negation stops at the table")
WRONG_APPLIES = {  # the lives in which the error can show at all
    "append at the next word": ("grow", "roll", "edit", "derived"),       # an append to a row count that is no multiple of 32
    "window keeps the rows behind it": ("roll", "edit", "derived"),                  # a window that ends in front of its source's last row
    "b without the padding": ("grow", "roll", "edit", "derived"),
    "arithmetic keeps stored values": ("grow", "roll", "edit", "derived"),
    "delete takes a row too many at a seam": ("edit",),
    "negation stops at the table": ("grow", "roll", "edit", "derived"),
}


class State:
    """ids: the universe rows the table holds (-1: a hole only a wrong model leaves); behind: universe rows a wrong model leaves
    set behind the table's own; mutation: what made the state; batch: the universe rows an append added."""

    def __init__(self, ids, mutation, behind=None, batch=None):
        self.ids = np.asarray(ids, np.int64)
        self.mutation, self.batch = mutation, batch
        self.behind = np.zeros(0, np.int64) if behind is None else np.asarray(behind, np.int64)

    @property
    def rows(self):
        return int(self.ids.size)

    @property
    def n_words(self):
        return n_words_of(self.rows)


def run(name, wrong=None):
    """The states of a life, the first one included.  wrong: one of WRONG that concerns a mutation (the others concern the
    battery and change nothing here)."""
    steps = LIVES[name]
    assert steps[0][0] == "start"
    states = [State(np.arange(steps[0][1]), steps[0])]
    cursor = steps[0][1]
    for step in steps[1:]:
        ids = states[-1].ids
        kind = step[0]
        if kind == "append":
            batch = np.arange(cursor, cursor + step[1])
            cursor += step[1]
            gap = (-ids.size) % 32 if wrong == "append at the next word" else 0
            states.append(State(np.concatenate([ids, np.full(gap, -1), batch]), step, batch=batch))
        elif kind in ("drop_front", "window"):
            first, n = (step[1], ids.size - step[1]) if kind == "drop_front" else step[1:]
            assert 0 <= first and first + n <= ids.size
            behind = ids[first + n:] if wrong == "window keeps the rows behind it" else None
            states.append(State(ids[first: first + n], step, behind=behind))
        elif kind == "delete":
            lo, hi = step[1:]
            assert 0 <= lo < hi <= ids.size
            if wrong == "delete takes a row too many at a seam" and lo // SEG != (hi - 1) // SEG:
                hi += 1
            states.append(State(np.concatenate([ids[:lo], ids[hi:]]), step))
        else:
            raise ValueError(kind)
    return states


def cuts(states):
    """Where the life's mutations cut a source: (ids of the source table, row) pairs -- an append cuts the index behind its last
    row and the batch behind its last, a window at both ends, a delete at both ends.  A cut at row 0 cuts nothing."""
    out = []
    for before, after in zip(states, states[1:]):
        step = after.mutation
        if step[0] == "append":
            out += [(before.ids, before.rows), (after.batch, after.batch.size)]
        elif step[0] == "drop_front":
            out.append((before.ids, step[1]))
        elif step[0] == "window":
            out += [(before.ids, step[1]), (before.ids, step[1] + step[2])]
        else:
            out += [(before.ids, step[1]), (before.ids, step[2])]
    return [(ids, row) for ids, row in out if row > 0]


# ---- the universe ---------------------------------------------------------------------------------------------------------------
def stretches():
    """(kind, first, end) of the special stretches, ascending: "constant" (one key and one value per attribute, everything
    exists) and "absent" (a and c do not exist).  They are laid around the universe rows next to every cut of every life, MARGIN
    rows to either side, so that every cut goes through fills and none lands on a stretch end; the kinds alternate."""
    near = set()
    for name in LIVES:
        for ids, row in cuts(run(name)):
            near.update(int(ids[r]) for r in (row - 1, row) if r < ids.size)
    spans = []
    for u in sorted(near):
        if spans and u - MARGIN <= spans[-1][1]:
            spans[-1][1] = min(u + MARGIN, N)
        else:
            spans.append([max(u - MARGIN, 0), min(u + MARGIN, N)])
    return [("constant" if i % 2 == 0 else "absent", lo, hi) for i, (lo, hi) in enumerate(spans)]


@functools.lru_cache(None)
def universe():
    """The columns of the universe: g, h keys; a, b, c values as they are handed in (a row without a value still has a number
    there: the index must store 0); ea, ec existence.  Rows of key g == 1 hold c in steps of 4096, so that a group has ties at
    its median; the constant stretches take turns in being inside the WHERE clause, the first one holds the largest c there is
    and the second one the smallest."""
    rng = np.random.default_rng(20261020)
    u = {"g": rng.integers(0, N_G, N), "h": rng.integers(0, N_H, N)}
    for name, bits in BITS.items():
        u[name] = rng.integers(0, 1 << bits, N)
    u["c"] = np.where(u["g"] == 1, u["c"] & ~0xFFF, u["c"])
    u["ea"], u["ec"] = rng.random(N) < 0.8, rng.random(N) < 0.9
    constants = 0
    for kind, lo, hi in stretches():
        if kind == "absent":
            u["ea"][lo:hi] = u["ec"][lo:hi] = False
            continue
        u["ea"][lo:hi] = u["ec"][lo:hi] = True
        u["g"][lo:hi], u["h"][lo:hi] = ((1, 2), (3, 1), (2, 0), (4, 2))[constants % 4]
        u["a"][lo:hi] = 2000 + 11 * constants
        u["b"][lo:hi] = 300 + constants
        u["c"][lo:hi] = (1 << 20) - 1 if constants == 0 else 0 if constants == 1 else 4096 * (37 + constants)
        constants += 1
    for v in u.values():
        v.setflags(write=False)
    return u


@functools.lru_cache(None)
def bounds():
    """lo, hi of the WHERE clause's range on a: the quartiles of the values a has."""
    u = universe()
    have = np.sort(u["a"][u["ea"]])
    return int(have[have.size // 4]), int(have[3 * have.size // 4])


@functools.lru_cache(None)
def c_constant():
    """A value c holds throughout a constant stretch (the third one)."""
    kinds = [s for s in stretches() if s[0] == "constant"]
    return int(universe()["c"][kinds[2][1]])


def columns_of(state, n_words=None):
    """The padded model: every column as 32 * n_words positions, as the index defines them."""
    u = universe()
    n_words = state.n_words if n_words is None else int(n_words)
    size = 32 * n_words
    assert state.rows <= size
    ids = np.concatenate([state.ids, state.behind])[:size]
    real = ids >= 0
    at = np.flatnonzero(real)
    m = {"n_words": n_words, "rows": state.rows}
    for key in ("g", "h"):
        m[key] = np.full(size, -1, np.int64)
        m[key][at] = u[key][ids[real]]
    for e, names in (("ea", "a"), ("ec", "c")):
        m[e] = np.zeros(size, bool)
        m[e][at] = u[e][ids[real]]
    for name in BITS:
        m[name] = np.zeros(size, np.int64)
        m[name][at] = u[name][ids[real]]
    m["a"], m["c"] = np.where(m["ea"], m["a"], 0), np.where(m["ec"], m["c"], 0)
    return m


def batch_of(ids):
    """The bare columns of universe rows `ids`, as an insert hands them in: keys, values and existence, no padding."""
    u = universe()
    return {k: np.ascontiguousarray(v[ids]) for k, v in u.items()}


# ---- derived columns ------------------------------------------------------------------------------------------------------------
S_BITS, P_BITS, P8_BITS, D_BITS = 13, 21, 8, 22  # the default widths: max(12, 9) + 1, 12 + 9, (asked for), max(20, 21) + 1


def computed(m, wrong=None):
    """s = a + b, p = a * b (21 bits and 8), d = c - p, with the existence each carries: (values, have) per name.  A row
    outside the carried existence bitmap is stored as 0."""
    keep = wrong == "arithmetic keeps stored values"
    ea, ed = m["ea"], m["ea"] & m["ec"]

    def stored(v, have):
        return (v if keep else np.where(have, v, 0)), have

    p = (m["a"] * m["b"]) & ((1 << P_BITS) - 1)
    out = {"s": stored((m["a"] + m["b"]) & ((1 << S_BITS) - 1), ea), "p": stored(p, ea),
           "p8": stored((m["a"] * m["b"]) & ((1 << P8_BITS) - 1), ea)}
    out["d"] = stored((m["c"] - out["p"][0]) & ((1 << D_BITS) - 1), ed)
    return out


def where_mask(m):
    lo, hi = bounds()
    return np.isin(m["g"], W_G) & (m["h"] >= 0) & ~np.isin(m["h"], W_NOT_H) & m["ea"] & (m["a"] >= lo) & (m["a"] <= hi)


def windows(total):
    """(first, limit) of the row listings: two that begin inside the selection, two that end behind it."""
    return [(min(7, total), 20), (total // 3, 50), (max(total - 3, 0), 10), (total + 5, 4)]


def listed_rows(m):
    """Row 0, the last table row, the first position behind the table and the last position of the column."""
    size = 32 * m["n_words"]
    return sorted({0, max(m["rows"] - 1, 0), min(m["rows"], size - 1), size - 1}, reverse=True)


def rank_of(values, num, den):
    """(value, total, less, equal) of the value of rank floor(num * (total - 1) / den) among `values`; no value: None."""
    v = np.sort(values)
    if v.size == 0:
        return None, 0, 0, 0
    value = int(v[num * (v.size - 1) // den])
    return value, int(v.size), int(np.count_nonzero(v < value)), int(np.count_nonzero(v == value))


def kth_of(values, k, largest=False):
    v = np.sort(values)
    if not 0 <= k < v.size:
        return None, int(v.size)
    return int(v[v.size - 1 - k] if largest else v[k]), int(v.size)


def top_of(values, selected, k, largest):
    """columns.top_rows: the strictly better rows in row order, then the ties in row order."""
    rows = np.flatnonzero(selected)
    k = min(k, rows.size)
    if k <= 0:
        return np.zeros(0, np.int64)
    v = values[rows]
    t = np.sort(v)[v.size - k if largest else k - 1]
    better = rows[v > t] if largest else rows[v < t]
    return np.concatenate([better, rows[v == t][: k - better.size]]).astype(np.int64)


STATS = (("c where W", "c", "W"), ("c", "c", None), ("b", "b", None), ("b where NOT W", "b", "NOT W"))
QUANTILES = ("min", "max", "median", (9, 10))
_QUANTILE = {"min": (0, 1), "max": (1, 1), "median": (1, 2)}


def battery(m, wrong=None):
    """name -> answer, on the padded model.  Row lists are int64 arrays, counts ints or int64 arrays, sums Python ints (object
    arrays of them), a value that does not exist None."""
    size = 32 * m["n_words"]
    table = np.arange(size) < m["rows"]
    w = where_mask(m)
    not_w = ~w & table if wrong == "negation stops at the table" else ~w
    masks = {"W": w, None: np.ones(size, bool), "NOT W": not_w}
    have = {"a": m["ea"], "b": table if wrong == "b without the padding" else np.ones(size, bool), "c": m["ec"]}
    comp = computed(m, wrong)
    out = {}
    # 1. counts and cross-tab
    out["count g"] = np.array([np.count_nonzero(m["g"] == v) for v in range(N_G)])
    out["count h"] = np.array([np.count_nonzero(m["h"] == v) for v in range(N_H)])
    out["crosstab g x h"] = np.array([[np.count_nonzero((m["g"] == i) & (m["h"] == j)) for j in range(N_H)] for i in range(N_G)])
    out["count g where W"] = np.array([np.count_nonzero((m["g"] == v) & w) for v in range(N_G)])
    out["count h where W"] = np.array([np.count_nonzero((m["h"] == v) & w) for v in range(N_H)])
    # 2. row listing
    rows_w = np.flatnonzero(w)
    out["rows W"] = (rows_w, int(rows_w.size))
    for first, limit in windows(rows_w.size):
        out[f"rows W [{first}, +{limit})"] = (rows_w[first: first + limit], int(rows_w.size))
    out["rows NOT W"] = (np.flatnonzero(not_w), int(np.count_nonzero(not_w)))
    # 3. constant comparisons on c
    for const in (c_constant(), 0, (1 << BITS["c"]) - 1):
        for op in CMP_OPS:
            hit = {"<": m["c"] < const, "<=": m["c"] <= const, ">": m["c"] > const, ">=": m["c"] >= const, "==": m["c"] == const}[op]
            out[f"c {op} {const}"] = np.flatnonzero(hit & m["ec"])
    # 4. column comparisons
    out["a < b"] = np.flatnonzero((m["a"] < m["b"]) & m["ea"])
    out["a == b"] = np.flatnonzero((m["a"] == m["b"]) & m["ea"])
    out["a >= b"] = np.flatnonzero((m["a"] >= m["b"]) & m["ea"])
    out["c != p"] = np.flatnonzero((m["c"] != comp["p"][0]) & m["ec"] & comp["p"][1])
    # 5. computed attributes, every position
    for name in ("s", "p", "p8", "d"):
        out[f"values of {name}"] = comp[name]
    # 6. sums
    out["sum d where W"] = int(comp["d"][0][w].sum())
    out["sum a * b where W"] = int((m["a"] * m["b"])[w].sum())
    out["sum b where NOT W"] = int(m["b"][not_w].sum())
    # 7. order statistics
    for label, attr, mask in STATS:
        v = m[attr][masks[mask] & have[attr]]
        out[f"min {label}"] = rank_of(v, 0, 1)[:2]
        out[f"max {label}"] = rank_of(v, 1, 1)[:2]
        out[f"median {label}"] = rank_of(v, 1, 2)[:2]
        out[f"99/100 {label}"] = rank_of(v, 99, 100)[:2]
        out[f"0th {label}"] = kth_of(v, 0)
        out[f"0th largest {label}"] = kth_of(v, 0, largest=True)
        out[f"last {label}"] = kth_of(v, max(v.size - 1, 0))
        out[f"one past the last {label}"] = kth_of(v, v.size)
    # 8. top rows of c
    for mask in ("W", None):
        sel = masks[mask] & m["ec"]
        for largest in (True, False):
            out[f"top 10 of c, {'largest' if largest else 'smallest'}, {mask}"] = top_of(m["c"], sel, 10, largest)
    sel = w & m["ec"]
    for largest in (True, False):
        out[f"top of c, more than there are, {'largest' if largest else 'smallest'}"] = top_of(m["c"], sel, int(np.count_nonzero(sel)) + 7, largest)
    # 9. grouped sums
    attrs = (("a", m["a"], m["ea"]), ("b", m["b"], None), ("d",) + comp["d"])
    for mask in ("W", None):
        rows = np.zeros((N_G, N_H), np.int64)
        sums = [np.empty((N_G, N_H), object) for _ in attrs]
        counts = [np.zeros((N_G, N_H), np.int64) for _ in attrs]
        for i in range(N_G):
            for j in range(N_H):
                grp = (m["g"] == i) & (m["h"] == j) & masks[mask]
                rows[i, j] = np.count_nonzero(grp)
                for t, (_, v, e) in enumerate(attrs):
                    sums[t][i, j] = int(v[grp].sum())
                    counts[t][i, j] = rows[i, j] if e is None else np.count_nonzero(grp & e)
        out[f"group by g, h: rows, {mask}"] = rows
        for t, (name, _, _) in enumerate(attrs):
            out[f"group by g, h: sum {name}, {mask}"] = sums[t]
            out[f"group by g, h: count {name}, {mask}"] = counts[t]
    # 10. grouped quantiles under W: of c, and of d, whose existence bitmap was carried through two arithmetic calls
    shape = (N_G, len(QUANTILES))
    for name, column, exists in (("c", m["c"], m["ec"]), ("d",) + comp["d"]):
        values = np.empty(shape, object)
        totals, less, equal = (np.zeros(shape, np.int64) for _ in range(3))
        for i in range(N_G):
            v = column[(m["g"] == i) & w & exists]
            for q, query in enumerate(QUANTILES):
                values[i, q], totals[i, q], less[i, q], equal[i, q] = rank_of(v, *_QUANTILE.get(query, query))
        out[f"quantiles of {name} by g: values"], out[f"quantiles of {name} by g: totals"] = values, totals
        out[f"quantiles of {name} by g: less"], out[f"quantiles of {name} by g: equal"] = less, equal
        out[f"extremes of {name} by g"] = (values[:, 0].copy(), values[:, 1].copy())
    # 11. listed rows
    at = np.array(listed_rows(m))
    out["keys g at listed rows"] = m["g"][at]
    first, limit = windows(rows_w.size)[1]
    picked = rows_w[first: first + limit]
    out["select a, d where W"] = (picked, [(m["a"][picked], m["ea"][picked]), (comp["d"][0][picked], comp["d"][1][picked])], int(rows_w.size))
    return out


def same(x, y):
    """Exact equality of two battery answers: type for type, entry for entry."""
    if isinstance(x, (tuple, list)) or isinstance(y, (tuple, list)):
        return isinstance(x, (tuple, list)) and isinstance(y, (tuple, list)) and len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
        if not (isinstance(x, np.ndarray) and isinstance(y, np.ndarray)) or x.shape != y.shape:
            return False
        if x.dtype == object or y.dtype == object:
            return all(same(p, q) for p, q in zip(x.reshape(-1).tolist(), y.reshape(-1).tolist()))
        return (x.dtype == bool) == (y.dtype == bool) and bool(np.array_equal(x, y))
    if x is None or y is None:
        return x is None and y is None
    return isinstance(x, (int, np.integer)) and isinstance(y, (int, np.integer)) and int(x) == int(y)


def differing(got, want):
    """The names whose answers differ (a name only one side has differs)."""
    return sorted(name for name in set(got) | set(want) if name not in got or name not in want or not same(got[name], want[name]))


# ---- bitmaps of the model, for the oracle ------------------------------------------------------------------------------------------
def words_of(bits):
    return np.packbits(np.ascontiguousarray(bits, dtype=np.uint8), bitorder="little").view("<u4").astype(np.uint32)


def bitmaps_of(m):
    """name -> the bitmap's words, for every column of the index of the padded model: one per key, one per slice (most
    significant first) and one per existence bitmap."""
    out = {}
    for key, count in (("g", N_G), ("h", N_H)):
        for v in range(count):
            out[f"{key} == {v}"] = words_of(m[key] == v)
    for name, bits in BITS.items():
        for i in range(bits):
            out[f"{name} slice {i}"] = words_of((m[name] >> (bits - 1 - i)) & 1)
    out["a exists"], out["c exists"] = words_of(m["ea"]), words_of(m["ec"])
    return out


# ---- the chain: build -> multiply -> range -> clause -> masked count / grouped sum --------------------------------------------------
P_RANGE = (100_000, 900_000)  # lo <= a * b <= hi of the chain's range predicate
CHAIN_ROWS = 2 * SEG + 5


def chain_stretches():
    """Four stretches of CHAIN_ROWS universe rows for the value columns of the chain: three random ones and one that repeats
    the rows of the first constant stretch, whose streams are a few fills."""
    kind, lo, hi = stretches()[0]
    assert kind == "constant"
    return [np.arange(CHAIN_ROWS), 7000 + np.arange(CHAIN_ROWS), lo + np.arange(CHAIN_ROWS) % (hi - lo), N - CHAIN_ROWS + np.arange(CHAIN_ROWS)]


def chain_answers(key_ids, value_ids):
    """The chain's answers for keys g, h of universe rows key_ids and values a, b of rows value_ids: the rows of
    `lo <= a * b <= hi AND g IN (1, 3)` per value of h, and their COUNT(*), SUM(a * b), COUNT(a * b) grouped by h."""
    u = universe()
    size = 32 * n_words_of(key_ids.size)
    g, h = np.full(size, -1, np.int64), np.full(size, -1, np.int64)
    g[: key_ids.size], h[: key_ids.size] = u["g"][key_ids], u["h"][key_ids]
    ea = np.zeros(size, bool)
    ea[: value_ids.size] = u["ea"][value_ids]
    p = np.zeros(size, np.int64)
    p[: value_ids.size] = u["a"][value_ids] * u["b"][value_ids]
    p = np.where(ea, p, 0)
    hit = ea & (p >= P_RANGE[0]) & (p <= P_RANGE[1]) & np.isin(g, W_G)
    sums = np.empty(N_H, object)
    for v in range(N_H):
        sums[v] = int(p[hit & (h == v)].sum())
    counts = np.array([np.count_nonzero(hit & (h == v)) for v in range(N_H)])
    return {"counts": counts, "rows": counts.copy(), "sum p": sums, "count p": np.array([np.count_nonzero(hit & (h == v) & ea) for v in range(N_H)])}
