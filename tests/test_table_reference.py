"""CPU proof of tests/_table.py: the lives reach the sizes and column lengths they name, their cuts go through fills of the
compressed columns, the battery's answers are not trivial wherever the table is large enough, and each of six plausible
composition errors changes at least one answer in every life it can show in.  Conditions on the inputs, no tolerances."""
import functools

import numpy as np
import pytest

from tests import _select, _table as T

SEG = T.SEG
LIFE_NAMES = list(T.LIVES)
N_WORDS = {  # in segments of 992 words: where the column length changes, and 992 words for the empty index
    "grow": [1, 1, 1, 1, 1, 1, 1, 2, 3],
    "roll": [3, 3, 3, 3, 3, 3, 4, 3, 3, 2, 3, 1],
    "edit": [2, 2, 2, 2, 2, 2],
    "derived": [1, 1, 2, 3, 2],
}
LARGE = 1000  # rows from which a state's answers are held to be non-trivial
SMALL_STATES = {"grow": [0, 1, 2, 3, 4], "roll": [11], "edit": [], "derived": []}  # the states below it, by their place in the life
TRIVIAL_WHEN_EMPTY = ("every count 0", "every statistic of c None", "the statistics of b 0 with total 32 * 992")


@functools.lru_cache(None)
def states(name, wrong=None):
    return T.run(name, wrong)


@functools.lru_cache(None)
def answers(name, i, wrong=None):
    return T.battery(T.columns_of(states(name, wrong)[i]), wrong)


# ---- reached states ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LIFE_NAMES)
def test_a_life_reaches_the_sizes_it_names(name):
    got = states(name)
    assert [s.rows for s in got] == T.SIZES[name]
    assert [s.n_words for s in got] == [992 * k for k in N_WORDS[name]]
    assert [i for i, s in enumerate(got) if s.rows < LARGE] == SMALL_STATES[name]
    for s in got:
        assert np.all(np.diff(s.ids) > 0) and (s.rows == 0 or (s.ids[0] >= 0 and s.ids[-1] < T.N)) and s.behind.size == 0


def test_the_seams_the_lives_are_named_for():
    grow = T.SIZES["grow"]
    assert grow[0] == 0 and grow[1:5] == [1, 31, 32, 33] and grow[5:8] == [SEG - 1, SEG, SEG + 1] and grow[8] > 2 * SEG
    assert len(T.LIVES["grow"]) - 1 == 8  # an index appended to eight times
    roll = T.LIVES["roll"]
    drops = [s[1] for s in roll if s[0] == "drop_front"]
    adds = [s[1] for s in roll if s[0] == "append"]
    assert drops == [1, 31, 32, SEG, SEG + 1] and len(adds) == 5 and all(k != k2 for k, k2 in zip(drops, adds))
    assert roll[-1] == ("window", 5, 0) and states("roll")[-1].n_words == 992 and states("grow")[0].n_words == 992
    kinds = {step[0] for steps in T.LIVES.values() for step in steps}
    assert kinds == {"start", "append", "drop_front", "window", "delete"}
    edit = T.LIVES["edit"]
    (_, lo0, hi0), (_, lo1, hi1), (_, lo2, hi2) = edit[1:4]
    kind, first, end = T.stretches()[0]
    assert kind == "constant" and first < lo0 < hi0 < end                       # a fill cut twice
    assert lo1 // SEG != hi1 // SEG and lo1 % SEG and hi1 % SEG                   # across a segment seam
    assert lo2 % 31 == 0 and hi2 % 32 == 0 and lo2 % 32 and hi2 % 31
    assert edit[4][:2] == ("window", 977) and edit[5] == ("append", 1)
    assert 31 in drops and 32 in drops  # windows that begin at row 31 and at row 32


def test_the_universe_is_made_of_the_stretches_it_names():
    u, spans = T.universe(), T.stretches()
    assert {k for k, _, _ in spans} == {"constant", "absent"} and sum(1 for k, _, _ in spans if k == "constant") >= 3
    at = 0
    for kind, lo, hi in spans:
        assert at < lo or (at == lo == 0)  # a random stretch in between
        assert hi - lo >= (3000 if kind == "constant" else 2000)
        if kind == "constant":
            for name in ("g", "h", "a", "b", "c"):
                assert np.all(u[name][lo:hi] == u[name][lo])
            assert u["ea"][lo:hi].all() and u["ec"][lo:hi].all()
        else:
            assert not u["ea"][lo:hi].any() and not u["ec"][lo:hi].any()
        at = hi
    assert at < T.N
    assert 0.7 < u["ea"].mean() < 0.85
    # no cut of a life lands on a stretch end, or nearer to one than two whole groups
    ends = np.array([e for _, lo, hi in spans for e in (lo, hi) if 0 < e < T.N])
    for name in LIFE_NAMES:
        for ids, row in T.cuts(states(name)):
            for r in (row - 1, row):
                if r < ids.size:
                    assert np.abs(ends - ids[r]).min() > 62, (name, row)
                    assert any(lo <= ids[r] < hi for _, lo, hi in spans), (name, row)


# ---- stream content ----------------------------------------------------------------------------------------------------------------
_STREAMS = {}


def _streams(oracle, ids):
    """Every column of the table of universe rows `ids`, compressed: name -> (fill?, groups, first group) per word."""
    key = (int(ids.size), int(ids[0]) if ids.size else -1, int(ids[-1]) if ids.size else -1)
    if key not in _STREAMS:
        m = T.columns_of(T.State(ids, None))
        _STREAMS[key] = {name: _select._walk(oracle.compress(words)) for name, words in T.bitmaps_of(m).items()}
    return _STREAMS[key]


@pytest.mark.parametrize("name", LIFE_NAMES)
def test_the_streams_hold_every_kind_of_word(oracle, name):
    for s in states(name):
        if s.rows < LARGE:
            continue
        kinds = set()
        for w, fill, n, _ in _streams(oracle, s.ids).values():
            kinds |= {"literal"} if (~fill).any() else set()
            kinds |= {"zero fill"} if (fill & ((w & 0x40000000) == 0)).any() else set()
            kinds |= {"one fill"} if (fill & ((w & 0x40000000) != 0)).any() else set()
        assert kinds == {"literal", "zero fill", "one fill"}, (name, s.rows)


@pytest.mark.parametrize("name", LIFE_NAMES)
def test_every_cut_goes_through_a_fill(oracle, name):
    """A cut at row r lies strictly inside a fill word of at least one column of the source it cuts.  A fill never crosses a
    multiple of 31 744 rows, so a cut on a segment seam has a fill ending at it and a fill beginning at it (in a table that ends
    there: the fill ending at it)."""
    found = 0
    for ids, row in T.cuts(states(name)):
        hit = False
        for w, fill, n, start in _streams(oracle, ids).values():
            lo, hi = 31 * start[fill], 31 * (start[fill] + n[fill])
            if row % SEG:
                hit = hit or bool(np.any((lo < row) & (row < hi)))
            else:
                hit = hit or (bool(np.any(hi == row)) and (bool(np.any(lo == row)) or 32 * T.n_words_of(ids.size) == row))
        assert hit, (name, ids.size, row)
        found += 1
    assert found >= len(T.LIVES[name]) - 1


# ---- non-vacuity -------------------------------------------------------------------------------------------------------------------
def _large(name):
    return [i for i, s in enumerate(states(name)) if s.rows >= LARGE]


@pytest.mark.parametrize("name", LIFE_NAMES)
def test_the_battery_bites_in_every_large_state(name):
    big = False
    for i in _large(name):
        s, b = states(name)[i], answers(name, i)
        m = T.columns_of(s)
        what = (name, i)
        selected = b["rows W"][1]
        assert 0.05 * s.rows <= selected <= 0.95 * s.rows, what
        assert np.all(b["group by g, h: rows, None"] > 0), what                              # all 15 groups have rows ...
        under = b["group by g, h: rows, W"]
        wanted = np.array([[g in T.W_G and h not in T.W_NOT_H for h in range(T.N_H)] for g in range(T.N_G)])
        assert np.array_equal(under > 0, wanted), what                                       # ... and each group W admits a selected one
        values, equal = b["quantiles of c by g: values"], b["quantiles of c by g: equal"]
        assert any(values[g, 0] is not None and values[g, 0] != values[g, 1] for g in range(T.N_G)), what
        assert any(equal[g, 2] > 1 for g in range(T.N_G)), what                              # a tie at a group's median
        assert any(values[g, 0] is None for g in range(T.N_G)), what                         # and a group with no row at all
        d, have = b["values of d"]
        top = (d >> (T.D_BITS - 1)) & 1
        assert top[have].any() and not top[have].all(), what                                 # the borrow slice set and clear
        p, p8 = b["values of p"][0], b["values of p8"][0]
        assert np.any(p != p8) and np.array_equal(p & 255, p8), what
        assert not have[s.rows:].any() and not d[s.rows:].any() and not d[~have].any(), what
        big = big or any(int(v) >= 1 << 32 for t in ("a", "b", "d") for v in b[f"group by g, h: sum {t}, None"].reshape(-1))
        for label, _, _ in T.STATS:
            assert b[f"min {label}"][0] is not None and b[f"one past the last {label}"][0] is None, what
        full = s.rows == 32 * s.n_words  # (one segment exactly: nothing lies behind the table)
        assert b["min c"][0] != b["max c"][0] and b["min b"][1] == 32 * s.n_words and (full or b["min b"][0] == 0), what
        for k in ("top 10 of c, largest, W", "top 10 of c, smallest, None"):
            assert b[k].size == 10, what
        ties = b["top 10 of c, smallest, None"]
        assert np.all(m["c"][ties] == m["c"][ties[0]]) and np.all(np.diff(ties) > 0), what     # ties, in row order
        assert np.count_nonzero(m["ec"] & (m["c"] == m["c"][ties[0]])) > 10, what                # and more of them than are listed
        assert b["top of c, more than there are, largest"].size == np.count_nonzero(T.where_mask(m) & m["ec"]), what
        assert b["c < 0"].size == 0 and b["c > %d" % ((1 << 20) - 1)].size == 0 and b["c >= 0"].size == np.count_nonzero(m["ec"]), what
        assert b["a < b"].size and b["a >= b"].size and b["c != p"].size, what
        assert b["rows NOT W"][1] > 32 * s.n_words - s.rows, what
        assert (full or b["keys g at listed rows"][0] == -1) and b["sum b where NOT W"] > 0 and b["sum d where W"] > 0, what
        assert b["select a, d where W"][0].size == 50, what
    assert big, name  # a grouped sum of 2^32 or more somewhere in the life


def test_a_constant_of_the_comparisons_is_met_and_equal_columns_exist():
    """The constant the comparisons on c use fills a constant stretch of some large state, and a == b holds somewhere."""
    large = [answers(n, j) for n in LIFE_NAMES for j in _large(n)]
    assert any(b["c == %d" % T.c_constant()].size >= 1000 for b in large)
    assert any(b["a == b"].size for b in large)


@pytest.mark.parametrize("name,i", [(n, i) for n in LIFE_NAMES for i in SMALL_STATES[n]])
def test_what_a_small_state_answers(name, i):
    """The states below 1000 rows run the whole battery too; the empty ones answer as TRIVIAL_WHEN_EMPTY says."""
    s, b = states(name)[i], answers(name, i)
    assert {k.split(" [")[0] for k in b} == {k.split(" [")[0] for k in answers("roll", 0)}  # no query is left out
    if s.rows:
        assert b["count g"].sum() == s.rows and b["max b"][1] == 32 * 992
        return
    assert not b["count g"].any() and not b["crosstab g x h"].any() and b["rows W"][1] == 0 and b["rows NOT W"][1] == 32 * 992
    for stat in ("min", "max", "median", "99/100", "0th", "last"):
        assert b[f"{stat} c"] == (None, 0) and b[f"{stat} c where W"] == (None, 0)
        assert b[f"{stat} b"] == (0, 32 * 992)
    assert len(TRIVIAL_WHEN_EMPTY) == 3


# ---- wrong models --------------------------------------------------------------------------------------------------------------------
def detected_by(name, wrong):
    """The battery answers the wrong model changes, over the states of the life: {state: names}."""
    right, bad = states(name), states(name, wrong)
    assert len(right) == len(bad)
    out = {}
    for i in range(len(right)):
        names = T.differing(answers(name, i, wrong), answers(name, i))
        if names:
            out[i] = names
    return out


@pytest.mark.parametrize("wrong", T.WRONG)
def test_a_wrong_model_changes_an_answer_in_every_life_it_applies_to(wrong):
    for name in LIFE_NAMES:
        found = detected_by(name, wrong)
        if name in T.WRONG_APPLIES[wrong]:
            assert found, (wrong, name)
        else:
            assert not found, (wrong, name)  # and it is the right model where it cannot show


def test_the_thinnest_place_of_the_net():
    """The wrong model that the fewest battery answers detect (over all lives, names counted once): recorded, so that a change
    of the battery that thins the net further is seen."""
    counts = {}
    for wrong in T.WRONG:
        names = set()
        for name in T.WRONG_APPLIES[wrong]:
            for found in detected_by(name, wrong).values():
                names.update(k.split(" [")[0] for k in found)
        counts[wrong] = len(names)
    assert min(counts, key=counts.get) == THINNEST[0] and counts[THINNEST[0]] == THINNEST[1], counts


# (Of the answers the battery was first drawn up with, NONE saw "negation stops at the table": the rows behind the table add 0 to
# SUM(b).  "rows NOT W" and the statistics of b under NOT W are in the battery for that reason, and are 9 names.)
THINNEST = ("arithmetic keeps stored values", 6)


def test_same_is_exact():
    assert T.same((1, None), (1, None)) and not T.same((1, None), (1, 0)) and not T.same(np.array([1]), np.array([1, 1]))
    assert not T.same(np.array([True]), np.array([1])) and T.same(np.array([3], object), np.array([3], object))
    assert not T.same(np.array([1 << 70], object), np.array([(1 << 70) + 1], object)) and not T.same(1, None)
