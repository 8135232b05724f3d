"""CPU proof of tests/_table_dml.py: the lives reach the sizes and column lengths recorded here, the masks of their mutations
hold every kind of word, the second battery's answers are not trivial -- and where they are, the place is recorded --, and each
of eight plausible composition errors changes an answer or a state in every life it can show in.  Conditions on the inputs, no
tolerances."""
import functools

import numpy as np
import pytest

from tests import _select, _table as T, _table_dml as D

SEG = T.SEG
LIFE_NAMES = list(D.LIVES)
SIZES = {
    "purge": [64188, 47978, 42258, 42291, 8721, 8721, 0, 0, 1],
    "amend": [37744, 37744, 37744, 37744, 37744, 25464, 25464, 25401],
    "cluster": [31743, 31743, 63489, 63489, 49048, 49048, 15511],
}
N_WORDS = {  # in segments of 992 words
    "purge": [3, 2, 2, 2, 2, 1, 1, 1, 1],  # state 4: 8721 rows kept under a bound of 42291
    "amend": [2, 2, 2, 2, 2, 1, 1, 1],
    "cluster": [1, 1, 3, 3, 3, 2, 1],      # state 4: 49048 rows left under a bound of 63489
}
LARGE = 1000
CONDITIONS = ("W selects 5 % to 95 %", "b == 0 occurs", "MAP_NULL is hit", "other is not empty", "more than one partition",
              "a partition of 1000 rows", "a streak above 31 rows", "the running sum's top slice is set and clear")
# The conditions a large state does NOT meet.  A table that W was just deleted from holds no row of W until an update or an
# append brings one, and a table that only W's rows were kept in holds nothing else; the constant stretches, which carry the
# long partitions and streaks, are scattered by the updates of `amend`.  Everything else holds everywhere.
THIN = {
    ("purge", 4): ("W selects 5 % to 95 %",),
    ("purge", 5): ("W selects 5 % to 95 %",),
    ("amend", 1): ("W selects 5 % to 95 %", "a partition of 1000 rows", "a streak above 31 rows"),
    ("amend", 2): ("a partition of 1000 rows",),
    ("amend", 3): ("a partition of 1000 rows",),
    ("amend", 4): ("a partition of 1000 rows",),
    ("amend", 5): ("W selects 5 % to 95 %", "a partition of 1000 rows", "a streak above 31 rows", "the running sum's top slice is set and clear"),
    ("amend", 6): ("W selects 5 % to 95 %", "a partition of 1000 rows", "a streak above 31 rows"),
    ("amend", 7): ("W selects 5 % to 95 %", "a partition of 1000 rows", "a streak above 31 rows"),
    ("cluster", 4): ("W selects 5 % to 95 %", "a streak above 31 rows", "the running sum's top slice is set and clear"),
    ("cluster", 5): ("W selects 5 % to 95 %", "a streak above 31 rows", "the running sum's top slice is set and clear"),
    ("cluster", 6): ("W selects 5 % to 95 %", "a partition of 1000 rows", "a streak above 31 rows", "the running sum's top slice is set and clear",
                     "other is not empty"),
}


@functools.lru_cache(None)
def states(name, wrong=None):
    return D.run(name, wrong)


@functools.lru_cache(None)
def answers(name, i, wrong=None):
    return D.battery_dml(D.columns(states(name, wrong)[i]), wrong)


def _large(name):
    return [i for i, s in enumerate(states(name)) if s.rows >= LARGE]


# ---- reached states ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LIFE_NAMES)
def test_a_life_reaches_the_sizes_recorded(name):
    got = states(name)
    assert [s.rows for s in got] == SIZES[name]
    assert [s.n_words for s in got] == [992 * k for k in N_WORDS[name]]
    for s in got:
        assert s.rows == 0 or (s.ids.min() >= 0 and s.ids.max() < T.N)
        assert s.n_words >= T.n_words_of(s.rows) and s.exists_from is None


def test_the_seams_the_lives_are_named_for():
    def shrinks(name):  # an exact-sized compaction after which the columns are shorter than its own bound would make them
        return [i for i, s in enumerate(states(name)) if s.mutation[0] in ("delete", "keep") and s.mutation[2] == "exact"
                and s.n_words < T.n_words_of(states(name)[i - 1].rows)]

    assert shrinks("purge") == [1] and shrinks("amend") == [5] and shrinks("cluster") == [6]
    # purge's state 5 is a delete that deletes nothing from columns longer than the rows need: the rows are those of state 4,
    # the result is sized by the rows, one segment from two
    assert np.array_equal(states("purge")[5].ids, states("purge")[4].ids) and states("purge")[5].n_words < states("purge")[4].n_words
    longer = {name: [i for i, s in enumerate(states(name)) if s.n_words > T.n_words_of(s.rows)] for name in LIFE_NAMES}
    assert longer == {"purge": [4], "amend": [], "cluster": [4]}  # a bound-sized result, longer than its rows need
    assert all(states(n)[i].mutation[2] == "bound" and states(n)[i].rows >= LARGE for n, at in longer.items() for i in at)
    assert [i for i, s in enumerate(states("purge")) if s.rows == 0] == [6, 7]  # the empty table, and a delete from it
    assert states("purge")[7].mutation == ("delete", "all", "exact") and states("purge")[8].rows == 1
    identity = [(n, i) for n in LIFE_NAMES for i, s in enumerate(states(n)) if s.mutation[0] == "update" and s.mutation[1] == "none"]
    assert identity == [("amend", 3)] and np.array_equal(states("amend")[3].ids, states("amend")[2].ids)
    kinds = {step[0] for steps in D.LIVES.values() for step in steps}
    assert kinds == {"start", "append", "trim", "delete", "keep", "update", "cluster"}
    used = {step[1] for steps in D.LIVES.values() for step in steps if step[0] in ("delete", "keep", "update")}
    assert used == {"W", "NOT W", "c top", "a absent", "all", "none"}
    # a clustering permutes: the rows no longer ascend, and k's clustering leaves eight partitions
    assert np.any(np.diff(states("cluster")[1].ids) < 0)
    k = D.cluster_key(D.columns(states("cluster")[3]), "k")
    assert np.all(np.diff(k) >= 0) and np.unique(k).size == 8


def test_the_facts_the_predicates_rest_on():
    u = T.universe()
    kind, lo, hi = T.stretches()[0]
    assert (kind, lo) == ("constant", 0) and hi == 5720 and np.all(u["c"][lo:hi] == D.C_TOP) and u["ec"][lo:hi].all()
    kind, lo, hi = T.stretches()[1]
    assert kind == "absent" and lo < SEG < hi - 1 and hi - lo > 4000
    assert not np.any(u["c"] == D.ABSENT_C) and D.ABSENT_C < 1 << T.BITS["c"]
    assert D.mp_lookup().size == 512 and np.count_nonzero(D.mp_lookup() == D.MAP_NULL) == 31
    assert int(D.mp_lookup()[D.mp_lookup() != D.MAP_NULL].max()).bit_length() == D.MP_BITS
    assert D.a_lookup().size < 1 << T.BITS["a"] and np.count_nonzero(D.a_lookup() == D.DROP) == 40
    assert D.a_lookup()[D.a_lookup() != D.DROP].max() == D.A_BUCKETS - 1 and D.k_lookup().max() == (1 << D.K_BITS) - 1


# ---- the masks ---------------------------------------------------------------------------------------------------------------------
def _kinds(oracle, bits):
    w, fill, n, start = _select._walk(oracle.compress(T.words_of(bits)))
    one = fill & ((w & 0x40000000) != 0)
    kinds = ({"literal"} if (~fill).any() else set()) | ({"zero fill"} if (fill & ~one).any() else set()) | ({"one fill"} if one.any() else set())
    return kinds, 31 * start[one], 31 * (start[one] + n[one])


# what each life's masks hold in its large states, in the order of its mutations that take one: "all" is one fills and "none"
# zero fills by definition; NOT W over amend's state 1, whose rows of W were just updated away, has no 62 rows of W in a row and
# so no zero fill.  Every other mask holds all three kinds.
MASK_KINDS = {
    "purge": [("a absent", "lzo"), ("c top", "lzo"), ("W", "lzo"), ("none", "z"), ("W", "lzo")],
    "amend": [("W", "lzo"), ("NOT W", "lo"), ("none", "z"), ("all", "o"), ("W", "lzo"), ("a absent", "lzo")],
    "cluster": [("W", "lzo"), ("a absent", "lzo")],
}
_LETTER = {"l": "literal", "z": "zero fill", "o": "one fill"}


@pytest.mark.parametrize("name", LIFE_NAMES)
def test_the_masks_hold_every_kind_of_word(oracle, name):
    """In every large state every mask a mutation uses holds literals, zero fills and one fills, but the two constant masks;
    "a absent" has a run of ones across a multiple of 31 744 rows inside the table (purge), "c top" one of at least 1000 rows."""
    got = []
    for before, pred in D.masks_used(states(name)):
        if before.rows < LARGE:
            continue
        kinds, lo, hi = _kinds(oracle, D.predicate(D.columns(before), pred))
        got.append((pred, "".join(k for k in "lzo" if _LETTER[k] in kinds)))
        if pred == "c top":
            assert np.any(hi - lo >= 1000), name
        if pred == "a absent" and name == "purge":  # a fill never crosses a segment seam: one ends at it, one begins at it
            assert before.rows > SEG + 31 and np.any(hi == SEG) and np.any(lo == SEG), name
    assert got == MASK_KINDS[name]


# ---- non-vacuity -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def missing(name, i):
    """The CONDITIONS that state i of the life does not meet."""
    s, b = states(name)[i], answers(name, i)
    m = D.columns(s)
    rows = s.rows
    selected = np.count_nonzero(T.where_mask(m))
    k = b["values of k"][0][:rows]
    first = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    top = (b["cumsum a where W, exclusive, all rows"][0][:rows] >> (D.CS_BITS - 1)) & 1
    others = [b["group by a >> 8: other"], b["group by b where W: other"]]
    met = (0.05 * rows <= selected <= 0.95 * rows, bool(np.any(m["b"][:rows] == 0)) and not b["values of q"][1][:rows][m["b"][:rows] == 0].any(),
           not b["values of mp"][1][:rows].all(), any(o[0] > 0 for o in others), first.size > 1, np.diff(np.r_[first, rows]).max() >= 1000,
           b["streak lengths of W"][0].max() > 31, bool(top.any() and not top.all()))
    return tuple(c for c, ok in zip(CONDITIONS, met) if not ok)


def test_where_the_second_battery_bites():
    got = {(name, i): missing(name, i) for name in LIFE_NAMES for i in _large(name)}
    assert {k: set(v) for k, v in got.items() if v} == {k: set(v) for k, v in THIN.items()}
    for name in LIFE_NAMES:  # all of them together are met in at least one state of every life (amend: its first), in most in four
        assert sum(1 for i in _large(name) if not got[(name, i)]) >= 1, name
        big = False
        for i in _large(name):
            b = answers(name, i)
            big = big or any(int(v) >= 1 << 32 for key in ("group by a >> 8: sum d", "group by b where W: sum d") for v in b[key])
            assert b["c != q * b + r"].size == 0 and np.array_equal(b["c == q * b + r"], np.flatnonzero(b["values of q"][1]))
            assert not b["values of q"][1][states(name)[i].rows:].any()  # behind the table b is 0: NULL
        assert big, name  # a bucket sum of 2^32 or more somewhere in the life


def test_a_partition_crosses_a_segment_seam_in_cluster():
    s = states("cluster")[3]
    k = D.cluster_key(D.columns(s), "k")
    assert s.rows > SEG and k[SEG - 1] == k[SEG] and np.count_nonzero(k == k[SEG]) >= 1000


def test_the_first_battery_runs_on_the_new_states():
    for name in LIFE_NAMES:
        for s in states(name):
            b = T.battery(D.columns(s))
            assert b["count g"].sum() == s.rows and b["max b"][1] == 32 * s.n_words


def test_the_empty_table_answers():
    s = states("purge")[6]
    b = answers("purge", 6)
    assert s.rows == 0 and s.n_words == 992
    for name, got in b.items():
        if isinstance(got, tuple) and isinstance(got[0], np.ndarray) and got[0].size == 32 * 992 and name != "values of greatest(b, k)":
            assert not got[0].any() and (got[1] is None or not got[1].any() or name.startswith("values of CASE")), name
    assert b["count distinct k"] == 0 and b["partition starts"].size == 0 and b["sum q where W"] == 0


# ---- wrong models --------------------------------------------------------------------------------------------------------------------
def detected_by(name, wrong):
    """What the wrong model changes, over the states of the life: {state: names}, "the state" for its rows or column length."""
    right, bad = states(name), states(name, wrong)
    assert len(right) == len(bad)
    out = {}
    for i in range(len(right)):
        names = D.differing(answers(name, i, wrong), answers(name, i))
        if not np.array_equal(right[i].ids, bad[i].ids) or right[i].n_words != bad[i].n_words:
            names = ["the state"] + names
        if names:
            out[i] = names
    return out


@pytest.mark.parametrize("wrong", D.WRONG)
def test_a_wrong_model_changes_an_answer_or_a_state_in_every_life_it_applies_to(wrong):
    for name in LIFE_NAMES:
        found = detected_by(name, wrong)
        if name in D.WRONG_APPLIES[wrong]:
            assert found, (wrong, name)
        else:
            assert not found, (wrong, name)


def test_the_thinnest_place_of_the_net():
    """Per wrong model the answers that detect it (over all lives, names counted once, "the state" among them): recorded, so
    that a change of the battery that thins the net is seen."""
    counts = {}
    for wrong in D.WRONG:
        names = set()
        for name in D.WRONG_APPLIES[wrong]:
            for found in detected_by(name, wrong).values():
                names.update(found)
        counts[wrong] = len(names)
    assert counts == DETECTED_BY, counts
    assert min(counts, key=counts.get) == THINNEST[0] and counts[THINNEST[0]] == THINNEST[1], counts


DETECTED_BY = {
    "a bound-sized result takes the exact length": 29,
    "update takes the source's row by rank, not by number": 75,
    "update leaves the existence bits": 72,
    "rows behind n_rows survive a delete under a negated mask": 81,
    "division by zero is 0 and exists": 5,
    "a partition starts only at a selected row": 9,
    "a running sum counts rows without a value": 2,
    "cluster is not stable": 47,
}
# (Under W a row without a value is not selected anyway, and it adds 0 to every sum: only the two answers without a filter, the
# grand total's existence bitmap and the partition mean's denominator, see a running sum that counts such rows.)
THINNEST = ("a running sum counts rows without a value", 2)
