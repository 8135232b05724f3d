"""Shared helpers of the map tests (wah_bsi_map_indexed_device, include/wah.h): a numpy model that answers from the VALUES and the
lookup, the kernel's steps restated in numpy from the SLICES, seven wrong models of that restatement, and the builders of the named
cases.  A bitmap of n words has 32 * n rows, row p at word p // 32, bit p % 32; keys are numpy uint64, a lookup is uint32.

A case is a dict: n (words, a multiple of 992), n_rows, ks (key slices), keys, exists (the key's existence bitmap or None), lookup
(uint32 [n_keys]), k_out (result slices) and partial.  An answer is (matrix, refused): the result's decoded slice matrix [k_out (+ 1),
n] -- most significant slice first, the rows that have a value last when the key has an existence bitmap or the call is partial --
and whether the status must be WAH_ERR_STREAM (the matrix of a refused call is unspecified: None)."""
import numpy as np

from tests import _bsi

SEG_WORDS, SEG_GROUPS, SEG_BITS = 992, 1024, 31 * 1024
BLOCK_ROWS, BLOCK_WORDS, BLOCKS = 2048, 64, 16  # a segment: fifteen blocks and a half one
HALF_START = 15 * BLOCK_ROWS                     # 30 720: the half block's first row
GRID_ITEMS = 512                                 # kMapGridItems of wah_map.hip: workgroups at the most
NULL = 0xFFFFFFFF
WRONG = ("rows behind n_rows mapped through lookup[0]", "map read behind n_keys", "a NULL entry stored as a value",
         "a row outside the existence bitmap mapped as key 0", "slices least significant first", "high word of a ballot dropped",
         "half block treated as a full one")


def has_exists_row(case):
    return case["exists"] is not None or case["partial"]


# ---- the value model -------------------------------------------------------------------------------------------------------------
def values_of(case):
    """(values uint64, has bool, refused): per row the looked-up value (0 without one) and whether it has one -- from the keys and
    the lookup, never from slices."""
    rows = 32 * case["n"]
    lookup = case["lookup"].astype(np.uint64)
    sel = np.arange(rows) < case["n_rows"]
    if case["exists"] is not None:
        sel &= case["exists"]
    keys = case["keys"]
    inside = keys < np.uint64(lookup.size)
    entry = np.where(inside, lookup[np.minimum(keys, np.uint64(lookup.size - 1)).astype(np.int64)], np.uint64(NULL))
    has = sel & (entry != np.uint64(NULL))
    miss = sel & ~has
    wide = has & ((entry >> np.uint64(case["k_out"])) != 0)
    refused = bool(wide.any() or (not case["partial"] and miss.any()))
    return np.where(has, entry, np.uint64(0)), has, refused


def expected(case):
    """The model: (matrix, refused)."""
    values, has, refused = values_of(case)
    if refused:
        return None, True
    return _bsi.build_slices(values, case["k_out"], has if has_exists_row(case) else None), False


# ---- the kernel's steps ------------------------------------------------------------------------------------------------------------
def kernel(case, wrong=None):
    """wah_map.hip restated: per segment the key words folded out of the slices (a row outside the existence bitmap is stored as
    0), the selection image (all ones clipped to n_rows, ANDed with the existence row), fifteen blocks of 2048 rows and the half
    block of 1024, lane l of step t owning row 2048 blk + 64 t + l; one bounds test and one load per selected row; the ballot of a
    step is two words, lanes 0 .. 31 then 32 .. 63; the result slices most significant first, then the ballots of "has a value"."""
    n, ks, k_out = case["n"], case["ks"], case["k_out"]
    assert n % SEG_WORDS == 0
    rows = 32 * n
    exists, lookup = case["exists"], case["lookup"].astype(np.int64)
    slices = _bsi.build_slices(case["keys"], ks, exists, zero_missing=True)
    words = np.zeros(rows, np.int64)
    for i in range(ks):  # the fold: slice i lands at bit ks - 1 - i of the row's word
        words |= _bsi.unpack_bits(slices[i]).astype(np.int64) << (ks - 1 - i)
    image = np.arange(rows) < (rows if wrong == WRONG[0] else case["n_rows"])
    if exists is not None and wrong != WRONG[3]:
        image &= _bsi.unpack_bits(slices[ks])
    behind = np.r_[lookup, np.zeros(1 << 13, np.int64)]  # what lies behind the map: zeros, for the model that reads there
    out_rows = k_out + (1 if has_exists_row(case) else 0)
    matrix = np.zeros((out_rows, n), np.uint32)
    late = []  # the stores of a half block that is not cut: they land last
    refused = False
    for seg in range(n // SEG_WORDS):
        for blk in range(BLOCKS):
            half = blk == BLOCKS - 1
            steps = 16 if half and wrong != WRONG[6] else 32
            r = seg * SEG_BITS + blk * BLOCK_ROWS + np.arange(64 * steps)  # step t, lane l: 64 t + l
            inside = r < (seg + 1) * SEG_BITS                               # (steps that do not exist hold nothing)
            rr = np.minimum(r, rows - 1)
            key, picked = words[rr], image[rr] & inside
            if wrong == WRONG[1]:
                load = picked & (key < behind.size)
                raw = np.where(load, behind[np.minimum(key, behind.size - 1)], NULL)
            else:
                load = picked & (key < lookup.size)
                raw = np.where(load, lookup[np.minimum(key, lookup.size - 1)], NULL)
            has = load if wrong == WRONG[2] else raw != NULL
            refused |= bool((has & ((raw >> k_out) != 0) & (raw != NULL)).any()) or bool(not case["partial"] and (picked & ~has).any())
            v = np.where(has, raw, 0)
            first = seg * SEG_WORDS + blk * BLOCK_WORDS
            for i in range(out_rows):
                if i < k_out:
                    bit = i if wrong == WRONG[4] else k_out - 1 - i
                    ballots = _bsi.pack_bits(((v >> bit) & 1).astype(bool))
                else:
                    ballots = _bsi.pack_bits(has)
                if wrong == WRONG[5]:
                    ballots[1::2] = 0
                if half and steps == 32:
                    late.append((i, first, ballots))
                else:
                    matrix[i, first: first + 2 * steps] = ballots
    for i, first, ballots in late:
        end = min(first + 64, n)
        matrix[i, first:end] = ballots[: end - first]
    return (None, True) if refused else (matrix, False)


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def make_lookup(rng, n_keys, k_out, kind="random"):
    top = min((1 << k_out) - 1, NULL - 1)  # the largest storable value: 2^32 - 1 is the null entry
    if kind == "constant":
        return np.full(n_keys, top, np.uint32)
    lookup = (_bsi.uniform_values(rng, n_keys, k_out) & np.uint64(top)).astype(np.uint32)
    lookup[lookup == NULL] = top
    lookup[rng.integers(0, n_keys)] = top
    if kind == "nulls":
        lookup[rng.random(n_keys) < 0.25] = NULL
        lookup[0] = top  # (key 0 has a value: what a model that maps the wrong rows as key 0 stores)
    return lookup


def make_case(n, ks, k_out, n_keys=None, with_exists=False, partial=False, n_rows=None, kind=None, seed=0):
    rng = np.random.default_rng(104729 * ks + 1299709 * k_out + n + seed)
    rows = 32 * n
    domain = 1 << ks
    if n_keys is None:
        n_keys = min(domain, 1 << 13)
    if kind is None:
        kind = "nulls" if partial else "random"
    lookup = make_lookup(rng, n_keys, k_out, kind)
    keys = _bsi.uniform_values(rng, rows, ks)
    if domain > n_keys:  # most keys inside the lookup, the rest anywhere in the width
        keys = np.where(rng.random(rows) < 0.9, rng.integers(0, n_keys, rows, dtype=np.uint64), keys)
    if not partial:  # no miss: every key inside the lookup
        keys = np.minimum(keys, np.uint64(n_keys - 1))
    exists = rng.random(rows) < 0.9 if with_exists else None
    return dict(n=n, n_rows=rows if n_rows is None else n_rows, ks=ks, keys=keys, exists=exists, lookup=lookup, k_out=k_out, partial=partial)


SIZES = (SEG_WORDS, 2 * SEG_WORDS, 3 * SEG_WORDS)
KEY_WIDTHS, OUT_WIDTHS = (1, 8, 12, 13, 32), (1, 7, 17, 31, 32)
MODES = ((False, False), (True, False), (False, True), (True, True))  # (existence row, partial)
BIG = 3 * SEG_WORDS


def row_edges(n):
    """n_rows at 0, 1, and on and beside a step, a word, a group, a block, the half block's start, a segment and 32 n."""
    edges = {0, 1, 32 * n - 1, 32 * n}
    for at in (64, 32, 31 * 1000, BLOCK_ROWS, HALF_START, SEG_BITS, SEG_BITS + HALF_START, 2 * SEG_BITS):
        edges |= {at - 1, at, at + 1}
    return sorted(e for e in edges if e <= 32 * n)


def named_cases():
    """name -> case: what tests/test_map_reference.py proves the restatement and the wrong models on, and tests/test_gpu_bsi_map.py
    runs on the device."""
    cases = {}
    i = 0
    for ks in KEY_WIDTHS:  # every pair of widths, the sizes and the four modes in turn
        for k_out in OUT_WIDTHS:
            with_exists, partial = MODES[i % 4]
            cases[f"widths {ks} x {k_out}"] = make_case(SIZES[i % 3], ks, k_out, with_exists=with_exists, partial=partial)
            i += 1
    for n in SIZES:
        for with_exists, partial in MODES:
            cases[f"size {n}{' exists' if with_exists else ''}{' partial' if partial else ''}"] = make_case(n, 12, 17, None, with_exists, partial, seed=1)
    for j, n_rows in enumerate(row_edges(BIG)):
        with_exists, partial = MODES[j % 4]
        cases[f"n_rows {n_rows}"] = make_case(BIG, 8, 7, None, with_exists, partial, n_rows=n_rows, seed=2)
    for n_keys, what in ((1, "1"), (3000, "below the domain"), (1 << 12, "the domain"), ((1 << 12) + 77, "beyond the domain")):
        for partial in (False, True):
            cases[f"n_keys {what}{' partial' if partial else ''}"] = make_case(2 * SEG_WORDS, 12, 17, n_keys, partial, partial, seed=3)
    cases["largest storable value"] = make_case(SEG_WORDS, 8, 32, kind="constant", seed=4)
    cases["constant lookup"] = make_case(2 * SEG_WORDS, 13, 7, kind="constant", seed=4)
    cases["constant lookup partial"] = make_case(2 * SEG_WORDS, 13, 7, with_exists=True, partial=True, kind="constant", seed=4)
    cases["nulls under a full key"] = make_case(2 * SEG_WORDS, 12, 17, None, True, True, seed=5)
    cases["rows behind n_rows"] = make_case(2 * SEG_WORDS, 8, 7, None, False, True, n_rows=SEG_BITS + 777, seed=5)
    return cases


def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.choice(SIZES[:2]))
    ks, k_out = int(rng.integers(1, 33)), int(rng.integers(1, 33))
    n_keys = int(rng.integers(1, min(1 << ks, 5000) + 1 + (7 if rng.random() < 0.3 else 0)))
    return make_case(n, ks, k_out, n_keys, bool(rng.random() < 0.5), bool(rng.random() < 0.6), n_rows=int(rng.integers(0, 32 * n + 1)), seed=seed)


def refused_cases():
    """name -> case the status refuses: a miss without PARTIAL (a key behind the lookup, a NULL entry) and an entry too wide for the
    result in both modes; and name -> case it does NOT refuse: a miss in a row that does not exist, a miss behind n_rows."""
    refused, fine = {}, {}
    base = make_case(2 * SEG_WORDS, 12, 17, 3000, True, False, n_rows=SEG_BITS + 5000, seed=6)
    live = int(np.flatnonzero(base["exists"][: base["n_rows"]])[-1])       # the last row that exists in front of n_rows
    gone = int(np.flatnonzero(~base["exists"][: base["n_rows"]])[-1])      # ... and the last one that does not
    back = base["n_rows"] + 3                                              # a row behind n_rows (it exists or not)

    def planted(row, key=None, entry=None, **kw):
        case = dict(base, keys=base["keys"].copy(), lookup=base["lookup"].copy(), **kw)
        if key is not None:
            case["keys"][row] = key
        if entry is not None:
            case["lookup"][int(case["keys"][row])] = entry
        return case

    refused["a key behind the lookup"] = planted(live, key=3000)
    refused["a NULL entry"] = planted(live, entry=NULL)
    refused["an entry too wide"] = planted(live, entry=1 << 17)
    refused["an entry too wide, partial"] = planted(live, entry=1 << 17, partial=True)
    fine["a key behind the lookup, partial"] = planted(live, key=3000, partial=True)
    fine["a miss in a row that does not exist"] = planted(gone, key=4095)
    fine["a miss behind n_rows"] = planted(back, key=4095, exists=base["exists"] | (np.arange(base["exists"].size) == back))
    return refused, fine


# the named case on which a wrong model has to change the answer
CAUGHT_BY = {
    WRONG[0]: "rows behind n_rows",
    WRONG[1]: "n_keys below the domain partial",
    WRONG[2]: "nulls under a full key",
    WRONG[3]: "nulls under a full key",
    WRONG[4]: "widths 8 x 17",
    WRONG[5]: "widths 1 x 1",
    WRONG[6]: "size 1984",
}
