"""CPU test of tests/_walk.py: the vectorised references of wah_validate_device, wah_build_index_device and
wah_merge_fills_device equal the word-by-word restatements (tests/test_gpu_parity.py's, and a plain loop for the index) on
every probe stream, on random foreign streams and on the hand streams; every constructor has the facts it states, shown by
restating the kernel's predicate for the one word; and the streams of more than 1024 tiles, too long for the loops, are
proven with the oracle's decoder and by property.
"""
import numpy as np
import pytest

from tests import _walk as wk
from tests.test_gpu_parity import _py_merge_fills, _py_report, _random_foreign_stream

F, K, MASK = 0x80000000, 0x40000000, 0x3FFFFFFF


def _py_index(st):
    """Word-by-word restatement of wah_build_index_device: offsets, or None where the stream is refused."""
    pos, offsets = 0, []
    for i, x in enumerate(int(v) for v in st):
        n = x & MASK if x & F else 1
        if n == 0 or pos % 1024 + n > 1024:
            return None
        if pos % 1024 == 0:
            offsets.append(i)
        pos += n
    return offsets + [len(st)]


def _same_as_the_loops(st, what):
    assert wk.report(st) == _py_report(st), what
    got = wk.merged(st)
    assert got.dtype == np.uint32 and np.array_equal(got, _py_merge_fills(st)), what
    want, got = _py_index(st), wk.index(st)
    if want is None:
        assert isinstance(got, str), what
    else:
        assert got.dtype == np.int64 and got.tolist() == want and got.size == wk.segments_of(st) + 1, what


@pytest.fixture(scope="module")
def probes():
    return wk.small_probes()


def test_constants_are_the_walks():
    assert (wk.TILE, wk.THREADS, wk.PER_THREAD, wk.PER_WAVE, wk.BLOCK, wk.SCAN_TILES) == (4096, 256, 16, 1024, 1 << 29, 1024)
    assert wk.PLACEMENT_BYTES == (0, 4, 8, 12)
    edges = [i for _, i in wk.WALK_EDGES]
    assert any(i % wk.PER_THREAD for i in edges)                                              # the control
    assert any(i % wk.PER_THREAD == 0 and i % wk.PER_WAVE for i in edges)                     # first word of a thread, from LDS
    assert any(i % wk.PER_WAVE == 0 and i % wk.TILE for i in edges)                           # ... of a wave: the sums of the waves in front
    assert sum(1 for i in edges if i % wk.TILE == 0) >= 2                                     # ... of a tile: from global memory, the tile base
    assert {c % wk.TILE for c in wk.END_WORDS} >= {0, 1, wk.TILE - 1, 15, 16, 17}
    t = wk.SCAN_TILES
    assert set(wk.SCAN_ROUND_TILE_COUNTS) == {t - 1, t, t + 1, 2 * t, 2 * t + 1} == {n for n, _ in wk.SCAN_ROUND_STREAMS.values()}
    assert 1 in wk.BLOCK_MULTIPLES and max(wk.BLOCK_MULTIPLES) * wk.BLOCK > 1 << 32


def test_references_equal_the_loops_on_every_probe(probes):
    n = 0
    for family, plist in probes.items():
        for p in plist:
            assert p.stream.dtype == np.uint32 and p.stream.size <= 4 * wk.TILE, p.name
            _same_as_the_loops(p.stream, f"{family}: {p.name}")
            n += 1
    assert n >= 150


@pytest.mark.parametrize("seed", range(12))
def test_references_equal_the_loops_on_random_foreign_streams(seed):
    rng = np.random.default_rng(4000 + seed)
    for n_words in (1, 2, 15, 16, 17, 31, 33, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 5):   # 12 x 17 = 204 streams
        st = _random_foreign_stream(rng, n_words, max_groups=1 << 40)
        assert st.size == n_words
        _same_as_the_loops(st, (seed, n_words))
    # and segmented ones, which have an index
    st = wk.segments(wk.split_words(int(rng.integers(1, 9000)), seed), rng)
    assert isinstance(wk.index(st), np.ndarray)
    _same_as_the_loops(st, (seed, "segmented"))


def test_references_on_the_hand_streams():
    hand = np.array([F | 1000, F | 24, F | 5, 0, 0x7FFFFFFF, 0xC0000000, 0xC0000000 | 2000], np.uint32)
    assert wk.report(hand)[2:] == (1, 2, 1, 1, False)
    _same_as_the_loops(hand, "the checker's hand stream")
    cut = np.array([F | ((1 << 29) - 4), F | 8, F | 9, 0xC0000000 | 1, 0xC0000000, 0xC0000000 | 2], np.uint32)
    _same_as_the_loops(cut, "the merger's hand stream")
    # (the fill of 8 lies across 2^29 and is kept; the fill of 9 is kept too: the word in front of it STARTS in the other block)
    assert wk.merged(cut).tolist() == [F | ((1 << 29) - 4), F | 8, F | 9, 0xC0000000 | 1, 0xC0000000 | 2]
    empty = np.zeros(0, np.uint32)
    assert wk.report(empty) == (0, 0, 0, 0, 0, 0, True) and wk.merged(empty).size == 0 and wk.index(empty).tolist() == [0]
    _same_as_the_loops(empty, "no words")


# ---- the facts of every constructor, by the kernel's predicate for the one word ------------------------------------------------
def _at(st, i):
    """(word, group position, word in front or None) of word i, by plain sums."""
    head = st[:i]
    pos = int(np.where(head & F, head & MASK, 1).astype(np.uint64).sum()) if i else 0
    return int(st[i]), pos, (int(st[i - 1]) if i else None)


def _unmerged(x, pos, prev):   # validate_kernel's n_unmerged
    return bool(x & F and x & MASK and prev is not None and prev & F and prev & MASK and not (prev ^ x) & K and pos % 1024)


def _dropped(x, pos, prev):    # merge_dropped
    if not x & F:
        return False
    if not x & MASK:
        return True
    if prev is None or not prev & F or not prev & MASK or (prev ^ x) & K:
        return False
    return (pos - (prev & MASK)) >> 29 == (pos + (x & MASK) - 1) >> 29


def _crossing(x, pos):         # validate_kernel's n_cross, index_kernel's bad (less the empty fill)
    return bool(x & F and x & MASK and pos % 1024 + (x & MASK) > 1024)


def test_pair_probes(probes):
    plist = probes["pairs"]
    assert len(plist) == (len(wk.WALK_EDGES) + 1) * len(wk.PAIR_KINDS)
    seen = set()
    for k in range(0, len(plist), len(wk.PAIR_KINDS)):
        group = plist[k: k + len(wk.PAIR_KINDS)]
        i = group[0].facts["i"]
        for p in group:
            st = p.stream
            x, pos, prev = _at(st, i)
            f = p.facts
            assert f["i"] == i and x == (0xC0000000 | 5), p.name
            assert _unmerged(x, pos, prev) == f["unmerged"] and _dropped(x, pos, prev) == f["dropped"], p.name
            assert _dropped(*_at(st, i - 1)) == f["prev_dropped"], p.name
            assert not st[i + 1] & F and (i < 2 or not st[i - 2] & F), p.name                    # literals around the pair
            assert np.array_equal(np.flatnonzero(st != group[0].stream), [i - 1] if p is not group[0] else []), p.name  # one word apart
            seen.add((f["unmerged"], f["dropped"], f["prev_dropped"], bool(prev & F), pos % 1024 == 0))
            # the report and the merged stream say so: with word i as a literal nothing of it is left
            ctl = st.copy()
            ctl[i] = 12345
            assert wk.report(st)[5] - wk.report(ctl)[5] == int(f["unmerged"]), p.name
            assert wk.merged(ctl).size - wk.merged(st).size == int(f["dropped"]), p.name
        assert [(_at(p.stream, i)[1] % 1024 == 0) for p in group] == [False, False, i == 1, False, True], i
    assert seen >= {(True, True, False, True, False), (False, False, False, True, False), (False, False, True, True, False),
                    (False, False, False, False, False), (False, True, False, True, True)}
    assert {p.facts["i"] for p in plist} == {1} | {i for _, i in wk.WALK_EDGES}


def test_position_probes(probes):
    plist = probes["positions"]
    assert len(plist) == len(wk.WALK_EDGES) * (2 * len(wk.POSITION_Q) + 1)
    for p in plist:
        f, st = p.facts, p.stream
        x, pos, _ = _at(st, f["i"])
        assert x & F and x & MASK == f["count"] and pos % 1024 == f["q"] and pos >= 1024 * (f["i"] > 100), p.name
        assert _crossing(x, pos) == f["crossing"] == (f["q"] + f["count"] > 1024), p.name
        # the one fill decides: the checker counts this crossing and no other, the stream has an index or has none
        assert wk.report(st)[2:6] == (0, 0, int(f["crossing"]), 0), p.name
        assert isinstance(wk.index(st), str) == f["crossing"], p.name
        assert sum(_crossing(*_at(st, j)[:2]) for j in range(max(f["i"] - 3, 0), f["i"] + 8)) == int(f["crossing"])
    for _, i in wk.WALK_EDGES:
        for q in wk.POSITION_Q:
            assert {(f["count"], f["crossing"]) for f in (p.facts for p in plist) if f["i"] == i and f["q"] == q} >= {(1024 - q, False), (1025 - q, True)}
        assert any(f["i"] == i and f["count"] == 2048 and f["crossing"] for f in (p.facts for p in plist))
    # a wrong wave sum or tile base moves q: no wave and no tile in front of a probed fill holds a multiple of 1024 groups.  (Where
    # q = 0 ALL the words in front are whole segments: a single wave or tile in front is then a multiple by construction, and
    # leaving it out cannot show; the probes of q = 1 and 1023 on the same edge are the ones that notice.)
    behind_waves = [p for p in plist if p.facts["i"] >= wk.PER_WAVE]
    assert len(behind_waves) == 4 * (2 * len(wk.POSITION_Q) + 1)
    checked = 0
    for p in behind_waves:
        i, q = p.facts["i"], p.facts["q"]
        for unit in (wk.PER_WAVE, wk.TILE):
            totals = [wk.groups(p.stream[w: w + unit]) for w in range(0, i - i % unit, unit)]
            assert len(totals) == i // unit
            if q or len(totals) > 1:
                assert all(g % 1024 for g in totals), (p.name, unit, totals)
                checked += len(totals)
            else:
                assert sum(totals) % 1024 == 0
    assert checked >= 100
    for _, i in wk.WALK_EDGES:                                        # every edge behind a wave has such probes, both ways
        if i >= wk.PER_WAVE:
            assert {(f["q"], f["crossing"]) for f in (p.facts for p in plist) if f["i"] == i and f["q"]} == {(1, False), (1, True), (1023, False), (1023, True)}


def test_end_probes_and_the_padding(probes):
    plist = probes["ends"]
    assert {p.facts["c_words"] for p in plist} == set(wk.END_WORDS) and len(plist) == 4 * len(wk.END_WORDS)
    for p in plist:
        st = p.stream
        assert st.size == p.facts["c_words"] and int(st[-1]) == p.facts["last"], p.name
        # what lies behind the end counts for nothing -- and would be noticed: every counter and the merged words move with it
        padded = np.concatenate([st, wk.PADDING])
        a, b = wk.report(st), wk.report(padded)
        assert all(b[k] > a[k] for k in (0, 2, 3, 4)) and b[5] >= a[5] and wk.merged(padded).size > wk.merged(st).size, p.name
    lasts = {p.facts["last"] for p in plist}
    assert lasts == {0xC0000000, 0, 0x7FFFFFFF, F | 11}
    assert any(_unmerged(*_at(wk.PADDING, j)) or _at(wk.PADDING, j)[1] % 1024 == 0 for j in range(1, wk.PADDING.size))


def test_index_probes(probes):
    plist = probes["index"]
    whole, ragged = plist[0], plist[1]
    edges = sorted(i for _, i in wk.WALK_EDGES)
    for p in (whole, ragged):
        idx = wk.index(p.stream)
        assert isinstance(idx, np.ndarray) and set(edges) <= set(idx.tolist()) and p.facts["starts"] == edges, p.name
        sizes = np.diff(idx)
        assert np.count_nonzero(sizes == 1) >= len(edges) and np.count_nonzero(sizes == 1024) >= 3
        for i in edges:                                                   # a one-word segment ON the edge: a fill of 1024 groups
            assert _at(p.stream, i)[1] % 1024 == 0 and p.stream[i] & MASK == 1024 and p.stream[i] & F
        full = [p.stream[a: b] for a, b in zip(idx[:-1], idx[1:]) if b - a == 1024]
        assert all(not np.any(s & F) for s in full)
    assert wk.groups(whole.stream) % 1024 == 0 and wk.groups(ragged.stream) % 1024 == 100
    rest = plist[2:]
    assert len(rest) == 2 * len(wk.WALK_EDGES)
    for ok, bad in zip(rest[0::2], rest[1::2]):
        i = ok.facts["i"]
        assert bad.facts["i"] == i and not ok.facts["refused"] and bad.facts["refused"]
        assert np.array_equal(np.flatnonzero(ok.stream != bad.stream), [i, i + 1])
        assert i in wk.index(ok.stream).tolist() and wk.index(bad.stream) == "an empty fill"
        assert wk.report(bad.stream)[2:6] == (1, 0, 0, 0) and wk.report(ok.stream)[2:6] == (0, 0, 0, 0)
        assert wk.groups(ok.stream) == wk.groups(bad.stream) and _at(ok.stream, i)[1] % 1024 == 0
        assert bad.stream[i] & F and not bad.stream[i] & MASK
    assert {p.facts["i"] for p in rest} == set(edges)


def _units_that_keep_nothing(st, unit):
    keep = ~wk.dropped(st)
    pad = (-keep.size) % unit
    return int(np.count_nonzero(~np.concatenate([keep, np.ones(pad, bool)]).reshape(-1, unit).any(axis=1)))


def test_run_probes(probes):
    plist = probes["runs"]
    by_run = {p.facts["run"]: p for p in plist if p.name.startswith("run of")}
    assert set(by_run) == set(wk.RUN_LENGTHS)
    for n, p in by_run.items():
        st, head = p.stream, p.facts["head"]
        assert head % wk.PER_THREAD and (head + 1 + n) % wk.PER_THREAD, "begins and ends inside a thread"
        d = wk.dropped(st)
        assert not d[head] and d[head + 1: head + 1 + n].all() and not d[head + 1 + n], p.name
        assert all(_dropped(*_at(st, j)) for j in (head + 1, head + n)) and not _dropped(*_at(st, head)) and not _dropped(*_at(st, head + 1 + n))
        assert (int(st[head]) ^ int(st[head + 1 + n])) & K and st[head + 1 + n] & F, "a kept fill of the other kind behind the run"
        m = wk.merged(st)
        at = head - int(np.count_nonzero(d[:head]))
        assert m[at] == (int(st[head]) & 0xC0000000) | p.facts["head_count"] and m[at + 1] == st[head + 1 + n], p.name
        whole = max(0, (head + 1 + n) // wk.PER_THREAD - (head + wk.PER_THREAD) // wk.PER_THREAD)   # threads inside words head + 1 .. head + n
        assert _units_that_keep_nothing(st, wk.PER_THREAD) == whole, p.name
    assert _units_that_keep_nothing(by_run[wk.PER_THREAD + 1].stream, wk.PER_THREAD) == 0      # (17 words inside two threads)
    assert _units_that_keep_nothing(by_run[wk.PER_WAVE].stream, wk.PER_THREAD) >= 62
    assert _units_that_keep_nothing(by_run[wk.TILE].stream, wk.PER_WAVE) == 3
    assert _units_that_keep_nothing(by_run[3 * wk.TILE + 5].stream, wk.TILE) == 2
    nothing = [p for p in plist if "nothing else" in p.name]
    assert {p.stream.size for p in nothing} == {1, wk.PER_THREAD, wk.TILE + 7}
    for p in nothing:
        assert wk.merged(p.stream).size == 0 and wk.groups(p.stream) == 0 and wk.report(p.stream)[2] == p.stream.size
        assert {int(x) for x in p.stream} == {F, 0xC0000000} or p.stream.size == 1
    to_end = [p for p in plist if "up to the end" in p.name]
    assert len(to_end) == 3 and max(p.stream.size for p in to_end) > wk.TILE
    for p in to_end:
        st, head = p.stream, p.facts["head"]
        d = wk.dropped(st)
        assert d[head + 1:].all() and not d[head] and not st[-1] & MASK and st[-1] & F
        m = wk.merged(st)
        assert m[-1] == 0xC0000000 | p.facts["head_count"] and wk.groups(st) == _at(st, head)[1] + p.facts["head_count"]
    between = plist[-1]
    m = wk.merged(between.stream)
    at = between.facts["head"] - int(np.count_nonzero(wk.dropped(between.stream)[: between.facts["head"]]))
    assert m[at: at + 3].tolist() == [0xC0000000 | 6, 0xC0000000 | 3, 0xC0000000 | 1]


def test_block_probes(probes):
    plist = probes["blocks"]
    assert {p.facts["k"] for p in plist} == set(wk.BLOCK_MULTIPLES)
    decided_by_the_cut = 0
    for p in plist:
        st, at, f = p.stream, p.facts["at"], p.facts
        b = f["k"] << 29
        for m, (drop, start) in enumerate(zip(f["dropped"], f["starts"])):
            x, pos, prev = _at(st, at + m)
            assert pos == start and x & F and _dropped(x, pos, prev) == drop, (p.name, m)
            if m and not drop:                                      # kept for the cut alone: one block, and it is dropped
                assert prev & F and prev & MASK and not (prev ^ x) & K
                decided_by_the_cut += 1
        assert not st[at - 1] & F and not st[at + len(f["dropped"])] & F, p.name
        ends = [s + (int(st[at + m]) & MASK) - 1 for m, s in enumerate(f["starts"])]
        if "ends at group B - 1" in p.name:
            assert ends[-1] == b - 1
        elif "ends at group B" in p.name:
            assert ends[-1] == b
        elif "starts at group B - 1" in p.name:
            assert f["starts"][0] == b - 1 and ends[0] >= b
        elif "starts at group B" in p.name:
            assert f["starts"][0] == b
        elif "chain" in p.name:
            assert f["starts"][1] == b and f["dropped"] == (False, False, True)
        else:                                                        # across an odd multiple of 2^28: not a cut
            assert f["starts"][0] < b - (1 << 28) <= ends[0] and f["dropped"] == (False, True)
        assert np.array_equal(wk.dropped(st)[at: at + len(f["dropped"])], f["dropped"])
        assert wk.groups(st) > f["starts"][-1] > b - (1 << 29)
    assert decided_by_the_cut == 3 * len(wk.BLOCK_MULTIPLES)
    assert max(wk.groups(p.stream) for p in plist) > 1 << 32


# ---- more than one round of the merge scan: by the oracle and by property -----------------------------------------------------
@pytest.mark.parametrize("name", list(wk.SCAN_ROUND_STREAMS))
def test_scan_round_streams(oracle, name):
    p = wk.scan_round_stream(name)
    st = p.stream
    n_tiles = p.facts["tiles"]
    assert st.size == n_tiles * wk.TILE and wk.groups(st) < wk.BLOCK // 8
    m = wk.merged(st)
    d = wk.dropped(st)
    assert m.size == st.size - int(np.count_nonzero(d))
    assert np.array_equal(oracle.decompress(m), oracle.decompress(st))
    assert wk.groups(m) == wk.groups(st) == oracle.decoded_groups(st)
    assert not np.any((m & F != 0) & (m & MASK == 0)), "an empty fill in the merged stream"
    assert not wk.dropped(m).any(), "a pair in the merged stream that the merger would drop"
    g, words, empty, lit, cross, unmerged, canonical = wk.report(st)
    assert (g, words) == (oracle.decoded_groups(st), oracle.decoded_words(g)) and empty == 0 and unmerged <= int(np.count_nonzero(d))
    assert wk.report(m)[5] == 0
    # the tiles differ in what they keep, neighbours too (outside the run): a scan that mixed up tiles inside a round would show
    per_tile = np.add.reduceat((~d).astype(np.int64), np.arange(0, st.size, wk.TILE))
    outside = np.ones(n_tiles, bool)
    if p.facts["run"] is not None:
        outside[p.facts["run"][0] // wk.TILE: p.facts["run"][1] // wk.TILE + 1] = False
    assert len(set(per_tile[outside].tolist())) >= 10 or outside.sum() < 10
    assert np.count_nonzero(np.diff(per_tile)[outside[1:] & outside[:-1]]) >= 0.8 * (outside.sum() - 3)
    # every round of 1024 tiles keeps words (the forward carry is not trivial), except the one the run covers
    kept = np.add.reduceat((~d).astype(np.int64), np.arange(0, st.size, wk.TILE))
    rounds = [int(kept[r: r + wk.SCAN_TILES].sum()) for r in range(0, n_tiles, wk.SCAN_TILES)]
    if p.facts["run"] is None:
        assert all(rounds) and len(rounds) == (n_tiles + wk.SCAN_TILES - 1) // wk.SCAN_TILES
        return
    lo, hi = p.facts["run"]
    assert lo % wk.PER_THREAD and hi % wk.PER_THREAD and not d[lo] and d[lo + 1: hi].all() and not d[hi]
    assert lo // wk.TILE // wk.SCAN_TILES < hi // wk.TILE // wk.SCAN_TILES, "the kept fill's count needs a first kept position from a later round"
    at = lo - int(np.count_nonzero(d[:lo]))
    count = int((st[lo: hi] & MASK).astype(np.uint64).sum())
    assert m[at] == (int(st[lo]) & 0xC0000000) | count and m[at + 1] == st[hi]
    if "keeps nothing" in name:
        assert rounds[1] == 0 and rounds[0] and rounds[2]
    else:
        assert all(rounds)
