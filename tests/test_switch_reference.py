"""CPU test of tests/_switch.py: every constructor has the property its name states (shown with the oracle), the thresholds
it restates are the ones in gpu-wah_amd/csrc, and every switch of its table has probes below, at and above its boundary
(the kernel's predicate restated in Python).

kPass2Plain, the pass-2 variant between kPairSparseBelow and kPairSwizzleFrom, does not exist while the two are equal:
test_thresholds_are_the_sources_own asserts that they are.
"""
import os
import re

import numpy as np
import pytest

from tests import _switch as sw

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-wah_amd", "csrc")

# name -> (file, expression whose group 1 is the value)
SOURCES = {
    "kScanTileWords": ("wah_internal.hpp", r"constexpr int kScanTileWords = (\d+);"),
    "kExpandWaves": ("wah_internal.hpp", r"constexpr int kExpandWaves = (\d+);"),
    "kMergeBlockShift": ("wah_aux.hip", r"constexpr u32 kMergeBlockShift = (\d+);"),
    "merge scan tiles": ("wah_aux.hip", r"__launch_bounds__\((\d+)\) void merge_scan_kernel\([\s\S]*?base < a\.n_tiles; base \+= (\d+)\)"),
    "walk vector load alignment": ("wah_aux.hip", r"\(reinterpret_cast<uintptr_t>\(comp\) & (\d+)u\) == 0 && tile_w0 \+ kScanTileWords <= c_words"),
    "kPairSparseBelow": ("wah_compress_pair.inc", r"constexpr u32 kPairSparseBelow = (\d+);"),
    "WAH_PAIR_SWIZZLE_FROM": ("wah_compress_pair.inc", r"#define WAH_PAIR_SWIZZLE_FROM (\d+)"),
    "WAH_DT_MAXG": ("wah_decode_tile.inc", r"#define WAH_DT_MAXG (\d+)"),
    "kDtTileWords": ("wah_decode_tile.inc", r"constexpr u32 kDtTileWords = (2u \* \(u32\)kScanTileWords);"),
    "kRunsMaxWordsPerSeg": ("wah_api.hip", r"constexpr uint64_t kRunsMaxWordsPerSeg = (\d+);"),
    "WAH_RUNS_LDS_WORDS": ("wah_bitop_runs.hip", r"#define WAH_RUNS_LDS_WORDS (\d+)"),
    "one pass up to": ("wah_api.hip", r"prefer_one_pass = .*out_capacity_words <= (\d+) \* c_words"),
    "one pass above": ("wah_api.hip", r"prefer_one_pass = .*out_capacity_words > (\d+) \* c_words"),
    "one pair per wave up to": ("wah_compress.hip", r"pairs <= (\d+) \? 1u :"),
    "two pairs per wave up to": ("wah_compress.hip", r"pairs <= (\d+) \? 2u :"),
    "one segment per wave up to": ("wah_compress.hip", r"if \(n_segments <= (\d+)\) return 1;"),
    "two segments per wave up to": ("wah_compress.hip", r"if \(n_segments <= (\d+)\) return 2;"),
    "WAH_TILE_WAVES": ("wah_internal.hpp", r"#define WAH_TILE_WAVES (\d+)"),
    "kNoWaitWaveSegs": ("wah_compress.hip", r"constexpr u32 kNoWaitWaveSegs = (\d+);"),
    "one-pass batch": ("wah_decode.hip", r"constexpr u32 batch = (\d+); // tiles per workgroup"),
    "runs shape spare": ("wah_bitop_runs.hip", r"fit = \(u64\)kRunsLdsWords \* a\.n_segments \* (\d+)u / (\d+)u;"),
    "runs image": ("wah_bitop_runs.hip", r"want = \(total \* kTileSegs \* (\d+)u / (\d+)u / a\.n_segments \+ (\d+)u\) & ~\(u64\)(\d+)u;"),
    "runs scan threads": ("wah_bitop_runs.hip", r"const u64 per = \(n_tiles \+ 1023u\) / (\d+)u;"),
    "sums offsets threads": ("wah_decode.hip", r"sums_offsets_kernel, dim3\(1\), dim3\((\d+)\)"),
    "kListShortFill": ("wah_list_walk.hpp", r"constexpr u32 kListShortFill = (\d+);"),
    "WAH_LIST_DEPTH": ("wah_list_walk.hpp", r"#define WAH_LIST_DEPTH (\d+)"),
    "list batch words": ("wah_list_walk.hpp", r"if \((\d+)u \* \(c\.b \+ 1u\) < cnt\)"),
    "list chunk operands": ("wah_list_walk.hpp", r"j0 < n_rows; j0 \+= (\d+)u\)"),
    "WAH_SEG_WAVES": ("wah_segdecode.hpp", r"#define WAH_SEG_WAVES (\d+)"),
    "list count clamp factor": ("wah_list_walk.hpp", r"n0 = in0 \? min\(word_groups\(w0\), (\d+)u \* kSegGroups\)"),
}


def _source_value(name, csrc=CSRC):
    file, pattern = SOURCES[name]
    with open(os.path.join(csrc, file)) as f:
        text = f.read()
    m = re.search(pattern, text)
    assert m, f"{name}: no longer defined as /{pattern}/ in {file} -- restate it in tests/_switch.py THRESHOLDS and in SOURCES here"
    if name == "kDtTileWords":  # two expand tiles
        scan = re.search(r"constexpr \w+ kScanTileWords = (\d+)", _read_all(csrc))
        assert scan, "kScanTileWords: definition not found"
        return 2 * int(scan.group(1))
    values = tuple(int(g) for g in m.groups())
    return values[0] if len(values) == 1 else values


def _read_all(csrc):
    out = []
    for f in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, f)) as h:
            out.append(h.read())
    return "\n".join(out)


def check_thresholds(csrc=CSRC):
    """Raises AssertionError naming the constant and the probe list of tests/_switch.py that has to move with it."""
    for name, (value, probes) in sw.THRESHOLDS.items():
        got = _source_value(name, csrc)
        where = "" if "(tests/" in probes else " (tests/_switch.py)"   # (the walk's probe lists name their own file)
        assert got == value, (f"{name} is {got} in gpu-wah_amd/csrc but tests/_switch.py THRESHOLDS says {value}: the probes no longer "
                              f"sit on the switch -- move {probes}{where} with it and update THRESHOLDS")


def test_thresholds_are_the_sources_own():
    check_thresholds()
    # no pair count between the skipping and the swizzled pass 2: the plain variant is unreachable (and untested)
    assert _source_value("kPairSparseBelow") == _source_value("WAH_PAIR_SWIZZLE_FROM")
    with open(os.path.join(os.path.dirname(CSRC), "Makefile")) as f:
        makefile = f.read()
    assert "WAH_PAIR_SWIZZLE_FROM" not in makefile and "WAH_DT_MAXG" not in makefile  # (no target builds with other values)
    assert "WAH_LIST_DEPTH" not in makefile and "WAH_SEG_WAVES" not in makefile


def test_a_retuned_threshold_is_noticed(tmp_path):
    """A copy of the sources with WAH_PAIR_SWIZZLE_FROM / WAH_DT_MAXG / WAH_LIST_DEPTH / kListShortFill / WAH_SEG_WAVES /
    kMergeBlockShift / kScanTileWords / kExpandWaves moved by one: the message names the probe list."""
    for name, probes in (("WAH_PAIR_SWIZZLE_FROM", "PAIR_COUNTS"), ("WAH_DT_MAXG", "TILE_TOTALS"), ("WAH_LIST_DEPTH", "LIST_SCHEDULES"),
                         ("kListShortFill", "LIST_FILL_GROUPS"), ("WAH_SEG_WAVES", "LIST_SEGMENTS"), ("kMergeBlockShift", "BLOCK_MULTIPLES"),
                         ("kScanTileWords", "WALK_EDGES"), ("kExpandWaves", "WALK_EDGES")):
        copy = tmp_path / name
        copy.mkdir()
        for f in os.listdir(CSRC):
            with open(os.path.join(CSRC, f)) as h:
                text = h.read()
            text = re.sub(rf"(#define {name} |constexpr (?:u32|int) {name} = )(\d+)", lambda m: m.group(1) + str(int(m.group(2)) + 1), text)
            (copy / f).write_text(text)
        with pytest.raises(AssertionError, match=rf"{name} is \d+ .* move {probes} "):
            check_thresholds(str(copy))


# ---- both sides of every switch, and the boundary itself --------------------------------------------------------------------
def _sides(values, predicate, boundary):
    """The probe values give the predicate both ways, and boundary - 1, boundary, boundary + 1 are among them."""
    got = {bool(predicate(v)) for v in values}
    assert got == {False, True}, (sorted(values), got)
    for v in (boundary - 1, boundary, boundary + 1):
        assert v in values, (v, "missing around", boundary)


def test_probe_lists_straddle_every_switch():
    counts = set(sw.PAIR_COUNTS)
    below, swizzle = sw.THRESHOLDS["kPairSparseBelow"][0], sw.THRESHOLDS["WAH_PAIR_SWIZZLE_FROM"][0]
    _sides(counts, lambda c: c < below, below)                       # pass 2: skipping variant
    _sides(counts, lambda c: c >= swizzle, swizzle)                  # pass 2: swizzled variant, park_pair's lane
    for t in range(1, 8):                                            # emit_pair: store t is issued
        _sides(counts, lambda c: 256 * t < c, 256 * t)
    assert {2046, 2047, 2048} <= counts                              # cnt == 2048 ...
    rng = np.random.default_rng(0)
    probes = sw.pair_probes(rng)
    full = [(name, bits) for name, c, bits in probes if c == sw.PAIR_GROUPS]
    kinds = {_all_literals(bits) for _, bits in full}                # ... && pair_all_literals: both ways
    assert kinds == {False, True}, [n for n, _ in full]
    assert sum(1 for _, b in full if not _all_literals(b)) >= 2 * len(sw.FULL_PAIR_FILL_AT)
    n0 = len(sw.pair_probes(np.random.default_rng(0), 0))            # (1st / 2nd / 3rd pair of a wave: the test below)
    for pad in sw.PAIR_PADDINGS:
        assert len(sw.pair_probes(np.random.default_rng(0), pad)) == n0 + pad
    limit = sw.DT_MAX_GROUPS
    _sides(set(sw.TILE_TOTALS), lambda g: g > limit, limit + 0)      # deferred[]: pos_total > kDtMaxGroups; the clamp n > kDtMaxGroups
    assert limit + 1 in sw.TILE_TOTALS and limit in sw.TILE_TOTALS
    c = 12345
    caps = sw.route_capacities(c)                                    # decode_common's default route
    lo, hi = sw.THRESHOLDS["one pass up to"][0], sw.THRESHOLDS["one pass above"][0]
    for cap, route in caps.items():
        assert route == (1 if cap <= lo * c or cap > hi * c else 2)
    assert {lo * c, lo * c + 1, hi * c, hi * c + 1} == set(caps) and sorted(caps.values()) == [1, 1, 2, 2]
    for s in (64, 700):                                              # bitop_runs_route: total > 112 S
        tot = sw.runs_totals(s)
        _sides(set(tot), lambda t: t > sw.RUNS_MAX_WORDS_PER_SEG * s, sw.RUNS_MAX_WORDS_PER_SEG * s)
        assert all(route == (2 if t > sw.RUNS_MAX_WORDS_PER_SEG * s else 1) for t, route in tot.items())
    for s in sw.RUNS_SHAPE_SEGMENTS:                                 # launch_bitop_runs: 256, 128 or 64 segments per workgroup
        fit = sw.RUNS_LDS_WORDS * s * 9 // 10
        totals = sw.runs_shape_totals(s)
        assert set(totals.values()) == {256, 128, 64}, (s, totals)
        for shape in (256, 128):
            _sides(set(totals), lambda t: t * shape <= fit, fit // shape)
        assert all(t <= sw.RUNS_MAX_WORDS_PER_SEG * s for t in totals)  # (all of them still take the run merge)
    assert {s % 256 for s in sw.RUNS_SHAPE_SEGMENTS} >= {0, 1, 63, 64, 255}
    assert (sw.MANY_TILES_64 + 63) // 64 == sw.SCAN_ROUND_TILES + 1 and (sw.MANY_TILES_256 + 255) // 256 == sw.SCAN_ROUND_TILES + 1


def _groups_of(bitmap):
    """The 31-bit groups of a bitmap of whole segments."""
    bits = np.unpackbits(np.ascontiguousarray(bitmap, "<u4").view(np.uint8), bitorder="little")
    assert bits.size % 31 == 0
    return (bits.reshape(-1, 31).astype(np.uint64) << np.arange(31, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def _all_literals(bitmap):
    g = _groups_of(bitmap)
    return not np.any((g == 0) | (g == sw.M31))


# ---- the constructors -------------------------------------------------------------------------------------------------------
def test_pack_is_the_oracles_group_order(oracle):
    rng = np.random.default_rng(1)
    g = rng.integers(0, 1 << 31, 1024 * 3, dtype=np.uint64).astype(np.uint32)
    bitmap = sw.pack(g)
    assert bitmap.size == 992 * 3
    assert all(oracle.group(bitmap, i) == int(g[i]) for i in (0, 1, 30, 31, 32, 1023, 1024, 3071))
    assert np.array_equal(_groups_of(bitmap), g)
    assert sw.pack(g[:5]).size == 5 and sw.pack(g[:33]).size == 32


@pytest.mark.parametrize("placement", sw.PLACEMENTS)
@pytest.mark.parametrize("fill_bit", [0, 1])
def test_segment_compresses_to_the_stated_words(oracle, placement, fill_bit):
    rng = np.random.default_rng(2)
    fill = (sw.FILL1 if fill_bit else sw.FILL0)
    for words in (1, 2, 3, 4, 31, 32, 33, 191, 192, 193, 511, 512, 1022, 1023, 1024):
        seg = sw.segment(words, placement, fill_bit, rng)
        comp = oracle.compress(seg)
        assert seg.size == sw.SEG_WORDS and comp.size == words, (words, placement, comp.size)
        long_fill = fill | (sw.SEG_GROUPS - (words - 1))
        if placement == "front":
            assert comp[-1] == long_fill and not np.any(comp[:-1] & sw.FILL0)
        elif placement == "behind":
            assert comp[0] == long_fill and not np.any(comp[1:] & sw.FILL0)
        else:  # lone fill groups: a fill word of ONE group at every second place, never merged with a neighbour
            assert comp[-1] == long_fill and not comp[-2:-1].any() & sw.FILL0
            lone = comp[:-1][(comp[:-1] & sw.FILL0) != 0]
            assert lone.size == (words - 1) // 2 and np.all(lone == (fill | 1)), (words, lone[:4])
    assert np.all(oracle.compress(sw.segment(1024, "literals", 0, rng)) < sw.FILL0)


def test_pairs_compress_to_the_stated_words(oracle):
    rng = np.random.default_rng(3)
    probes = sw.pair_probes(rng, padding=2)
    assert {c for _, c, _ in probes} >= set(sw.PAIR_COUNTS)
    for name, c, bits in probes:
        assert bits.size == 2 * sw.SEG_WORDS, name
        a, b = oracle.compress(bits[: sw.SEG_WORDS]), oracle.compress(bits[sw.SEG_WORDS:])
        assert a.size + b.size == c == oracle.compress(bits).size, (name, a.size, b.size)
    for c in sw.PAIR_COUNTS:  # the splits are what they say
        assert sw.split_counts(c, "even") == (c // 2, c - c // 2)
        first = sw.split_counts(c, "most first")
        assert first == ((c - 1, 1) if c <= 1025 else (1024, c - 1024)) and sw.split_counts(c, "most last") == first[::-1]
    bitmap, counts = sw.probe_bitmap(np.random.default_rng(3), padding=1)
    assert oracle.compress(bitmap).size == sum(counts) and bitmap.size == 1984 * len(counts)
    # more than 112 words per segment on average: the indexed bit operation on it takes the decode-based route
    assert sum(counts) > sw.RUNS_MAX_WORDS_PER_SEG * 2 * len(counts)


def test_full_pairs_with_one_fill_group(oracle):
    rng = np.random.default_rng(4)
    for at in sw.FULL_PAIR_FILL_AT:
        for ones in (0, 1):
            bits = sw.full_pair_with_fill(at, ones, rng)
            comp = oracle.compress(bits)
            assert comp.size == sw.PAIR_GROUPS and not _all_literals(bits)
            assert comp[at] == ((sw.FILL1 if ones else sw.FILL0) | 1)
            assert np.count_nonzero(comp & sw.FILL0) == 1
    assert 0 < (sw.FULL_PAIR_FILL_AT[-1] % 32) < 31


def test_ragged_ends(oracle):
    rng = np.random.default_rng(5)
    groups = []
    for w in sw.LAST_SEGMENT_WORDS:
        bitmap = sw.ragged_end_bitmap(rng, w)
        g = oracle.decoded_groups(oracle.compress(bitmap))
        assert (g // 1024) % 2 == 1, "the short segment is the SECOND of its pair"
        groups.append(g % 1024)
    assert groups == [2, 31, 32, 34, 1023]
    lone = sw.ragged_end_bitmap(rng, 0, lone_segment=True)
    assert lone.size % sw.SEG_WORDS == 0 and (lone.size // sw.SEG_WORDS) % 2 == 1


@pytest.mark.parametrize("way", sw.TILE_WAYS)
@pytest.mark.parametrize("total", sw.TILE_TOTALS)
def test_tile_limit_streams(oracle, total, way):
    rng = np.random.default_rng(6)
    for place in sw.TILE_PLACES:
        st, t, groups = sw.tile_limit_stream(total, way, place, rng)
        lo = t * sw.DT_TILE_WORDS
        tile = st[lo: lo + sw.DT_TILE_WORDS]
        assert oracle.decoded_groups(tile) == groups == sw.tile_groups(st, t)
        if way == "single count" and place != "last":
            assert groups == total + sw.DT_TILE_WORDS - 1 and np.count_nonzero(tile & sw.FILL0) == 1
        else:
            assert groups == total
        if way == "single count":
            assert int((tile[(tile & sw.FILL0) != 0] & 0x3FFFFFFF).max()) == total
        assert (tile.size < sw.DT_TILE_WORDS) == (place == "last")
        if place == "second of a batch":
            assert t % 2 == 1
        if place == "middle":
            assert t % 2 == 0 and 0 < t < st.size // sw.DT_TILE_WORDS - 1
        # the neighbouring tiles are plain literals
        for n in (t - 1, t + 1):
            if 0 <= n and (n + 1) * sw.DT_TILE_WORDS <= st.size:
                assert not np.any(st[n * sw.DT_TILE_WORDS: (n + 1) * sw.DT_TILE_WORDS] & sw.FILL0)
        assert oracle.decompress(st).size == oracle.decoded_words(oracle.decoded_groups(st))


def test_other_tile_streams(oracle):
    rng = np.random.default_rng(7)
    st = sw.tile_with_empty_fill(rng)
    assert sw.tile_groups(st, 1) < sw.DT_MAX_GROUPS // 2 and np.count_nonzero(st == sw.FILL0) == 1
    alt = sw.alternating_tile_stream(rng)
    n = alt.size // sw.DT_TILE_WORDS
    assert [sw.tile_groups(alt, t) for t in range(n)] == [sw.DT_MAX_GROUPS + t % 2 for t in range(n)] and alt.size % sw.DT_TILE_WORDS


def test_operands_with_exact_totals(oracle):
    rng = np.random.default_rng(8)
    for k, s, total in ((2, 64, 112 * 64), (2, 64, 112 * 64 + 1), (5, 70, 112 * 70), (5, 70, 112 * 70 + 1), (3, 513, 36 * 513 - 1),
                        (2, 300, 2 * 300), (8, 65, 72 * 65 + 1)):
        maps = sw.operands_with_total(k, s, total, rng)
        assert len(maps) == k and all(m.size == s * sw.SEG_WORDS for m in maps)
        assert sum(oracle.compress(m).size for m in maps) == total, (k, s, total)


def test_dense_tile_exceeds_the_lds_image(oracle):
    """bitop_runs_kernel stages a tile's operand words in LDS when they fit the image (launch_runs_k sizes it): with eight
    incompressible segments in one tile that tile does not, every other one does."""
    rng = np.random.default_rng(9)
    s = 1024
    for tile in (0, 3):
        maps = sw.operands_with_dense_tile(2, s, tile, rng)
        per_seg = np.stack([[oracle.compress(m[sw.SEG_WORDS * i: sw.SEG_WORDS * (i + 1)]).size for i in range(s)] for m in maps]).sum(axis=0)
        total = int(per_seg.sum())
        assert sw.runs_shape(total, s) == 256 and total <= sw.RUNS_MAX_WORDS_PER_SEG * s
        image = sw.runs_lds_image_words(total, s, 256)
        tiles = per_seg.reshape(-1, 256).sum(axis=1)
        assert [int(t) > image for t in tiles] == [t == tile for t in range(4)], (tiles, image)


def test_tile_of_exactly_the_lds_image(oracle):
    """staged = tile words <= image: a tile of exactly the image's words and one of a word more, in the first and the last tile."""
    rng = np.random.default_rng(10)
    s, k = 1024, 2
    w = sw.lds_boundary_tile_words(k, s)
    for tile in (0, 3):
        for words, staged in ((w, True), (w + 1, False)):
            maps = sw.operands_with_tile_words(k, s, tile, words, rng)
            per_seg = np.stack([[oracle.compress(m[sw.SEG_WORDS * i: sw.SEG_WORDS * (i + 1)]).size for i in range(s)] for m in maps]).sum(axis=0)
            total = int(per_seg.sum())
            assert sw.runs_shape(total, s) == 256 and total <= sw.RUNS_MAX_WORDS_PER_SEG * s
            image = sw.runs_lds_image_words(total, s, 256)
            tiles = [int(t) for t in per_seg.reshape(-1, 256).sum(axis=1)]
            assert tiles[tile] == words and (tiles[tile] <= image) == staged and image == w, (tiles, image)
            assert all(t <= image for i, t in enumerate(tiles) if i != tile)


def test_every_probe_pair_lands_in_every_slot_of_every_shape():
    """compress_tile_shape restated (sw.tile_shape): the bitmaps of PAIR_PADDINGS and SHAPE_CASES put EVERY probe pair into
    every slot j of one, two and three pairs per wave on the one-launch routes -- in the body and in the tails of one and two
    -- and into both slots of the no-wait routes; and each SHAPE_CASES bitmap runs the kernel instance it names."""
    n_probes = len(sw.pair_probes(np.random.default_rng(0)))
    fronts = {f"padding {p}": p for p in sw.PAIR_PADDINGS}
    fronts.update({name: front for name, (front, _) in sw.SHAPE_CASES.items()})
    seen = {"one launch": [set() for _ in range(n_probes)], "no wait": [set() for _ in range(n_probes)]}
    instances = set()
    for name, front in fronts.items():
        n_pairs = front + n_probes
        body, tail, body_pairs = sw.tile_shape(n_pairs)
        instances.add((body, tail))
        if name in sw.SHAPE_CASES:
            assert (body, tail) == sw.SHAPE_CASES[name][1], (name, body, tail)
            assert body_pairs <= front or body == tail, "the probes lie in ONE kind of tile"
        for route, slots in seen.items():
            for i in range(n_probes):
                k, j = sw.pair_slot(front + i, n_pairs, route)
                in_tail = route == "one launch" and body != tail
                slots[i].add((k, j, in_tail))
    want = {(1, 0, False)} | {(2, j, False) for j in range(2)} | {(3, j, False) for j in range(3)} | {(1, 0, True)} | {(2, j, True) for j in range(2)}
    assert all(s == want for s in seen["one launch"]), seen["one launch"][0] ^ want
    assert all(s == {(2, 0, False), (2, 1, False)} for s in seen["no wait"])
    assert instances == {(1, 1), (2, 2), (3, 3), (3, 1), (3, 2)}
    # the rule itself at its edges (MI355X: 512 slots, a round of 12 288 pairs)
    assert [sw.tile_shape(p)[:2] for p in (1, 1400, 1401, 3000, 3001, 12287, 12288, 12289, 12288 + 4096, 12288 + 4097, 12288 + 8192,
                                           12288 + 8193, 2 * 12288)] == [(1, 1), (1, 1), (2, 2), (2, 2), (3, 3), (3, 3), (3, 3), (3, 1), (3, 1), (3, 2),
                                                                         (3, 2), (3, 3), (3, 3)]
    # compress_tile_body (wah_bitop_device) takes one, two or five segments per wave: a case in each class
    assert [sw.wave_segs(2 * (fronts[name] + n_probes)) for name in ("padding 0", "two pairs per wave, shift 0", "three pairs per wave, shift 0")] == [1, 2, 5]
    bitmap, pairs = sw.shaped_probe_bitmap(np.random.default_rng(1), 5)
    assert pairs == 5 + n_probes and bitmap.size == pairs * 2 * sw.SEG_WORDS and not bitmap[: 5 * 2 * sw.SEG_WORDS].any()


# ---- the operand-list bit operation ------------------------------------------------------------------------------------------
def _segment_streams(oracle, bitmap):
    """[(the oracle's words of a segment, its groups)] of a bitmap."""
    out = []
    for lo in range(0, bitmap.size, sw.SEG_WORDS):
        part = bitmap[lo: lo + sw.SEG_WORDS]
        out.append((oracle.compress(part), (32 * part.size + 30) // 31))
    return out


def _is_layout(comp, layout):
    """comp is list_layout_words(layout): the fills where it says, with their counts, literals elsewhere."""
    want = sw.list_layout_words(layout)
    fills = want != 0
    return comp.size == want.size and np.array_equal(comp[fills], want[fills]) and not np.any(comp[~fills] & sw.FILL0)


def test_list_segments_compress_to_the_stated_words(oracle):
    rng = np.random.default_rng(20)
    probes = sw.list_words_probes()
    assert {w for w, _, _, _ in probes} == set(sw.LIST_SEGMENT_WORDS) >= {1, 2, 127, 128, 129, 255, 256, 257, 384, 511, 512, 513, 1023, 1024}
    for way in sw.LIST_WAYS:  # every way gives every count it can give: all of them but the few a way excludes by its nature
        assert {w for w, y, _, _ in probes if y == way} >= {w for w in sw.LIST_SEGMENT_WORDS if w > sw.LIST_BATCH}, way
    assert {b for _, _, b, _ in probes} == {0, 1}
    for words, way, bit, layout in probes:
        seg = sw.list_segment(layout, rng)
        comp = oracle.compress(seg)
        assert seg.size == sw.SEG_WORDS and comp.size == words and _is_layout(comp, layout), (words, way)
        fill = np.flatnonzero(comp & sw.FILL0)
        if way == "fill ends a batch":
            assert fill[0] % sw.LIST_BATCH == sw.LIST_BATCH - 1 and fill[0] + 1 == words // sw.LIST_BATCH * sw.LIST_BATCH, (words, fill)
        elif way == "fill starts the next batch":
            assert list(fill) == [(words - 1) // sw.LIST_BATCH * sw.LIST_BATCH], (words, fill)
        elif way == "fill first":
            assert list(fill) == [0]
        else:
            assert list(fill) == ([words - 1] if words < sw.SEG_GROUPS else [])
    bitmap = sw.list_probe_bitmap([p[3] for p in probes], rng)
    assert [w.size for w, _ in _segment_streams(oracle, bitmap)] == [p[0] for p in probes]


def test_list_fills_are_where_they_are_stated(oracle):
    rng = np.random.default_rng(21)
    probes = sw.list_fill_probes()
    assert {(wi, n) for wi, _, n, _ in probes} >= {(wi, n) for wi in sw.LIST_FILL_WORD_INDEX for n in sw.LIST_FILL_GROUPS}
    assert {1, 2, 7, 8, 9, 63, 64, 65, 128, 129} <= set(sw.LIST_FILL_GROUPS) and set(sw.LIST_FILL_WORD_INDEX) == {0, 1, 126, 127, 128, 129, 255, 256}
    for wi, bit, n, total in probes:
        seg = sw.list_fill_at(wi, bit, n, total, rng)
        comp = oracle.compress(seg)
        assert comp.size == total and comp[wi] == ((sw.FILL1 if bit else sw.FILL0) | n), (wi, bit, n, total)
        assert not np.any(comp[:wi] & sw.FILL0), "literals in front: the fill starts at group wi"
        assert np.count_nonzero(comp & sw.FILL0) == (2 if total > wi + 1 else 1)
        assert _is_layout(comp, sw.list_fill_layout(wi, bit, n, total))
    for layout in sw.list_many_fills_layouts():
        assert _is_layout(oracle.compress(sw.list_segment(layout, rng)), layout)


def test_list_schedules_hold_the_stated_words(oracle):
    rng = np.random.default_rng(22)
    for schedule in sw.LIST_SCHEDULES:
        n_segments = 5 if len(schedule) <= sw.LIST_CHUNK else 2
        for bit in (0, 1):
            maps = sw.list_schedule_operands(schedule, bit, n_segments, rng)
            counts = sw.list_schedule_counts(schedule, n_segments)
            assert len(maps) == len(schedule) and counts[0] == list(schedule)
            got = [[w.size for w, _ in _segment_streams(oracle, m)] for m in maps]
            assert [list(c) for c in zip(*got)] == counts, schedule
            ones = [int(w[0]) for m in maps for w, _ in _segment_streams(oracle, m) if w.size == 1]
            assert all(w == ((sw.FILL1 if bit else sw.FILL0) | sw.SEG_GROUPS) for w in ones)


def test_list_ragged_ends(oracle):
    rng = np.random.default_rng(23)
    groups = []
    for tail in sw.LAST_SEGMENT_WORDS:
        ways = sw.list_ragged_layouts(tail)
        for name, layout in ways.items():
            bitmap = sw.list_probe_bitmap([[("lit", 1024)]], rng, tail=(layout, tail))
            assert bitmap.size == sw.SEG_WORDS + tail
            comp, nvalid = _segment_streams(oracle, bitmap)[1]
            assert nvalid == sum(n for _, n in layout) and oracle.decoded_groups(comp) == nvalid
            if name == "zeros":
                assert list(comp) == [sw.FILL0 | nvalid]
            elif name == "ones":
                assert comp[0] == (sw.FILL1 | (nvalid if comp.size == 1 else nvalid - 1)) and comp.size == (1 if tail % 31 == 0 else 2)
            else:
                assert comp.size == nvalid and not np.any(comp & sw.FILL0)
        groups.append(nvalid)
    assert groups == [2, 31, 32, 34, 1023]


def test_list_tables_and_refusals(oracle):
    rng = np.random.default_rng(24)
    pool = sw.list_pool(rng)
    assert all(p.size == 3 * sw.SEG_WORDS for p in pool[1:])
    for op in sw.LIST_OPS:
        pool[0] = sw.list_trivial(op, pool[1].size)
        for w, nvalid in _segment_streams(oracle, pool[0]):
            assert sw.list_paths(w, nvalid, op)["settled"] and sw.list_paths(w, nvalid, op, first=True)["settled"]
        for k in (1, 2, 5, 9, 64, 129):  # list_fold is the plain fold of the stacked rows
            rows = sw.list_table_rows(k, len(pool))
            fold = {"and": np.bitwise_and.reduce, "or": np.bitwise_or.reduce, "xor": np.bitwise_xor.reduce}.get(op)
            stack = np.stack([pool[i] for i in rows])
            want = fold(stack) if fold else (stack[0] & ~np.bitwise_or.reduce(stack[1:]) if k > 1 else stack[0])
            assert np.array_equal(sw.list_fold(op, pool, rows), want), (op, k)
        for name, (n_rows, placed) in sw.LIST_PLACED.items():
            rows = sw.list_table_rows(n_rows, len(pool), placed)
            assert len(rows) == n_rows and all(rows[r] == e for r, e in placed.items()) and sum(1 for e in rows if e) == len(placed)
    a = pool[1]
    n_rows, placed = sw.LIST_PLACED["row 0 again in rows 64 and 128"]
    rows = sw.list_table_rows(n_rows, len(pool), placed)
    assert not sw.list_fold("andnot", [sw.list_trivial("andnot", a.size)] + pool[1:], rows).any() and a.any()   # A and not A
    valid = [w for w, _ in _segment_streams(oracle, pool[2])]
    for name, words in sw.list_refusals(rng):
        assert 1 <= words.size <= sw.SEG_GROUPS and words.dtype == np.uint32, name
        for op in sw.LIST_OPS:
            for first in (False, True):
                path = sw.list_paths(words, sw.SEG_GROUPS, op, first)
                assert not path["settled"] and not path["ok"], (name, op)
                for b in path["batches"]:  # nothing is put outside the accumulator: every applied word ends at or below group 1024
                    assert all(p + n <= sw.SEG_GROUPS for way, n, p in b["words"] if way not in ("outside", "empty", "identity")), name
        stream, index = sw.list_refused_stream(valid, 1, words)
        assert index[0] == 0 and index[-1] == stream.size and np.all(np.diff(index) >= 1) and np.array_equal(stream[index[1]: index[2]], words)
        assert np.array_equal(stream[: index[1]], valid[0]) and np.array_equal(stream[index[2]:], valid[2])


def test_list_probes_reach_every_path(oracle):
    """list_paths() over the oracle's streams of the probe bitmaps of tests/test_gpu_switch_points.py: every predicate of the
    list kernel is seen true and false, with the boundary and its neighbours where it is a comparison."""
    rng = np.random.default_rng(25)
    segments = []  # (words, nvalid)
    words_bitmap = sw.list_probe_bitmap([p[3] for p in sw.list_words_probes()], rng)
    fills_bitmap = sw.list_probe_bitmap([sw.list_fill_layout(wi, bit, n, total) for wi, bit, n, total in sw.list_fill_probes()]
                                        + sw.list_many_fills_layouts(), rng)
    segments += _segment_streams(oracle, words_bitmap) + _segment_streams(oracle, fills_bitmap)
    for tail in sw.LAST_SEGMENT_WORDS:
        for layout in sw.list_ragged_layouts(tail).values():
            segments.append(_segment_streams(oracle, sw.list_probe_bitmap([], rng, tail=(layout, tail)))[0])
    refused = [w for _, w in sw.list_refusals(rng)]
    for op in sw.LIST_OPS:
        for first in (False, True):
            paths = [sw.list_paths(w, nv, op, first) for w, nv in segments]
            assert all(p["ok"] for p in paths)
            batches = [b for p in paths for b in p["batches"]]
            ways = {way for b in batches for way, _, _ in b["words"]}
            assert ways == {"fast", "literal", "identity", "own first", "own rest", "wave"}, (op, first, ways)
            # identity or effect: both kinds of fill both ways (list_op); under ANDNOT row 0 is applied as OR
            effect_kind = sw.FILL0 if (op == "and") else sw.FILL1
            kinds = {(int(w[wi0 + i]) & sw.FILL1, way != "identity") for (w, _), p in zip(segments, paths)
                     for wi0, b in zip(range(0, 1024, sw.LIST_BATCH), p["batches"]) if not b["fast"]
                     for i, (way, _, _) in enumerate(b["words"]) if int(w[wi0 + i]) & sw.FILL0}
            assert kinds == {(effect_kind, True), (effect_kind ^ 0x40000000, False)}, (op, first, kinds)
            # kListShortFill; the first store alone, list_put_rest, list_put_long and its steps of 64 groups
            effect = [(n, p, i) for b in batches for i, (way, n, p) in enumerate(b["words"]) if way in ("own first", "own rest", "wave")]
            counts = {n for n, _, _ in effect}
            _sides(counts, lambda n: n <= sw.LIST_SHORT_FILL, sw.LIST_SHORT_FILL)
            _sides(counts, lambda n: n > 1, 2)                     # s0 > 1: list_put_rest
            _sides(counts, lambda n: n >= 64, 64)                  # lane 63 has a group in the first step
            _sides(counts, lambda n: n > 128, 128)                 # a third step
            assert {True, False} == {b["rest"] for b in batches if not b["fast"]}
            wave = [(n, p, i) for n, p, i in effect if n > sw.LIST_SHORT_FILL]
            assert {p % 64 == 0 for _, p, _ in wave} == {True, False}
            assert {i for _, _, i in wave} >= {0, 1, sw.LIST_BATCH - 2, sw.LIST_BATCH - 1}   # lane 0 and lane 63, w0 and w1
            assert {i for n, _, i in effect if 1 < n <= sw.LIST_SHORT_FILL} >= {0, 1, sw.LIST_BATCH - 2, sw.LIST_BATCH - 1}
            # list_put_long's mask: many long fills in one batch, in the lanes' first words and in their second ones
            for parity in (0, 1):
                assert max(sum(1 for i, (way, _, _) in enumerate(b["words"]) if way == "wave" and i % 2 == parity) for b in batches) >= 56
                assert max(sum(1 for i, (way, _, _) in enumerate(b["words"]) if way == "own rest" and i % 2 == parity) for b in batches) >= 10
            assert any({"wave", "own rest", "own first", "identity", "literal"} <= {way for way, _, _ in b["words"]} for b in batches)
            # the batches of a segment: 128 (b + 1) < cnt, and which batch is the last
            live = [(w.size, p) for (w, _), p in zip(segments, paths) if not p["settled"]]
            sizes = {c for c, _ in live}
            for b in range(1, 8):
                _sides(sizes, lambda c: sw.LIST_BATCH * b < c, sw.LIST_BATCH * b)
            assert {len(p["batches"]) for _, p in live} == set(range(1, 9))
            assert all((len(p["batches"]) == (c + sw.LIST_BATCH - 1) // sw.LIST_BATCH) and [b["last"] for b in p["batches"]] == [False] * (len(p["batches"]) - 1) + [True]
                       for c, p in live)
            # the fast path: each of its three conditions decides somewhere
            assert {(b["fast"], b["last"]) for b in batches} == {(True, True), (True, False), (False, True), (False, False)}
            general = [b for b in batches if not b["fast"]]
            assert any(b["full"] for b in general) and any(not b["full"] and all(way == "literal" for way, _, _ in b["words"]) for b in general)
            assert any(b["full"] and sum(1 for way, _, _ in b["words"] if way != "literal") == 1 and b["words"][-1][0] != "literal" for b in general)
            assert sw.SEG_GROUPS - sw.LIST_BATCH in {b["pos"] for b in batches if b["fast"]}       # pos + 128 == 1024 ...
            late = [sw.list_paths(w, sw.SEG_GROUPS, op, first) for w in refused]                   # ... and 1025: only when refused
            assert any(not b["fast"] and b["full"] and b["pos"] == sw.SEG_GROUPS - sw.LIST_BATCH + 1 and all(way in ("literal", "outside") for way, _, _ in b["words"])
                       for p in late for b in p["batches"])
            # the settled test: each of its four conditions decides somewhere
            one = [(int(w[0]), nv, p["settled"]) for (w, nv), p in zip(segments, paths) if w.size == 1]
            assert {(s, nv == sw.SEG_GROUPS) for _, nv, s in one} == {(True, True), (True, False), (False, True), (False, False)}, (op, first)
            assert any(p["settled"] is False and w.size == 2 and w[0] & sw.FILL0 for (w, _), p in zip(segments, paths))  # cnt == 2
            lone = [sw.list_paths(w, sw.SEG_GROUPS, op, first) for w in refused if w.size == 1]
            assert lone and not any(p["settled"] or p["ok"] for p in lone)                          # a literal
            for nv in (2, 31, 1024):                                                                 # a count that is not nvalid
                ident = (sw.FILL1 if op == "and" else sw.FILL0)
                assert sw.list_paths([ident | nv], nv, op, first)["settled"]
                for d in (-1, 1):
                    wrong = sw.list_paths([ident | (nv + d)], nv, op, first)
                    assert not wrong["settled"] and not wrong["ok"]
    # the clamp of a count
    _sides(set(sw.LIST_BAD_COUNTS), lambda n: n > sw.LIST_CLAMP, sw.LIST_CLAMP)
    assert sw.COUNT_MASK in sw.LIST_BAD_COUNTS and sw.LIST_BATCH * sw.LIST_CLAMP < 2**32 <= sw.LIST_BATCH * sw.COUNT_MASK
    # 64 operands a chunk: the tables' lengths, the rows of a live operand
    for chunk in (sw.LIST_CHUNK, 2 * sw.LIST_CHUNK):
        _sides(set(sw.LIST_OPERAND_COUNTS), lambda k: k > chunk, chunk)
    assert max(sw.LIST_OPERAND_COUNTS) > 64 * sw.LIST_CHUNK
    _sides(set(sw.LIST_POSITIONS), lambda r: r >= sw.LIST_CHUNK, sw.LIST_CHUNK)            # j0 += 64: the second chunk
    lanes = {r % sw.LIST_CHUNK for r in sw.LIST_POSITIONS}
    assert {0, 1, sw.LIST_CHUNK - 2, sw.LIST_CHUNK - 1} <= lanes                              # c.j >= 63u: lanes 62 and 63
    assert {r for r in sw.LIST_POSITIONS if r % sw.LIST_CHUNK == 0} >= {0, sw.LIST_CHUNK, 2 * sw.LIST_CHUNK}   # j0 + cons.j == 0u: lane 0 of every chunk
    assert any(set(pl) >= {sw.LIST_CHUNK - 2, sw.LIST_CHUNK - 1} for _, pl in sw.LIST_PLACED.values())       # live lanes 62 AND 63
    # kSegDecodeWaves segments a workgroup
    _sides(set(sw.LIST_SEGMENTS), lambda s: s > sw.SEG_WAVES, sw.SEG_WAVES)
    assert {(-s) % sw.SEG_WAVES for s in sw.LIST_SEGMENTS} >= {0, 1, sw.SEG_WAVES - 1}       # idle waves of the last workgroup
    # kListDepth batches in flight: the batches of a chunk, the operand boundaries between consumer and producer
    totals, ahead, between, all_settled_then_live = set(), set(), False, False
    for schedule in sw.LIST_SCHEDULES:
        for op in sw.LIST_OPS:
            for bit in (0, 1):
                word = (sw.FILL1 if bit else sw.FILL0) | sw.SEG_GROUPS
                settled = sw.list_paths([word], sw.SEG_GROUPS, op)["settled"]
                for counts in sw.list_schedule_counts(schedule, 5 if len(schedule) <= sw.LIST_CHUNK else 2):
                    chunks = [counts[j0: j0 + sw.LIST_CHUNK] for j0 in range(0, len(counts), sw.LIST_CHUNK)]
                    lives = [[c for c in chunk if not (c == 1 and settled)] for chunk in chunks]
                    for chunk, alive in zip(chunks, lives):
                        totals.add(sum((c + sw.LIST_BATCH - 1) // sw.LIST_BATCH for c in alive))
                        ahead |= set(sw.list_chunk_rotation(alive))
                        flags = [not (c == 1 and settled) for c in chunk]
                        between |= any(flags[i] and not flags[i + 1] and any(flags[i + 2:]) for i in range(len(flags) - 2))
                    all_settled_then_live |= len(lives) > 1 and not lives[0] and bool(lives[1])
    _sides(totals, lambda b: b > sw.LIST_DEPTH, sw.LIST_DEPTH)
    assert {0, 1, 3, 4, 5, 8} <= totals and max(totals) >= 9, totals
    assert {0, 1, 2, sw.LIST_CHUNK} <= ahead, ahead
    assert between and all_settled_then_live
