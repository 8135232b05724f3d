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
        assert got == value, (f"{name} is {got} in gpu-wah_amd/csrc but tests/_switch.py THRESHOLDS says {value}: the probes no longer "
                              f"sit on the switch -- move {probes} (tests/_switch.py) with it and update THRESHOLDS")


def test_thresholds_are_the_sources_own():
    check_thresholds()
    # no pair count between the skipping and the swizzled pass 2: the plain variant is unreachable (and untested)
    assert _source_value("kPairSparseBelow") == _source_value("WAH_PAIR_SWIZZLE_FROM")
    with open(os.path.join(os.path.dirname(CSRC), "Makefile")) as f:
        makefile = f.read()
    assert "WAH_PAIR_SWIZZLE_FROM" not in makefile and "WAH_DT_MAXG" not in makefile  # (no target builds with other values)


def test_a_retuned_threshold_is_noticed(tmp_path):
    """A copy of the sources with WAH_PAIR_SWIZZLE_FROM / WAH_DT_MAXG moved by one: the message names the probe list."""
    for name, probes in (("WAH_PAIR_SWIZZLE_FROM", "PAIR_COUNTS"), ("WAH_DT_MAXG", "TILE_TOTALS")):
        copy = tmp_path / name
        copy.mkdir()
        for f in os.listdir(CSRC):
            with open(os.path.join(CSRC, f)) as h:
                text = h.read()
            text = re.sub(rf"(#define {name} )(\d+)", lambda m: m.group(1) + str(int(m.group(2)) + 1), text)
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
