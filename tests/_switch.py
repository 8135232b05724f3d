"""Inputs that sit exactly ON the integer thresholds at which the kernels change code, and the table of those thresholds.

TEST INFRASTRUCTURE (tests/test_switch_reference.py proves every constructor with the oracle on the CPU,
tests/test_gpu_switch_points.py runs the inputs through the kernels).

The switches (gpu-wah_amd/csrc) and the probes that sit on them:

  switch                                   where                                  probes
  ---------------------------------------  -------------------------------------  ------------------------------------------
  words of a segment pair < / >= 384       wah_compress_pair.inc (pass 2 variant  PAIR_COUNTS (383, 384, 385)
    (kPairSparseBelow, kPairSwizzleFrom)   and park_pair's lane: pair_pass2_park,
                                           run by both pair-layout bodies)
  pair of 2048 words, all literals or not  wah_compress_pair.inc                  PAIR_COUNTS (2046 .. 2048), FULL_PAIR_FILL_AT
    (store_literals / swizzled pass 2)       (pair_all_literals)
  256 t < count, t = 0 .. 7                emit_pair                              PAIR_COUNTS (256 k - 1, 256 k, 256 k + 1)
  1st / 2nd / 3rd pair of a wave, the      compress_pair_body, compress_tile_     SHAPE_CASES (the probes in every size class of
    kernel instances <1,1> <2,2> <3,3>       shape, with_tile_shape                 compress_tile_shape, shifted by 0, 1, 2 pairs),
    <3,1> <3,2>; two pairs (no wait)                                                PAIR_PADDINGS
  one-pass tile <= 61440 groups            wah_decode_tile.inc (deferred[],       TILE_TOTALS x TILE_WAYS x TILE_PLACES,
    (WAH_DT_MAXG x 1024), one count above    the clamp of a single count)           alternating_tile_stream
  out_capacity <= 7 c or > 40 c            wah_api.hip (decode_common)            route_capacities
  operands' words <= 112 per segment       wah_api.hip (kRunsMaxWordsPerSeg)      RUNS_ROUTE_TOTALS
  total * 256 <= fit, total * 128 <= fit   wah_bitop_runs.hip (launch_bitop_runs) RUNS_SHAPE_TOTALS, RUNS_SHAPE_SEGMENTS
    (fit = WAH_RUNS_LDS_WORDS x S x 9/10)
  a tile's words <= the LDS image          wah_bitop_runs.hip (staged)            lds_boundary_tile_words (the image, + 1),
                                                                                  operands_with_dense_tile (far above it)
  more than 1024 tiles                     bitop_runs_scan_kernel (per >= 2),     MANY_TILES_*; a stream of > 1024 x 4096 words
                                           sums_offsets_kernel, wah_decode.hip

The operand-list bit operation (wah_bitop_list.hip; list_paths() restates which way every batch and word of a segment goes):

  64 operands per chunk, one per lane      list_gather, j0 += 64, list_advance's  LIST_OPERAND_COUNTS, LIST_POSITIONS (a live operand in
    (row 0 alone takes m_first)              c.j >= 63u, op_of: j == 0u             rows 0, 1, 62 .. 65, 128; row 0 again in 64, 128)
  128 words per batch                      list_advance, list_issue,              LIST_SEGMENT_WORDS (128 b - 1, 128 b, 128 b + 1) x
                                             list_apply_batch                       LIST_WAYS
  kListDepth = 4 batches in flight         the producer / consumer rotation       LIST_SCHEDULES (0, 1, 3, 4, 5, 8 and more batches a
                                                                                    chunk; list_chunk_rotation)
  a full batch of literals                 list_apply_batch's fast path           LIST_WAYS ("fill ends a batch", "fill starts the next
                                                                                    batch", "fill first": a fast batch that ends AT 1024)
  kListShortFill = 8; 64 groups a step     s0 / s1, list_put_rest, list_put_long  LIST_FILL_GROUPS x LIST_FILL_WORD_INDEX
  identity or effect                       list_op, eff0 / eff1, the settled test both kinds of fill under all of LIST_OPS
  one-word segment settled                 list_gather                            list_fill_probes (one word), list_ragged_layouts
  kSegDecodeWaves = 4 segments a           wah_segdecode.hpp, the grid            LIST_SEGMENTS
    workgroup
  counts clamped to 2 x 1024               list_apply_batch                       LIST_BAD_COUNTS (refused: tests/test_gpu_switch_points.py)

The walk kernels of wah_aux.hip (checker, index builder, fill merger; the probes are built by tests/_walk.py, proven by
tests/test_walk_reference.py and run by tests/test_gpu_walk_kernels.py):

  4096 words a tile, 256 threads of 16       walk_load_tile, the position sum       WALK_EDGES (word 16 t, 1024 w, 4096 k and a word
    words, 4 waves of 1024 (kScanTileWords,    (wave scan + s_wave_sum + tile_base),   inside a thread) x pair_probes, position_probes,
    kExpandWaves)                              prev from registers / LDS / global      index_probes; END_WORDS (4096 k - 1, 4096 k, + 1)
  the 16-byte test of the tile load          walk_load_tile's `& 15u`               PLACEMENT_BYTES (0, 4, 8, 12 behind a boundary)
  1024 groups a segment                      n_cross, n_unmerged, index_kernel      position_probes (q + count = 1024 and 1025),
                                                                                      pair_probes ("aligned second")
  a thread / wave / tile keeps nothing       the suffix minima of merge_scatter_    RUN_LENGTHS, run_probes
                                               kernel, tile_first
  1024 tiles a round of the merge scan       merge_scan_kernel (s_carry both ways)  SCAN_ROUND_TILE_COUNTS, scan_round_streams
  no run across 2^29 groups                  merge_dropped (kMergeBlockShift)       BLOCK_MULTIPLES, block_probes
  offsets_capacity, out_capacity             index_kernel, merge_scan_kernel        the capacity tests of test_gpu_walk_kernels.py

THRESHOLDS restates the constants; tests/test_switch_reference.py reads them out of the sources and fails when they differ,
naming the probe list that has to move with them.

Found while reading, not reachable: launch_runs_k gives bitop_runs_kernel NO image (lds_words == 0) when an average tile
exceeds WAH_RUNS_LDS_WORDS; launch_bitop_runs picks the tile shape so that an average tile fits with a tenth to spare, and 64
segments of at most 112 words always do, so that branch is never taken.

Of the list kernel, by list_paths(): in list_apply_batch's fast-path test `pos + 128 <= 1024` is never false for a FULL batch
of literals of a valid segment (128 literals are 128 groups of at most 1024), and list_gather's `only >= kFillZero` is never
false for a valid one-word segment (a segment never has exactly one group).  Both are false only for streams that are
refused; tests/test_gpu_switch_points.py holds one refusal for each (a batch of literals behind 897 groups, a lone literal).
Two comparisons of the list kernel can be moved without any change of what it computes, so no probe can sit on them:
list_advance's `128 (b + 1) < cnt` as `<=` gives an operand of 128 b words one more batch, which holds no word (its descriptor
ends in front of it, every lane is outside cnt): the same groups, the same total, the same verdict; and the fast path's
`wi + 128 <= cnt` as `<` sends an operand's last full batch of literals through the general code, which puts the same 128
literals at the same 128 groups (the fast path is that code without the scan).  Libraries built with either change pass
every test of tests/test_gpu_switch_points.py and tests/test_gpu_bitop_list.py; "fill first" segments of 128 b words and the
LIST_SEGMENT_WORDS of 128 b are the inputs on which the two versions run different code.

Of the walk kernels: `have_prev` (validate_kernel, merge_load_tile) can be `true` without any change of what they compute --
walk_load_tile gives the word in front of the stream's first word as 0, a literal, which is no predecessor to merge with; a
library built that way passes every test of tests/test_gpu_walk_kernels.py.  The merger looks at the word IN FRONT of a fill
only: two fills of a kind with an empty fill between them both stay (run_probes' last stream).

Pass 2 had a third variant, kPass2Plain (pair_pass2_0..3.inc), for the pairs between kPairSparseBelow and kPairSwizzleFrom.
Both are 384, no pair reached it, and it is gone: a static_assert in wah_compress_pair.inc and
test_thresholds_are_the_sources_own keep the two thresholds equal.

Which pair slot a probe lands in depends on the SIZE of the bitmap: compress_tile_shape (wah_compress.hip) gives a bitmap of
up to 1400 pairs one pair per wave, up to 3000 two, beyond that three, and from a full round of the chip's workgroup slots
(slots x 8 waves x 3 pairs) on a body of three pairs per wave and a tail of one, two or three.  The no-wait routes always
take two pairs per wave.  tile_shape() / pair_slot() restate the rule, SHAPE_CASES puts the probe pairs behind all-zero
pairs into every size class, shifted so that every probe lands in every slot (tests/test_switch_reference.py shows it).
"""
import numpy as np

M31 = 0x7FFFFFFF
FILL0 = 0x80000000
FILL1 = 0xC0000000
SEG_GROUPS = 1024
SEG_WORDS = 992
PAIR_GROUPS = 2048

# name -> (value, the probe list that has to move when the constant does)
THRESHOLDS = {
    "kScanTileWords": (4096, "WALK_EDGES / END_WORDS / SCAN_ROUND_TILE_COUNTS (tests/_walk.py)"),
    "kExpandWaves": (4, "WALK_EDGES (tests/_walk.py: 64 x this many threads, words per thread and per wave)"),
    "kMergeBlockShift": (29, "BLOCK_MULTIPLES / block_probes (tests/_walk.py)"),
    "merge scan tiles": ((1024, 1024), "SCAN_ROUND_TILE_COUNTS / scan_round_streams (tests/_walk.py)"),
    "walk vector load alignment": (15, "PLACEMENT_BYTES (tests/_walk.py)"),
    "kPairSparseBelow": (384, "PAIR_COUNTS"),
    "WAH_PAIR_SWIZZLE_FROM": (384, "PAIR_COUNTS"),
    "WAH_DT_MAXG": (60, "TILE_TOTALS"),
    "kDtTileWords": (8192, "TILE_PLACES / tile_limit_stream"),
    "kRunsMaxWordsPerSeg": (112, "RUNS_ROUTE_TOTALS"),
    "WAH_RUNS_LDS_WORDS": (10240, "RUNS_SHAPE_TOTALS"),
    "one pass up to": (7, "route_capacities"),
    "one pass above": (40, "route_capacities"),
    "one pair per wave up to": (1400, "SHAPE_CASES / tile_shape"),
    "two pairs per wave up to": (3000, "SHAPE_CASES / tile_shape"),
    "one segment per wave up to": (2400, "SHAPE_CASES (compress_tile_body: wah_bitop_device)"),
    "two segments per wave up to": (6000, "SHAPE_CASES (compress_tile_body: wah_bitop_device)"),
    "WAH_TILE_WAVES": (8, "SHAPE_CASES / tile_shape"),
    "kNoWaitWaveSegs": (4, "NO_WAIT_WAVE_PAIRS / pair_slot"),
    "one-pass batch": (2, "TILE_PLACES / tile_limit_stream (the second tile of a batch)"),
    "runs shape spare": ((9, 10), "runs_fit / RUNS_SHAPE_TOTALS"),
    "runs image": ((3, 2, 1024, 255), "runs_lds_image_words / lds_boundary_tile_words"),
    "runs scan threads": (1024, "SCAN_ROUND_TILES / MANY_TILES_64, MANY_TILES_256"),
    "sums offsets threads": (1024, "SCAN_ROUND_TILES (test_no_wait_decoder_beyond_one_scan_round)"),
    "kListShortFill": (8, "LIST_FILL_GROUPS"),
    "WAH_LIST_DEPTH": (4, "LIST_SCHEDULES"),
    "list batch words": (128, "LIST_SEGMENT_WORDS / LIST_FILL_WORD_INDEX / LIST_SCHEDULES"),
    "list chunk operands": (64, "LIST_OPERAND_COUNTS / LIST_POSITIONS"),
    "WAH_SEG_WAVES": (4, "LIST_SEGMENTS"),
    "list count clamp factor": (2, "LIST_BAD_COUNTS"),
}
PAIR_SWITCH = THRESHOLDS["kPairSparseBelow"][0]
DT_MAX_GROUPS = THRESHOLDS["WAH_DT_MAXG"][0] * 1024
DT_TILE_WORDS = THRESHOLDS["kDtTileWords"][0]
RUNS_MAX_WORDS_PER_SEG = THRESHOLDS["kRunsMaxWordsPerSeg"][0]
RUNS_LDS_WORDS = THRESHOLDS["WAH_RUNS_LDS_WORDS"][0]
TILE_WAVES = THRESHOLDS["WAH_TILE_WAVES"][0]
NO_WAIT_WAVE_PAIRS = THRESHOLDS["kNoWaitWaveSegs"][0] // 2
DT_BATCH = THRESHOLDS["one-pass batch"][0]
MI355X_SLOTS = 2 * 256  # workgroup slots compress_tile_shape counts with: two per compute unit

# ---- the probe lists --------------------------------------------------------------------------------------------------------
PAIR_COUNTS = tuple(sorted({2, 3, 4} | {256 * k + d for k in range(1, 8) for d in (-1, 0, 1)}
                           | {PAIR_SWITCH - 1, PAIR_SWITCH, PAIR_SWITCH + 1} | {2046, 2047, 2048}))
PAIR_SPLITS = ("even", "most first", "most last")
PLACEMENTS = ("front", "behind", "spread")
PAIR_PADDINGS = (0, 1, 2)
FULL_PAIR_FILL_AT = (0, 31, 32, 1023, 1024, 2047, 32 * 17 + 13)  # (the last: in the middle of a lane's 32 groups)
LAST_SEGMENT_WORDS = (1, 30, 31, 32, 991)  # 2, 31, 32, 34, 1023 groups (ragged_end_bitmap)

TILE_TOTALS = (DT_MAX_GROUPS - 1, DT_MAX_GROUPS, DT_MAX_GROUPS + 1)
TILE_WAYS = ("literals + fill", "short fills", "single count")
TILE_PLACES = ("first", "middle", "second of a batch", "last")

RUNS_ROUTE_TOTALS = (RUNS_MAX_WORDS_PER_SEG, )  # x S, and + 1: runs_totals()


# ---- groups <-> bitmap words ------------------------------------------------------------------------------------------------
def pack(groups):
    """31-bit groups -> the bitmap's words: bit j of group g is bit 31 g + j of the bitmap, bit k of the bitmap is bit k % 32
    of word k / 32 (the format of oracle/wah_oracle.c).  The last word is zero padded."""
    g = np.ascontiguousarray(groups, dtype=np.uint32)
    assert not np.any(g >> 31)
    bits = ((g[:, None] >> np.arange(31, dtype=np.uint32)) & 1).astype(np.uint8).reshape(-1)
    pad = (-bits.size) % 32
    if pad:
        bits = np.concatenate([bits, np.zeros(pad, np.uint8)])
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def literals(rng, n):
    """n random groups that are neither all zeros nor all ones."""
    return rng.integers(1, M31, n, dtype=np.uint64).astype(np.uint32)


def segment_groups(words, placement, fill_bit, rng):
    """The 1024 groups of segment(); words == 1024 and placement "literals": no fill at all."""
    assert 1 <= words <= SEG_GROUPS, words
    fill = M31 if fill_bit else 0
    if placement == "literals":
        assert words == SEG_GROUPS
        return literals(rng, SEG_GROUPS)
    n_fill = SEG_GROUPS - (words - 1)  # groups of the one long fill (a lone group when words == 1024)
    if placement == "front":
        return np.concatenate([literals(rng, words - 1), np.full(n_fill, fill, np.uint32)])
    if placement == "behind":
        return np.concatenate([np.full(n_fill, fill, np.uint32), literals(rng, words - 1)])
    assert placement == "spread", placement
    # words - 1 single groups, a literal and a lone fill group in turn, ending in a literal; then the fill of the rest
    head = literals(rng, words - 1)
    lone = np.arange(words - 1) % 2 == (words - 1) % 2  # index words - 2 (the last of the head) is a literal
    head[lone] = fill
    return np.concatenate([head, np.full(n_fill, fill, np.uint32)])


def segment(words, placement, fill_bit, rng):
    """992 bitmap words (1024 groups) that compress to exactly `words` words (1 .. 1024).  Placements: "front" words - 1
    literals in front of one fill, "behind" behind it, "spread" a literal and a lone fill group in turn, then the fill;
    fill_bit: fills of ones or of zeros.  "literals": 1024 literals (words == 1024 only)."""
    return pack(segment_groups(words, placement, fill_bit, rng))


def split_counts(c, split):
    """The words of the two segments of a pair of c words."""
    assert 2 <= c <= PAIR_GROUPS and split in PAIR_SPLITS
    if split == "even":
        a = c // 2
    elif split == "most first":
        a = min(c - 1, SEG_GROUPS)
    else:
        a = max(1, c - SEG_GROUPS)
    return a, c - a


def pair(c, split, placement, fill_bit, rng):
    """Two segments (1984 words) of c words together: split evenly, c - 1 | 1 or 1 | c - 1 (1024 | c - 1024 where a segment
    cannot hold c - 1 words).  A segment of 1024 words is all literals under "front" and "behind" (2048: the incompressible
    pair) and keeps its lone fill groups under "spread" (2048 words that are NOT all literals)."""
    a, b = split_counts(c, split)
    place = [("literals" if w == SEG_GROUPS and placement != "spread" else placement) for w in (a, b)]
    return np.concatenate([segment(a, place[0], fill_bit, rng), segment(b, place[1], 1 - fill_bit if split == "even" else fill_bit, rng)])


def full_pair_with_fill(at, ones, rng):
    """2048 random literals with group `at` all zeros or all ones: 2048 words, not all of them literals."""
    g = literals(rng, PAIR_GROUPS)
    g[at] = M31 if ones else 0
    return pack(g)


def pair_probes(rng, padding=0):
    """[(name, words of the pair, its 1984 bitmap words)]: `padding` incompressible-but-for-a-word pairs, then every count of
    PAIR_COUNTS x PAIR_SPLITS x PLACEMENTS (fills of zeros and of ones in turn), then the full pairs with one fill group."""
    out = [(f"padding {i}", 1000 + i, pair(1000 + i, "even", "front", i & 1, rng)) for i in range(padding)]
    k = 0
    for c in PAIR_COUNTS:
        for split in PAIR_SPLITS:
            for placement in PLACEMENTS:
                out.append((f"{c} {split} {placement}", c, pair(c, split, placement, k & 1, rng)))
                k += 1
    for at in FULL_PAIR_FILL_AT:
        for ones in (0, 1):
            out.append((f"2048 with a fill group at {at} ({'ones' if ones else 'zeros'})", PAIR_GROUPS, full_pair_with_fill(at, ones, rng)))
    return out


def probe_bitmap(rng, padding=0):
    """(bitmap, [words per pair]): the pairs of pair_probes() back to back."""
    probes = pair_probes(rng, padding)
    return np.concatenate([p[2] for p in probes]), [p[1] for p in probes]


# ---- the tile shapes of a compress launch -----------------------------------------------------------------------------------
def tile_shape(n_pairs, slots=MI355X_SLOTS):
    """compress_tile_shape restated: (pairs per wave of the body tiles, of the tail tiles, pairs the body tiles take)."""
    one, two = THRESHOLDS["one pair per wave up to"][0], THRESHOLDS["two pairs per wave up to"][0]
    full = slots * TILE_WAVES * 3  # pairs of a full round of body tiles
    rounds, rest = divmod(n_pairs, full)
    if rounds == 0 or rest == 0:
        p = (1 if n_pairs <= one else 2 if n_pairs <= two else 3) if rounds == 0 else 3
        return p, p, n_pairs
    tail = 1 if rest <= slots * TILE_WAVES else 2 if rest <= slots * TILE_WAVES * 2 else 3
    return 3, tail, rounds * full


def wave_segs(n_segments):
    """compress_wave_segs restated: segments per wave of compress_tile_body (the compress stage of wah_bitop_device)."""
    return 1 if n_segments <= THRESHOLDS["one segment per wave up to"][0] else 2 if n_segments <= THRESHOLDS["two segments per wave up to"][0] else 5


def pair_slot(pair, n_pairs, route, slots=MI355X_SLOTS):
    """(pairs per wave, slot j) in which pair `pair` of a bitmap of n_pairs pairs is compressed: route "no wait" or "one launch"."""
    if route == "no wait":
        return NO_WAIT_WAVE_PAIRS, pair % NO_WAIT_WAVE_PAIRS
    body, tail, body_pairs = tile_shape(n_pairs, slots)
    return (body, pair % body) if pair < body_pairs else (tail, (pair - body_pairs) % tail)


_ROUND = MI355X_SLOTS * THRESHOLDS["WAH_TILE_WAVES"][0] * 3
# name -> (all-zero pairs in front of the probe pairs, the kernel instance <body, tail> of the one-launch routes)
SHAPE_CASES = {}
for _shift in range(2):
    SHAPE_CASES[f"two pairs per wave, shift {_shift}"] = (THRESHOLDS["one pair per wave up to"][0] + 2 + _shift, (2, 2))
for _shift in range(3):
    SHAPE_CASES[f"three pairs per wave, shift {_shift}"] = (THRESHOLDS["two pairs per wave up to"][0] + 3 + _shift, (3, 3))
SHAPE_CASES["a round of three, tail of one"] = (_ROUND, (3, 1))
for _shift in range(2):
    SHAPE_CASES[f"a round of three, tail of two, shift {_shift}"] = (_ROUND + MI355X_SLOTS * THRESHOLDS["WAH_TILE_WAVES"][0] + 2 + _shift, (3, 2))


def shaped_probe_bitmap(rng, front_pairs):
    """(bitmap, pairs): front_pairs all-zero pairs, then the probe pairs of pair_probes()."""
    probes, _ = probe_bitmap(rng)
    return np.concatenate([np.zeros(front_pairs * 2 * SEG_WORDS, np.uint32), probes]), front_pairs + probes.size // (2 * SEG_WORDS)


def ragged_end_bitmap(rng, tail_words, lone_segment=False):
    """A few probe pairs, then a pair whose last segment is cut short: the bitmap ends `tail_words` words into it.  A bitmap
    is whole words behind whole segments of 992 words, so its last segment has ceil(32 w / 31) groups: never 1 or 33; the
    LAST_SEGMENT_WORDS 1, 30, 31, 32, 991 give 2, 31, 32, 34, 1023 groups.  lone_segment: the bitmap ends with the FIRST
    segment of a pair instead (an odd number of segments)."""
    head = np.concatenate([pair(PAIR_SWITCH, "even", "spread", 0, rng), pair(PAIR_GROUPS, "even", "front", 0, rng),
                           pair(PAIR_SWITCH - 1, "most first", "behind", 1, rng)])
    if lone_segment:
        return np.concatenate([head, segment(PAIR_SWITCH, "spread", 1, rng)])
    first = segment(PAIR_SWITCH - 1 - min(tail_words, 300), "spread", 0, rng)
    tail = rng.integers(0, 2**32, tail_words, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([head, first, tail])


# ---- one-pass decoder tiles -------------------------------------------------------------------------------------------------
def _tile_words(total, way, n_words, rng):
    """n_words stream words that expand to `total` groups ("single count": one fill of `total` groups among literals)."""
    if way == "literals + fill":
        st = literals(rng, n_words)
        st[int(rng.integers(0, n_words))] = FILL0 | (total - (n_words - 1))
        return st
    if way == "short fills":
        base, extra = divmod(total, n_words)
        assert base >= 1
        counts = np.full(n_words, base, np.uint32)
        counts[rng.permutation(n_words)[:extra]] += 1
        kinds = np.where(np.arange(n_words) % 2 == 0, FILL0, FILL1).astype(np.uint32)
        return kinds | counts
    assert way == "single count", way
    st = literals(rng, n_words)
    st[int(rng.integers(0, n_words))] = FILL1 | total
    return st


def tile_limit_stream(total, way, place, rng, n_tiles=6, batch=DT_BATCH):
    """(stream, tile, groups of that tile): a foreign stream of n_tiles one-pass tiles (8192 words) of plain literals, in which
    tile `place` -- first / middle / the second tile of a workgroup's batch / the last, partial one -- expands to exactly `total`
    groups: 8191 literals and one fill; 8192 short fills; or ("single count") ONE word whose count alone is `total` -- the only
    word of the last tile, among 8191 literals elsewhere (that tile's groups are then total + 8191: what is probed is the
    clamp of a single count)."""
    t = {"first": 0, "middle": n_tiles // 2 - (n_tiles // 2) % batch, "second of a batch": n_tiles // 2 - (n_tiles // 2) % batch + 1,
         "last": n_tiles}[place]
    tiles = [literals(rng, DT_TILE_WORDS) for _ in range(n_tiles)]
    if place == "last":
        n_words = 1 if way == "single count" else 1000 if way == "literals + fill" else 4097
        probe = _tile_words(total, way, n_words, rng)
        tiles.append(probe)
    else:
        probe = _tile_words(total, way, DT_TILE_WORDS, rng)
        tiles[t] = probe
    groups = int(np.where(probe & FILL0, probe & 0x3FFFFFFF, 1).astype(np.uint64).sum())
    return np.concatenate(tiles), t, groups


def tile_with_empty_fill(rng, n_tiles=4):
    """Plain literal tiles; tile 1 is far under the limit but holds one empty fill (it is deferred for that reason)."""
    st = literals(rng, n_tiles * DT_TILE_WORDS + 77)
    st[DT_TILE_WORDS + 4000] = FILL0
    st[DT_TILE_WORDS + 100] = FILL1 | 500
    return st


def alternating_tile_stream(rng, n_tiles=9):
    """Tiles of exactly 61440 and 61441 groups in turn (by short fills and by literals + fill in turn), a partial tile last."""
    tiles = []
    for t in range(n_tiles):
        tiles.append(_tile_words(DT_MAX_GROUPS + t % 2, TILE_WAYS[(t // 2) % 2], DT_TILE_WORDS, rng))
    tiles.append(literals(rng, 333))
    return np.concatenate(tiles)


def tile_groups(stream, tile):
    """Groups the stream's one-pass tile `tile` expands to."""
    w = stream[tile * DT_TILE_WORDS: (tile + 1) * DT_TILE_WORDS]
    return int(np.where(w & FILL0, w & 0x3FFFFFFF, 1).astype(np.uint64).sum())


def default_route(c, capacity):
    """The decoder wah_decompress_device takes for a 16-byte aligned stream of c words (1 one pass, 2 two launches)."""
    lo, hi = THRESHOLDS["one pass up to"][0], THRESHOLDS["one pass above"][0]
    return 1 if capacity <= lo * c or capacity > hi * c else 2


def route_capacities(c):
    """out_capacity -> the default decoder of wah_decompress_device for a stream of c words (1 one pass, 2 two launches)."""
    lo, hi = THRESHOLDS["one pass up to"][0], THRESHOLDS["one pass above"][0]
    return {lo * c: 1, lo * c + 1: 2, hi * c: 2, hi * c + 1: 1}


# ---- operands of the run-merge bit operations -------------------------------------------------------------------------------
def operands_with_total(k, n_segments, total, rng, block=64):
    """k bitmaps of n_segments whole segments whose compressed streams hold exactly `total` words together: every segment of
    every operand gets total / (k n_segments) words, the first few one more.  Segments are built `block` at a time and
    repeated beyond that (a bitmap of many segments is then cheap)."""
    cells = k * n_segments
    q, r = divmod(total, cells)
    assert 1 <= q and q + (1 if r else 0) <= SEG_GROUPS, (total, cells)
    n_block = min(block, n_segments)
    # the r cells of one more word: the first r in operand-major order over the first rows -- taken inside the first block only
    # where they fit, otherwise spread by whole operands
    maps = []
    left = r
    for j in range(k):
        more = min(left, n_segments)  # this operand's first `more` segments hold q + 1 words
        left -= more
        rows = []
        proto = {w: [segment(w, PLACEMENTS[(i + j) % 3], (i + j) & 1, rng) for i in range(n_block)] for w in ({q} | ({q + 1} if more else set()))}
        for s in range(n_segments):
            rows.append(proto[q + 1 if s < more else q][s % n_block])
        maps.append(np.concatenate(rows))
    assert left == 0
    return maps


def runs_totals(n_segments):
    """Totals of all operands' words on both sides of the run-merge route's limit: {total: route}."""
    t = RUNS_MAX_WORDS_PER_SEG * n_segments
    return {t - 1: 1, t: 1, t + 1: 2}


def runs_fit(n_segments):
    num, den = THRESHOLDS["runs shape spare"][0]
    return RUNS_LDS_WORDS * n_segments * num // den


def runs_shape(total, n_segments):
    """Segments per workgroup launch_bitop_runs chooses."""
    fit = runs_fit(n_segments)
    return 256 if total * 256 <= fit else 128 if total * 128 <= fit else 64


def runs_shape_totals(n_segments):
    """Totals just below, at and above the 256 / 128 and the 128 / 64 choice: {total: segments per workgroup}."""
    fit = runs_fit(n_segments)
    out = {}
    for shape in (256, 128):
        at = fit // shape
        for t in (at - 1, at, at + 1):
            out[t] = runs_shape(t, n_segments)
    return out


def runs_lds_image_words(total, n_segments, shape):
    """Words of the LDS image launch_runs_k gives bitop_runs_kernel (0: none); a tile of more words is read from global memory."""
    if total * shape > RUNS_LDS_WORDS * n_segments:
        return 0
    num, den, more, mask = THRESHOLDS["runs image"][0]
    return min((total * shape * num // den // n_segments + more) & ~mask, RUNS_LDS_WORDS)


def operands_with_dense_tile(k, n_segments, tile, rng, shape=256):
    """k sparse operands (two words per segment) of which the first has eight incompressible segments inside tile `tile`."""
    maps = operands_with_total(k, n_segments, 2 * k * n_segments, rng)
    at = shape * tile + 100
    maps[0][SEG_WORDS * at: SEG_WORDS * (at + 8)] = np.concatenate([segment(SEG_GROUPS, "literals", 0, rng) for _ in range(8)])
    return maps


def lds_boundary_tile_words(k, n_segments, shape=256):
    """W such that, in k operands of two words per segment except for one tile of W words, the LDS image is exactly W words
    -- and stays W when the tile holds one word more (that tile is then the first that is NOT staged)."""
    rest = 2 * k * (n_segments - shape)
    for w in range(2 * k * shape, RUNS_LDS_WORDS + 1):
        if runs_lds_image_words(rest + w, n_segments, shape) == w == runs_lds_image_words(rest + w + 1, n_segments, shape):
            return w
    raise AssertionError("no tile size equals its own LDS image")


def operands_with_tile_words(k, n_segments, tile, tile_words, rng, shape=256):
    """k operands of two words per segment, except that the segments of tile `tile` hold tile_words words together."""
    counts = np.full((k, n_segments), 2)
    q, r = divmod(tile_words, k * shape)
    cells = np.full(k * shape, q)
    cells[:r] += 1
    counts[:, shape * tile: shape * (tile + 1)] = cells.reshape(shape, k).T
    assert counts.max() <= SEG_GROUPS and counts.min() >= 1
    proto = {}
    maps = []
    for j in range(k):
        rows = []
        for i, w in enumerate(counts[j]):
            key = (int(w), (i + j) % 6)
            if key not in proto:
                proto[key] = segment(int(w), PLACEMENTS[key[1] % 3], key[1] // 3, rng)
            rows.append(proto[key])
        maps.append(np.concatenate(rows))
    return maps


RUNS_SHAPE_SEGMENTS = (256 * 2, 256 * 2 + 1, 256 * 2 + 63, 256 * 2 + 64, 256 * 2 + 255, 256 * 3, 256 * 3 + 1)  # S mod 256 (and 64, 128)
MANY_TILES_64 = 64 * 1024 + 1     # segments: 1025 tiles of 64
MANY_TILES_256 = 256 * 1024 + 1   # segments: 1025 tiles of 256
SCAN_ROUND_TILES = THRESHOLDS["runs scan threads"][0]           # tiles one round of the scans takes (4096-word tiles in the decoder)


# ---- the operand-list bit operation (wah_bitop_list.hip) --------------------------------------------------------------------
LIST_OPS = ("and", "or", "xor", "andnot")
LIST_SHORT_FILL = THRESHOLDS["kListShortFill"][0]
LIST_DEPTH = THRESHOLDS["WAH_LIST_DEPTH"][0]
LIST_BATCH = THRESHOLDS["list batch words"][0]
LIST_CHUNK = THRESHOLDS["list chunk operands"][0]
SEG_WAVES = THRESHOLDS["WAH_SEG_WAVES"][0]
LIST_CLAMP = THRESHOLDS["list count clamp factor"][0] * SEG_GROUPS
COUNT_MASK = 0x3FFFFFFF

# groups of a fill: by its own lane up to 8 (1 group: the first store only), by the whole wave 64 a step beyond
LIST_FILL_GROUPS = (1, 2, 3, LIST_SHORT_FILL - 1, LIST_SHORT_FILL, LIST_SHORT_FILL + 1, 63, 64, 65, 127, 128, 129, 700)
# the word that holds it: lane 0's first, its second, lane 63's first and second, the same of the second batch, the third's first
LIST_FILL_WORD_INDEX = (0, 1, LIST_BATCH - 2, LIST_BATCH - 1, LIST_BATCH, LIST_BATCH + 1, 2 * LIST_BATCH - 1, 2 * LIST_BATCH)
LIST_SEGMENT_WORDS = tuple(sorted({1, 2, SEG_GROUPS - 1, SEG_GROUPS} | {LIST_BATCH * b + d for b in range(1, 8) for d in (-1, 0, 1)}))
LIST_WAYS = ("literals + fill", "fill ends a batch", "fill starts the next batch", "fill first")
LIST_OPERAND_COUNTS = (1, 2, LIST_CHUNK - 1, LIST_CHUNK, LIST_CHUNK + 1, 2 * LIST_CHUNK - 1, 2 * LIST_CHUNK, 2 * LIST_CHUNK + 1, 4097)
LIST_POSITIONS = (0, 1, LIST_CHUNK - 2, LIST_CHUNK - 1, LIST_CHUNK, LIST_CHUNK + 1, 2 * LIST_CHUNK)  # table rows of a non-trivial operand
LIST_SEGMENTS = (1, SEG_WAVES - 1, SEG_WAVES, SEG_WAVES + 1)
LIST_BAD_COUNTS = (LIST_CLAMP - 1, LIST_CLAMP, LIST_CLAMP + 1, COUNT_MASK)
# words per segment of the operands of ONE chunk (1: a single fill word, settled where it is the operation's identity)
LIST_SCHEDULES = ((5,), (257,), (1024,), (128, 128, 128, 128), (128, 128, 128, 128, 1), (128, 128, 128, 128, 2), (129, 1, 257, 128, 1024),
                  (300, 1, 1, 129, 1, 513, 1, 1, 1, 2), (1,) * 64, (1,) * 64 + (129, 1, 640), (1024, 1024, 1024))


def list_groups(layout, rng):
    """The groups of a segment from runs (kind, n): "lit" n random literals, "ones" / "zeros" n groups of a fill."""
    parts = []
    for kind, n in layout:
        assert n >= 1 and kind in ("lit", "ones", "zeros"), (kind, n)
        parts.append(literals(rng, n) if kind == "lit" else np.full(n, M31 if kind == "ones" else 0, np.uint32))
    return np.concatenate(parts)


def list_layout_words(layout):
    """What the layout compresses to: 0 per literal, the fill word per maximal run of one kind of fill."""
    out = []
    last = None
    for kind, n in layout:
        if kind == "lit":
            out.extend([0] * n)
        elif kind == last:
            out[-1] += n
        else:
            out.append((FILL1 if kind == "ones" else FILL0) | n)
        last = kind
    return np.array(out, np.uint32)


def list_segment(layout, rng, tail_words=None):
    """The bitmap words of one segment: 992 words from a layout of 1024 groups; or, for the bitmap's last segment, tail_words
    words from a layout of ceil(32 tail_words / 31) groups -- the last group then holds only the bits the bitmap has (a literal
    keeps its lowest bit set; a fill of ones cannot end there unless the group is whole: tail_words a multiple of 31)."""
    g = list_groups(layout, rng)
    if tail_words is None:
        assert g.size == SEG_GROUPS, g.size
        return pack(g)
    assert g.size == (32 * tail_words + 30) // 31, (g.size, tail_words)
    bits = 32 * tail_words - 31 * (g.size - 1)  # of the last group
    if bits < 31:
        assert layout[-1][0] != "ones"
        g[-1] &= (1 << bits) - 1
        if layout[-1][0] == "lit":
            g[-1] |= 1
    words = pack(g)
    assert not words[tail_words:].any()
    return words[:tail_words]


def list_fill_layout(word_index, fill_bit, n_groups, total_words):
    """The layout of list_fill_at: word_index literals, the fill, literals, and one trailing fill of the other kind."""
    fill, other = ("ones", "zeros") if fill_bit else ("zeros", "ones")
    if total_words == word_index + 1:  # the fill is the segment's last word
        assert n_groups == SEG_GROUPS - word_index
        return ([("lit", word_index)] if word_index else []) + [(fill, n_groups)]
    lits = total_words - word_index - 2
    rest = SEG_GROUPS - word_index - n_groups - lits
    assert lits >= 0 and rest >= 1, (word_index, n_groups, total_words)
    return ([("lit", word_index)] if word_index else []) + [(fill, n_groups)] + ([("lit", lits)] if lits else []) + [(other, rest)]


def list_fill_at(word_index, fill_bit, n_groups, total_words, rng):
    """A segment of exactly total_words words whose word word_index is a fill of fill_bit of n_groups groups (it starts at
    group word_index: only literals lie in front of it); the rest is literals, padded by a trailing fill of the other kind."""
    return list_segment(list_fill_layout(word_index, fill_bit, n_groups, total_words), rng)


def list_fill_probes():
    """[(word index, fill bit, groups, words of the segment)]: LIST_FILL_WORD_INDEX x LIST_FILL_GROUPS x both kinds, with 0 to
    139 literals behind the fill; and the one-word segments."""
    out = []
    for wi in LIST_FILL_WORD_INDEX:
        for n in LIST_FILL_GROUPS:
            lits = min((7 * wi + n) % 140, SEG_GROUPS - wi - n - 1)
            out.extend((wi, bit, n, wi + 2 + lits) for bit in (0, 1))
    return out + [(0, 0, SEG_GROUPS, 1), (0, 1, SEG_GROUPS, 1)]


def list_many_fills_layouts():
    """Segments whose batches hold MANY fills with an effect: 56 fills of 9 groups of either kind side by side (a lane's first
    word and its second, both orders: list_put_long's mask has 56 bits), short fills in every lane (list_put_rest in all of
    them), fills of 64 groups back to back, and long and short ones mixed in one batch."""
    out = []
    for a, b in (("ones", "zeros"), ("zeros", "ones")):
        out.append([(a, LIST_SHORT_FILL + 1), (b, LIST_SHORT_FILL + 1)] * 56 + [("lit", 16)])
        out.append([(a, 2), ("lit", 1), (b, 3), ("lit", 2)] * 128)  # (five words: either kind in first and in second words)
        out.append([(a, 64), (b, 64)] * 8)
        out.append([("lit", 1), (a, 17), (b, LIST_SHORT_FILL), ("lit", 2), (b, 1), (a, LIST_SHORT_FILL)] * 27 + [(b, 25)])
    assert all(sum(n for _, n in layout) == SEG_GROUPS for layout in out)
    return out


def list_words_layout(words, way, fill_bit):
    """A layout of exactly `words` words (None: this way cannot give that count)."""
    fill, other = ("ones", "zeros") if fill_bit else ("zeros", "ones")
    lit = lambda n: [("lit", n)] if n else []  # noqa: E731
    if way == "literals + fill":  # literals only where 1024
        return lit(SEG_GROUPS) if words == SEG_GROUPS else lit(words - 1) + [(fill, SEG_GROUPS - words + 1)]
    if way == "fill ends a batch":  # a fill as the very last word of the last FULL batch, 127 literals in front: not the fast path
        if words < LIST_BATCH:
            return None
        at = LIST_BATCH * (words // LIST_BATCH) - 1
        after = words - at - 1  # words behind the fill: literals and one fill of the other kind
        if after == 0:
            return lit(at) + [(fill, SEG_GROUPS - at)]
        room = SEG_GROUPS - words + 2  # groups of the two fills together
        mine = min(3, room - 1)
        return lit(at) + [(fill, mine)] + lit(after - 1) + [(other, room - mine)]
    if way == "fill starts the next batch":  # full batches of literals (the fast path), then a batch whose FIRST word is a fill
        full = LIST_BATCH * ((words - 1) // LIST_BATCH)
        if full == 0:
            return None
        return lit(full) + [(fill, SEG_GROUPS - words + 1)] + lit(words - full - 1)
    assert way == "fill first", way  # where words is a multiple of 128 the last batch is full, literals, and ENDS at group 1024
    return [(fill, SEG_GROUPS - words + 1)] + lit(words - 1) if words > 1 else None


def list_words_probes():
    """[(words, way, fill bit, layout)]: every LIST_SEGMENT_WORDS by every way that can give it, the fill kinds in turn."""
    out = []
    for words in LIST_SEGMENT_WORDS:
        for way in LIST_WAYS:
            bit = len(out) & 1
            layout = list_words_layout(words, way, bit)
            if layout is not None:
                out.append((words, way, bit, layout))
    return out


def list_probe_bitmap(layouts, rng, tail=None):
    """The segments of the layouts back to back; tail: (layout, tail_words) of a last, short segment."""
    segs = [list_segment(layout, rng) for layout in layouts]
    if tail is not None:
        segs.append(list_segment(tail[0], rng, tail[1]))
    return np.concatenate(segs)


def list_schedule_layout(words, one_word_bit, j=0):
    """A layout of `words` words for a schedule's operand: literals around one fill (1: the fill alone, of one_word_bit)."""
    if words == 1:
        return [("ones" if one_word_bit else "zeros", SEG_GROUPS)]
    return list_words_layout(words, LIST_WAYS[j % 2 * 3], j // 2 % 2)


def list_schedule_operands(schedule, one_word_bit, n_segments, rng):
    """len(schedule) bitmaps of n_segments segments: operand j holds schedule[(j + s) % k] words in segment s when k <= 64 (every
    segment sees the schedule rotated), schedule[j] in every segment beyond (the chunks stay what the schedule says)."""
    k = len(schedule)
    maps = []
    for j in range(k):
        counts = [schedule[(j + s) % k if k <= LIST_CHUNK else j] for s in range(n_segments)]
        maps.append(list_probe_bitmap([list_schedule_layout(c, one_word_bit, j + s) for s, c in enumerate(counts)], rng))
    return maps


def list_schedule_counts(schedule, n_segments):
    """[segment][operand] -> the words list_schedule_operands gives it."""
    k = len(schedule)
    return [[schedule[(j + s) % k if k <= LIST_CHUNK else j] for j in range(k)] for s in range(n_segments)]


def list_ragged_layouts(tail_words):
    """The last segment of tail_words words, three ways: one fill of zeros (the identity except under AND), the nearest to one
    fill of ones (the identity under AND alone: one word only where the last group is whole), literals up to the last group."""
    g = (32 * tail_words + 30) // 31
    whole = (32 * tail_words) % 31 == 0
    return {"zeros": [("zeros", g)], "ones": [("ones", g)] if whole else [("ones", g - 1), ("lit", 1)], "literals": [("lit", g)]}


def list_paths(words, nvalid, op, first=False):
    """bitop_list_segments_kernel restated for ONE operand's words of one segment of nvalid groups under operation op (first:
    the operand is row 0 of the table): which way every batch and every word goes.  Returns a dict:
      settled   list_gather settles it (one identity fill of exactly nvalid groups): no batch at all
      batches   [{fast, last, pos (groups covered before it), rest (list_put_rest runs), words: [(way, groups, first group)]}]
                way: "literal" / "identity" / "own first" (an effect fill of 1 group) / "own rest" (2 .. 8) / "wave" (9 and more)
                / "outside" (it would end behind group 1024: nothing is put) / "empty"; a fast batch lists 128 x "fast"
      ok        the verdict: no empty word and exactly nvalid groups at the last batch"""
    words = np.asarray(words, np.uint32)
    cnt = int(words.size)
    assert op in LIST_OPS and 1 <= cnt <= nvalid <= SEG_GROUPS  # (list_gather refuses any other range)
    rest_effect = FILL0 if op == "and" else FILL1               # m_rest.fill: what the settled test looks at
    only = int(words[0])
    if cnt == 1 and only >= FILL0 and (only & COUNT_MASK) == nvalid and (only & FILL1) != rest_effect:
        return {"settled": True, "batches": [], "ok": True}
    applied = "or" if first and op == "andnot" else op          # m_first
    effect = FILL0 if applied == "and" else FILL1
    pos, empty, batches = 0, False, []
    for wi in range(0, cnt, LIST_BATCH):
        batch = [int(w) for w in words[wi: wi + LIST_BATCH]]
        full = wi + LIST_BATCH <= cnt
        info = {"last": wi + LIST_BATCH >= cnt, "pos": pos, "full": full, "rest": False}
        if full and pos + LIST_BATCH <= SEG_GROUPS and not any(w & FILL0 for w in batch):
            info.update(fast=True, words=[("fast", 1, pos + i) for i in range(LIST_BATCH)])
            pos += LIST_BATCH
        else:
            ways = []
            for w in batch:
                n = min(w & COUNT_MASK, LIST_CLAMP) if w & FILL0 else 1
                empty |= n == 0
                if n == 0:
                    way = "empty"
                elif pos + n > SEG_GROUPS:
                    way = "outside"
                elif not w & FILL0:
                    way = "literal"
                elif (w & FILL1) != effect:
                    way = "identity"
                else:
                    way = "own first" if n == 1 else "own rest" if n <= LIST_SHORT_FILL else "wave"
                ways.append((way, n, pos))
                pos += n
            info.update(fast=False, words=ways, rest=any(way == "own rest" for way, _, _ in ways))
        batches.append(info)
    return {"settled": False, "batches": batches, "ok": not empty and pos == nvalid}


def list_chunk_rotation(counts, depth=None):
    """The producer / consumer rotation over ONE chunk's live operands (counts: their words, settled ones left out): for every
    batch the consumer applies, how many operand boundaries lie between it and the producer's cursor (64: the producer is done)."""
    depth = LIST_DEPTH if depth is None else depth
    seq = [(j, b) for j, c in enumerate(counts) for b in range((c + LIST_BATCH - 1) // LIST_BATCH)]
    return [(seq[i + depth][0] - seq[i][0]) if i + depth < len(seq) else LIST_CHUNK for i in range(len(seq))]


def list_table_rows(n_rows, pool_size, placed=None):
    """Row -> pool entry of a table of n_rows rows: the pool's entries 1 .. in turn (0: the trivial operand, used by `placed`
    tables only); placed {row: entry}: every other row is entry 0."""
    if placed is None:
        return [1 + r % (pool_size - 1) for r in range(n_rows)]
    assert all(0 <= r < n_rows for r in placed)
    return [placed.get(r, 0) for r in range(n_rows)]


def list_fold(op, pool, rows):
    """The bitmap a table of rows (indices into pool) combines to, without stacking 4097 bitmaps: AND / OR over the distinct rows,
    XOR over those that occur an odd number of times, ANDNOT the first row and not the OR of the others."""
    pool = [np.asarray(p, np.uint32) for p in pool]
    if op == "and":
        return np.bitwise_and.reduce([pool[i] for i in sorted(set(rows))])
    if op == "or":
        return np.bitwise_or.reduce([pool[i] for i in sorted(set(rows))])
    if op == "xor":
        odd = [i for i in sorted(set(rows)) if rows.count(i) % 2]
        return np.bitwise_xor.reduce([pool[i] for i in odd]) if odd else np.zeros_like(pool[0])
    assert op == "andnot", op
    rest = sorted(set(rows[1:]))
    return pool[rows[0]] & ~np.bitwise_or.reduce([pool[i] for i in rest]) if rest else pool[rows[0]].copy()


def list_pool(rng, n_segments=3, size=5):
    """A small pool of bitmaps of n_segments segments for the tables of LIST_OPERAND_COUNTS / LIST_POSITIONS: entries 1 .. are
    literals around fills of both kinds (2 to 1024 words a segment); entry 0 is left to the caller (the operation's trivial
    operand: all zeros, or all ones under AND -- one identity fill per segment, settled)."""
    counts = (2, LIST_BATCH + 2, SEG_GROUPS, 40, 2 * LIST_BATCH)
    pool = [None]
    for j in range(1, size):
        pool.append(list_probe_bitmap([list_words_layout(counts[(j + s) % len(counts)], LIST_WAYS[(j + s) % 2 * 3], (j + s) // 2 % 2)
                                       for s in range(n_segments)], rng))
    return pool


def list_trivial(op, n_words):
    """The operand that changes nothing (and, as row 0 of ANDNOT, leaves nothing): one identity fill per whole segment."""
    return np.full(n_words, 0xFFFFFFFF if op == "and" else 0, np.uint32)


# tables in which only the `placed` rows are not the trivial operand: {name: (rows of the table, {row: pool entry})}
LIST_PLACED = {f"alone in row {r}": (max(r + 1, LIST_CHUNK + 1), {r: 1}) for r in LIST_POSITIONS}
LIST_PLACED["rows 0, 1, 63, 64 and 128"] = (2 * LIST_CHUNK + 1, {0: 1, 1: 2, LIST_CHUNK - 1: 3, LIST_CHUNK: 4, 2 * LIST_CHUNK: 2})
LIST_PLACED["row 0 again in rows 64 and 128"] = (2 * LIST_CHUNK + 1, {0: 1, LIST_CHUNK: 1, 2 * LIST_CHUNK: 1})
LIST_PLACED["rows 62 and 63"] = (LIST_CHUNK, {0: 3, LIST_CHUNK - 2: 1, LIST_CHUNK - 1: 2})


def list_refusals(rng):
    """[(name, the words of one segment of 1024 groups)]: hand-built words that must be refused.  Every one is a range of 1 to
    1024 words (list_gather accepts it), so it is refused by what the words say -- and list_paths() says the same."""
    def lits_with(cnt, at, word):
        w = literals(rng, cnt)
        w[at] = word
        return w

    out = []
    for k, (cnt, at) in enumerate(((50, 10), (200, 150), (1000, 900))):  # the fill in batch 1, 2 and 8
        for d in (-1, 1):
            out.append((f"{SEG_GROUPS + d} groups, the fill in batch {at // LIST_BATCH + 1}",
                        lits_with(cnt, at, (FILL1 if (k + d) & 2 else FILL0) | (SEG_GROUPS - (cnt - 1) + d))))
    for k, n in enumerate(LIST_BAD_COUNTS):
        out.append((f"one count of {n}", lits_with(40, 7, (FILL1 if k & 1 else FILL0) | n)))
    out.append((f"{LIST_BATCH} counts of {COUNT_MASK}", np.full(LIST_BATCH, FILL1 | COUNT_MASK, np.uint32)))
    out.append((f"a second batch of {LIST_BATCH} counts of {COUNT_MASK}",
                np.concatenate([literals(rng, LIST_BATCH), np.full(LIST_BATCH, FILL0 | COUNT_MASK, np.uint32)])))
    for cnt, at, kind in ((200, LIST_BATCH - 1, FILL0), (400, 300, FILL1)):  # the groups ARE 1024: only the empty word is wrong
        w = lits_with(cnt, at, kind)
        w[-1] = (FILL0 if kind == FILL1 else FILL1) | (SEG_GROUPS - (cnt - 2))
        out.append((f"an empty fill in word {at}", w))
    out.append(("a full batch of literals behind 897 groups", np.concatenate([[FILL0 | 770], literals(rng, 2 * LIST_BATCH - 1)]).astype(np.uint32)))
    out.append(("a lone literal", literals(rng, 1)))
    return out


def list_refused_stream(bitmap_streams, segment, words):
    """(stream, index) of an operand whose segments are bitmap_streams (the oracle's, one array per segment) except that
    `segment` holds `words`: the index is the stream's own, every range inside it."""
    segs = [np.asarray(words if s == segment else w, np.uint32) for s, w in enumerate(bitmap_streams)]
    return np.concatenate(segs), np.concatenate([[0], np.cumsum([w.size for w in segs])]).astype(np.int64)
