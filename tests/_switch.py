"""Inputs that sit exactly ON the integer thresholds at which the kernels change code, and the table of those thresholds.

TEST INFRASTRUCTURE (tests/test_switch_reference.py proves every constructor with the oracle on the CPU,
tests/test_gpu_switch_points.py runs the inputs through the kernels).

The switches (gpu-wah_amd/csrc) and the probes that sit on them:

  switch                                   where                                  probes
  ---------------------------------------  -------------------------------------  ------------------------------------------
  words of a segment pair < / >= 384       wah_compress_pair.inc (pass 2 variant  PAIR_COUNTS (383, 384, 385)
    (kPairSparseBelow, kPairSwizzleFrom)   and park_pair's lane), the same line
                                           in wah_compress_unseg_pair.inc
  pair of 2048 words, all literals or not  wah_compress_pair.inc                  PAIR_COUNTS (2046 .. 2048), FULL_PAIR_FILL_AT
    (store_literals / swizzled pass 2)       (pair_all_literals)
  256 t < count, t = 0 .. 7                emit_pair                              PAIR_COUNTS (256 k - 1, 256 k, 256 k + 1)
  1st / 2nd / 3rd pair of a wave, the      compress_pair_body, compress_tile_     SHAPE_CASES (the probes in every size class of
    kernel instances <1,1> <2,2> <3,3>       shape, launch_pairs / launch_unseg     compress_tile_shape, shifted by 0, 1, 2 pairs),
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

THRESHOLDS restates the constants; tests/test_switch_reference.py reads them out of the sources and fails when they differ,
naming the probe list that has to move with them.

Found while reading, not reachable: launch_runs_k gives bitop_runs_kernel NO image (lds_words == 0) when an average tile
exceeds WAH_RUNS_LDS_WORDS; launch_bitop_runs picks the tile shape so that an average tile fits with a tenth to spare, and 64
segments of at most 112 words always do, so that branch is never taken.

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
