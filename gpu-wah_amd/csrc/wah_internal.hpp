// wah_internal.hpp -- declarations shared by the kernel TU and the C-ABI TU.
//
// gfx950 / CDNA4 only: 64-lane wavefronts, 8 XCDs with private L2s.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>

namespace wah {

// The one experiment switch, WAH_BITOP_ROUTE (forces the route of the indexed bit operations: "runs" / "groups", for
// tools/bitop_density_time.py, which compares the two), is read from the environment only by builds made with
// -DWAH_EXPERIMENTS (`make -C gpu-wah_amd exp` -> libwah_hip_exp.so, used through WAH_LIB_PATH); the shipped library
// does not read it.  (What it does read is documented in include/wah.h: WAH_HOST_CACHE, WAH_FORCE_FALLBACK,
// WAH_FAULT_INJECT.)
inline const char *experiment_env(const char *name) {
#ifdef WAH_EXPERIMENTS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// ---- wire format (reference const.h:3-16) ---------------------------------
constexpr uint32_t kOnes31 = 0x7FFFFFFFu;    // ONES31
constexpr uint32_t kFillZero = 0x80000000u;  // BIT31
constexpr uint32_t kFillOne = 0xC0000000u;   // BIT3130
constexpr uint32_t kCountMask = 0x3FFFFFFFu; // BIT30 - 1 (kernels.cu:300)

// ---- segment geometry (kernels.cu:68: one CUDA block = 1024 groups) ------
constexpr uint32_t kSegWords = 992;
constexpr uint32_t kSegGroups = 1024;
constexpr uint32_t kSteps = 16; // 64 groups (one wavefront) per step

// ---- inter-workgroup control block (uint32 words)
// decode / aux kernels: zeroed before each launch.  compress: zeroed ONCE (wah_workspace_init_device), then kept up by
// the kernel itself (launch epochs, see compress_tile_body).
constexpr uint32_t kCtlStart = 0;        // arrival ticket: order in which workgroups start running (alone on its 128-byte line:
                                         // every workgroup of a launch adds to it)
constexpr uint32_t kCtlEpoch = 64;       // tile kernels: epoch of the NEXT launch (0 = fresh workspace); read-mostly line
constexpr uint32_t kCtlMagic = 65;       // tile kernels: kWorkspaceMagic once a launch has completed (0 = fresh workspace)
constexpr uint32_t kCtlWraps = 66;       // tile kernels: how often the epoch space has been used up
constexpr uint32_t kCtlClearDone = 96;   // tile kernels: == kCtlWraps + 1 once tile 0 of a wrapping launch has cleared the scan area
constexpr uint32_t kCtlError = 160;      // sticky error bits
constexpr uint32_t kCtlResult = 162;     // host-pointer entry points: two 64-bit results of the launch live here, beside the
                                         // error word, so that ONE 32-byte copy brings status and sizes to the host
constexpr uint32_t kCtlDefer = 192;      // the decoders' list of tiles that are decoded by workgroups of their own: two 64-bit counter pairs
                                         // {entries:32, sum of their parts:32} at words [0..1] and [2..3], used in turn, and at word
                                         // [kDeferSeq] the number of launches that could append so far (launch s counts in pair s & 1; its
                                         // last tile zeroes the other pair -- nobody reads it any more -- and stores s + 1: whoever walks
                                         // the list needs no atomics to hand the counters back).  HERE, not beside the list: where the list
                                         // lies depends on the size of the workspace a call names, and a counter at a place that moves
                                         // would be found holding an earlier call's data
constexpr uint32_t kDeferSeq = 4;
constexpr uint32_t kDeferBuckets = 0x80000000u; // in a list entry's parts field: the tile's bucket sums are in tile_buckets
constexpr uint32_t kBucketSaturated = 0xFFFFFFFFu; // a bucket holding a count above 2^25: the tile is staged whole
#ifndef WAH_DEFER_PART_SEGS
#define WAH_DEFER_PART_SEGS 32 // (clustered GiB through the list, one box: 16: 0.281 ms, 24: 0.251, 32: 0.2455, 48: 0.253)
#endif
constexpr uint32_t kDeferPartSegs = WAH_DEFER_PART_SEGS;  // output segments per work item of the list's launch (eight per wave: the chip writes faster the
                                         // shorter its waves live: launch_decode_expand)
constexpr uint32_t kCtlWords = 256;      // 1 KiB
constexpr uint32_t kErrTimeout = 1u;     // a bounded wait expired
constexpr uint32_t kErrCapacity = 2u;    // output would exceed its capacity
constexpr uint32_t kErrStream = 4u;      // malformed compressed stream
constexpr uint32_t kErrWorkspace = 8u;   // compress workspace neither zeroed nor left by an earlier launch
constexpr uint32_t kWorkspaceMagic = 0x57414832u; // "WAH2"
constexpr uint32_t kEpochWrap = (1u << 16) - 1u;  // stored epoch >= this: the next launch clears the scan area first

// ---- compress geometry: one wavefront owns one segment, a workgroup (tile) kCompressTileWaves of them ------------
#ifndef WAH_TILE_WAVES
#define WAH_TILE_WAVES 8
#endif
constexpr int kCompressTileWaves = WAH_TILE_WAVES;
constexpr int kCompressMaxWaveSegs = 5; // segments a wavefront compresses one after the other: 1, 2 or this (by bitmap size)
uint32_t compress_wave_segs(uint64_t n_segments);
// pair-layout kernel: the tile shapes of a launch (compress_pair_kernel): body tiles of body_pairs pairs per wavefront, then
// tail tiles of tail_pairs
struct TileShape {
    uint32_t body_pairs, tail_pairs, big_tiles, n_tiles;
};
TileShape compress_tile_shape(uint64_t n_segments);
// scan area of the compress kernels (see compress_tile_body): one block per superrow of 64 rows x 256 tiles
constexpr uint32_t kRowSlots = 65;                 // u64 slots of a superrow: words in front of it, words of each of its rows
constexpr uint32_t kScanSlotsAt = 64 * 256;        // 32-bit words: the slots follow the superrow's granules
constexpr uint32_t kScanBlockWords = 64 * 256 + 256; // granules + slots, padded to 1 KiB
constexpr uint64_t kScanBlockTiles = 64 * 256;
// ... and of its unsegmented mode (compress_unseg_pair_kernel): 8-byte granules, two slot arrays
constexpr uint32_t kUnsegSlotsAAt = 2 * 64 * 256;          // 32-bit words
constexpr uint32_t kUnsegSlotsBAt = 2 * 64 * 256 + 256;
constexpr uint32_t kUnsegBlockWords = 2 * 64 * 256 + 512;

// ---- decode geometry -------------------------------------------------------
constexpr int kScanTileWords = 4096; // compressed words per tile (both decode passes)
constexpr int kSumTilesPerGroup = 8;  // expand tiles per workgroup tile of the sums kernel (= its worker waves)
constexpr int kExpandWaves = 4;      // wavefronts of an expand workgroup (each expands whole segments)
// scan area of the sums kernel: one block per superrow of 64 rows x 256 workgroup tiles, 8-byte granules
constexpr uint32_t kSumScanSlotsAt = 2 * 64 * 256;          // 32-bit words: the slots follow the superrow's granules
constexpr uint32_t kSumScanBlockWords = 2 * 64 * 256 + 256; // granules + 65 slots, padded to 1 KiB
constexpr uint64_t kSumScanBlockTiles = 64 * 256;

struct CompressArgs {
    const uint32_t *in;
    const uint32_t *in2;   // pair mode (wah_bitop_device): second bitmap of the same length, combined word by word
    uint32_t op;           // ... with WAH_OP_AND / OR / XOR / ANDNOT
    uint64_t n_words;
    uint32_t n_segments;          // ceil(G / 1024)
    uint32_t wave_segs;           // segments per wavefront of this launch (compress_wave_segs); pair layout (the plain compress:
                                  // a lane owns 32 consecutive groups): wave_segs / 2 pairs per wavefront
    uint32_t reserved;            // (unused: keeps the kernels' offsets of the fields behind it, and so their machine code)
    uint32_t n_tiles;             // ceil(n_segments / (kCompressTileWaves * wave_segs)); pair layout: body + tail tiles
    uint32_t big_tiles;           // pair layout: tiles [0, big_tiles) have wave_segs / 2 pairs per wave, the rest tail_pairs
    uint32_t tail_pairs;          // pair layout: pairs per wave of the tail tiles (== wave_segs / 2: one shape)
    uint32_t fast_segments;       // 1: input 16-byte aligned -> prefetched buffer loads; 0: scalar staging
    uint32_t last_segment_groups; // groups of the last segment (1..1024)
    uint32_t full_segments;       // n_words / 992: segments that lie wholly inside the bitmap
    uint32_t tail_bytes;          // bytes of the partial segment after them (0 if none)
    uint32_t *out;
    uint64_t out_capacity;
    uint64_t *out_words;   // device scalar: C
    uint64_t *seg_offsets; // optional, n_segments + 1 entries
    uint32_t *ctrl;        // kCtlWords
    uint32_t *gen_desc;    // scan area: blocks of kScanBlockWords (see compress_tile_body)
    uint32_t *unseg_desc;  // non-null: unsegmented mode, its scan area: blocks of kUnsegBlockWords (compress_unseg_pair_kernel)
    uint64_t *tile_counts; // no-wait route only: one entry per tile, its word count, then where its words start
    uint64_t scan_words;   // 32-bit words of the whole scan area
    int keep_error;        // 1: the control block was cleared by the caller and may already hold an upstream error
    uint64_t *host_result; // optional, page-locked HOST memory: [0] = 1 | error bits << 32, [1] = C, written by the last tile
                           // (the host-pointer entry points read them after one event wait, without a copy)
    uint32_t tune;         // WAH_DIAG builds only (WAH_TUNE): 78 = the time line of tools/pair_timeline.py; 0 otherwise
};

struct ScanArgs {
    const uint32_t *comp;
    uint64_t c_words;
    uint64_t n_tiles;
    uint64_t *info;      // [0] decoded words, [1] groups
    uint64_t *tile_base; // n_tiles + 1: groups in front of each tile, last = total
    uint32_t *ctrl;
    uint32_t *gen_desc;  // scan area: blocks of kSumScanBlockWords (see decode_sums_kernel)
    uint64_t scan_words; // 32-bit words of the whole scan area
    uint8_t *tile_flags; // n_tiles: bit 0 = the tile contains a fill word of count 0, bit 1 = it is on defer_list
    int aligned16;
    uint64_t *host_result; // optional, page-locked HOST memory: [0] = 1 | error bits << 32, [1..2] = info, by the last tile
    int no_wait;           // 1: the no-wait route (per-tile totals, then one scan launch): nobody waits for anybody
    uint64_t *defer_list;  // optional: tiles that expand to more than kListSegs segments go onto this list (dt_defer) and
    uint32_t defer_capacity; // are left to the expand launch's list workgroups; their tile_flags get bit 1
};
constexpr uint32_t kListSegs = 1024; // (a tile of 4096 words that expands to more than a million groups)
// entries (16 bytes each) the list of deferred / shared-out tiles has room for: a tile goes onto it once at most, the
// one-pass decoder may add the tile of a tile's last segment once more
inline uint32_t decode_defer_capacity(uint64_t n_tiles, uint64_t) {
    const uint64_t n = 2 * n_tiles + 64;
    return n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
}

struct ExpandArgs {
    const uint32_t *comp;
    uint64_t c_words;
    uint32_t *out;
    uint64_t out_capacity;
    const uint64_t *info;
    const uint64_t *tile_base;
    const uint8_t *tile_flags; // from the sums pass: bit 0 = the tile has fill words of count 0, bit 1 = it is on the list
    uint32_t *ctrl;
    int aligned16;
    uint32_t parts; // workgroups that share one tile's output segments (set by the launcher)
    const uint64_t *defer_list; // optional: the list the sums pass left (ScanArgs::defer_list), shared out over the launch's workgroups
    const uint32_t *defer_count; // control block, kCtlDefer
    uint32_t defer_capacity;
    uint32_t n_tile_wgs;        // workgroups in front of them: tiles x parts (set by the launcher)
    const uint32_t *tile_buckets; // per expand tile 64 sums of group counts, one per 64 words (kBucketSaturated: no sum), written by
                                  // decode_tile_kernel for the tiles it puts on the list with kDeferBuckets: a work item of the list's
                                  // launch then stages only the words its segments need (tiles of fewer than 2^31 groups)
};

// wah_decompress_segments_device: decode a range of segments through the index of wah_compress_device_indexed
struct SegmentsArgs {
    const uint32_t *comp;
    uint64_t c_words;
    const uint64_t *seg_offsets; // first compressed word of every segment of the bitmap, then C
    uint64_t first_segment, n_segments;
    uint64_t groups;    // G of the whole bitmap
    uint64_t out_words; // ceil(31 G / 32): where the bitmap's last segment is cut
    uint32_t *out;      // receives segment first_segment at word 0
    uint32_t *ctrl;
};

// wah_bitop_indexed_device (fused route): the two indexed operands of bitop_tile_kernel
constexpr uint32_t kIndexedSegsPerWave = 2; // segments a wavefront of bitop_tile_kernel handles one after the other
struct BitopOperands {
    const uint32_t *comp_a, *comp_b;
    uint64_t c_words_a, c_words_b;
    const uint64_t *offs_a, *offs_b;
    uint64_t groups; // G of the bitmap both describe
    uint32_t op;     // WAH_OP_*
};
hipError_t launch_bitop_tiles(const struct CompressArgs &a, const BitopOperands &ops, hipStream_t s);

// wah_bitop_many_indexed_device: g = geometry, output and control block (its comp / seg_offsets are not used)
constexpr int kMaxBitopOperands = 8;
struct BitopManyArgs {
    SegmentsArgs g;
    const uint32_t *comp[kMaxBitopOperands];
    uint64_t c_words[kMaxBitopOperands];
    const uint64_t *offs[kMaxBitopOperands];
    int n;  // operands
    int op; // WAH_OP_*
};

// wah_bitop_list_indexed_device (wah_bitop_list.hip): any number of operands, named by a table in DEVICE memory that only
// the kernel reads (the mirror of wah_bitop_operand, include/wah.h); g as above
struct BitopListOperand {
    const uint32_t *comp;
    uint64_t c_words;
    const uint64_t *offs;
};
constexpr uint64_t kMaxBitopListOperands = 1ull << 24; // WAH_BITOP_LIST_MAX_OPERANDS
struct BitopListArgs {
    SegmentsArgs g;
    const BitopListOperand *table;
    uint32_t n;  // operands
    uint32_t op; // WAH_OP_*
};
hipError_t launch_bitop_list_segments(const BitopListArgs &a, hipStream_t s);

// wah_bitop_clauses_indexed_device (wah_bitop_list.hip): AND over clauses of (negated) ORs.  table: the flattened operands of
// all clauses; clause_ends: one word per clause in DEVICE memory, the index one past its last operand | kClauseNegate
constexpr uint64_t kClauseNegate = 1ull << 63; // WAH_CLAUSE_NEGATE
struct BitopClausesArgs {
    SegmentsArgs g;
    const BitopListOperand *table;
    const uint64_t *clause_ends;
    uint32_t n;         // operands
    uint32_t n_clauses; // 1 .. n
};
hipError_t launch_bitop_clauses_segments(const BitopClausesArgs &a, hipStream_t s);

// wah_bsi_range_indexed_device (wah_bitop_list.hip): lo <= value <= hi over a bit-sliced attribute.  table: n_slices rows,
// most significant slice first, then the existence bitmap if has_exists; bounds: lo, hi in DEVICE memory
constexpr uint32_t kMaxBsiSlices = 64; // WAH_BSI_MAX_SLICES
struct BsiRangeArgs {
    SegmentsArgs g;
    const BitopListOperand *table;
    const uint64_t *bounds;
    uint32_t n_slices;   // 1 .. 64
    uint32_t has_exists; // 0 or 1: one more row
};
hipError_t launch_bsi_range_segments(const BsiRangeArgs &a, hipStream_t s);

// wah_bsi_compare_indexed_device (wah_bitop_list.hip): A op B row by row over two bit-sliced attributes.  table: the slices of
// both interleaved by significance, most significant first (A's before B's where both have one), then A's existence bitmap if
// exists_a, then B's if exists_b
constexpr uint32_t kCmpLT = 0, kCmpLE = 1, kCmpGT = 2, kCmpGE = 3, kCmpEQ = 4, kCmpNE = 5; // WAH_CMP_*
struct BsiCompareArgs {
    SegmentsArgs g;
    const BitopListOperand *table;
    uint32_t n_slices_a, n_slices_b; // 1 .. 64 each
    uint32_t exists_a, exists_b;     // 0 or 1: one more row each
    uint32_t op;                     // kCmp*
};
hipError_t launch_bsi_compare_segments(const BsiCompareArgs &a, hipStream_t s);

// wah_bsi_arith_indexed_device (wah_bitop_list.hip): A + B or A - B row by row as a new bit-sliced attribute.  table: A's existence
// bitmap if exists_a, then B's if exists_b, then the slices of both interleaved by significance, LEAST significant first (A's
// before B's where both have one).  matrix: the decoded slice matrix [n_slices_out (+ 1 with an existence row), n_words] the
// kernel writes every word of, most significant slice first, the AND of the existence bitmaps last
constexpr uint32_t kArithAdd = 0, kArithSub = 1; // WAH_ARITH_*
struct BsiArithArgs {
    const BitopListOperand *table;
    uint32_t *matrix;
    uint32_t *ctrl;
    uint64_t n_words;                // words of one slice, a multiple of kSegWords
    uint64_t groups, n_segments;     // of one slice
    uint32_t n_slices_a, n_slices_b; // 1 .. 64 each
    uint32_t n_slices_out;           // 1 .. 64
    uint32_t exists_a, exists_b;     // 0 or 1: one more row each
    uint32_t sub;                    // 0: A + B, 1: A - B
};
hipError_t launch_bsi_arith_segments(const BsiArithArgs &a, hipStream_t s);

// wah_bsi_mul_indexed_device (wah_bitop_list.hip): A * B row by row as a new bit-sliced attribute.  table: A's existence bitmap if
// exists_a, then B's if exists_b, then ALL of A's slices, least significant first, then ALL of B's, least significant first.
// matrix: as BsiArithArgs.  work: n_segments areas of (n_slices_a + n_slices_out) slices of kSegGroups groups each, a wave's own:
// A's image, then the accumulator; uninitialised
struct BsiMulArgs {
    const BitopListOperand *table;
    uint32_t *matrix;
    uint32_t *work;
    uint32_t *ctrl;
    uint64_t n_words;                // words of one slice, a multiple of kSegWords
    uint64_t groups, n_segments;     // of one slice
    uint32_t n_slices_a, n_slices_b; // 1 .. 64 each
    uint32_t n_slices_out;           // 1 .. 64
    uint32_t exists_a, exists_b;     // 0 or 1: one more row each
};
hipError_t launch_bsi_mul_segments(const BsiMulArgs &a, hipStream_t s);

// wah_bsi_div_indexed_device (wah_bitop_list.hip): floor(A / B) or A mod B row by row as a new bit-sliced attribute.  table: A's
// existence bitmap if exists_a, then B's if exists_b, then ALL of B's slices, least significant first, then ALL of A's, MOST
// significant first.  matrix: [n_slices_out + 1, n_words], the existence row -- the bitmaps present AND (B != 0) -- always there.
// work: n_segments areas of (3 n_slices_b + 2) slices of kSegGroups groups each, a wave's own: B's image, then the two
// remainder buffers of n_slices_b + 1 slices (the top slot of the second holds the last quotient slice); uninitialised
constexpr uint32_t kDivQuotient = 0, kDivRemainder = 1; // WAH_DIV_*
struct BsiDivArgs {
    const BitopListOperand *table;
    uint32_t *matrix;
    uint32_t *work;
    uint32_t *ctrl;
    uint64_t n_words;                // words of one slice, a multiple of kSegWords
    uint64_t groups, n_segments;     // of one slice
    uint32_t n_slices_a, n_slices_b; // 1 .. 64 each
    uint32_t n_slices_out;           // 1 .. 64
    uint32_t exists_a, exists_b;     // 0 or 1: one more row each
    uint32_t remainder;              // 0: the quotient, 1: the remainder
};
hipError_t launch_bsi_div_segments(const BsiDivArgs &a, hipStream_t s);

// wah_bsi_kth_indexed_device (wah_bitop_list.hip): the value of a given rank among the rows the filters select -- a radix select
// over the slices, kBsiKthDigitBits of them per pass, most significant digit first.  table: n_filters filter rows, then
// n_slices slice rows, most significant first; query: kind, a, b in DEVICE memory; result: found, value, total, less, equal.
// state and hist lie in the scratch (cleared by the caller): what the decide kernel of one pass leaves for the next pass,
// and per pass kBsiKthCopies histograms of kBsiKthBuckets counts, added into by the pass kernel's waves.
#ifndef WAH_BSI_KTH_DIGIT_BITS
#define WAH_BSI_KTH_DIGIT_BITS 4 // (32 incompressible slices of 32 MiB: 2: 2.63 ms, 3: 2.06, 4: 1.55 -- DESIGN.md 5.14)
#endif
#ifndef WAH_BSI_KTH_COPIES
#define WAH_BSI_KTH_COPIES 8 // (the same: 1: 1.75 ms, 8: 1.55, 64: 1.56)
#endif
constexpr uint32_t kBsiKthDigitBits = WAH_BSI_KTH_DIGIT_BITS; // 1 .. 4
constexpr uint32_t kBsiKthBuckets = 1u << kBsiKthDigitBits;
constexpr uint32_t kBsiKthCopies = WAH_BSI_KTH_COPIES; // histograms per pass, chosen by workgroup index; each on 128-byte lines of its own
constexpr uint32_t kBsiKthMaxFilters = 64;
constexpr uint32_t kBsiKthStateWords = 16; // u64: kKth* below
constexpr uint32_t kKthPrefix = 0; // the value's bits decided so far, at their own significance
constexpr uint32_t kKthRank = 1;   // the rank from the bottom among the rows that share the prefix
constexpr uint32_t kKthLess = 2;   // selected rows below the prefix's range
constexpr uint32_t kKthFound = 3;  // 1: the query names a row
constexpr uint32_t kKthTotal = 4;  // selected rows
struct BsiKthArgs {
    const BitopListOperand *table;
    const uint64_t *query;
    uint64_t *result;
    uint64_t *state; // kBsiKthStateWords
    uint64_t *hist;  // passes x kBsiKthCopies x kBsiKthBuckets
    uint32_t *ctrl;
    uint64_t groups, n_segments;
    uint32_t n_filters; // 0 .. 64
    uint32_t n_slices;  // 1 .. 64
    uint32_t pass;      // 0 .. ceil(n_slices / kBsiKthDigitBits) - 1
    uint32_t pad_bits;  // as SelectCountArgs
};
hipError_t launch_bsi_kth_pass(const BsiKthArgs &a, hipStream_t s);
hipError_t launch_bsi_kth_decide(const BsiKthArgs &a, hipStream_t s);

// wah_bsi_kth_grouped_indexed_device (wah_bitop_list.hip): the same radix select for n_groups x n_queries SELECTS at once --
// select g * n_queries + q asks query q of the rows that the filters AND rows g * rows_per_group .. of `keys` select.  The three
// tables are contiguous each; queries: n_queries x {kind, a, b}, results: five words per select, both in DEVICE memory.  state
// (kBsiKthStateWords per select) and hist (per pass and select kBsiKthGroupCopies histograms of kBsiKthBuckets counts) lie in the
// scratch, cleared by the caller.
#ifndef WAH_BSI_KTH_GROUP_COPIES
#define WAH_BSI_KTH_GROUP_COPIES 1 // (one address sees a select's segments only, not a whole pass: DESIGN.md 5.14.1)
#endif
constexpr uint32_t kBsiKthGroupCopies = WAH_BSI_KTH_GROUP_COPIES; // histograms per pass and select, chosen by workgroup index
constexpr uint32_t kBsiKthGroupMaxSelects = 4096;                 // WAH_BSI_KTH_GROUPED_MAX_LANES
struct BsiKthGroupArgs {
    const BitopListOperand *filters, *keys, *slices;
    const uint64_t *queries;
    uint64_t *results;
    uint64_t *state; // selects x kBsiKthStateWords
    uint64_t *hist;  // passes x selects x kBsiKthGroupCopies x kBsiKthBuckets
    uint32_t *ctrl;
    uint64_t groups, n_segments; // (groups: G of the bitmap)
    uint32_t n_filters;          // 0 .. 64
    uint32_t rows_per_group;     // 1 .. kGroupMaxRows
    uint32_t n_groups, n_queries; // n_groups * n_queries <= kBsiKthGroupMaxSelects
    uint32_t n_slices;           // 1 .. 64
    uint32_t pass;               // 0 .. ceil(n_slices / kBsiKthDigitBits) - 1
    uint32_t pad_bits;           // as SelectCountArgs
};
hipError_t launch_bsi_kth_group_pass(const BsiKthGroupArgs &a, hipStream_t s);
hipError_t launch_bsi_kth_group_decide(const BsiKthGroupArgs &a, hipStream_t s);

// wah_fetch_indexed_device (wah_bitop_list.hip): the values of listed rows -- per listed row the one bit it has in every row
// of the table.  rows: n_rows positions in DEVICE memory, non-descending; out: one u64 per listed row.  The check pass cuts the
// list into ITEMS -- at most 64 consecutive listed rows of one segment -- and appends the list index of every item's first row
// to `items` (capacity entries, in the scratch); how many there are stays in the control block at kCtlFetchItems (64 bits,
// cleared by the caller).  The items pass walks one segment per item.
constexpr uint32_t kCtlFetchItems = 224; // (a 128-byte line of the control block that no other call of this scratch uses)
constexpr uint32_t kFetchBits = 0, kFetchFirst = 1; // WAH_FETCH_BITS, WAH_FETCH_FIRST
struct FetchArgs {
    const BitopListOperand *table;
    const uint64_t *rows;
    uint64_t *out;
    uint64_t *items;
    uint32_t *ctrl;
    uint64_t n_rows;
    uint64_t n_bits;   // 32 n_words: a row is below it
    uint64_t groups;   // G of the bitmap
    uint64_t capacity; // entries of `items`
    uint32_t n_operands;
};
hipError_t launch_fetch_check(const FetchArgs &a, hipStream_t s);
hipError_t launch_fetch_items(const FetchArgs &a, uint32_t mode, hipStream_t s);

// wah_values_indexed_device (wah_values.hip): the values of the row RANGE [first_row, first_row + n_rows), the modes as above.
// An item is a segment of the window (n_segments of them from first_segment on), under kFetchBits with more than 32 table rows
// a segment and a half of the value: n_items = n_segments x halves, item t being segment first_segment + t / halves, half
// t % halves.  out: one u64 per row of the window.
struct ValuesArgs {
    const BitopListOperand *table;
    uint64_t *out;
    uint32_t *ctrl;
    uint64_t first_row, n_rows; // n_rows >= 1, first_row + n_rows <= 32 n_words
    uint64_t groups;            // G of the bitmap
    uint64_t first_segment, n_items;
    uint32_t n_operands;
};
hipError_t launch_values_items(const ValuesArgs &a, uint32_t mode, hipStream_t s);

// wah_bsi_member_indexed_device (wah_member.hip): value IN (set) over a bit-sliced attribute.  table: n_slices rows, most
// significant slice first, then the existence bitmap if has_exists.  set: a list of set_capacity u64, the first *set_count (or
// all, set_count == nullptr) non-decreasing, or with `bitset` the words of a bit array of set_capacity bits.  An item is a
// segment, above 32 slices a segment and a half of its groups: n_items = n_segments x (n_slices > 32 ? 2 : 1), item t being
// segment t / halves, groups 512 (t % halves) .. of it.  g as in BitopListArgs (first_segment is 0).
struct MemberArgs {
    SegmentsArgs g;
    const BitopListOperand *table;
    const void *set;
    uint64_t set_capacity;
    const uint64_t *set_count;
    uint64_t n_items;
    uint32_t n_slices;   // 1 .. 64
    uint32_t has_exists; // 0 or 1: one more row
    uint32_t negate;     // 0 or 1: NOT IN
    uint32_t bitset;     // 0 or 1
};
hipError_t launch_member(const MemberArgs &a, hipStream_t s); // the list's check, then the items

// wah_bsi_group_by_indexed_device (wah_group_by.hip): COUNT and SUM per value of a bit-sliced key.  filters: n_filters rows; key:
// n_slices_key rows, most significant slice first, then the existence bitmap if has_exists; val: n_slices_val rows, most
// significant first (0: count only, val and sums are nullptr).  map: n_keys u32, key -> bucket, or nullptr (n_keys is 0): the key
// is the bucket.  counts: n_buckets + 1 u64, sums: as many (low, high) pairs, both added into; the last bucket is "other".  An item
// is a segment, with a value attribute a segment and a half of its groups: n_items = n_segments x (n_slices_val ? 2 : 1).
struct GroupByArgs {
    const BitopListOperand *filters, *key, *val;
    const uint32_t *map;
    uint64_t *counts, *sums;
    uint32_t *ctrl;
    uint64_t n_rows;  // rows at or behind it are never selected; <= 32 n_words
    uint64_t groups;  // G of the bitmap
    uint64_t n_items;
    uint64_t n_keys;  // 0 .. 2^32
    uint32_t n_buckets;    // 1 .. 2^30
    uint32_t n_filters;    // 0 .. kGroupMaxFilters
    uint32_t n_slices_key; // 1 .. 32
    uint32_t n_slices_val; // 0 .. 32
    uint32_t has_exists;   // 0 or 1: one more key row
};
hipError_t launch_group_by(const GroupByArgs &a, hipStream_t s);

// wah_bsi_map_indexed_device (wah_map.hip): a bit-sliced key through a lookup table, as a new bit-sliced attribute.  key:
// n_slices_key rows, most significant slice first, then the existence bitmap if has_exists.  map: n_keys u32, key -> value,
// 0xFFFFFFFF: no value.  matrix: the decoded slice matrix [n_slices_out (+ 1 with out_exists), n_words] the kernel writes every
// word of, most significant slice first, the rows that have a value last.  An item is a segment.
struct BsiMapArgs {
    const BitopListOperand *key;
    const uint32_t *map;
    uint32_t *matrix;
    uint32_t *ctrl;
    uint64_t n_rows;             // rows at or behind it never have a value; <= 32 n_words
    uint64_t n_words;            // words of one slice, a multiple of kSegWords
    uint64_t groups, n_segments; // of one slice
    uint64_t n_keys;             // 1 .. 2^32
    uint32_t n_slices_key;       // 1 .. 32
    uint32_t n_slices_out;       // 1 .. 32
    uint32_t has_exists;         // 0 or 1: one more key row
    uint32_t out_exists;         // 0 or 1: one more matrix row
    uint32_t partial;            // 0: a miss is refused; 1: a miss is a row without a value
};
hipError_t launch_bsi_map(const BsiMapArgs &a, hipStream_t s);

// wah_bsi_cumsum_indexed_device (wah_cumsum.hip): the running sum of a bit-sliced value over the selected rows, as a new bit-sliced
// attribute.  filters: n_filters rows; val: n_slices_val rows, most significant slice first (0: every selected row counts 1),
// then the existence bitmap if has_exists.  totals: n_segments u64 in the scratch: a segment's sum, then -- scanned in place -- the
// sum of the segments in front of it.  matrix: the decoded slice matrix [n_slices_out (+ 1 without all_rows), n_words] the last
// kernel writes every word of, most significant slice first, the selection last.  An item is a segment.
struct BsiCumsumArgs {
    const BitopListOperand *filters, *val;
    uint64_t *totals;
    uint32_t *matrix;
    uint32_t *ctrl;
    uint64_t n_rows;             // rows at or behind it are never selected and hold 0; <= 32 n_words
    uint64_t n_words;            // words of one slice, a multiple of kSegWords
    uint64_t groups, n_segments; // of one slice
    uint32_t n_filters;          // 0 .. kGroupMaxFilters
    uint32_t n_slices_val;       // 0 .. 32
    uint32_t n_slices_out;       // 1 .. 64
    uint32_t has_exists;         // 0 or 1: one more value row
    uint32_t exclusive;          // 0: rows q <= p; 1: rows q < p
    uint32_t all_rows;           // 0: unselected rows hold 0, the selection is the last matrix row; 1: they carry the sum, no such row
};
hipError_t launch_bsi_cumsum(const BsiCumsumArgs &a, hipStream_t s); // the segment totals, their scan, the rows

// wah_bsi_cumsum_parts_indexed_device (wah_cumsum.hip): the same, starting again at every row set in `starts`, ONE row.  c: as
// above, c.totals unused.  records: n_segments of them in the scratch: whether the segment holds a start and the sum of its
// selected values at or behind its last one, then -- scanned in place -- in `sum` what flows into the segment.
struct BsiCumsumPartsRecord {
    uint64_t sum;
    uint64_t has_start; // 0 or 1
};
struct BsiCumsumPartsArgs {
    BsiCumsumArgs c;
    const BitopListOperand *starts;
    BsiCumsumPartsRecord *records;
};
hipError_t launch_bsi_cumsum_parts(const BsiCumsumPartsArgs &a, hipStream_t s);

// wah_bsi_total_parts_indexed_device (wah_cumsum.hip): the partition's TOTAL in every row.  p: as above, p.records unused,
// p.c.exclusive 0.  records: n_segments of them in the scratch: whether the segment holds a start, the sum of its selected values in
// front of its first one (head) and at or behind its last one (tail), both the whole segment's where it holds none; then -- scanned
// in place -- in `tail` what flows into the segment from the front and in `head` what flows into it from behind.
struct BsiTotalPartsRecord {
    uint64_t head;
    uint64_t tail;
    uint64_t has_start; // 0 or 1
};
struct BsiTotalPartsArgs {
    BsiCumsumPartsArgs p;
    BsiTotalPartsRecord *records;
};
hipError_t launch_bsi_total_parts(const BsiTotalPartsArgs &a, hipStream_t s);

// ... on operands of few words per segment: their runs merged in the compressed domain, one lane per segment
// (wah_bitop_runs.hip): count pass, scan of the tile totals, write pass
struct BitopRunsArgs {
    const uint32_t *comp[kMaxBitopOperands];
    uint64_t c_words[kMaxBitopOperands];
    const uint64_t *offs[kMaxBitopOperands];
    int n;  // operands
    int op; // WAH_OP_*
    uint64_t groups, n_segments;
    uint32_t *seg_count;  // scratch: n_segments
    uint64_t *tile_total; // scratch: one entry per tile of segments: its words, then the words in front of it
    uint32_t *temp;       // scratch: the segments' results before they are moved together: sum of c_words + 16 words
    uint32_t *out;
    uint64_t out_capacity;
    uint64_t *out_words;
    uint64_t *out_offsets; // optional, n_segments + 1 entries
    uint32_t *ctrl;
};
hipError_t launch_bitop_runs(const BitopRunsArgs &a, hipStream_t s);

// wah_count_list_indexed_device / wah_positions_indexed_device (wah_select.hip): set bits counted and listed in the compressed
// domain.  The count pass: per table row (table != nullptr: counts has n_operands entries, cleared by the caller, added into)
// or per segment of the one operand `one` (counts has n_segments entries, every one stored).
struct SelectCountArgs {
    const BitopListOperand *table;
    BitopListOperand one;
    uint32_t n_operands;
    uint32_t pad_bits;   // 31 G - 32 n_words: bits of the bitmap's last group that lie behind the bitmap (0 .. 30)
    uint64_t groups, n_segments;
    uint64_t *counts;
    uint32_t *ctrl;
};
hipError_t launch_select_count(const SelectCountArgs &a, hipStream_t s);
// wah_count_masked_indexed_device (wah_select.hip): the set bits of (mask AND operand) for every pair of a mask table and an
// operand table, no operand decoded and no bitmap written.  counts: n_masks x n_operands entries, row-major, cleared by the
// caller, added into.
struct CountMaskedArgs {
    const BitopListOperand *masks, *operands;
    uint32_t n_masks, n_operands; // n_masks * n_operands <= kMaxBitopListOperands
    uint32_t pad_bits;            // as SelectCountArgs
    uint32_t chunk;               // operands that share one mask image, 1 .. 64 (set by the launcher)
    uint64_t groups, n_segments;
    uint64_t *counts;
    uint32_t *ctrl;
};
hipError_t launch_count_masked(const CountMaskedArgs &a, hipStream_t s);
// wah_group_sum_indexed_device (wah_select.hip): the masked count with a CONJUNCTION for a mask -- group g's is the AND of the
// n_filters rows of `filters` and of rows g * rows_per_group .. of `keys` --, the conjunction's own set bits beside the counts
// (rows: n_groups entries), and the fold of the counts of every attribute's slices into its sum.  rows and counts (n_groups x
// n_operands, row-major) are cleared by the caller and added into; every entry of sums is stored.
constexpr uint32_t kGroupMaxFilters = 64, kGroupMaxRows = 8, kGroupMaxAttrs = 64; // WAH_GROUP_MAX_*
struct GroupCountArgs {
    const BitopListOperand *filters, *keys, *operands;
    uint32_t n_filters, rows_per_group;
    uint32_t n_groups, n_operands; // n_groups * n_operands <= kMaxBitopListOperands
    uint32_t pad_bits;             // as SelectCountArgs
    uint32_t chunk;                // operands that share one image, 1 .. 64 (set by the launcher)
    uint64_t groups, n_segments;   // (groups: G of the bitmap)
    uint64_t *rows, *counts;
    uint32_t *ctrl;
};
struct GroupFoldArgs {
    const uint64_t *counts;
    uint64_t *sums; // n_groups x n_attrs x (low, high)
    uint32_t n_groups, n_operands, n_attrs;
    uint8_t bits[kGroupMaxAttrs]; // slices of every attribute, most significant first: they add up to n_operands
};
hipError_t launch_group_sum(const GroupCountArgs &a, const GroupFoldArgs &f, hipStream_t s);
// the rank table's scan: chunks of this many entries, one entry per chunk a level up
constexpr uint32_t kRankChunk = 4096;
hipError_t launch_select_rank_scan(uint64_t *ranks, uint64_t n_segments, uint64_t *level1, uint64_t *level2, hipStream_t s);
// the emit pass: g = stream, index, geometry and control block of the one operand (first_segment, out, out_words not used)
constexpr uint32_t kSelectStageSlots = 64 * 31; // 16-bit LDS slots per wavefront: the set bits of one step of 64 groups
struct SelectEmitArgs {
    SegmentsArgs g;
    const uint64_t *ranks; // n_segments + 1: set bits in front of every segment, then the total
    uint64_t first, end;   // the window of ranks (end = first + capacity, saturating)
    uint64_t capacity;
    uint64_t *out;         // capacity entries
    uint64_t *info;        // [0] total, [1] written
    uint32_t pad_bits;
};
hipError_t launch_select_emit(const SelectEmitArgs &a, hipStream_t s);

// wah_from_positions_device (wah_from_positions.hip): sorted lists of row numbers in, their compress() streams back to back and
// the segment index of the whole out.  offsets: n_lists * n_segments + 1 entries -- the count pass stores every (list, segment)'s
// words there, launch_select_rank_scan turns them into the index in place, the emit pass reads it.
struct FromPositionsArgs {
    const uint64_t *rows;      // n_rows positions, the lists back to back
    const uint64_t *list_ends; // n_lists: one past every list's last row
    uint64_t n_rows, n_lists;
    uint64_t n_bits;           // 32 n_words: a row is below it
    uint64_t groups;           // G of ONE bitmap
    uint64_t n_segments;       // S = ceil(G / 1024), per list
    uint32_t *out;
    uint64_t out_capacity;
    uint64_t *out_words;
    uint64_t *offsets;
    uint32_t *ctrl;
};
hipError_t launch_from_positions_check(const FromPositionsArgs &a, hipStream_t s);
hipError_t launch_from_positions_segments(const FromPositionsArgs &a, bool emit, hipStream_t s);

// wah_splice_indexed_device (wah_splice.hip): row ranges of indexed bitmaps concatenated into new ones, for all columns of an
// index at once.  pieces and table are read by the device only; the check launch leaves start(0 .. n_pieces) in `starts` (a
// refused piece counts as no rows); offsets is used as FromPositionsArgs::offsets, n_columns * n_segments + 1 entries.
struct SplicePiece {
    uint64_t n_words, first_row, n_rows; // wah_splice_piece
};
constexpr uint64_t kSpliceMaxPieces = 1ull << 16; // WAH_SPLICE_MAX_PIECES
struct SpliceArgs {
    const SplicePiece *pieces;     // n_pieces
    const BitopListOperand *table; // n_pieces * n_columns, piece-major
    uint64_t *starts;              // scratch: n_pieces + 1
    uint64_t n_pieces, n_columns;
    uint64_t n_bits;               // 32 n_words_out: the rows of all pieces fit below it
    uint64_t groups;               // G of ONE output bitmap
    uint64_t n_segments;           // S = ceil(G / 1024), per column
    uint32_t *out;
    uint64_t out_capacity;
    uint64_t *out_words;
    uint64_t *offsets;
    uint32_t *ctrl;
};
hipError_t launch_splice_check(const SpliceArgs &a, hipStream_t s);
hipError_t launch_splice_segments(const SpliceArgs &a, bool emit, hipStream_t s);

// wah_compact_indexed_device (wah_compact.hip): the rows a mask bitmap selects (or, with del, does not select) of every column of
// an index, moved together into new indexed bitmaps.  mask and table are read by the device only; the check launches leave the
// selected rows in front of every source segment, then their total T, in `starts` (src_segments + 1 entries; level1 / level2: the
// upper levels of that scan); offsets is used as FromPositionsArgs::offsets, n_columns * n_segments + 1 entries.
struct CompactArgs {
    const BitopListOperand *mask;  // one row
    const BitopListOperand *table; // n_columns rows
    uint64_t *starts;              // scratch: src_segments + 1
    uint64_t *level1, *level2;     // scratch: launch_select_rank_scan's levels over starts
    uint64_t *out_rows;            // receives T
    uint64_t n_columns;
    uint64_t src_rows;             // n_rows: only positions below it are rows
    uint64_t src_groups;           // G of ONE source bitmap
    uint64_t src_segments;         // ceil(src_groups / 1024)
    uint32_t del;                  // 0: a row is selected where the mask bit is 1; 1: where it is 0
    uint64_t n_bits;               // 32 n_words_out: T is at most this
    uint64_t groups;               // G of ONE output bitmap
    uint64_t n_segments;           // S = ceil(G / 1024), per column
    uint32_t *out;
    uint64_t out_capacity;
    uint64_t *out_words;
    uint64_t *offsets;
    uint32_t *ctrl;
};
hipError_t launch_compact_check(const CompactArgs &a, hipStream_t s);
hipError_t launch_compact_segments(const CompactArgs &a, bool emit, hipStream_t s);

// wah_update_indexed_device (wah_update.hip): per column the blend of two indexed bitmaps under a mask bitmap -- then_c where the
// mask selects a row below n_rows, else_c everywhere else -- as new indexed bitmaps.  The three tables are read by the device
// only; an else or then row whose stream and index pointers are both null is a constant (stream_words 0 or 1).  offsets is used
// as FromPositionsArgs::offsets, n_columns * n_segments + 1 entries.  The call has no check launch: launch_update_check launches
// nothing.
struct UpdateArgs {
    const BitopListOperand *mask;       // one row
    const BitopListOperand *else_table; // n_columns rows
    const BitopListOperand *then_table; // n_columns rows
    uint64_t n_columns;
    uint64_t n_rows;                    // only positions below it are selected
    uint64_t n_bits;                    // 32 n_words
    uint64_t groups;                    // G of ONE bitmap
    uint64_t n_segments;                // S = ceil(G / 1024), per column
    uint32_t *out;
    uint64_t out_capacity;
    uint64_t *out_words;
    uint64_t *offsets;
    uint32_t *ctrl;
};
hipError_t launch_update_check(const UpdateArgs &a, hipStream_t s);
hipError_t launch_update_segments(const UpdateArgs &a, bool emit, hipStream_t s);

// wah_bsi_build_device (wah_bsi_build.hip): a column of 64-bit values in, the decoded slice matrix [n_bits (+ 1), n_words] out --
// most significant slice first, the existence bitmap last when exists != nullptr.  Every word of the matrix is written.
struct BsiBuildArgs {
    const uint64_t *values; // n_rows values (may be null when n_rows == 0)
    const uint8_t *exists;  // optional: n_rows bytes, 0 = the row has no value
    uint64_t n_rows;        // <= 32 n_words; rows behind them hold the value 0 and do not exist
    uint64_t n_words;       // words of one slice
    uint32_t n_bits;        // 1 .. 64
    uint32_t *out;
    uint32_t *ctrl;
};
hipError_t launch_bsi_slices(const BsiBuildArgs &a, hipStream_t s);

// wah_bitop_device: what the operands' decodes left behind, checked on the device before the combining pass
struct PairCheck {
    const uint64_t *info_a, *info_b; // [decoded words, groups] of the two operands
    const uint32_t *ctrl_a, *ctrl_b; // their decode control blocks (error bits)
    uint64_t groups;                 // what both must have expanded to
};

// launchers (wah_compress.hip, wah_decode.hip, wah_aux.hip)
hipError_t launch_compress(const CompressArgs &a, hipStream_t s); // pair mode when a.in2 != nullptr
hipError_t launch_compress_nowait(const CompressArgs &a, hipStream_t s); // count, scan, place: nobody waits for anybody
uint32_t compress_nowait_wave_segs();
hipError_t launch_bitop_check(const uint64_t *info_a, const uint64_t *info_b, const uint32_t *ctrl_a, const uint32_t *ctrl_b, uint64_t groups,
                              uint32_t *ctrl, hipStream_t s);
hipError_t launch_decode_sums(const ScanArgs &a, hipStream_t s);
hipError_t launch_decode_expand(const ExpandArgs &a, uint64_t n_tiles, hipStream_t s);
hipError_t launch_decode_tiles(const ScanArgs &sa, const ExpandArgs &xa, uint64_t *defer, hipStream_t s); // one pass: decode_tile_kernel
// which decoder a call ran (wah_last_decode_route)
constexpr int kRouteNone = 0, kRouteOnePass = 1, kRouteTwoLaunches = 2, kRouteNoWait = 3;
constexpr uint32_t kDecodeTileWords = 2 * kScanTileWords; // ... whose workgroup tiles are this long
hipError_t launch_clear(void *p, size_t bytes, hipStream_t s);
hipError_t launch_build_index(const uint32_t *comp, uint64_t c_words, const uint64_t *tile_base, const uint64_t *info, uint64_t *offsets,
                              uint64_t capacity, uint32_t *ctrl, uint64_t n_tiles, hipStream_t s);
hipError_t launch_decode_segments(const SegmentsArgs &a, hipStream_t s);
hipError_t launch_bitop_many_segments(const BitopManyArgs &a, hipStream_t s);

// wah_merge_fills_device (after the sums pass): kept-word counts and first kept positions per tile, their scans, scatter
struct MergeArgs {
    const uint32_t *comp;
    uint64_t c_words;
    uint64_t n_tiles;
    const uint64_t *tile_base; // groups in front of every tile (sums pass)
    const uint64_t *info;      // [decoded words, groups] (sums pass)
    uint64_t *tile_kept;       // n_tiles + 1: kept words per tile, then their exclusive scan
    uint64_t *tile_first;      // n_tiles: group position of a tile's first kept word, then of the first kept word BEHIND the tile
    uint32_t *out;
    uint64_t out_capacity;
    uint64_t *out_words;
    uint32_t *ctrl;
};
hipError_t launch_merge_fills(const MergeArgs &a, hipStream_t s);
hipError_t launch_validate(const uint32_t *comp, uint64_t c_words, const uint64_t *tile_base, const uint64_t *info, uint64_t *report,
                           uint64_t n_tiles, hipStream_t s);
hipError_t launch_gen_uniform(uint32_t *out, uint64_t n, uint64_t seed, uint64_t thr, hipStream_t s);
hipError_t launch_gen_clustered(uint32_t *out, uint64_t n, uint64_t seed, uint64_t thr, hipStream_t s);
hipError_t launch_copy(const uint32_t *in, uint32_t *out, uint64_t n, hipStream_t s);

} // namespace wah
