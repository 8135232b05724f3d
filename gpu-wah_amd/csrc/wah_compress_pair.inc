// wah_compress_pair.inc -- the PAIR layout of the compressor (included by wah_compress.hip, inside namespace wah::{anonymous}):
// its building blocks, the passes of a wave over its pairs that BOTH pair-layout bodies run, and the segmented body, which
// adds to them the segment index and the 4-byte granule of the row scan (the unsegmented one: wah_compress_unseg_pair.inc).
//
// Same tile protocol as compress_tile_body (arrival tickets, launch epochs, row scan: see there), different use of the
// wavefront.  There a step is 64 consecutive groups across the lanes, so "the next group" is a DPP move, every step needs
// its own rank (v_mbcnt + v_bcnt pairs) and fill lengths come out of a position array in LDS: 395 vector + 67 LDS
// instructions per segment, and the kernel spends half of its wave cycles issuing them (profiles/r02_pmc_sq_counters).
// Here a LANE owns 32 CONSECUTIVE groups:
//   * 32 groups = 992 bits = 31 words EXACTLY, so every lane's words start on a word boundary and the funnel shifts of
//     the regroup (kernels.cu:72-79) are the same compile-time constants in every lane; a wavefront = 64 x 32 groups =
//     a PAIR of segments (1984 words, staged in 8 KB of wave-private LDS by eight coalesced 16-byte loads per lane and
//     re-read with a lane stride of 31 words: conflict-free on 32 banks);
//   * "the next group" is the next register: classify + run detect (kernels.cu:93-141 and the cross-warp merge of
//     :188-229) is 5 vector instructions per group with no cross-lane traffic except ONE DPP move per pair (the first
//     group of the lane above; the last group of a segment never matches), and the run-end flags of a lane are one
//     32-bit register;
//   * rank = ONE DPP prefix sum of the lanes' popcounts per pair; fill length = distance to the previous run end, which
//     inside a lane is a register (nl) and across lanes ONE DPP max-scan per pair (kernels.cu:156-174, :188-229);
//   * a lane's final words (kernels.cu:244-249) go to LDS at its rank under EXEC = "ends a run at group k", with no
//     select, no dump slot and no position array; the pair's words are then parked in registers as 16-byte pieces (the
//     wave's last pair stays in LDS) and leave the chip as 16-byte-per-lane stores (a store that straddles the end of its descriptor writes exactly the
//     dwords inside it, 4-byte aligned addresses are fine: tools/store_bounds.hip, checked on gfx950).
// 301 vector + 33 LDS instructions per segment on the sparse GiB (profiles/r03_pmc_sq_counters_sparse.txt; round 2: 395 + 67).

constexpr u32 kPairSegs = 2;
constexpr u32 kPairWords = kPairSegs * kSegWords;    // 1984
constexpr u32 kPairGroups = kPairSegs * kSegGroups;  // 2048
constexpr u32 kPairStageWords = 2048;                // 8 KB per wave: the staged pair, later its compacted words
constexpr u32 kLaneGroups = 32;
constexpr u32 kLaneWords = 31;
static_assert(64u * kLaneWords == kPairWords && 64u * kLaneGroups == kPairGroups, "a wavefront = a pair of segments");

struct PairLoad {
    u32x4 v[8];
};
struct LaneGroups {
    u32 x[kLaneGroups]; // group 32 lane + k of the pair
};

// issue the eight coalesced 16-byte loads of one pair (7936 B = 496 x 16 B; lanes 48..63 of the eighth load and everything
// past the end of the bitmap read as zero: the descriptor's bounds do the zero padding of the tail, F5)
template <bool kAligned>
__device__ __forceinline__ void prefetch_pair(const CompressArgs &a, u32 pair, u32 lane, PairLoad &p) {
    const u64 w0 = (u64)pair * kPairWords;
    const u64 left = a.n_words > w0 ? a.n_words - w0 : 0ull;
    const u32 bytes = left >= kPairWords ? kPairWords * 4u : (u32)left * 4u;
    const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(a.in + w0, bytes);
    const u32 off = lane * 16u;
    // (the piece's offset in the scalar operand: one offset register for all eight loads)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (kAligned)
            p.v[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 1024 * i, 2); // nontemporal: see load16
        else
            p.v[i] = load16<false>(rsrc, off + 1024u * i);
    }
}

__device__ __forceinline__ void stage_pair(const PairLoad &p, u32 *lds, u32 lane) {
    u32x4 *dst = reinterpret_cast<u32x4 *>(lds);
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[lane + 64 * i] = p.v[i];
}

// regroup (kernels.cu:72-79): the lane's 31 words -> its 32 groups.  Group k starts at bit 31 k of the lane's words.
__device__ __forceinline__ void regroup_pair(const u32 *stage, u32 lane, LaneGroups &g) {
    const u32 *sp = stage + kLaneWords * lane;
    u32 w[kLaneWords];
#pragma unroll
    for (int j = 0; j < (int)kLaneWords; ++j) w[j] = sp[j];
    // from the top down, so that a group can take the register of the word it no longer needs; every group is pinned as
    // a finished value (otherwise the compiler keeps the unmasked funnel shifts for pass 1 AND the masked groups for
    // pass 2: 32 more registers)
    g.x[31] = w[30] >> 1;
    asm volatile("" : "+v"(g.x[31]));
#pragma unroll
    for (int k = (int)kLaneWords - 1; k >= 1; --k) {
        g.x[k] = __builtin_amdgcn_alignbit(w[k], w[k - 1], 32 - k) & kOnes31;
        asm volatile("" : "+v"(g.x[k]));
    }
    g.x[0] = w[0] & kOnes31;
    asm volatile("" : "+v"(g.x[0]));
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // every staged word is in registers before the buffer is reused
}

// f = 2 f + (z != 0): the run-end flag of one more group, pushed into the lane's flag word from below
__device__ __forceinline__ void flag_push(u32 &f, u32 z) {
    asm volatile("v_cmp_ne_u32 vcc, 0, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(f) : "v"(z) : "vcc");
}

// PASS 1: classify (kernels.cu:93-112) + run ends (kernels.cu:126-141 and the merge of :188-229).  A group does NOT end a
// run iff it is a fill and the next group of its segment has the same value:
//     z = (x ^ next) | ((x + 1) & 0x7FFFFFFE)  is zero  <=>  x is 0 or 0x7FFFFFFF AND the next group equals it
// Returns the lane's flag word: bit 31 - k says whether group k of the lane ends a run.  The group after a segment's last
// one (lanes 31 and 63, k = 31) never matches, so every segment closes its last run (tests.cpp:166-172).
// nvalid: groups of the pair that exist (F5: the bitmap's last segment may be short, and it may be alone in its pair).
// Groups that do not exist get no flag, and the last one that does always ends its run.
// kCutMiddle = false (the unsegmented mode): a run may cross from the pair's first segment into its second.
template <bool kCutMiddle = true>
__device__ __forceinline__ u32 pair_pass1(const LaneGroups &g, u32 lane, u32 never, u32 nvalid) {
    // lane l <- group 0 of lane l + 1 (wave_shl:1); lane 63 has no source lane and keeps `never`, lane 31 is given it
    u32 nx = (u32)__builtin_amdgcn_update_dpp((int)never, (int)g.x[0], 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
    if (kCutMiddle) nx = lane == 31u ? never : nx;
    u32 f = 0;
#pragma unroll
    for (int k = 0; k < (int)kLaneGroups; ++k) {
        const u32 x = g.x[k];
        const u32 next = k + 1 < (int)kLaneGroups ? g.x[k + 1] : nx;
        flag_push(f, (x ^ next) | ((x + 1u) & 0x7FFFFFFEu));
    }
    if (nvalid != kPairGroups) {
        const int vl = (int)nvalid - (int)(kLaneGroups * lane); // groups of this lane that exist
        const u32 keep = vl >= 32 ? ~0u : vl <= 0 ? 0u : ~0u << (32 - vl);
        const u32 last = vl >= 1 && vl <= 32 ? 1u << (32 - vl) : 0u;
        f = (f | last) & keep;
    }
    return f;
}

// PASS 2: the lane's final words (kernels.cu:244-249) to LDS at their rank.
//   rank0   words of the pair in front of this lane's (exclusive prefix sum of the popcounts)
//   f       the lane's flag word
// The hand-scheduled blocks (WAH_PP2_BLOCK, wah_asm_blocks.hpp) do the work; what they need to start with is nl = 1 + the
// distance from this lane's group 0 back to the last run end of the lanes below, minus one: length of a fill that ends at
// group k of this lane = k + nl.  The last group of a segment always ends a run, so a lane of the pair's second segment never
// looks back beyond its segment's start.
//   variant kPass2Skip (few words: steps without a run end are branched over) / kPass2Swizzled (the words land in the
//           piece layout of store_literals; park_pair reads with the swizzled lane number)
enum : int { kPass2Skip = 1, kPass2Swizzled = 2 };
__device__ __forceinline__ void pair_pass2(const LaneGroups &g, u32 f, u32 rank0, u32 lane, u32 *lds, int variant) {
    // 1 + pair position of my last run end (0: none), its prefix maximum over the lanes, and that of the lanes BELOW me
    const u32 p1 = f ? kLaneGroups * lane + 32u - (u32)__builtin_ctz(f) : 0u;
    const u32 incl = wave_scan_max32(p1);
    u32 below = (u32)__builtin_amdgcn_update_dpp(0, (int)incl, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    // keep the move a move: folded into the subtraction below (v_subrev_u32_dpp, ROCm 7.2) the SHIFT lands on the other
    // operand -- seen on gfx950 as nl = (32 (lane - 1) + 1) - incl[lane] (tools/pair_debug.py)
    asm volatile("" : "+v"(below));
    u32 nl = kFillZero + kLaneGroups * lane + 1u - below; // (the fill marker rides along)
    u32 ad = (u32)(uintptr_t)(lds_u32_ptr)lds + 4u * rank0;
    u32 u, tb;
    u64 m0, m1, m2, m3, m4, m5, m6, m7, sv;
#define WAH_PP2_OUT                                                                                                                     \
    [f] "+&v"(f), [ad] "+&v"(ad), [nl] "+&v"(nl), [u] "=&v"(u), [tb] "=&v"(tb), [m0] "=&s"(m0), [m1] "=&s"(m1), [m2] "=&s"(m2),             \
        [m3] "=&s"(m3), [m4] "=&s"(m4), [m5] "=&s"(m5), [m6] "=&s"(m6), [m7] "=&s"(m7), [sv] "=&s"(sv)
#define WAH_PP2_IN(b)                                                                                                                   \
    [x0] "v"(g.x[b]), [x1] "v"(g.x[b + 1]), [x2] "v"(g.x[b + 2]), [x3] "v"(g.x[b + 3]), [x4] "v"(g.x[b + 4]), [x5] "v"(g.x[b + 5]),         \
        [x6] "v"(g.x[b + 6]), [x7] "v"(g.x[b + 7])
    if (variant == kPass2Skip) {
        asm volatile(WAH_PP2_BLOCK(skip, 0) : WAH_PP2_OUT : WAH_PP2_IN(0) : "vcc", "scc", "memory");
        asm volatile(WAH_PP2_BLOCK(skip, 8) : WAH_PP2_OUT : WAH_PP2_IN(8) : "vcc", "scc", "memory");
        asm volatile(WAH_PP2_BLOCK(skip, 16) : WAH_PP2_OUT : WAH_PP2_IN(16) : "vcc", "scc", "memory");
        asm volatile(WAH_PP2_BLOCK(skip, 24) : WAH_PP2_OUT : WAH_PP2_IN(24) : "vcc", "scc", "memory");
    } else {
        asm volatile(WAH_PP2_BLOCK(swz, 0) : WAH_PP2_OUT : WAH_PP2_IN(0), [c70] "s"(0x70u) : "vcc", "scc", "memory");
        asm volatile(WAH_PP2_BLOCK(swz, 8) : WAH_PP2_OUT : WAH_PP2_IN(8), [c70] "s"(0x70u) : "vcc", "scc", "memory");
        asm volatile(WAH_PP2_BLOCK(swz, 16) : WAH_PP2_OUT : WAH_PP2_IN(16), [c70] "s"(0x70u) : "vcc", "scc", "memory");
        asm volatile(WAH_PP2_BLOCK(swz, 24) : WAH_PP2_OUT : WAH_PP2_IN(24), [c70] "s"(0x70u) : "vcc", "scc", "memory");
    }
#undef WAH_PP2_OUT
#undef WAH_PP2_IN
}

// Incompressible pairs (every group a literal: the p = 0.5 bitmap) need no compaction -- rank = position -- but the plain
// transposition "lane l writes its words 32 l .. 32 l + 31, lane r reads words 4 r .. 4 r + 3 of every KiB" would put all
// 64 lanes of a store on the same LDS banks (lane stride 128 B).  The 16-byte pieces are therefore stored XOR-swizzled:
//   piece c = 8 l + q of the pair lives at piece c ^ ((c >> 3) & 7) = 8 l + (q ^ (l & 7))
// which is conflict-free for the stores (8 consecutive lanes of a ds_write_b128 hit 8 different bank quads) and for
// the 16-byte reads of park_pair (lane_sw = lane ^ ((lane >> 3) & 7): the 16 lanes of a read group differ in the low four
// bits of their piece number).
__device__ __forceinline__ bool pair_all_literals(const LaneGroups &g) {
    u32 lo = g.x[0], hi = g.x[0];
#pragma unroll
    for (int k = 1; k + 1 < (int)kLaneGroups; k += 2) {
        lo = min(lo, min(g.x[k], g.x[k + 1]));
        hi = max(hi, max(g.x[k], g.x[k + 1]));
    }
    lo = min(lo, g.x[31]);
    hi = max(hi, g.x[31]);
    return __ballot(lo == 0u || hi == kOnes31) == 0;
}
__device__ __forceinline__ void store_literals(const LaneGroups &g, u32 lane, u32 *lds) {
    u32x4 *dst = reinterpret_cast<u32x4 *>(lds) + 8u * lane;
    u32 l7 = lane & 7u;
    asm volatile("" : "+v"(l7)); // opaque: the eight addresses are made here, not hoisted to the top of the kernel
#pragma unroll
    for (u32 q = 0; q < 8; ++q) dst[q ^ l7] = u32x4{g.x[4 * q], g.x[4 * q + 1], g.x[4 * q + 2], g.x[4 * q + 3]};
}

// the pair's compacted words from LDS into registers, 16 bytes per lane and piece: words 256 t + 4 lane .. + 3 -> q[t]
// (lane: the lane's number, or its swizzled number after store_literals)
// All eight pieces, whatever the count: of pieces that are only read under a condition the compiler makes ONE 32-register
// value and a copy of it per condition (1600 spilled registers, ROCm 7.2).  What is read behind the count is never
// stored (emit_pair).
__device__ __forceinline__ void park_pair(const u32 *stage, u32 lane, u32x4 (&q)[8]) {
    const u32x4 *s4 = reinterpret_cast<const u32x4 *>(stage) + lane;
#pragma unroll
    for (int t = 0; t < 8; ++t) q[t] = s4[64 * t];
}

constexpr u32 kPairSparseBelow = 384; // words per pair below which pass 2 takes its group-skipping variant
#ifndef WAH_PAIR_SWIZZLE_FROM
#define WAH_PAIR_SWIZZLE_FROM 384
#endif
// ... and from which it stores into the swizzled piece layout.  What the plain layout costs shows where many lanes have
// the SAME number of words: at p = 1/8 (C/N = 1.032: four in ten pairs are literals but for a word or two, so 32 lanes store
// to one bank 32 times over) the 992 MiB bitmap of the report sweep took 0.613 ms against 0.39 ms at p = 1/4 and p = 1/16.
constexpr u32 kPairSwizzleFrom = WAH_PAIR_SWIZZLE_FROM;
// (The two thresholds were separate knobs while pass 2 had a third variant -- plain layout, no skipping -- for the pairs in
//  between; the A/B builds with -DWAH_PAIR_SWIZZLE_FROM=1984 / 4096 behind profiles/r03_pass2_swizzle_ab.txt used it.  The variant
//  is gone, those builds are retired, and the two have to move together.)
static_assert(kPairSparseBelow == kPairSwizzleFrom, "pass 2 has no variant for the pairs in between (plain layout, no skipping)");

// ... and from the registers to their place in the output (kernels.cu:256 + moveData, kernels.cu:273-280): dense 1 KiB
// stores through a descriptor that ends with the pair's words (and with the output's capacity: what lies behind is dropped)
__device__ __forceinline__ void emit_pair(const CompressArgs &a, u64 base, u32 count, u32 lane, const u32x4 (&q)[8]) {
    const u64 room = base < a.out_capacity ? a.out_capacity - base : 0ull;
    const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(a.out + base, (room < count ? (u32)room : count) * 4u);
    const u32 off = lane * 16u;
#pragma unroll
    for (int t = 0; t < 8; ++t)
        if (256u * t < count) __builtin_amdgcn_raw_buffer_store_b128(q[t], rsrc, off, 1024 * t, 0);
}

// ---- the wave's work on its pairs, shared by the two bodies (compress_pair_body below, compress_unseg_pair_body) ------------
//   pair_wave_begin   what a wave knows before its first pair, and that pair's loads -- issued right behind the ticket; the body
//                     decides the launch epoch (tile_begin) with them in flight
//   pair_count        PASS 1 of one pair: its words staged and regrouped, the next pair's loads issued, run ends flagged and ranked
//   pair_pass2_park   PASS 2 of one pair: final words compacted in LDS, then parked in registers (the wave's last pair: left in LDS)
//   emit_wave_pair    one pair's words, parked or still in LDS, to their place in the output
// kWavePairs: pairs a wavefront compresses one after the other (the tile = kTileWaves x kWavePairs pairs): 1, 2 or 3.
// More pairs per wave = fewer tiles = the fixed costs of a tile (ticket, first load, two barriers, the wait for the
// offset, the burst of stores) paid less often: 1 GiB sparse 0.391 / 0.303 / 0.289 ms with 1 / 2 / 3 pairs; three is what
// 128 registers hold (32 per pair of groups, then 32 per pair of parked words).
// kMode = kTileScan: tile = arrival ticket, offsets by the row scan.  kTileCount / kTilePlace (the no-wait route): tile =
// blockIdx.  (Workgroups that take TILE AFTER TILE were built on this body and measured: slower, tools/experiments.)
// There are no "does this pair exist" branches: behind the bitmap's end the loads return zeros (a descriptor of no
// bytes), no group is valid and no word comes out.
// The workgroup's LDS, its tile number and the launch epoch come from the kernel (ONE launch may run tiles of two shapes
// through two instances of a body over the same LDS: run_tile_shape).
struct PairLds { // of a workgroup
    u32 (*stage)[kPairStageWords]; // [kTileWaves]: the staged pair, later its compacted words
    u32 *count, *prefix;           // [kTileWaves]: words of a wave's pairs / of the waves below it
    u64 &base;                     // the tile's first word in the output
};
// (separate arrays, a set per kMode: a kernel is given only those it reads -- the no-wait count launch neither prefix nor base)
template <int kMode>
__device__ __forceinline__ PairLds pair_lds() {
    __shared__ __attribute__((aligned(1024))) u32 s_stage[kTileWaves][kPairStageWords]; // (the swizzle is made of address bits 7-9)
    __shared__ u32 s_count[kTileWaves];
    __shared__ u32 s_prefix[kTileWaves];
    __shared__ u64 s_base;
    return {s_stage, s_count, s_prefix, s_base};
}
// the pairs' words parked in registers (the wave's LAST pair waits for the offset where it is: in LDS, read with `last_lane`)
template <u32 kWavePairs>
using Parked = u32x4[kWavePairs > 1 ? kWavePairs - 1 : 1][8];

struct PairWave {
    u32 lane, wave, n_pairs;
    u32 pair0, never; // this wave's pairs: pair0 .. pair0 + kWavePairs - 1; "group after the last one": a value no 31-bit group can equal
    u32 *stage;       // the wave's part of PairLds::stage
};
template <bool kAligned, u32 kWavePairs, int kMode>
__device__ __forceinline__ PairWave pair_wave_begin(const CompressArgs &a, const PairLds &sm, u32 tile, u32 first_pair, PairLoad &pre) {
    PairWave w;
    w.lane = lane_id();
    w.wave = wave_id();
    w.n_pairs = (a.n_segments + 1u) >> 1;
    if (kMode == kTileCount) count_launch_reset(a, tile);
    w.stage = sm.stage[w.wave];
    w.pair0 = first_pair + w.wave * kWavePairs;
    asm volatile("v_mov_b32 %0, -1" : "=v"(w.never));
    if (tile_live<kMode>(a, tile)) prefetch_pair<kAligned>(a, w.pair0, w.lane, pre); // (a ticket outside the grid indexes nothing)
    return w;
}

// PASS 1 of pair pair0 + j, whose loads are in `pre` (more: the wave has another pair behind it, whose loads replace them).
// Nothing but counts comes out of it, which is all the other workgroups wait for.
struct PairCount {
    u32 flags, rank0, incl; // the lane's flag word (pair_pass1); words of the pair in front of this lane's, and with them
    u32 cnt, nvalid;        // words of the pair; its groups that exist: all except in the bitmap's last pair (and behind it)
};
template <bool kAligned, bool kCutMiddle>
__device__ __forceinline__ PairCount pair_count(const CompressArgs &a, const PairWave &w, u32 j, bool more, PairLoad &pre, LaneGroups &g,
                                                u64 *dg_regrouped = nullptr) {
    const u32 pair = w.pair0 + j;
    stage_pair(pre, w.stage, w.lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the wave re-reads other lanes' words
    if (more) prefetch_pair<kAligned>(a, pair + 1, w.lane, pre); // in flight while this pair is classified
    regroup_pair(w.stage, w.lane, g);
#ifdef WAH_DIAG
    if (dg_regrouped) *dg_regrouped = __builtin_amdgcn_s_memrealtime();
#endif
    PairCount c;
    c.nvalid = kPairGroups;
    if (pair + 1u >= w.n_pairs) c.nvalid = pair >= w.n_pairs ? 0u : (a.n_segments - 1u - 2u * pair) * kSegGroups + a.last_segment_groups;
    c.flags = pair_pass1<kCutMiddle>(g, w.lane, w.never, c.nvalid);
    const u32 mine = (u32)__builtin_popcount(c.flags);
    c.incl = wave_scan_incl32(mine);
    c.rank0 = c.incl - mine;
    c.cnt = (u32)__builtin_amdgcn_readlane((int)c.incl, 63);
    return c;
}

// PASS 2 of the wave's pair j: final words compacted in LDS, then parked in registers -- but for the wave's last pair, which
// nothing else needs the buffer after: it stays in LDS (read with last_lane), 32 registers less at the kernel's tightest spot.
// (One pair, the loop over j in the bodies: as one function over the arrays of all the wave's pairs the compiler made the
//  lane's constants of pair_pass2 again for every pair -- profiles/pair_body_refactor_asm.txt.)
template <u32 kWavePairs>
__device__ __forceinline__ void pair_pass2_park(const LaneGroups &g, u32 flags, u32 rank0, u32 cnt, const PairWave &w, u32 j, Parked<kWavePairs> &parked,
                                                u32 &last_lane) {
    const bool literals = cnt == kPairGroups && pair_all_literals(g);
    if (literals)
        store_literals(g, w.lane, w.stage);
    else
        pair_pass2(g, flags, rank0, w.lane, w.stage, cnt < kPairSparseBelow ? kPass2Skip : kPass2Swizzled);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const u32 read_lane = literals || cnt >= kPairSwizzleFrom ? w.lane ^ ((w.lane >> 3) & 7u) : w.lane;
    if (j + 1 < kWavePairs) {
        park_pair(w.stage, read_lane, parked[j]);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the buffer is written again next
    } else {
        last_lane = read_lane;
    }
}

// the first n_out words of the wave's pair j to out[base ..]; ci: onto the first word (the unsegmented mode's count of a
// leading fill that continues a run; the segmented body passes none and pays nothing for it)
template <u32 kWavePairs>
__device__ __forceinline__ void emit_wave_pair(const CompressArgs &a, const PairWave &w, u32 j, u64 base, u32 n_out, Parked<kWavePairs> &parked,
                                               u32 last_lane, u32 ci = 0u) {
    if (j + 1 < kWavePairs) {
        if (w.lane == 0) parked[j][0].x += ci;
        emit_pair(a, base, n_out, w.lane, parked[j]);
    } else {
        u32x4 q[8];
        park_pair(w.stage, last_lane, q);
        if (w.lane == 0) q[0].x += ci;
        emit_pair(a, base, n_out, w.lane, q);
    }
}

// ---- the segmented body adds: the words of a pair's FIRST segment (cnt_a) for the index, the 4-byte granule, (WAH_DIAG) the time line
template <bool kAligned, u32 kWavePairs, int kMode = kTileScan>
__device__ __forceinline__ void compress_pair_body(const CompressArgs &a, const PairLds &sm, u32 tile, u32 first_pair, const EpochAsk &ask, u64 dg_start = 0) {
#ifdef WAH_DIAG
    u64 dg_t[8] = {};
    dg_t[0] = dg_start ? dg_start : __builtin_amdgcn_s_memrealtime(); // (the kernel's entry: the time line includes ask and ticket)
#define DG(i) dg_t[i] = __builtin_amdgcn_s_memrealtime()
#define DG_AT(i) (dg_t + (i))
#else
#define DG(i)
#define DG_AT(i) nullptr
#endif
    PairLoad pre;
    const PairWave w = pair_wave_begin<kAligned, kWavePairs, kMode>(a, sm, tile, first_pair, pre);
    const LaunchEpoch le = kMode == kTileScan ? tile_begin(a, ask, tile) : LaunchEpoch{};
    if (le.bad) return;
    const u32 lane = w.lane, wave = w.wave;

    LaneGroups grp[kWavePairs];
    u32 flags[kWavePairs], rank0[kWavePairs];
    u32 cnt[kWavePairs], cnt_a[kWavePairs]; // words of the pair / of its first segment
    Parked<kWavePairs> parked;
    u32 last_lane = lane;
    u32 count = 0;
#pragma unroll
    for (u32 j = 0; j < kWavePairs; ++j) {
        const PairCount c = pair_count<kAligned, true>(a, w, j, j + 1 < kWavePairs, pre, grp[j], j == 0 ? DG_AT(7) : nullptr);
        flags[j] = c.flags, rank0[j] = c.rank0, cnt[j] = c.cnt;
        cnt_a[j] = (u32)__builtin_amdgcn_readlane((int)c.incl, 31);
        count += cnt[j];
    }
    if (lane == 0) sm.count[wave] = count;
    DG(2);
    __syncthreads();
    DG(1);

    // ---- wave 0: the tile's count goes out --------------------------------------------------------------------------------
    const ScanGeom g = scan_geom(tile);
    u32 *const block = a.gen_desc + (u64)g.sup * kScanBlockWords;
    u32 total = 0;
    if (wave == 0) {
        total = fold_wave_counts(sm.count, sm.prefix, lane);
        if (kMode == kTileCount) {
            if (lane == 0) a.tile_counts[tile] = total;
        } else if (kMode == kTilePlace) {
            if (lane == 0) sm.base = a.tile_counts[tile]; // (an offset by now: tile_offsets_kernel)
        } else if (lane == 0) {
            __hip_atomic_store(block + (g.row - g.row0) * kRowTiles + g.idx, (le.epoch << kGranuleCountBits) | total, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (kMode == kTileCount) return;

#pragma unroll
    for (u32 j = 0; j < kWavePairs; ++j) pair_pass2_park<kWavePairs>(grp[j], flags[j], rank0[j], cnt[j], w, j, parked, last_lane);
    DG(5);
    if (kMode == kTileScan && wave == 0) { // (the sweep goes out only here, late: scan_issue)
        TileScan poll = {};
        scan_issue(a, g, lane, true, g.has_prev, true, poll);
#ifdef WAH_DIAG
        u32 dg_polls = 0;
        const u64 base = tile_scan_resolve(a, g, block, le, tile, total, lane, poll, dg_t, &dg_polls);
        dg_t[3] = dg_t[4];
#else
        const u64 base = tile_scan_resolve(a, g, block, le, tile, total, lane, poll, nullptr, nullptr);
#endif
        if (lane == 0) sm.base = base;
    }
    __syncthreads();
#ifdef WAH_DIAG
    // per-tile time line (tools/pair_timeline.py): the stamps go to the END of the output buffer (8 x u64 per tile, the last
    // tile's first; a stream that needs the space: no stamps) -- the launch runs as it always does, emission included
    u64 *const dg_out = a.tune == 78u && (u64)a.n_tiles * 16u + 16u < a.out_capacity
                            ? reinterpret_cast<u64 *>(a.out + ((a.out_capacity - 16u * ((u64)tile + 1u)) & ~1ull)) : nullptr;
    if (wave == 0 && lane == 0 && dg_out) {
        dg_out[0] = dg_t[0]; // start
        dg_out[1] = dg_t[1]; // counts known (barrier 1 passed) = publish
        dg_out[2] = dg_t[7]; // the first pair's words are in registers
        dg_out[3] = dg_t[3]; // offset known
        dg_out[4] = dg_t[2]; // wave 0's pass 1 done
        dg_out[5] = dg_t[5]; // pass 2 + parking done
        dg_out[6] = __builtin_amdgcn_s_memrealtime(); // barrier 2 passed
    }
#endif

    // ---- the parked words to their place, the pair's two segments into the index ---------------------------------------------
    u64 base = wave_out_base(sm.base, sm.prefix, wave);
#pragma unroll
    for (u32 j = 0; j < kWavePairs; ++j) {
        const u32 pair = w.pair0 + j;
        if (lane == 0 && a.seg_offsets && pair < w.n_pairs) {
            a.seg_offsets[2u * pair] = base;
            if (2u * pair + 1u < a.n_segments) a.seg_offsets[2u * pair + 1u] = base + cnt_a[j];
        }
        emit_wave_pair<kWavePairs>(a, w, j, base, cnt[j], parked, last_lane);
        base += cnt[j];
    }
#ifdef WAH_DIAG
    if (dg_out) {
        __syncthreads();
        if (wave == 0 && lane == 0) dg_out[7] = __builtin_amdgcn_s_memrealtime(); // every wave's stores issued
    }
#endif
#undef DG
#undef DG_AT
}

// One launch, tiles of up to TWO shapes.  Tiles [0, a.big_tiles) are BODY tiles of kBody pairs per wave; the tiles behind
// them are TAIL tiles of kTail pairs per wave (kTail <= kBody; kTail == kBody: one shape).  The host (compress_tile_shape)
// fills whole rounds of the chip's workgroup slots with body tiles and gives what is left over the smallest shape that
// fits it into ONE more round: a launch used to end with a nearly empty round of full-size tiles (1 GiB: 6 tiles of 48
// segments, 128 MiB: 193) that cost a full tile's life all the same.
// body(WavePairs<n>, first pair of the tile): the body of either kernel family with n pairs per wave.
template <u32 kN>
struct WavePairs { static constexpr u32 value = kN; };
template <u32 kBody, u32 kTail, class Body>
__device__ __forceinline__ void run_tile_shape(const CompressArgs &a, u32 tile, const Body &body) {
    if (kTail == kBody || tile < a.big_tiles)
        body(WavePairs<kBody>{}, tile * (kTileWaves * kBody));
    else
        body(WavePairs<kTail>{}, a.big_tiles * (kTileWaves * kBody) + (tile - a.big_tiles) * (kTileWaves * kTail));
}

template <bool kAligned, u32 kBody, u32 kTail>
__global__ __launch_bounds__(kTileWaves * 64, 4) void compress_pair_kernel(const CompressArgs a) {
    const PairLds lds = pair_lds<kTileScan>();
    __shared__ u32 s_tile;
    u32 tile;
#ifdef WAH_DIAG
    const u64 dg_start = __builtin_amdgcn_s_memrealtime();
#else
    const u64 dg_start = 0;
#endif
    const EpochAsk ask = tile_ticket(a, &s_tile, tile);
    run_tile_shape<kBody, kTail>(a, tile, [&](auto n, u32 first_pair) __attribute__((always_inline)) {
        compress_pair_body<kAligned, decltype(n)::value>(a, lds, tile, first_pair, ask, dg_start);
    });
}

// ---- the no-wait route (kTileCount / kTilePlace): two pairs per wave, whatever the size of the bitmap; no ticket, no epoch ------
template <bool kAligned, int kMode>
__global__ __launch_bounds__(kTileWaves * 64, 4) void compress_nowait_kernel(const CompressArgs a) {
    compress_pair_body<kAligned, kNoWaitWaveSegs / 2, kMode>(a, pair_lds<kMode>(), blockIdx.x, blockIdx.x * (kTileWaves * (kNoWaitWaveSegs / 2)), EpochAsk{});
}
