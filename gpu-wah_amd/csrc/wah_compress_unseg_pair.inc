// wah_compress_unseg_pair.inc -- the unsegmented mode (WAH_UNSEGMENTED) on the PAIR-layout body of compress_pair_kernel
// (included by wah_compress.hip behind the unsegmented section, inside namespace wah::{anonymous}).
//
// The bookkeeping described at the head of that section, with the PAIR of segments a wavefront classifies at once as the unit
// (round 2 did it per segment on the tile body, compress_tile_body): inside a pair nothing is cut (pair_pass1<false>:
// a run crosses from the pair's first segment into its second by itself), the pair's last group closes its run as it
// does in the segmented mode, and where that cut falls inside a run the same two local rules apply to the pair:
//   drop_p  = the trailing fill of pair p continues into p + 1     -> the pair emits one word less (its last)
//   merge_p = the leading fill of pair p continues one from p - 1  -> its first word's count grows by the open run's length
// (never across a multiple of 2^29 groups = 2^18 pairs).  A pair that is ONE continuing run is transparent; waves, tiles,
// rows and superrows fold (T, L) exactly as before (unseg_tile_resolve).  The stream is the same bit for bit.
// kMode: kTileScan = the one launch; kTileCount / kTilePlace = the two halves of its NO-WAIT route (tile = blockIdx, nobody
// waits): count leaves {words, (T, L)} of every tile in a table, unseg_offsets_kernel turns them into {first word, length of
// the run that is open where the tile begins}, place does the tile again and writes.
template <bool kAligned, u32 kWavePairs, int kMode = kTileScan>
__device__ __forceinline__ void compress_unseg_pair_body(const CompressArgs &a, const PairShared &sm, u32 *s_t, u32 *s_l, u32 *s_carry, u32 tile,
                                                         u32 first_pair, const LaunchEpoch &le) {
    u32(*const s_stage)[kPairStageWords] = sm.stage;
    u32 *const s_count = sm.count;
    u32 *const s_prefix = sm.prefix;
    const u32 lane = lane_id();
    const u32 wave = wave_id();
    const u32 n_pairs = (a.n_segments + 1u) >> 1;
    const u32 epoch = le.epoch;
    constexpr u32 kCutPairs = kCutSegs / 2u;
    if (kMode == kTileCount && tile == 0 && threadIdx.x == 0 && !a.keep_error)
        __hip_atomic_store(a.ctrl + kCtlError, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    u32 *const stage = s_stage[wave];
    const u32 pair0 = first_pair + wave * kWavePairs;
    u32 never;
    asm volatile("v_mov_b32 %0, -1" : "=v"(never));
    PairLoad pre;
    prefetch_pair<kAligned>(a, pair0, lane, pre);
    // the group in front of the wave's first pair and the one behind its last: one word of the bitmap each.  Loads without a
    // branch around them (a descriptor of four bytes or of none), looked at only after pass 1: as `if (...) x = a.in[i]` each
    // of them was waited for on the spot -- two memory round trips in a row in front of every tile's first pass.
    const u32 pair_next = pair0 + kWavePairs;
    const bool has_prev = pair0 > 0 && pair0 < n_pairs, has_next = pair_next < n_pairs;
    const u64 i_prev = has_prev ? (u64)pair0 * kPairWords - 1u : 0ull, i_next = has_next ? (u64)pair_next * kPairWords : 0ull;
    const u32 w_prev = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(a.in + i_prev, has_prev ? 4u : 0u), 0, 0, 0);
    const u32 w_next = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(a.in + i_next, has_next && i_next < a.n_words ? 4u : 0u), 0, 0, 0);

    LaneGroups grp[kWavePairs];
    u32 flags[kWavePairs], rank0[kWavePairs], cnt[kWavePairs];
    u32 first[kWavePairs], last[kWavePairs], tail[kWavePairs];
    bool single[kWavePairs], merge[kWavePairs], drop[kWavePairs];
    u32x4 parked[kWavePairs > 1 ? kWavePairs - 1 : 1][8];
    u32 last_lane = lane;

    // ---- pass 1 of all the wave's pairs, and what each of them has at its two ends --------------------------------------
#pragma unroll
    for (u32 j = 0; j < kWavePairs; ++j) {
        const u32 pair = pair0 + j;
        stage_pair(pre, stage, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (j + 1 < kWavePairs) prefetch_pair<kAligned>(a, pair + 1, lane, pre);
        regroup_pair(stage, lane, grp[j]);
        u32 nvalid = kPairGroups;
        if (pair + 1u >= n_pairs) nvalid = pair >= n_pairs ? 0u : (a.n_segments - 1u - 2u * pair) * kSegGroups + a.last_segment_groups;
        flags[j] = pair_pass1<false>(grp[j], lane, never, nvalid);
        const u32 mine = (u32)__builtin_popcount(flags[j]);
        const u32 incl = wave_scan_incl32(mine);
        rank0[j] = incl - mine;
        cnt[j] = (u32)__builtin_amdgcn_readlane((int)incl, 63);
        first[j] = uniform32(grp[j].x[0]);
        last[j] = 1u;
        tail[j] = 0;
        single[j] = false;
        if (nvalid == kPairGroups) { // (wave-uniform)
            last[j] = (u32)__builtin_amdgcn_readlane((int)grp[j].x[kLaneGroups - 1], 63);
            single[j] = cnt[j] == 1u;
            // length of the trailing run = distance from the last run end in front of group 2047 (flag word: bit 31 - k =
            // group k of the lane ends a run; group 2047 always does)
            const u32 fm = flags[j] & ~(lane == 63u ? 1u : 0u);
            const u32 p1 = fm ? kLaneGroups * lane + 32u - (u32)__builtin_ctz(fm) : 0u; // 1 + position of my last run end
            const u32 mx = (u32)__builtin_amdgcn_readlane((int)wave_scan_max32(p1), 63);
            tail[j] = is_fill_group(last[j]) ? kPairGroups - mx : 0u;
        }
    }
    const u32 prev_last = has_prev ? uniform32(w_prev) >> 1 : 1u;           // 1: not a fill group
    const u32 next_first = has_next ? uniform32(w_next) & kOnes31 : 1u;     // (behind the bitmap's last word: zeros)
    u32 count = 0, wave_t = 1u, wave_l = 0u;
#pragma unroll
    for (u32 j = 0; j < kWavePairs; ++j) {
        const u32 pair = pair0 + j;
        merge[j] = drop[j] = false;
        if (pair < n_pairs) {
            const u32 before = j ? last[j - 1] : prev_last;
            merge[j] = pair > 0 && is_fill_group(before) && first[j] == before && (pair & (kCutPairs - 1u)) != 0u;
            const u32 after = j + 1 < kWavePairs ? first[j + 1] : next_first;
            drop[j] = pair + 1 < n_pairs && is_fill_group(last[j]) && after == last[j] && ((pair + 1u) & (kCutPairs - 1u)) != 0u;
            count += cnt[j] - (drop[j] ? 1u : 0u);
            if (single[j] && merge[j]) {
                wave_l += kPairGroups;
            } else {
                wave_t = 0u;
                wave_l = tail[j];
            }
        }
    }
    if (lane == 0) {
        s_count[wave] = count;
        s_t[wave] = wave_t;
        s_l[wave] = wave_l;
    }
    __syncthreads();

    // ---- wave 0: count and (T, L) of the tile go out in one granule ----------------------------------------------------------
    const ScanGeom g = scan_geom(tile);
    u32 *const block = a.unseg_desc + (u64)g.sup * kUnsegBlockWords;
    u64 *const my_row = reinterpret_cast<u64 *>(block) + (u64)(g.row - g.row0) * kRowTiles;
    u32 total = 0, tile_t = 1u, tile_l = 0u;
    if (wave == 0) {
        const u32 mine = lane < kTileWaves ? s_count[lane] : 0u;
        const u32 incl = wave_scan_incl32(mine);
        if (lane < kTileWaves) s_prefix[lane] = incl - mine;
        total = (u32)__builtin_amdgcn_readlane((int)incl, 63);
        unseg_fold_tile(s_t, s_l, lane, tile_t, tile_l);
        if (kMode == kTileCount) {
            if (lane == 0) {
                a.tile_counts[2ull * tile] = total;
                a.tile_counts[2ull * tile + 1] = (tile_t ? kSlotT : 0ull) | tile_l;
            }
        } else if (kMode == kTileScan && lane == 0) {
            __hip_atomic_store(my_row + g.idx, ((u64)epoch << 48) | ((u64)total << 32) | (tile_t ? kUnsegT : 0ull) | tile_l, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (kMode == kTileCount) return;

    // ---- pass 2 of all the wave's pairs: final words compacted in LDS, then parked in registers -----------------------------
#pragma unroll
    for (u32 j = 0; j < kWavePairs; ++j) {
        const bool literals = cnt[j] == kPairGroups && pair_all_literals(grp[j]);
        if (literals)
            store_literals(grp[j], lane, stage);
        else
            pair_pass2(grp[j], flags[j], rank0[j], lane, stage,
                       cnt[j] < kPairSparseBelow ? kPass2Skip : kPass2Swizzled);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const u32 read_lane = literals || cnt[j] >= kPairSwizzleFrom ? lane ^ ((lane >> 3) & 7u) : lane;
        if (j + 1 < kWavePairs) {
            park_pair(stage, read_lane, parked[j]);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        } else {
            last_lane = read_lane;
        }
    }

    if (kMode == kTilePlace && wave == 0) { // both out of the table (unseg_offsets_kernel)
        (void)unseg_wave_carries(s_t, s_l, s_carry, a.tile_counts[2ull * tile + 1], lane);
        if (lane == 0) *sm.base = a.tile_counts[2ull * tile];
    }
    if (kMode == kTileScan && wave == 0) unseg_tile_resolve(a, g, block, my_row, le, tile, total, tile_t, tile_l, lane, s_t, s_l, s_carry, sm.base);
    __syncthreads();

    // ---- the parked words to their place: a continuing leading fill gets the open run's length, a continuing trailing
    //      fill is left to the pair in which the run ends ----------------------------------------------------------------------
    u64 base = uniform64(*sm.base) + uniform32(s_prefix[wave]);
    u32 c = uniform32(s_carry[wave]);
#pragma unroll
    for (u32 j = 0; j < kWavePairs; ++j) {
        if (pair0 + j < n_pairs) { // (wave-uniform)
            const u32 ci = merge[j] ? c : 0u;
            const u32 n_out = cnt[j] - (drop[j] ? 1u : 0u);
            if (j + 1 < kWavePairs) {
                if (lane == 0) parked[j][0].x += ci; // (count of the leading fill; ci = 0 otherwise)
                emit_pair(a, base, n_out, lane, parked[j]);
            } else {
                u32x4 q[8];
                park_pair(stage, last_lane, q);
                if (lane == 0) q[0].x += ci;
                emit_pair(a, base, n_out, lane, q);
            }
            base += n_out;
            c = single[j] && merge[j] ? ci + kPairGroups : tail[j];
        }
    }
}

template <bool kAligned, u32 kBody, u32 kTail>
__global__ __launch_bounds__(kTileWaves * 64, 4) void compress_unseg_pair_kernel(const CompressArgs a) {
    __shared__ __attribute__((aligned(1024))) u32 s_stage[kTileWaves][kPairStageWords]; // (the swizzle is made of address bits 7-9)
    __shared__ u32 s_count[kTileWaves];
    __shared__ u32 s_prefix[kTileWaves];
    __shared__ u32 s_t[kTileWaves], s_l[kTileWaves], s_carry[kTileWaves];
    __shared__ u64 s_base;
    __shared__ u32 s_tile;
    const u32 tile = draw_tile(a.ctrl, &s_tile);
    const LaunchEpoch le = launch_epoch_begin(a.ctrl, tile, a.n_tiles, a.gen_desc, a.scan_words, a.keep_error);
    if (le.bad) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *a.out_words = 0;
        return;
    }
    const PairShared sm = {s_stage, s_count, s_prefix, &s_base};
    if (kTail == kBody || tile < a.big_tiles)
        compress_unseg_pair_body<kAligned, kBody>(a, sm, s_t, s_l, s_carry, tile, tile * (kTileWaves * kBody), le);
    else
        compress_unseg_pair_body<kAligned, kTail>(a, sm, s_t, s_l, s_carry, tile,
                                                  a.big_tiles * (kTileWaves * kBody) + (tile - a.big_tiles) * (kTileWaves * kTail), le);
}

// ---- the no-wait route of the unsegmented mode: two pairs per wave, whatever the size of the bitmap ------------------------
template <bool kAligned, int kMode>
__global__ __launch_bounds__(kTileWaves * 64, 4) void compress_unseg_pair_nowait_kernel(const CompressArgs a) {
    __shared__ __attribute__((aligned(1024))) u32 s_stage[kTileWaves][kPairStageWords];
    __shared__ u32 s_count[kTileWaves];
    __shared__ u32 s_prefix[kTileWaves];
    __shared__ u32 s_t[kTileWaves], s_l[kTileWaves], s_carry[kTileWaves];
    __shared__ u64 s_base;
    const PairShared sm = {s_stage, s_count, s_prefix, &s_base};
    const LaunchEpoch le = {};
    compress_unseg_pair_body<kAligned, kNoWaitWaveSegs / 2, kMode>(a, sm, s_t, s_l, s_carry, blockIdx.x, blockIdx.x * (kTileWaves * (kNoWaitWaveSegs / 2)), le);
}
