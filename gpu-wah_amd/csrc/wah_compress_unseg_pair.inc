// wah_compress_unseg_pair.inc -- the unsegmented mode (WAH_UNSEGMENTED) on the shared passes of wah_compress_pair.inc
// (included by wah_compress.hip behind the unsegmented section, inside namespace wah::{anonymous}).
//
// What it adds to them: the two bitmap words next to the wave's pairs, what each pair has at its two ends, merge / drop and
// the wave's (T, L) out of those, the 8-byte granule {words, (T, L)} with unseg_tile_resolve, and the carry onto a merged
// pair's first word.  That is the bookkeeping described at the head of the unsegmented section, with the PAIR of segments a
// wavefront classifies at once as the unit: inside a pair nothing is cut (pair_pass1<false>:
// a run crosses from the pair's first segment into its second by itself), the pair's last group closes its run as it
// does in the segmented mode, and where that cut falls inside a run the same two local rules apply to the pair:
//   drop_p  = the trailing fill of pair p continues into p + 1     -> the pair emits one word less (its last)
//   merge_p = the leading fill of pair p continues one from p - 1  -> its first word's count grows by the open run's length
// (never across a multiple of 2^29 groups = 2^18 pairs).  A pair that is ONE continuing run is transparent; waves, tiles,
// rows and superrows fold (T, L) (unseg_fold_tile, unseg_tile_resolve).  The stream is the same bit for bit.
// kMode: kTileScan = the one launch; kTileCount / kTilePlace = the two halves of its NO-WAIT route (tile = blockIdx, nobody
// waits): count leaves {words, (T, L)} of every tile in a table, unseg_offsets_kernel turns them into {first word, length of
// the run that is open where the tile begins}, place does the tile again and writes.
struct UnsegLds { // of a workgroup, beside PairLds: per wave (T, L) and the length of the run that is open where the wave begins
    u32 *t, *l, *carry;
};
template <int kMode>
__device__ __forceinline__ UnsegLds unseg_lds() {
    __shared__ u32 s_t[kTileWaves], s_l[kTileWaves], s_carry[kTileWaves];
    return {s_t, s_l, s_carry};
}

template <bool kAligned, u32 kWavePairs, int kMode = kTileScan>
__device__ __forceinline__ void compress_unseg_pair_body(const CompressArgs &a, const PairLds &sm, const UnsegLds &us, u32 tile, u32 first_pair,
                                                         const EpochAsk &ask) {
    constexpr u32 kCutPairs = kCutSegs / 2u;
    PairLoad pre;
    const PairWave w = pair_wave_begin<kAligned, kWavePairs, kMode>(a, sm, tile, first_pair, pre);
    const u32 lane = w.lane, wave = w.wave, n_pairs = w.n_pairs, pair0 = w.pair0;
    const bool live = tile_live<kMode>(a, tile); // (the loads below go out with the first pair's, in front of tile_begin)
    // the group in front of the wave's first pair and the one behind its last: one word of the bitmap each.  Loads without a
    // branch around them (a descriptor of four bytes or of none), looked at only after pass 1: as `if (...) x = a.in[i]` each
    // of them was waited for on the spot -- two memory round trips in a row in front of every tile's first pass.
    const u32 pair_next = pair0 + kWavePairs;
    const bool has_prev = live && pair0 > 0 && pair0 < n_pairs, has_next = live && pair_next < n_pairs;
    const u64 i_prev = has_prev ? (u64)pair0 * kPairWords - 1u : 0ull, i_next = has_next ? (u64)pair_next * kPairWords : 0ull;
    const u32 w_prev = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(a.in + i_prev, has_prev ? 4u : 0u), 0, 0, 0);
    const u32 w_next = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(a.in + i_next, has_next && i_next < a.n_words ? 4u : 0u), 0, 0, 0);
    const LaunchEpoch le = kMode == kTileScan ? tile_begin(a, ask, tile) : LaunchEpoch{};
    if (le.bad) return;

    LaneGroups grp[kWavePairs];
    u32 flags[kWavePairs], rank0[kWavePairs], cnt[kWavePairs];
    u32 first[kWavePairs], last[kWavePairs], tail[kWavePairs];
    bool single[kWavePairs], merge[kWavePairs], drop[kWavePairs];
    Parked<kWavePairs> parked;
    u32 last_lane = lane;

    // ---- pass 1 of all the wave's pairs, and what each of them has at its two ends --------------------------------------
#pragma unroll
    for (u32 j = 0; j < kWavePairs; ++j) {
        const PairCount c = pair_count<kAligned, false>(a, w, j, j + 1 < kWavePairs, pre, grp[j]);
        flags[j] = c.flags, rank0[j] = c.rank0, cnt[j] = c.cnt;
        first[j] = uniform32(grp[j].x[0]);
        last[j] = 1u;
        tail[j] = 0;
        single[j] = false;
        if (c.nvalid == kPairGroups) { // (wave-uniform)
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
        sm.count[wave] = count;
        us.t[wave] = wave_t;
        us.l[wave] = wave_l;
    }
    __syncthreads();

    // ---- wave 0: count and (T, L) of the tile go out in one granule ----------------------------------------------------------
    const ScanGeom g = scan_geom(tile);
    u32 *const block = a.unseg_desc + (u64)g.sup * kUnsegBlockWords;
    u64 *const my_row = reinterpret_cast<u64 *>(block) + (u64)(g.row - g.row0) * kRowTiles;
    u32 total = 0, tile_t = 1u, tile_l = 0u;
    if (wave == 0) {
        total = fold_wave_counts(sm.count, sm.prefix, lane);
        unseg_fold_tile(us.t, us.l, lane, tile_t, tile_l);
        if (kMode == kTileCount) {
            if (lane == 0) {
                a.tile_counts[2ull * tile] = total;
                a.tile_counts[2ull * tile + 1] = (tile_t ? kSlotT : 0ull) | tile_l;
            }
        } else if (kMode == kTileScan && lane == 0) {
            __hip_atomic_store(my_row + g.idx, ((u64)le.epoch << 48) | ((u64)total << 32) | (tile_t ? kUnsegT : 0ull) | tile_l, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (kMode == kTileCount) return;

#pragma unroll
    for (u32 j = 0; j < kWavePairs; ++j) pair_pass2_park<kWavePairs>(grp[j], flags[j], rank0[j], cnt[j], w, j, parked, last_lane);

    if (kMode == kTilePlace && wave == 0) { // both out of the table (unseg_offsets_kernel)
        (void)unseg_wave_carries(us.t, us.l, us.carry, a.tile_counts[2ull * tile + 1], lane);
        if (lane == 0) sm.base = a.tile_counts[2ull * tile];
    }
    if (kMode == kTileScan && wave == 0) // (issues its sweep only here, late: scan_issue)
        unseg_tile_resolve(a, g, block, my_row, le, tile, total, tile_t, tile_l, lane, us.t, us.l, us.carry, &sm.base);
    __syncthreads();

    // ---- the parked words to their place: a continuing leading fill gets the open run's length, a continuing trailing
    //      fill is left to the pair in which the run ends ----------------------------------------------------------------------
    u64 base = wave_out_base(sm.base, sm.prefix, wave);
    u32 c = uniform32(us.carry[wave]);
#pragma unroll
    for (u32 j = 0; j < kWavePairs; ++j) {
        if (pair0 + j < n_pairs) { // (wave-uniform)
            const u32 ci = merge[j] ? c : 0u;
            const u32 n_out = cnt[j] - (drop[j] ? 1u : 0u);
            emit_wave_pair<kWavePairs>(a, w, j, base, n_out, parked, last_lane, ci); // (ci: onto the count of the leading fill)
            base += n_out;
            c = single[j] && merge[j] ? ci + kPairGroups : tail[j];
        }
    }
}

template <bool kAligned, u32 kBody, u32 kTail>
__global__ __launch_bounds__(kTileWaves * 64, 4) void compress_unseg_pair_kernel(const CompressArgs a) { // tile shapes: run_tile_shape
    const PairLds lds = pair_lds<kTileScan>();
    const UnsegLds us = unseg_lds<kTileScan>();
    __shared__ u32 s_tile;
    u32 tile;
    const EpochAsk ask = tile_ticket(a, &s_tile, tile);
    run_tile_shape<kBody, kTail>(a, tile, [&](auto n, u32 first_pair) __attribute__((always_inline)) {
        compress_unseg_pair_body<kAligned, decltype(n)::value>(a, lds, us, tile, first_pair, ask);
    });
}

// ---- the no-wait route of the unsegmented mode: two pairs per wave, whatever the size of the bitmap ------------------------
template <bool kAligned, int kMode>
__global__ __launch_bounds__(kTileWaves * 64, 4) void compress_unseg_pair_nowait_kernel(const CompressArgs a) {
    compress_unseg_pair_body<kAligned, kNoWaitWaveSegs / 2, kMode>(a, pair_lds<kMode>(), unseg_lds<kMode>(), blockIdx.x, blockIdx.x * (kTileWaves * (kNoWaitWaveSegs / 2)), EpochAsk{});
}
