// wah_decode_tile.inc -- decode_tile_kernel: the general decoder in ONE pass over the stream (included by wah_decode.hip,
// inside namespace wah::{anonymous}).
//
// decode_sums_kernel + decode_expand_kernel read the compressed stream twice (tile bases first, expansion second): HBM
// traffic 1.35 x (sparse GiB) to 1.51 x (dense GiB) the algorithmic 4C + 4N'.  Here a workgroup loads a BATCH of kP tiles of
// the stream ONCE and keeps it on the chip -- the batch's last tile in LDS, the others in registers (16 per lane and
// tile) -- until the groups in front of the batch are known:
//   every wave : its 1024 words of every tile of the batch (four coalesced 16-byte loads per lane and tile); their group
//                counts (getCounts, kernels.cu:291-309), summed per tile
//   barrier    : the batch's total goes out as ONE 8-byte granule (wave 0); nothing else of this batch is waited for
//   every wave : while the other batches' totals are on their way: one START FLAG per word of the tile in LDS -- a bit mask
//                over the tile's groups, bit p set iff a word starts at group p of the tile (LDS atomics: ds_or_b32)
//   wave 0     : resolves the groups in front of the batch with the sums kernel's row scan (sums_resolve, swept late; wah_rowscan.hpp)
//   every wave : the output segments that START inside the tile, one wavefront per segment (decompressWords + mergeWords,
//                kernels.cu:321-385): per step of 64 groups the step's 64 start flags are two scalar registers, a group's
//                source word is word number (starts at positions <= mine) - 1 of the tile (v_mbcnt + a running scalar
//                count), one LDS gather, fill / literal decode, 31 -> 32 repack with one DPP shift, dense 248-byte
//                stores.  No per-segment marking, no byte flags, no search: the flags of the WHOLE tile are made once,
//                by all lanes at once.
//   then       : the batch's other tiles, last to first, take the LDS image in turn: registers -> LDS, flags, expansion.
//                (Why a batch: ticket, first load, the count barrier and above all the WAIT for the groups in front -- about
//                6 us from publication to base whatever the kernel -- are paid once per workgroup; with one tile per
//                workgroup they were 11 of a tile's 20 us, tools/experiments/README.md.)
// A tile's last segment may need words from behind the tile (at most 1024: every word holds a group).  For the batch's
// last tile they are loaded with the tile (the only bytes read twice); for the others they are the first words of the tile
// expanded just before, copied aside inside LDS.
// PLAIN tiles -- every word of the tile and of the 1152 words behind it a literal: incompressible data -- need none of the
// flags: group p of the tile is word p (a wave-uniform short cut per tile, decided by what the count pass sees anyway).
// What this kernel does not do itself is DEFERRED to decode_expand_kernel, which a second launch runs over the list of
// such tiles (normally empty): tiles that expand to more than kDtMaxGroups groups (giant fills of foreign streams) and
// tiles with fill words of count 0 (foreign streams; their words would have no start flag).  It leaves behind what the
// two-pass route leaves: tile_base[] and tile_flags[] of the 4096-word expand tiles, info[], and the error word.
// The output is written as the tiles come by: stores are cut at the output's capacity (an output that turns out too
// small is reported by the LAST batch, WAH_ERR_CAPACITY, with the part that fits written).
#ifndef WAH_DT_MINW
#define WAH_DT_MINW 6 // waves per SIMD the kernel is compiled for (80 registers)
#endif
#ifndef WAH_DT_LOAD_AUX
#define WAH_DT_LOAD_AUX 2 // cache policy of the stream's loads: 2 = nontemporal
#endif
#ifndef WAH_DT_GROUP
#define WAH_DT_GROUP 4 // steps whose gathers are in flight together
#endif
constexpr u32 kDtWaves = 8;
constexpr u32 kDtTileWords = 2u * (u32)kScanTileWords;        // 8192 compressed words = two expand tiles
constexpr u32 kDtWaveWords = kDtTileWords / kDtWaves;          // 1024
constexpr u32 kDtLaneWords = kDtWaveWords / 64u;               // 16 consecutive words per lane
constexpr u32 kDtBehind = kSegGroups + 128u;                   // words behind the tile that its last segment may need
#ifndef WAH_DT_MAXG
#define WAH_DT_MAXG 60 // (x 1024 groups)
#endif
constexpr u32 kDtMaxGroups = WAH_DT_MAXG * 1024u;              // groups a tile may expand to and still be decoded here
constexpr u32 kDtMaskBits = kDtMaxGroups + kSegGroups + 64u;   // (the last segment's groups behind the tile's own)
constexpr u32 kDtMaskWords = ((kDtMaskBits + 31u) / 32u + 3u) & ~3u;
constexpr u32 kDtCoarse = (kDtMaskWords + 31u) / 32u;          // starts in front of every 32nd mask word
static_assert(kDtCoarse <= 64 && kDtMaskWords % 4 == 0, "one lane per coarse entry; the mask is cleared 16 bytes at a time");

struct TileDecodeArgs {
    const u32 *comp;
    u64 c_words;
    u32 n_wg_tiles;      // workgroup BATCHES of kP x kDtTileWords words
    u32 *out;
    u64 out_capacity;
    u64 *info;           // [0] decoded words, [1] groups
    u64 *tile_base;      // per 4096-word expand tile (+ 1): groups in front of it (for the deferred tiles, build_index, ...)
    uint8_t *tile_flags; // per expand tile: 1 = contains a fill word of count 0
    u64 *defer_list;     // expand tiles left to decode_expand_kernel's tile routine: {tile:32, part:16, parts:16} (dt_defer)
    u32 *defer_count;    // control block, kCtlDefer (wah_internal.hpp): the counter pairs of defer_list, the launches so far
    u32 defer_capacity;  // entries the list has room for
    u32 *tile_buckets;   // per expand tile 64 sums of group counts per 64 words, written for the tiles that go onto the list
    u32 *ctrl;
    u32 *gen_desc;
    u64 scan_words;
    u64 *host_result;    // optional, page-locked HOST memory (as ScanArgs::host_result)
};

__device__ __forceinline__ u32 dt_word_groups_clamped(u32 w) { // a count above the cap defers the tile whatever the rest is
    const u32 n = word_groups(w);
    return n > kDtMaxGroups ? kDtMaxGroups + 1u : n;
}

// Group counts of the wave's 1024 words of one tile (getCounts, kernels.cu:291-309), in the layout of the loads (a total does
// not care about the order): `b0` = batch-local index of the wave's first word, `left` = words of the stream from the
// batch's start on.  Words behind the stream's end are made fill words of count 0 in `h` (they hold no group; a zero word
// would be a literal).  wave_pos = the total with every count clamped at the cap + 1 (a count above the cap defers the
// tile), wave_total = the exact one.
// wave_fills: one of the words is a fill word (bit 31; behind the stream's end they all are).
__device__ __forceinline__ void dt_count_wave(u32x4 (&h)[4], u32 b0, u32 left, u32 lane, u64 &wave_total, u32 &wave_pos, bool &wave_empty, bool &wave_fills) {
    u64 lane_total = 0;
    u32 lane_pos = 0;
    bool empty = false;
    // Common case (wave-uniform): the wave's 1024 words lie inside the stream and none of their counts is above the cap --
    // then sum, largest and smallest count are all that is needed (six instructions per word)
    u32 sum = 0, largest = 0, smallest = 0xFFFFFFFFu;
    u64 fill_lanes = 0; // (scalar: the compare is the one word_groups() selects by -- no vector instruction, no vector register)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u32 wd[4] = {h[k].x, h[k].y, h[k].z, h[k].w};
#pragma unroll
        for (u32 c = 0; c < 4; ++c) {
            fill_lanes |= __ballot((int)wd[c] < 0);
            const u32 n = word_groups(wd[c]);
            sum += n; // (wraps only when a count is above the cap)
            largest = max(largest, n);
            smallest = min(smallest, n);
        }
    }
    if (b0 + kDtWaveWords <= left && !__any(largest > kDtMaxGroups)) {
        lane_total = sum;
        lane_pos = sum;
        empty = smallest == 0u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32 i0 = b0 + 256u * k + 4u * lane; // batch-local index of the piece's first word
            if (i0 + 3u >= left) {
                if (i0 >= left) h[k].x = kFillZero;
                if (i0 + 1u >= left) h[k].y = kFillZero;
                if (i0 + 2u >= left) h[k].z = kFillZero;
                if (i0 + 3u >= left) h[k].w = kFillZero;
            }
            const u32 wd[4] = {h[k].x, h[k].y, h[k].z, h[k].w};
#pragma unroll
            for (u32 c = 0; c < 4; ++c) {
                const u32 n = word_groups(wd[c]);
                lane_pos += n > kDtMaxGroups ? kDtMaxGroups + 1u : n; // (64 lanes x 16 words x (cap + 1) < 2^32)
                lane_total += n;
                empty |= n == 0u && i0 + c < left; // a fill word of count 0 INSIDE the stream
            }
        }
    }
    // (DPP only; the 64-bit total differs from the clamped one only when a count was clamped -- then the tile is deferred)
    wave_pos = wave_total32(lane_pos);
    wave_total = wave_pos <= kDtMaxGroups ? (u64)wave_pos : uniform64(wave_sum(lane_total));
    wave_empty = __any(empty);
    wave_fills = b0 + kDtWaveWords > left || fill_lanes != 0ull;
}

template <u32 kP>
__global__ __launch_bounds__(kDtWaves * 64, (kP <= 2 ? WAH_DT_MINW : 4)) void decode_tile_kernel(const TileDecodeArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_words[kDtTileWords + kDtBehind];
    __shared__ __attribute__((aligned(16))) u32 s_mask[kDtMaskWords];
    __shared__ u32 s_coarse[64];
    __shared__ u64 s_wave_total[kP][kDtWaves];
    __shared__ u32 s_wave_pos[kP][kDtWaves];
    __shared__ u32 s_wave_empty[kP][kDtWaves];
    __shared__ u64 s_base;
    __shared__ u32 s_tile;
    __shared__ u32 s_behind[2]; // groups of the words parked behind the tile; position of the first fill word of count 0 among them
    __shared__ u32 s_behind_fills[kDtWaves]; // per wave: one of the words it loaded from behind the BATCH is not a literal (or lies behind the stream)
    // wave 0's held words while it runs the row scan (whose code needs about 70 registers of its own: with the held tiles
    // beside them the kernel would not fit the 80 registers that six waves per SIMD leave)
    __shared__ __attribute__((aligned(16))) u32 s_park[kP > 1 ? (kP - 1) * kDtWaveWords : 4];

    // ISSUE PRIORITY (DESIGN 6.8).  A SIMD holds six waves of three workgroups of different ages, and at equal priority the oldest
    // wave wins every issue slot.  The youngest workgroup is the one still loading, counting and publishing -- what every later batch
    // of the launch waits for -- and it would lose to the older workgroups' expansion steps, which nothing waits for.  So every wave
    // runs at priority 1 from here to the publication of the batch's total, and wave 0 again for its row scan until the batch's base
    // is in LDS; everything else, and every wait (the epoch wrap's, row_scan_wait's), runs at 0.
    __builtin_amdgcn_s_setprio(1);
    const u32 lane = lane_id();
    const u32 wave = wave_id();
#ifdef WAH_DIAG
    u64 dg[16] = {};
    dg[0] = __builtin_amdgcn_s_memrealtime();
#define DGT(i) dg[i] = __builtin_amdgcn_s_memrealtime()
#else
#define DGT(i)
#endif
    // ask, ticket, decide (wah_device.hpp): what the control block says -- the launch epoch's words, and which of the two counters
    // of deferred tiles this launch uses (read by every workgroup at its start, advanced by the last batch at its end: the
    // protocol of the launch epoch) -- is asked for in front of the ticket and is in flight with it; the batch's loads go out right
    // behind the ticket, which is all they depend on, and the epoch is decided with them in flight
    EpochAsk ask = launch_epoch_ask(a.ctrl);
    u32 defer_seq = defer_seq_ask(a.defer_count);
    const u32 wt = draw_tile(a.ctrl, &s_tile, ask);
    defer_seq = uniform32(defer_seq); // (taken with the epoch's words, in front of the loads: draw_tile)
    asm volatile("" : "+s"(defer_seq)); // (here, not where it is first used: behind the branches of the loads below the wait would be for some of them too)
    constexpr u32 kBatchWords = kP * kDtTileWords;
    const u64 batch_w0 = (u64)wt * kBatchWords;
    const u64 left64 = a.c_words - batch_w0;                                  // words of the stream from the batch's start on
    // (a ticket outside the grid -- a workspace that is not ours, le.bad below -- has no words left: every descriptor of the loads
    //  is one of no bytes then, and nothing is read with a number that was not checked)
    const u32 left = wt < a.n_wg_tiles ? (left64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)left64) : 0u;
    u32x4 *const words4 = reinterpret_cast<u32x4 *>(s_words);

    // ---- the wave's words of all the batch's tiles are loaded ---------------------------------------------------------------------
    const u32 w0 = wave * kDtWaveWords; // tile-local index of the wave's first word
    u32x4 hold[kP][4];                  // (the last tile's go to LDS at once)
#pragma unroll
    for (u32 j = 0; j < kP; ++j) {
        const u32 b0 = j * kDtTileWords + w0; // batch-local
        const u32 bytes = left > b0 ? (left - b0 >= kDtWaveWords ? kDtWaveWords * 4u : (left - b0) * 4u) : 0u;
        const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(a.comp + batch_w0 + b0, bytes);
#pragma unroll
        for (int k = 0; k < 4; ++k) hold[j][k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16u, 1024 * k, WAH_DT_LOAD_AUX); // nontemporal: read once
    }
    u32 behind_w[3] = {0, 0, 0};
    {
        // ... and the wave's share of the words BEHIND the batch (18 batches of 64: what the last tile's last segment may need)
        const __amdgpu_buffer_rsrc_t rb = make_rsrc(a.comp + batch_w0 + kBatchWords, left > kBatchWords ? (left - kBatchWords >= kDtBehind ? kDtBehind * 4u : (left - kBatchWords) * 4u) : 0u);
#pragma unroll
        for (u32 b = 0; b < 3; ++b)
            if (wave + 8u * b < kDtBehind / 64u) behind_w[b] = __builtin_amdgcn_raw_buffer_load_b32(rb, (64u * (wave + 8u * b) + lane) * 4u, 0, 0);
    }

    // ---- decide: the launch epoch, from what was asked for in front of the ticket ------------------------------------------------
    const bool wrap_wait = ask.stored >= kEpochWrap; // (scalar: draw_tile) the one launch in 65 535 whose tiles wait for tile 0 in there
    if (wrap_wait) __builtin_amdgcn_s_setprio(0);
    const LaunchEpoch le = launch_epoch_begin(a.ctrl, ask, wt, a.n_wg_tiles, a.gen_desc, a.scan_words, 0);
    if (wrap_wait) __builtin_amdgcn_s_setprio(1);
    if (le.bad) {
        if (blockIdx.x == 0 && threadIdx.x == 0) a.info[0] = a.info[1] = 0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the batch's loads (bounded descriptors over the stream) are not left behind
        return;
    }
    const u32 epoch = le.epoch;
    u64 *const defer_count = defer_counters_mine(a.defer_count, defer_seq);

    // ---- the start flags are cleared; the words behind the batch go to their place ------------------------------------------------
    for (u32 i = threadIdx.x; i < kDtMaskWords / 4u; i += kDtWaves * 64u) reinterpret_cast<uint4 *>(s_mask)[i] = make_uint4(0, 0, 0, 0);
    {
        u32 any_fill = 0;
#pragma unroll
        for (u32 b = 0; b < 3; ++b) {
            const u32 i = 64u * (wave + 8u * b) + lane; // index among the words behind the batch
            if (wave + 8u * b < kDtBehind / 64u) {
                const u32 w = behind_w[b];
                const u32 v = kBatchWords + i < left ? w : kFillZero;
                s_words[kDtTileWords + i] = v;
                any_fill |= v;
            }
        }
        const bool some = __any((int)any_fill < 0);
        if (lane == 0) s_behind_fills[wave] = some ? 1u : 0u;
    }

    // ---- group counts per tile (in the layout of the loads: a tile's total does not care about the order) ---------------------
#pragma unroll
    for (u32 j = 0; j < kP; ++j) {
        u64 wave_total;
        u32 wave_pos;
        bool wave_empty, wave_fills;
        dt_count_wave(hold[j], j * kDtTileWords + w0, left, lane, wave_total, wave_pos, wave_empty, wave_fills);
        if (lane == 0) {
            s_wave_total[j][wave] = wave_total;
            s_wave_pos[j][wave] = wave_pos;
            s_wave_empty[j][wave] = (wave_empty ? 1u : 0u) | (wave_fills ? 2u : 0u); // (bit 1: only for `plain` below)
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) words4[w0 / 4u + 64 * k + lane] = hold[kP - 1][k];
    DGT(1);
    __syncthreads();
    DGT(2);

    // ---- the tiles' totals (every wave works them out for itself); wave 0 publishes the batch's ---------------------------------
    u64 total[kP], first_half[kP]; // first_half: groups of a tile's first expand tile (4096 words = the first four waves)
    u32 empties_a[kP], empties_b[kP], fills[kP];
    bool deferred[kP];
    u64 batch_total = 0;
#pragma unroll
    for (u32 j = 0; j < kP; ++j) {
        u32 pos_total = 0;
        total[j] = first_half[j] = 0;
        empties_a[j] = empties_b[j] = fills[j] = 0;
#pragma unroll
        for (u32 w = 0; w < kDtWaves; ++w) {
            const u64 t = s_wave_total[j][w];
            const u32 p = s_wave_pos[j][w];
            const u32 ef = s_wave_empty[j][w];
            fills[j] |= ef >> 1;
            if (w < kDtWaves / 2) {
                first_half[j] += t;
                empties_a[j] |= ef & 1u;
            } else {
                empties_b[j] |= ef & 1u;
            }
            total[j] += t;
            pos_total = pos_total + p < pos_total ? 0xFFFFFFFFu : pos_total + p;
        }
        // (values out of LDS: the same in every lane, but only readfirstlane tells the compiler -- scalar registers from here on)
        total[j] = uniform64(total[j] > kSumSaturate ? kSumSaturate : total[j]);
        first_half[j] = uniform64(first_half[j]);
        empties_a[j] = uniform32(empties_a[j]);
        empties_b[j] = uniform32(empties_b[j]);
        fills[j] = uniform32(fills[j]);
        deferred[j] = uniform32((empties_a[j] | empties_b[j]) != 0u || pos_total > kDtMaxGroups ? 1u : 0u) != 0u; // (not deferred: no count was clamped)
        batch_total = sat_add(batch_total, total[j]);
    }
#ifndef WAH_DT_EARLY
#define WAH_DT_EARLY 1
#endif
    // PLAIN tiles: every word of the tile and of the 1152 words behind it is a literal (incompressible data: the p = 0.5 bitmap
    // is nothing else) -- group p of the tile is word p: no start flags, no ranks, no fill decode.  Wave-uniform, and known from
    // the count pass (the words' sign bits OR-ed together: a fill of count 1 holds one group like a literal); the words behind it
    // are the tile behind it (plain itself), or, for the batch's last tile, were looked at as they were loaded.
    bool plain[kP];
    {
        u32 behind_fills = 0;
#pragma unroll
        for (u32 w = 0; w < kDtWaves; ++w) behind_fills |= s_behind_fills[w];
        bool behind_plain = uniform32(behind_fills) == 0u;
#pragma unroll
        for (u32 jj = 0; jj < kP; ++jj) {
            const u32 j = kP - 1u - jj;
            plain[j] = !deferred[j] && fills[j] == 0u && behind_plain;
            behind_plain = plain[j];
        }
    }
    if (WAH_DT_EARLY && wave == 0 && lane == 0) sums_publish(a.gen_desc, wt, epoch, batch_total);
    __builtin_amdgcn_s_setprio(0); // published: from the flags on the workgroup is one of those that nothing waits for

    u64 base = 0; // groups in front of the batch (known after the first tile's flags are made)

    // ---- the batch's tiles, last to first --------------------------------------------------------------------------------------
#pragma unroll
    for (u32 jj = 0; jj < kP; ++jj) {
        const u32 j = kP - 1u - jj;
        if (jj > 0) {
            __syncthreads(); // the image is free: the tile behind this one has been expanded
            // its first words are what THIS tile's last segment may need: aside with them, then this tile's words in
            if (wave == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) words4[kDtTileWords / 4u + 64 * k + lane] = words4[64 * k + lane];
            } else if (wave == 1 && lane < (kDtBehind - kDtWaveWords) / 4u) {
                words4[kDtTileWords / 4u + 256u + lane] = words4[256u + lane];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) words4[w0 / 4u + 64 * k + lane] = hold[j][k];
            if (!plain[j] && !deferred[j])
                for (u32 i = threadIdx.x; i < kDtMaskWords / 4u; i += kDtWaves * 64u) reinterpret_cast<uint4 *>(s_mask)[i] = make_uint4(0, 0, 0, 0);
            __syncthreads();
        }

        // ---- a tile that goes onto the list: its group counts summed per 64 words, for the work items that will expand it (each
        //      stages only the words of its own 32 segments then: expand_tile).  The tile's words are in the image (load layout:
        //      a lane's four words of a piece, sixteen lanes = a bucket of 64 words: one DPP row sum); counts above 2^25 -- 64 of
        //      them would not fit 32 bits -- mark the bucket instead, and the tile is staged whole.  (64 unmarked buckets still
        //      hold up to 2^37 groups: the list offers the sums only for tiles of fewer than 2^31, dt_defer_many.)
        if (deferred[j]) {
            const u64 n_et = (a.c_words + kScanTileWords - 1) / kScanTileWords;
            const u64 et = 2ull * ((u64)wt * kP + j) + (wave >> 2);
#pragma nounroll
            for (int k = 0; k < 4; ++k) { // (a loop, not four copies: this is the rare path, and the kernel has no register to spare)
                const u32x4 q = words4[w0 / 4u + 64 * k + lane];
                const u32 n0 = word_groups(q.x), n1 = word_groups(q.y), n2 = word_groups(q.z), n3 = word_groups(q.w);
                const bool big = __any(max(max(n0, n1), max(n2, n3)) > (1u << 25));
                u32 sum = n0 + n1 + n2 + n3;
                sum += __builtin_amdgcn_update_dpp(0u, sum, 0x111, 0xf, 0xf, true);
                sum += __builtin_amdgcn_update_dpp(0u, sum, 0x112, 0xf, 0xf, true);
                sum += __builtin_amdgcn_update_dpp(0u, sum, 0x114, 0xf, 0xf, true);
                sum += __builtin_amdgcn_update_dpp(0u, sum, 0x118, 0xf, 0xf, true);
                if ((lane & 15u) == 15u && et < n_et) a.tile_buckets[et * 64u + (wave & 3u) * 16u + 4u * (u32)k + (lane >> 4)] = big ? kBucketSaturated : sum;
            }
        }

        // ---- one start flag per word (the tile's own groups only; the words behind the tile: wave 2 below) --------------------
        if (!deferred[j] && !plain[j]) {
            const u32 my_w0 = w0 + kDtLaneWords * lane;
            u32 wds[kDtLaneWords];
#pragma unroll
            for (int k = 0; k < (int)kDtLaneWords / 4; ++k) {
                const u32x4 q = words4[my_w0 / 4u + k];
                wds[4 * k] = q.x, wds[4 * k + 1] = q.y, wds[4 * k + 2] = q.z, wds[4 * k + 3] = q.w;
            }
            u32 lane_pos = 0;
#pragma unroll
            for (int k = 0; k < (int)kDtLaneWords; ++k) lane_pos += word_groups(wds[k]);
            u32 p = wave_scan_incl32(lane_pos) - lane_pos;
#pragma unroll
            for (u32 w = 0; w < kDtWaves; ++w)
                if (w < wave) p += s_wave_pos[j][w];
#pragma unroll
            for (int k = 0; k < (int)kDtLaneWords; ++k) {
                // (every word of a tile that is not deferred holds a group, so every word starts one)
                atomicOr(&s_mask[p >> 5], 1u << (p & 31u));
                p += word_groups(wds[k]);
            }
        }
        __syncthreads();
        if (jj == 0) DGT(3);

        // ---- wave 0, first time round: the groups in front of the batch (row scan), what the batch leaves behind; wave 1:
        //      coarse flag counts; wave 2: the flags of the words behind the tile ---------------------------------------------------
        if (wave == 0 && jj == 0) {
#pragma unroll
            for (u32 t = 0; t + 1 < kP; ++t)
#pragma unroll
                for (int k = 0; k < 4; ++k) *reinterpret_cast<volatile u32x4 *>(s_park + ((t * 4u + k) * 64u + lane) * 4u) = hold[t][k];
            u64 end;
            __builtin_amdgcn_s_setprio(1); // the seven other waves wait for this one (row_scan_wait drops it before it sleeps)
            const u64 b = sums_resolve<!WAH_DT_EARLY, true>(a.ctrl, a.gen_desc, wt, epoch, batch_total, lane, end);
            DGT(4);
#pragma unroll
            for (u32 t = 0; t + 1 < kP; ++t)
#pragma unroll
                for (int k = 0; k < 4; ++k) hold[t][k] = *reinterpret_cast<const volatile u32x4 *>(s_park + ((t * 4u + k) * 64u + lane) * 4u);
            if (lane == 0) s_base = b;
            __builtin_amdgcn_s_setprio(0);
            // barrier 3, for wave 0 HERE: the other waves (theirs is below) go on into their first segments while lane 0 does the
            // batch's bookkeeping, which no expansion needs.  (wave is a scalar: the branch is the whole wave's.)
            __syncthreads();
            DGT(5);
            if (lane == 0) {
                const u64 n_et = (a.c_words + kScanTileWords - 1) / kScanTileWords;
                u64 bj = b;
                u64 d_tile[2 * kP], d_groups[2 * kP]; // the expand tiles that go onto the list (bit set in d_valid): appended by ONE atomic below
                u32 d_valid = 0;
#pragma unroll
                for (u32 t = 0; t < kP; ++t) {
                    const u64 et = 2ull * ((u64)wt * kP + t); // the tile's two expand tiles
                    d_tile[2 * t] = et, d_groups[2 * t] = first_half[t];
                    d_tile[2 * t + 1] = et + 1, d_groups[2 * t + 1] = total[t] - first_half[t];
                    if (et < n_et) {
                        a.tile_base[et] = bj;
                        a.tile_flags[et] = (uint8_t)empties_a[t];
                        if (et + 1 < n_et) {
                            a.tile_base[et + 1] = sat_add(bj, first_half[t]);
                            a.tile_flags[et + 1] = (uint8_t)empties_b[t];
                        }
                        if (deferred[t]) { // left to decode_expand_kernel's tile routine (launch_decode_tiles runs it over this list)
                            d_valid |= 1u << (2u * t);
                            if (et + 1 < n_et) d_valid |= 2u << (2u * t);
                        }
                    }
                    bj = sat_add(bj, total[t]);
                }
                // (a full list -- it has room for every tile twice -- means counters that are not this launch's: nobody would decode
                //  the tiles, so the launch must not end WAH_OK)
                if (!dt_defer_many<2 * kP>(defer_count, a.defer_list, a.defer_capacity, d_valid, d_tile, d_groups, true)) atomicOr(a.ctrl + kCtlError, kErrWorkspace);
                if (end >= kSumSaturate) atomicOr(a.ctrl + kCtlError, kErrStream);
                if (wt == a.n_wg_tiles - 1) {
                    const u64 words = (31ull * end + 31ull) / 32ull; // decompress.cu:84-93
                    a.tile_base[n_et] = end;
                    a.info[1] = end;
                    a.info[0] = words;
                    if (words > a.out_capacity) atomicOr(a.ctrl + kCtlError, kErrCapacity);
                    if (a.host_result) { // every scan of the launch can complete now; the deferred tiles are checked by their own launch
                        a.host_result[1] = words;
                        a.host_result[2] = end;
                        a.host_result[0] = 1ull | ((u64)__hip_atomic_load(a.ctrl + kCtlError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << 32);
                    }
                    launch_epoch_end(a.ctrl, le);
                    defer_counters_next(a.defer_count); // (the other counter zeroed for the next launch, this one to the list's launch)
                }
            }
        } else if (wave == 2 && !deferred[j] && !plain[j]) {
            // the words behind the tile: their start flags go behind the tile's own (positions total32 ..), 18 consecutive
            // words per lane; a fill word of count 0 among them cannot be flagged (see the segment loop)
            static_assert(kDtBehind == 18u * 64u, "18 words per lane");
            u32 l2 = lane;
            asm volatile("" : "+v"(l2)); // (as for s_coarse below)
            const u32 i0 = kDtTileWords + 18u * l2;
            const u32 left_t = left > j * kDtTileWords ? left - j * kDtTileWords : 0u; // words of the stream from this tile's start on
            // (the eighteen counts kept two to a register -- a clamped count fits sixteen bits: this block beside the held tile is
            //  what decides the kernel's register count)
            static_assert(kDtMaxGroups + 1u < 65536u, "two clamped counts per register");
            u32 n2[9];
            u32 lane_sum = 0, first_bad = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < 18; ++k) {
                const u32 nk = dt_word_groups_clamped(s_words[i0 + k]);
                if (nk == 0u && i0 + (u32)k < left_t && first_bad == 0xFFFFFFFFu) first_bad = lane_sum; // (in-lane position, made absolute below)
                lane_sum += nk;
                n2[k >> 1] = (k & 1) ? n2[k >> 1] | (nk << 16) : nk;
            }
            const u32 incl = wave_scan_incl32(lane_sum);
            u32 p = (u32)total[j] + (incl - lane_sum); // (not deferred: total = the clamped total)
            if (first_bad != 0xFFFFFFFFu) first_bad += p;
#pragma unroll
            for (int k = 0; k < 18; ++k) {
                const u32 nk = (k & 1) ? n2[k >> 1] >> 16 : n2[k >> 1] & 0xFFFFu;
                // (the first word BEHIND the stream's end is flagged too -- see the segment loop: the groups a last segment lacks)
                if ((nk != 0u || i0 + (u32)k == left_t) && p < kDtMaskBits) atomicOr(&s_mask[p >> 5], 1u << (p & 31u));
                p += nk;
            }
            // the first such word of the wave: minimum over the lanes (DPP max-scan of the complement)
            const u32 inv = (u32)__builtin_amdgcn_readlane((int)wave_scan_max32(~first_bad), 63);
            if (lane == 0) {
                s_behind[0] = (u32)__builtin_amdgcn_readlane((int)incl, 63);
                s_behind[1] = ~inv;
            }
        } else if (wave == 1 && !deferred[j] && !plain[j]) {
            // s_coarse[c] = start flags in mask words [0, 32 c): lane c counts its 32 words (rotated start: one bank each)
            u32 cnt = 0;
            if (lane < kDtCoarse) {
#pragma unroll 8
                for (u32 i = 0; i < 32u; ++i) {
                    const u32 jw = 32u * lane + ((i + lane) & 31u);
                    cnt += jw < kDtMaskWords ? (u32)__builtin_popcount(s_mask[jw]) : 0u;
                }
            }
            const u32 incl = wave_scan_incl32(cnt);
            u32 lc = lane;
            asm volatile("" : "+v"(lc)); // (opaque: the address is made here, not hoisted to the kernel's top and kept -- or spilled)
            s_coarse[lc] = incl - cnt;
        }
        if (!(wave == 0 && jj == 0)) __syncthreads(); // barrier 3 (wave 0, first time round: above, in front of its bookkeeping)
        if (jj == 0) {
            if (wave != 0) { DGT(5); } // (wave 0: at its own barrier 3)
            base = uniform64(s_base);
        }
        if (deferred[j]) continue;

        // ---- the output segments that start inside the tile: [tb, tb + total) -> segments k_begin .. k_end - 1 -------------------
        u64 tb = base;
#pragma unroll
        for (u32 t = 0; t < kP; ++t)
            if (t < j) tb = sat_add(tb, total[t]);
        const u32 total32 = (u32)total[j]; // <= kDtMaxGroups
        // (made here, per tile, not once per kernel: four registers less across the scan and the other tiles' flag making)
        u32 lv = lane;
        asm volatile("" : "+v"(lv));
        const u32 o = lv & 31u;
        const u32 up = 31u - ((lv - 1u) & 31u);             // what my group is shifted up by in my LEFT neighbour's word
        u32 soff = o != 31u ? (lv - (lv >> 5)) * 4u : 0xFFFFF000u; // lanes 31, 63 only lend their group: out of range, dropped
        asm volatile("" : "+v"(soff));                      // (opaque: the store offsets stay instruction immediates)
        const u32 wbase = (u32)(uintptr_t)(lds_u32_ptr)s_words;
        const u64 k_begin = (tb + kSegGroups - 1) / kSegGroups;
        const u64 k_end = (tb + total32 + kSegGroups - 1) / kSegGroups;
#ifdef WAH_DIAG
        if (jj == 0) DGT(8); else DGT(14);
#endif
        if (plain[j]) {
            // group p of the tile = word p (its own 8192 words, then the 1152 behind it: all literals, all inside the stream): the
            // gather's address is the lane's plus an immediate, a literal is its own group (bit 31 = 0); repack and stores as below
            for (u64 seg = k_begin + wave; seg < k_end; seg += kDtWaves) {
                const u32 t0 = (u32)(seg * kSegGroups - tb);
                const u64 seg_w0 = seg * kSegWords;
                if (seg_w0 >= a.out_capacity) continue;
                const u32 seg_words = a.out_capacity - seg_w0 < kSegWords ? (u32)(a.out_capacity - seg_w0) : kSegWords;
                const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(a.out + seg_w0, seg_words * 4u); // stores past the end are dropped
                const u32 a0 = wbase + ((t0 + lv) << 2);
#pragma unroll
                for (int g4 = 0; g4 < (int)kSteps / WAH_DT_GROUP; ++g4) {
                    u32 src[WAH_DT_GROUP];
#pragma unroll
                    for (int q = 0; q < WAH_DT_GROUP; ++q) src[q] = *(lds_u32_ptr)(uintptr_t)(a0 + 256u * (u32)(WAH_DT_GROUP * g4 + q));
#pragma unroll
                    for (int q = 0; q < WAH_DT_GROUP; ++q) {
                        const int s = WAH_DT_GROUP * g4 + q;
                        const u32 hi_part = (u32)__builtin_amdgcn_mov_dpp((int)(src[q] << up), 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_amdgcn_ubfe(src[q], o, 31u - o) | hi_part, rsrc, soff, 248u * s, 0);
                    }
                }
            }
            continue;
        }
        for (u64 seg = k_begin + wave; seg < k_end; seg += kDtWaves) {
            const u32 t0 = (u32)(seg * kSegGroups - tb); // tile-relative position of the segment's first group (< total32)
            u32 nvalid = kSegGroups;
            if (t0 + kSegGroups > total32) {
                // The tile's LAST segment: its groups behind the tile's own come from the words parked behind the tile (flagged by
                // wave 2 meanwhile).  A fill word of count 0 among those it needs (foreign stream): the segment starts in one of
                // the tile's two expand tiles, which decode_expand_kernel then decodes again as a whole, this segment included.
                const u32 behind = uniform32(s_behind[0]), first_bad = uniform32(s_behind[1]);
                if (first_bad < t0 + kSegGroups) {
                    if (lane == 0) {
                        const bool second = t0 >= (u32)first_half[j];
                        if (!dt_defer(defer_count, a.defer_list, a.defer_capacity, 2ull * ((u64)wt * kP + j) + (second ? 1u : 0u),
                                      second ? total[j] - first_half[j] : first_half[j]))
                            atomicOr(a.ctrl + kCtlError, kErrWorkspace);
                    }
                    continue;
                }
                const u32 avail = total32 - t0 + behind; // (no wrap: both below 2^27)
                if (avail < kSegGroups) nvalid = avail;    // the stream ends inside the segment: the bitmap's last segment
            }
            // output words of the segment: all 992, or what ceil(31 G / 32) leaves for the bitmap's last one
            const u64 seg_w0 = seg * kSegWords;
            u32 seg_words = kSegWords;
            if (nvalid != kSegGroups) {
                const u64 words = (31ull * (seg * kSegGroups + nvalid) + 31ull) / 32ull;
                seg_words = words > seg_w0 ? (u32)(words - seg_w0) : 0u;
            }
            if (seg_w0 >= a.out_capacity) continue;
            if (a.out_capacity - seg_w0 < seg_words) seg_words = (u32)(a.out_capacity - seg_w0);
            const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(a.out + seg_w0, seg_words * 4u); // stores past the end are dropped

            // start flags of the segment's groups, 32 per lane, aligned to the segment: lane l = groups 32 l .. 32 l + 31
            const u32 k0 = t0 >> 5, r = t0 & 31u;
            const u32 m_lo = s_mask[k0 + (lane & 31u)], m_hi = s_mask[k0 + (lane & 31u) + 1u];
            const u32 seg_flags = __builtin_amdgcn_alignbit(m_hi, m_lo, r);
            // words that start in front of the segment: coarse count + the mask words between + the bits below r
            const u32 cb = k0 & ~31u;
            const u32 between = s_mask[cb + (lane & 31u)]; // (read by every lane: a load under a condition is waited for on its own)
            u32 part = lane < (k0 & 31u) ? (u32)__builtin_popcount(between) : 0u;
            const u32 mk0 = (u32)__builtin_amdgcn_readlane((int)m_lo, 0); // mask word k0: the segment starts at its bit r
            if (lane == (k0 & 31u)) part = (u32)__builtin_popcount(mk0 & ((1u << r) - 1u));
            // starts at positions < t0, as the byte address of word number (that count - 1) of the tile (running: <= the step before)
            u32 before = uniform32(s_coarse[k0 >> 5]) + wave_total32(part) - 1u; // (word number of the last start in front of the step)
#ifdef WAH_DIAG
            if (jj == 0 && seg == k_begin + wave) { asm volatile("" : "+s"(before)); DGT(9); }
#endif
            // (The bitmap's last segment may lack groups, nvalid < 1024: the words behind the stream's end are fill words of
            //  count 0, the first of them has a start flag at the position where the stream ends -- the flags of the tile's own
            //  words are made for padding words too, wave 2 flags the one behind the tile -- so the missing groups find that word
            //  and come out as zeros without a test in the steps.)
            // WAH_DT_GROUP steps at a time: their ranks first, then the gathers together, then decode and store
#pragma unroll
            for (int g4 = 0; g4 < (int)kSteps / WAH_DT_GROUP; ++g4) {
                u32 addr[WAH_DT_GROUP], src[WAH_DT_GROUP];
#pragma unroll
                for (int q = 0; q < WAH_DT_GROUP; ++q) {
                    const int s = WAH_DT_GROUP * g4 + q;
                    // the step's 64 start flags as two scalar registers; word number = (starts at positions <= mine) - 1, and
                    // starts at or below lane L = bits of (flags >> 1) below L (v_mbcnt) + bit 0
                    const u32 mlo = (u32)__builtin_amdgcn_readlane((int)seg_flags, 2 * s);
                    const u32 mhi = (u32)__builtin_amdgcn_readlane((int)seg_flags, 2 * s + 1);
                    const u64 m1 = (((u64)mhi << 32) | mlo) >> 1;
                    const u32 below = __builtin_amdgcn_mbcnt_hi((u32)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((u32)m1, 0u));
                    addr[q] = wbase + ((below + (before + (mlo & 1u))) << 2); // (v_add_lshl_u32; the base is the LDS read's offset field)
                    before += (u32)__builtin_popcountll(((u64)mhi << 32) | mlo);
                }
#pragma unroll
                for (int q = 0; q < WAH_DT_GROUP; ++q) src[q] = *(lds_u32_ptr)(uintptr_t)addr[q];
#pragma unroll
                for (int q = 0; q < WAH_DT_GROUP; ++q) {
                    const int s = WAH_DT_GROUP * g4 + q;
                    // fill -> 31 copies of bit 30, literal -> itself (kernels.cu:332-354); bit 31 of a fill's group is not
                    // cleared: the repack below takes bits 0..30 only
                    u32 grp = (int)src[q] < 0 ? (u32)__builtin_amdgcn_sbfe((int)src[q], 30, 1) : src[q];
                    // 31 -> 32 repack (mergeWords, kernels.cu:375): see expand_steps
                    const u32 hi_part = (u32)__builtin_amdgcn_mov_dpp((int)(grp << up), 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_amdgcn_ubfe(grp, o, 31u - o) | hi_part, rsrc, soff, 248u * s, 0);
                }
            }
#ifdef WAH_DIAG
            if (jj == 0) {
                asm volatile("" ::: "memory");
                if (seg == k_begin + wave) DGT(10); else if (seg == k_begin + wave + kDtWaves) DGT(11);
                dg[15] += 1;
            }
#endif
        }
#ifdef WAH_DIAG
        if (jj == 0) {
            DGT(12);
            __syncthreads();
            DGT(13);
        }
#endif
    }
#ifdef WAH_DIAG
    __syncthreads();
    if (threadIdx.x == 0 && a.host_result == nullptr && a.out_capacity >= (u64)a.n_wg_tiles * 32u + 32u) { // diagnostic build: time line instead of output head
        u64 *t = reinterpret_cast<u64 *>(a.out) + (u64)wt * 16u;
        for (int i = 0; i < 6; ++i) t[i] = dg[i];
        t[6] = __builtin_amdgcn_s_memrealtime();
        t[7] = blockIdx.x; // (how far the ticket order is from the dispatch order)
        for (int i = 8; i < 16; ++i) t[i] = dg[i];
    }
#endif
}
