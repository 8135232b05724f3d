// wah_cumsum.hip -- wah_bsi_cumsum_indexed_device: the RUNNING SUM of a bit-sliced value over the rows a conjunction of filters
// selects, R[p] = sum of the values of the selected rows q <= p (q < p: exclusive) mod 2^n_slices_out, leaving as a NEW bit-sliced
// attribute of up to 64 slices: `SUM(x) OVER (ORDER BY rowid)`, and with no value slices at all the running COUNT -- ROW_NUMBER()
// over the selected rows, or with all_rows the rank of ANY row among them.  No value column is written and read again.  It is the
// one call of the family whose answer for a row depends on the rows in front of it, so it is three launches, none of which waits
// for another workgroup: segments are independent items of a capped grid-stride grid in the first and the last.
//
// cumsum_totals_kernel   one workgroup of eight wavefronts per segment.  Wavefront 7 makes the SELECTION image as the group-by
//             kernel does (wah_group_by.hip): all ones clipped to segment_groups / segment_rows(n_rows), the value's existence row
//             and the filter rows walked into it under AND.  Behind a barrier wavefronts 0 .. 6 walk their share of the value's
//             slices under OR, one row at a time in the zeroed image, and where a row is complete add popcount(slice & selection)
//             << significance: a total needs no per-row fold.  Without value slices the total is the selection's popcount.  One
//             u64 per segment leaves, EVERY segment's: the scratch needs no clearing.  32 KiB of LDS.
// cumsum_scan_kernel     ONE workgroup turns the totals in place into the sum of the segments in front of each: 8192 entries per
//             round (eight per thread, a wave scan, sixteen wave totals through LDS), a carry from round to round.
// cumsum_rows_kernel     bsi_map_segments_kernel's frame (wah_map.hip): s_rows[kSegBits] plus eight images, 159 872 bytes of LDS,
//             one workgroup per CU.  Wavefronts 0 .. 6 fold the value's slices into one word per row, wavefront 7 makes the
//             selection.  Behind the barrier wavefront w takes blocks w and w + 8 with map_block's row ownership (lane l of step t:
//             row 2048 blk + 64 t + l), twice:
//   totals    a block's selected values are reduced to one u64, sixteen of them in LDS; a barrier.
//   scan      per block the base is the segment's base plus the block totals in front of it (wave-uniform).  Per step one
//             inclusive scan of the 64 lanes with DPP -- values of up to 26 bits in one u32 scan, wider ones as two scans of
//             their 16-bit halves, which 64 lanes cannot overflow -- added to the carry of the steps in front in 64 bits; minus
//             the lane's own value when exclusive; zero for an unselected row unless all_rows, and for a row at or behind n_rows.
//             The block's results stay in two statically indexed register arrays, low and high halves.
//   transpose a RUNTIME loop over the result's slices, most significant first: slice_words (wah_slice_words.hpp) on the high half
//             for slices 63 .. 32, on the low half below, and one store of 256 contiguous bytes (128 in the half block) per slice
//             and block.  Without all_rows the ballots of the selection are the last row.
// Every word of every result row is written exactly once: the matrix needs no clearing.  No register array is indexed by a
// runtime value.  Every table row's every segment is walked by the first kernel and again by the last: both report what the walk
// refuses.
#include "wah_fold_bits.hpp"
#include "wah_slice_words.hpp"

namespace wah {
namespace {

constexpr u32 kCumsumGridItems = 512;  // workgroups of the two segment kernels at the most (bsi_map_segments_kernel's cap)
constexpr u32 kCumsumWaves = 8;        // wavefronts of their workgroups
constexpr u32 kCumsumSliceWaves = kCumsumWaves - 1u; // ... that walk slices; the last one walks the selection rows
constexpr u32 kCumsumBlockWords = 64;  // slice words per block: one per lane (map_block's block)
constexpr u32 kCumsumBlockSteps = 32;  // steps of 64 rows per block
constexpr u32 kCumsumBlockRows = 2048; // 32 * kCumsumBlockWords
constexpr u32 kCumsumBlocks = 16;      // blocks of a segment: 15 of kCumsumBlockRows rows and a half one
constexpr u32 kCumsumNarrowBits = 26;  // value slices up to which 64 lanes' sum stays below 2^32: one u32 scan
constexpr u32 kScanWaves = 16;         // wavefronts of cumsum_scan_kernel's one workgroup
constexpr u32 kScanPer = 8;            // entries per thread and round
static_assert((kSegBits + kCumsumWaves * kSegGroups) * sizeof(u32) + kCumsumBlocks * sizeof(u64) <= 160u * 1024u, "one workgroup fits a CU's LDS");
static_assert((kCumsumBlocks - 1u) * kCumsumBlockRows + kCumsumBlockRows / 2u == kSegBits &&
                  (kCumsumBlocks - 1u) * kCumsumBlockWords + kCumsumBlockWords / 2u == kSegWords,
              "a segment: fifteen blocks and a half");
static_assert(kCumsumBlocks == 2u * kCumsumWaves, "two blocks per wavefront");
static_assert(64u * ((1u << kCumsumNarrowBits) - 1u) < (1ull << 32) && 64u * 0xFFFFu < (1ull << 32), "neither scan can wrap");

// the selection image of segment seg before the walks: every row of the segment that lies in front of n_rows
__device__ __forceinline__ void selection_preset(u32 *acc, u64 n_rows, u64 seg, u32 nvalid, u32 lane) {
    const u32 rows = segment_rows(n_rows, seg), full = rows / 31u, rest = rows % 31u;
#pragma unroll
    for (u32 i = 0; i < kSegGroups / 64u; ++i) {
        const u32 g = 64u * i + lane;
        acc[g] = g >= nvalid ? 0u : g < full ? kOnes31 : g == full ? (1u << rest) - 1u : 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// ... and the walks: the value table's last row if it is an existence row, then the filter rows, ANDed in
__device__ __forceinline__ void selection_walk(const BsiCumsumArgs &a, u32 *acc, u64 seg, u32 nvalid, u32 lane) {
    const ListOp m_and = list_op(0u);
    bool ok = true;
    if (a.has_exists)
        ok = list_walk(a.val + a.n_slices_val, 1u, seg, nvalid, m_and.fill, acc, lane, [&](u32) -> const ListOp & { return m_and; }, [](u32) {});
    if (a.n_filters != 0u)
        ok = list_walk(a.filters, a.n_filters, seg, nvalid, m_and.fill, acc, lane, [&](u32) -> const ListOp & { return m_and; }, [](u32) {}) && ok;
    if (!ok) report_stream_error(a.ctrl, lane);
}

// the table rows [lo, hi) of the value's n slices that wavefront `wave` of the seven walks
__device__ __forceinline__ void slice_share(u32 n, u32 wave, u32 &lo, u32 &hi) {
    const u32 per = (n + kCumsumSliceWaves - 1u) / kCumsumSliceWaves;
    lo = min(wave * per, n);
    hi = wave < kCumsumSliceWaves ? min(lo + per, n) : lo;
}

// The slices [w_lo, w_hi) of the value walked under OR one row at a time in the zeroed image; done(sig) is called, wave-uniform,
// while the image holds exactly the slice of significance sig.  (A slice settled in the gather is all zeros here and is not seen.)
template <class Done>
__device__ __forceinline__ void walk_slices(const BsiCumsumArgs &a, u32 w_lo, u32 w_hi, u64 seg, u32 nvalid, u32 *acc, u32 lane, Done done) {
    const ListOp m_or = list_op(1u);
    u32 cur = 0;       // the table row the image holds (wave-uniform)
    bool open = false; // ... if it holds one
    auto close = [&]() {
        done(a.n_slices_val - 1u - w_lo - cur);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        image_fill(acc, 0u, lane);
    };
    const bool ok = list_walk(a.val + w_lo, w_hi - w_lo, seg, nvalid, m_or.fill, acc, lane, [&](u32) -> const ListOp & { return m_or; }, [&](u32 j) {
        if (open) close(); // this row's words begin: the one in the image is complete
        cur = j;
        open = true;
    });
    if (open) close();
    // (no early return: the workgroup's barriers are for all its wavefronts; the output of a refused call is unspecified)
    if (!ok) report_stream_error(a.ctrl, lane);
}

__global__ __launch_bounds__(kCumsumWaves * 64) void cumsum_totals_kernel(const BsiCumsumArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kCumsumWaves][kSegGroups];
    __shared__ u64 s_part[kCumsumWaves];
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    const u32 *sel = s_acc[kCumsumSliceWaves];
    u32 w_lo, w_hi;
    slice_share(a.n_slices_val, wave, w_lo, w_hi);

#pragma nounroll
    for (u64 seg = blockIdx.x; seg < a.n_segments; seg += gridDim.x) { // (workgroup-uniform)
        const u32 nvalid = segment_groups(a.groups, seg);
        if (wave < kCumsumSliceWaves) {
            image_fill(acc, 0u, lane);
        } else {
            selection_preset(acc, a.n_rows, seg, nvalid, lane);
            selection_walk(a, acc, seg, nvalid, lane);
        }
        __syncthreads();

        u64 sum = 0; // the lane's share of the wavefront's
        auto count = [&](u32 sig) { // the image's set bits among the selected rows, at weight 2^sig
            u32 c = 0;
#pragma unroll
            for (u32 i = 0; i < kSegGroups / 64u; ++i) c += (u32)__popc((wave < kCumsumSliceWaves ? acc[64u * i + lane] : kOnes31) & sel[64u * i + lane]);
            sum += (u64)c << sig;
        };
        if (wave < kCumsumSliceWaves) {
            if (w_lo < w_hi) walk_slices(a, w_lo, w_hi, seg, nvalid, acc, lane, count); // (wave-uniform)
        } else if (a.n_slices_val == 0u) {
            count(0u);
        }
        sum = wave_sum(sum);
        if (lane == 0) s_part[wave] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 total = 0;
#pragma unroll
            for (u32 w = 0; w < kCumsumWaves; ++w) total += s_part[w];
            a.totals[seg] = total;
        }
        // (no third barrier: the next segment's selection is written by wavefront 7 behind this one, its partial sums behind the next)
    }
}

// totals[i] becomes the sum of totals[0 .. i), mod 2^64
__global__ __launch_bounds__(kScanWaves * 64) void cumsum_scan_kernel(u64 *totals, u64 n) {
    __shared__ u64 s_wave[kScanWaves];
    const u32 wave = wave_id(), lane = lane_id();
    u64 carry = 0; // the sum of the rounds in front (workgroup-uniform)
#pragma nounroll
    for (u64 i0 = 0; i0 < n; i0 += (u64)kScanWaves * 64u * kScanPer) {
        const u64 first = i0 + (u64)threadIdx.x * kScanPer;
        u64 v[kScanPer], mine = 0;
#pragma unroll
        for (u32 i = 0; i < kScanPer; ++i) {
            v[i] = first + i < n ? totals[first + i] : 0ull;
            mine += v[i];
        }
        const u64 incl = wave_scan_incl(mine, lane);
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        u64 before = 0, all = 0;
#pragma unroll
        for (u32 w = 0; w < kScanWaves; ++w) {
            const u64 x = s_wave[w];
            before += w < wave ? x : 0ull;
            all += x;
        }
        u64 run = carry + before + incl - mine;
#pragma unroll
        for (u32 i = 0; i < kScanPer; ++i) {
            if (first + i < n) totals[first + i] = run;
            run += v[i];
        }
        carry += all;
        __syncthreads(); // the next round's wave totals
    }
}

// Block blk of a segment: the values of its kSteps steps of 64 rows -- a row that is not selected holds 0, a selected one its
// value, or 1 where the value has no slices.  Returns the selection: bit t for the lane's row of step t.
template <u32 kSteps>
__device__ __forceinline__ u32 load_block(const u32 *s_rows, const u32 *sel, u32 n_slices_val, u32 blk, u32 lane, u32 (&v)[kSteps]) {
    u32 row0 = (u32)kCumsumBlockRows * blk + lane;
    // (opaque: the steps' selection words and shifts depend on lane and block alone, and hoisted out of the loop over the
    //  segments they would take two hundred registers)
    asm volatile("" : "+v"(row0));
    u32 picked = 0u;
#pragma unroll
    for (u32 t = 0; t < kSteps; ++t) {
        const u32 r = row0 + 64u * t;
        const u32 bit = (sel[r / 31u] >> (r % 31u)) & 1u;
        picked |= bit << t;
        v[t] = n_slices_val == 0u ? bit : s_rows[r] & (0u - bit); // (wave-uniform choice)
    }
    return picked;
}

// the sum of block blk's selected values (wave-uniform)
template <u32 kSteps>
__device__ __forceinline__ u64 block_total(const u32 *s_rows, const u32 *sel, u32 n_slices_val, u32 blk, u32 lane) {
    u32 v[kSteps];
    load_block<kSteps>(s_rows, sel, n_slices_val, blk, lane, v);
    u64 sum = 0;
#pragma unroll
    for (u32 t = 0; t < kSteps; ++t) sum += v[t];
    return uniform64(wave_sum(sum));
}

// Block blk of segment seg, rows of it in front of n_rows: the running sums of its kSteps steps from `base` on, stored as
// 2 kSteps words of every result row.  kWide: values above kCumsumNarrowBits slices; kHigh: a result above 32 slices.
template <u32 kSteps, bool kWide, bool kHigh>
__device__ __forceinline__ void scan_block(const BsiCumsumArgs &a, const u32 *s_rows, const u32 *sel, u64 seg, u32 rows, u32 blk, u32 lane, u64 base) {
    u32 lo[kSteps], hi[kSteps];
    u32 have = 0u; // lane j: word j of the block's selection
    {
        u32 v[kSteps];
        const u32 picked = load_block<kSteps>(s_rows, sel, a.n_slices_val, blk, lane, v);
        const u32 row0 = (u32)kCumsumBlockRows * blk + lane;
        u64 carry = base; // the sum in front of the step (wave-uniform)
#pragma unroll
        for (u32 t = 0; t < kSteps; ++t) {
            const u32 x = v[t];
            const u64 s = kWide ? (u64)wave_scan_incl32(x & 0xFFFFu) + ((u64)wave_scan_incl32(x >> 16) << 16) : (u64)wave_scan_incl32(x);
            u64 r = carry + s - (a.exclusive != 0u ? x : 0u);
            carry += ((u64)(kWide ? (u32)__builtin_amdgcn_readlane((int)(u32)(s >> 32), 63) : 0u) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)s, 63);
            const bool on = ((picked >> t) & 1u) != 0u;
            if (!((on || a.all_rows != 0u) && row0 + 64u * t < rows)) r = 0ull;
            lo[t] = (u32)r;
            hi[t] = (u32)(r >> 32);
            const u64 m = __ballot(on);
            have = put_lane((u32)m, 2u * t, have);
            have = put_lane((u32)(m >> 32), 2u * t + 1u, have);
        }
    }
    const bool store = lane < 2u * kSteps; // (the half block: 32 words)
    u32 *out = a.matrix + (seg * kSegWords + kCumsumBlockWords * blk + lane); // row 0 of the matrix; every row is n_words further
    u32 b = a.n_slices_out;
    if (kHigh) {
#pragma nounroll
        for (; b > 32u; --b) {
            const u32 w = slice_words(hi, 1u << (b - 33u));
            if (store) *out = w;
            out += a.n_words;
        }
    }
#pragma nounroll
    for (; b > 0u; --b) {
        const u32 w = slice_words(lo, 1u << (b - 1u));
        if (store) *out = w;
        out += a.n_words;
    }
    if (a.all_rows == 0u && store) *out = have;
}

template <bool kWide, bool kHigh>
__global__ __launch_bounds__(kCumsumWaves * 64) void cumsum_rows_kernel(const BsiCumsumArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_rows[kSegBits];
    __shared__ __attribute__((aligned(16))) u32 s_acc[kCumsumWaves][kSegGroups];
    __shared__ u64 s_block[kCumsumBlocks];
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    const u32 *sel = s_acc[kCumsumSliceWaves];
    const u32 nv = a.n_slices_val;
    u32 w_lo, w_hi;
    slice_share(nv, wave, w_lo, w_hi);
    const bool last_half = wave + kCumsumWaves == kCumsumBlocks - 1u; // (wave-uniform: the wavefront whose second block is the half one)

#pragma nounroll
    for (u64 seg = blockIdx.x; seg < a.n_segments; seg += gridDim.x) { // (workgroup-uniform)
        const u32 nvalid = segment_groups(a.groups, seg);
        const u32 rows = segment_rows(a.n_rows, seg);

        if (nv != 0u) // (without value slices the rows' words are never read)
            for (u32 p = threadIdx.x * 4u; p < kSegBits; p += kCumsumWaves * 64u * 4u) *reinterpret_cast<uint4 *>(s_rows + p) = make_uint4(0u, 0u, 0u, 0u);
        if (wave < kCumsumSliceWaves)
            image_fill(acc, 0u, lane);
        else
            selection_preset(acc, a.n_rows, seg, nvalid, lane);
        __syncthreads();

        if (wave < kCumsumSliceWaves) {
            if (w_lo < w_hi) // (wave-uniform)
                walk_slices(a, w_lo, w_hi, seg, nvalid, acc, lane, [&](u32 sig) { fold_slice_bits(acc, s_rows, 0u, kSegGroups / 64u, sig, lane); });
        } else {
            selection_walk(a, acc, seg, nvalid, lane);
        }
        __syncthreads();

        {
            const u64 t0 = block_total<kCumsumBlockSteps>(s_rows, sel, nv, wave, lane);
            const u64 t1 = last_half ? block_total<kCumsumBlockSteps / 2u>(s_rows, sel, nv, kCumsumBlocks - 1u, lane)
                                     : block_total<kCumsumBlockSteps>(s_rows, sel, nv, wave + kCumsumWaves, lane);
            if (lane == 0) {
                s_block[wave] = t0;
                s_block[wave + kCumsumWaves] = t1;
            }
        }
        __syncthreads();

        u64 base = a.totals[seg]; // (scanned: the sum of the segments in front)
#pragma nounroll
        for (u32 b = 0; b < wave; ++b) base += s_block[b];
        base = uniform64(base);
        scan_block<kCumsumBlockSteps, kWide, kHigh>(a, s_rows, sel, seg, rows, wave, lane, base);
#pragma nounroll
        for (u32 b = wave; b < wave + kCumsumWaves; ++b) base += s_block[b];
        base = uniform64(base);
        if (last_half)
            scan_block<kCumsumBlockSteps / 2u, kWide, kHigh>(a, s_rows, sel, seg, rows, kCumsumBlocks - 1u, lane, base);
        else
            scan_block<kCumsumBlockSteps, kWide, kHigh>(a, s_rows, sel, seg, rows, wave + kCumsumWaves, lane, base);
        __syncthreads(); // the next segment clears the rows and the images
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_bsi_cumsum_parts_indexed_device: the same running sum, starting again at every row that is set in ONE more bitmap, the
// partition STARTS -- `SUM(x) OVER (PARTITION BY g ORDER BY rowid)` on a table clustered by g.  The frame is the one above: three
// launches, no workgroup waits for another.  Plain addition becomes the segmented operator on pairs (has_start, sum),
//   (f1, s1) o (f2, s2) = (f1 | f2, f2 ? s2 : s1 + s2),
// at every level:
// cumsum_parts_totals_kernel  as cumsum_totals_kernel, but wavefront 7 first walks the starts row into its image, clips it to the
//             rows in front of n_rows and finds its last set bit; then it makes the selection in the same image and ANDs "rows at
//             or behind the last start" into it.  What the popcounts then see is the segment's TAIL: the selected values at or
//             behind its last start, the whole segment where it has none.  A record (tail, has_start) per segment leaves, EVERY
//             segment's.
// cumsum_parts_scan_kernel    cumsum_scan_kernel on the pairs: a record's sum becomes what flows INTO the segment, the tails
//             since the last segment that held a start; the carry from round to round is a pair too.
// cumsum_parts_rows_kernel    cumsum_rows_kernel's frame and footprint: SIX wavefronts share the value's slices, wavefront 6 walks
//             the starts row into its image (clipped to the rows in front of n_rows), wavefront 7 makes the selection.  A
//             block's total is a pair (has_start, the values at or behind its last start); a block's base is the fold of the
//             segment's incoming sum and the blocks in front.  Per step of 64 rows the heads are one ballot of the start bits:
//   no head   (wave-uniform, the common case) the step above: one DPP scan, the carry on the scalar unit.
//   heads     the same DPP scan S, minus the EXCLUSIVE scan value at the lane's own head lane -- the last head at or in front
//             of it, from the ballot masked to the lanes <= lane: one ds_bpermute per scanned word.  The lanes in front of the
//             first head keep the carry, the others drop it; the carry out is S[63] minus the exclusive value at the last head.
//             The u32 scans cannot wrap, so the differences are exact.
constexpr u32 kPartsSliceWaves = kCumsumWaves - 2u; // wavefronts of cumsum_parts_rows_kernel that walk slices
constexpr u32 kPartsStartsWave = kCumsumWaves - 2u; // ... the one that walks the starts row; the last one walks the selection rows
static_assert((kSegBits + kCumsumWaves * kSegGroups) * sizeof(u32) + kCumsumBlocks * (sizeof(u64) + sizeof(u32)) <= 160u * 1024u,
              "one workgroup fits a CU's LDS");

// group g of a segment of nvalid groups and `rows` rows in front of n_rows: the bits of its rows
__device__ __forceinline__ u32 rows_mask(u32 g, u32 nvalid, u32 rows) {
    const u32 full = rows / 31u, rest = rows % 31u;
    return g >= nvalid ? 0u : g < full ? kOnes31 : g == full ? (1u << rest) - 1u : 0u;
}

// the starts row of segment seg walked under OR into the zeroed image, then clipped to the rows in front of n_rows
__device__ __forceinline__ void starts_walk(const BsiCumsumPartsArgs &a, u32 *acc, u64 seg, u32 nvalid, u32 rows, u32 lane) {
    const ListOp m_or = list_op(1u);
    const bool ok = list_walk(a.starts, 1u, seg, nvalid, m_or.fill, acc, lane, [&](u32) -> const ListOp & { return m_or; }, [](u32) {});
    if (!ok) report_stream_error(a.c.ctrl, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (u32 i = 0; i < kSegGroups / 64u; ++i) acc[64u * i + lane] &= rows_mask(64u * i + lane, nvalid, rows);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

__global__ __launch_bounds__(kCumsumWaves * 64) void cumsum_parts_totals_kernel(const BsiCumsumPartsArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kCumsumWaves][kSegGroups];
    __shared__ u64 s_part[kCumsumWaves];
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    const u32 *sel = s_acc[kCumsumSliceWaves];
    u32 w_lo, w_hi;
    slice_share(a.c.n_slices_val, wave, w_lo, w_hi);

#pragma nounroll
    for (u64 seg = blockIdx.x; seg < a.c.n_segments; seg += gridDim.x) { // (workgroup-uniform)
        const u32 nvalid = segment_groups(a.c.groups, seg);
        image_fill(acc, 0u, lane);
        if (wave == kCumsumSliceWaves) {
            const u32 rows = segment_rows(a.c.n_rows, seg);
            starts_walk(a, acc, seg, nvalid, rows, lane);
            u32 last = 0u; // 1 + the last start among the lane's groups, 0: none
#pragma unroll
            for (u32 i = 0; i < kSegGroups / 64u; ++i) {
                const u32 g = 64u * i + lane, w = acc[g];
                if (w != 0u) last = 31u * g + 32u - (u32)__clz(w);
            }
            last = (u32)__builtin_amdgcn_readlane((int)wave_scan_max32(last), 63);
            if (lane == 0) a.records[seg].has_start = last != 0u ? 1ull : 0ull;
            const u32 first = last != 0u ? last - 1u : 0u; // the rows from here on are the segment's tail
            selection_preset(acc, a.c.n_rows, seg, nvalid, lane);
            selection_walk(a.c, acc, seg, nvalid, lane);
#pragma unroll
            for (u32 i = 0; i < kSegGroups / 64u; ++i) {
                const u32 g = 64u * i + lane;
                acc[g] &= g < first / 31u ? 0u : g == first / 31u ? (kOnes31 << (first % 31u)) & kOnes31 : kOnes31;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        __syncthreads();

        u64 sum = 0; // the lane's share of the wavefront's
        auto count = [&](u32 sig) { // the image's set bits among the selected rows of the tail, at weight 2^sig
            u32 c = 0;
#pragma unroll
            for (u32 i = 0; i < kSegGroups / 64u; ++i) c += (u32)__popc((wave < kCumsumSliceWaves ? acc[64u * i + lane] : kOnes31) & sel[64u * i + lane]);
            sum += (u64)c << sig;
        };
        if (wave < kCumsumSliceWaves) {
            if (w_lo < w_hi) walk_slices(a.c, w_lo, w_hi, seg, nvalid, acc, lane, count); // (wave-uniform)
        } else if (a.c.n_slices_val == 0u) {
            count(0u);
        }
        sum = wave_sum(sum);
        if (lane == 0) s_part[wave] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 total = 0;
#pragma unroll
            for (u32 w = 0; w < kCumsumWaves; ++w) total += s_part[w];
            a.records[seg].sum = total;
        }
        // (no third barrier, as above; has_start went out from wavefront 7's own registers)
    }
}

struct PartsPair {
    u64 s;
    u32 f;
};
// x in front of y
__device__ __forceinline__ PartsPair parts_fold(PartsPair x, PartsPair y) { return {y.f != 0u ? y.s : x.s + y.s, x.f | y.f}; }

// records[i].sum becomes what flows into segment i: the fold of records[0 .. i)
__global__ __launch_bounds__(kScanWaves * 64) void cumsum_parts_scan_kernel(BsiCumsumPartsRecord *records, u64 n) {
    __shared__ u64 s_wave_s[kScanWaves];
    __shared__ u32 s_wave_f[kScanWaves];
    const u32 wave = wave_id(), lane = lane_id();
    PartsPair carry = {0ull, 0u}; // the fold of the rounds in front (workgroup-uniform)
#pragma nounroll
    for (u64 i0 = 0; i0 < n; i0 += (u64)kScanWaves * 64u * kScanPer) {
        const u64 first = i0 + (u64)threadIdx.x * kScanPer;
        PartsPair v[kScanPer], mine = {0ull, 0u};
#pragma unroll
        for (u32 i = 0; i < kScanPer; ++i) {
            v[i] = {0ull, 0u};
            if (first + i < n) v[i] = {records[first + i].sum, (u32)records[first + i].has_start};
            mine = parts_fold(mine, v[i]);
        }
        PartsPair incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const PartsPair t = {__shfl_up(incl.s, off), (u32)__shfl_up((int)incl.f, off)};
            if (lane >= (u32)off) incl = parts_fold(t, incl);
        }
        if (lane == 63u) {
            s_wave_s[wave] = incl.s;
            s_wave_f[wave] = incl.f;
        }
        PartsPair excl = {__shfl_up(incl.s, 1), (u32)__shfl_up((int)incl.f, 1)};
        if (lane == 0u) excl = {0ull, 0u};
        __syncthreads();
        PartsPair before = carry, all = carry;
#pragma unroll
        for (u32 w = 0; w < kScanWaves; ++w) {
            const PartsPair x = {s_wave_s[w], s_wave_f[w]};
            if (w < wave) before = parts_fold(before, x);
            all = parts_fold(all, x);
        }
        PartsPair run = parts_fold(before, excl);
#pragma unroll
        for (u32 i = 0; i < kScanPer; ++i) {
            if (first + i < n) records[first + i].sum = run.s;
            run = parts_fold(run, v[i]);
        }
        carry = all;
        __syncthreads(); // the next round's wave totals
    }
}

// load_block with the starts beside it: `heads` gets bit t where the lane's row of step t starts a partition
template <u32 kSteps>
__device__ __forceinline__ u32 load_block_parts(const u32 *s_rows, const u32 *sel, const u32 *st, u32 n_slices_val, u32 blk, u32 lane, u32 (&v)[kSteps],
                                                u32 &heads) {
    u32 row0 = (u32)kCumsumBlockRows * blk + lane;
    asm volatile("" : "+v"(row0)); // (opaque, as in load_block)
    u32 picked = 0u, hd = 0u;
#pragma unroll
    for (u32 t = 0; t < kSteps; ++t) {
        const u32 r = row0 + 64u * t;
        const u32 bit = (sel[r / 31u] >> (r % 31u)) & 1u;
        picked |= bit << t;
        hd |= ((st[r / 31u] >> (r % 31u)) & 1u) << t;
        v[t] = n_slices_val == 0u ? bit : s_rows[r] & (0u - bit); // (wave-uniform choice)
    }
    heads = hd;
    return picked;
}

// block blk's pair (wave-uniform): whether it holds a start, and the sum of its selected values at or behind its last one
template <u32 kSteps>
__device__ __forceinline__ PartsPair block_pair(const u32 *s_rows, const u32 *sel, const u32 *st, u32 n_slices_val, u32 blk, u32 lane) {
    u32 v[kSteps], heads;
    load_block_parts<kSteps>(s_rows, sel, st, n_slices_val, blk, lane, v, heads);
    // 1 + the block row (64 t + lane) of the lane's last start
    u32 last = heads != 0u ? 64u * (31u - (u32)__clz(heads)) + lane + 1u : 0u;
    last = (u32)__builtin_amdgcn_readlane((int)wave_scan_max32(last), 63);
    const u32 first = last != 0u ? last - 1u : 0u;
    u64 sum = 0;
#pragma unroll
    for (u32 t = 0; t < kSteps; ++t) sum += 64u * t + lane >= first ? v[t] : 0u;
    return {uniform64(wave_sum(sum)), last != 0u ? 1u : 0u};
}

// scan_block with the starts: a step without a head is scan_block's
template <u32 kSteps, bool kWide, bool kHigh>
__device__ __forceinline__ void scan_block_parts(const BsiCumsumArgs &a, const u32 *s_rows, const u32 *sel, const u32 *st, u64 seg, u32 rows, u32 blk,
                                                 u32 lane, u64 base) {
    u32 lo[kSteps], hi[kSteps];
    u32 have = 0u; // lane j: word j of the block's selection
    {
        u32 v[kSteps], heads;
        const u32 picked = load_block_parts<kSteps>(s_rows, sel, st, a.n_slices_val, blk, lane, v, heads);
        const u32 row0 = (u32)kCumsumBlockRows * blk + lane;
        const u64 le = ~0ull >> (63u - lane); // the lanes at or in front of this one
        u64 carry = base; // the sum in front of the step since the last start (wave-uniform)
#pragma unroll
        for (u32 t = 0; t < kSteps; ++t) {
            const u32 x = v[t];
            const u64 s = kWide ? (u64)wave_scan_incl32(x & 0xFFFFu) + ((u64)wave_scan_incl32(x >> 16) << 16) : (u64)wave_scan_incl32(x);
            const u64 hm = __ballot(((heads >> t) & 1u) != 0u);
            u64 r;
            if (hm == 0ull) { // (wave-uniform)
                r = carry + s - (a.exclusive != 0u ? x : 0u);
                carry += ((u64)(kWide ? (u32)__builtin_amdgcn_readlane((int)(u32)(s >> 32), 63) : 0u) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)s, 63);
            } else {
                const u64 e = s - x; // the exclusive scan
                const u64 mine = hm & le;
                const u32 hl = 63u - (u32)__clzll((long long)(mine | 1ull)); // the lane's head lane (lane 0 where it has none: not used)
                const u64 eh = ((u64)(kWide ? (u32)__builtin_amdgcn_ds_bpermute((int)(4u * hl), (int)(u32)(e >> 32)) : 0u) << 32) |
                               (u32)__builtin_amdgcn_ds_bpermute((int)(4u * hl), (int)(u32)e);
                r = (mine != 0ull ? s - eh : carry + s) - (a.exclusive != 0u ? x : 0u);
                const int hlast = 63 - (int)__clzll((long long)hm); // (scalar)
                const u64 s63 = ((u64)(kWide ? (u32)__builtin_amdgcn_readlane((int)(u32)(s >> 32), 63) : 0u) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)s, 63);
                const u64 el = ((u64)(kWide ? (u32)__builtin_amdgcn_readlane((int)(u32)(e >> 32), hlast) : 0u) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)e, hlast);
                carry = s63 - el;
            }
            const bool on = ((picked >> t) & 1u) != 0u;
            if (!((on || a.all_rows != 0u) && row0 + 64u * t < rows)) r = 0ull;
            lo[t] = (u32)r;
            hi[t] = (u32)(r >> 32);
            const u64 m = __ballot(on);
            have = put_lane((u32)m, 2u * t, have);
            have = put_lane((u32)(m >> 32), 2u * t + 1u, have);
        }
    }
    const bool store = lane < 2u * kSteps; // (the half block: 32 words)
    u32 *out = a.matrix + (seg * kSegWords + kCumsumBlockWords * blk + lane); // row 0 of the matrix; every row is n_words further
    u32 b = a.n_slices_out;
    if (kHigh) {
#pragma nounroll
        for (; b > 32u; --b) {
            const u32 w = slice_words(hi, 1u << (b - 33u));
            if (store) *out = w;
            out += a.n_words;
        }
    }
#pragma nounroll
    for (; b > 0u; --b) {
        const u32 w = slice_words(lo, 1u << (b - 1u));
        if (store) *out = w;
        out += a.n_words;
    }
    if (a.all_rows == 0u && store) *out = have;
}

template <bool kWide, bool kHigh>
__global__ __launch_bounds__(kCumsumWaves * 64) void cumsum_parts_rows_kernel(const BsiCumsumPartsArgs pa) {
    __shared__ __attribute__((aligned(16))) u32 s_rows[kSegBits];
    __shared__ __attribute__((aligned(16))) u32 s_acc[kCumsumWaves][kSegGroups];
    __shared__ u64 s_block[kCumsumBlocks];
    __shared__ u32 s_block_f[kCumsumBlocks];
    const BsiCumsumArgs &a = pa.c;
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    const u32 *sel = s_acc[kCumsumSliceWaves];
    const u32 *st = s_acc[kPartsStartsWave];
    const u32 nv = a.n_slices_val;
    const u32 per = (nv + kPartsSliceWaves - 1u) / kPartsSliceWaves; // the value's slices shared among six wavefronts
    const u32 w_lo = min(wave * per, nv), w_hi = wave < kPartsSliceWaves ? min(w_lo + per, nv) : w_lo;
    const bool last_half = wave + kCumsumWaves == kCumsumBlocks - 1u; // (wave-uniform: the wavefront whose second block is the half one)

#pragma nounroll
    for (u64 seg = blockIdx.x; seg < a.n_segments; seg += gridDim.x) { // (workgroup-uniform)
        const u32 nvalid = segment_groups(a.groups, seg);
        const u32 rows = segment_rows(a.n_rows, seg);

        if (nv != 0u) // (without value slices the rows' words are never read)
            for (u32 p = threadIdx.x * 4u; p < kSegBits; p += kCumsumWaves * 64u * 4u) *reinterpret_cast<uint4 *>(s_rows + p) = make_uint4(0u, 0u, 0u, 0u);
        if (wave < kCumsumSliceWaves)
            image_fill(acc, 0u, lane);
        else
            selection_preset(acc, a.n_rows, seg, nvalid, lane);
        __syncthreads();

        if (wave < kPartsSliceWaves) {
            if (w_lo < w_hi) // (wave-uniform)
                walk_slices(a, w_lo, w_hi, seg, nvalid, acc, lane, [&](u32 sig) { fold_slice_bits(acc, s_rows, 0u, kSegGroups / 64u, sig, lane); });
        } else if (wave == kPartsStartsWave) {
            starts_walk(pa, acc, seg, nvalid, rows, lane);
        } else {
            selection_walk(a, acc, seg, nvalid, lane);
        }
        __syncthreads();

        {
            const PartsPair t0 = block_pair<kCumsumBlockSteps>(s_rows, sel, st, nv, wave, lane);
            const PartsPair t1 = last_half ? block_pair<kCumsumBlockSteps / 2u>(s_rows, sel, st, nv, kCumsumBlocks - 1u, lane)
                                           : block_pair<kCumsumBlockSteps>(s_rows, sel, st, nv, wave + kCumsumWaves, lane);
            if (lane == 0) {
                s_block[wave] = t0.s;
                s_block_f[wave] = t0.f;
                s_block[wave + kCumsumWaves] = t1.s;
                s_block_f[wave + kCumsumWaves] = t1.f;
            }
        }
        __syncthreads();

        u64 base = pa.records[seg].sum; // (scanned: what flows into the segment)
#pragma nounroll
        for (u32 b = 0; b < wave; ++b) base = s_block_f[b] != 0u ? s_block[b] : base + s_block[b];
        base = uniform64(base);
        scan_block_parts<kCumsumBlockSteps, kWide, kHigh>(a, s_rows, sel, st, seg, rows, wave, lane, base);
#pragma nounroll
        for (u32 b = wave; b < wave + kCumsumWaves; ++b) base = s_block_f[b] != 0u ? s_block[b] : base + s_block[b];
        base = uniform64(base);
        if (last_half)
            scan_block_parts<kCumsumBlockSteps / 2u, kWide, kHigh>(a, s_rows, sel, st, seg, rows, kCumsumBlocks - 1u, lane, base);
        else
            scan_block_parts<kCumsumBlockSteps, kWide, kHigh>(a, s_rows, sel, st, seg, rows, wave + kCumsumWaves, lane, base);
        __syncthreads(); // the next segment clears the rows and the images
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_bsi_total_parts_indexed_device: the partition's TOTAL in every one of its rows -- `SUM(x) OVER (PARTITION BY g)` without an
// ORDER BY.  A row's total is the running sum at its partition's last row, so what the kernels above send forward has to come
// back: the frame stays (three launches, no workgroup waits for another), every level keeps TWO sums beside has_start,
//   head  the selected values in front of the first start (the whole item where it holds none): what it gives to the partition
//         that is open in front of it,
//   tail  the selected values at or behind the last start (the whole item likewise): what it gives to the one open behind it,
// and is folded in both directions -- forward with the operator above on (has_start, tail), backward with its mirror on
// (has_start, head): what flows in from BEHIND an item is the heads of the items behind it up to and including the first that
// holds a start.
// total_parts_records_kernel  cumsum_parts_totals_kernel with two masks: wavefront 7 finds the first and the last start of the starts
//             row and leaves them in LDS, the selection stays whole, and every popcount is taken twice, under "rows in front of
//             the first start" and under "rows at or behind the last start".  A record (head, tail, has_start) per segment, EVERY
//             segment's.
// total_parts_scan_kernel     ONE workgroup, both directions one after the other: cumsum_parts_scan_kernel's rounds over the tails
//             from the front, then the same rounds over the heads from the end (entry k of a round is record n - 1 - k, so the
//             short round is the last one and the carry pair crosses the same seams mirrored).  `tail` becomes what flows into
//             the segment from the front, `head` what flows into it from behind.
// total_parts_rows_kernel     cumsum_parts_rows_kernel's frame and footprint with a triple per block.  Per block the forward base is
//             folded as there, the backward inflow from the heads of the blocks behind it (and the segment's where none of them
//             holds a start).  The forward pass is the inclusive step above and leaves the segmented running sum r of every
//             row in the two register arrays.  The backward pass walks the steps from the last to the first with a wave-uniform
//             `after`, the total of the partition that is open at the step's end: a lane's total is r at the lane in front of
//             the next head behind it in the step (one ds_bpermute per word) and `after` where there is none; behind a step
//             with a first head at lane f, `after` is r[t][f - 1], for f = 0 r[t - 1][63], at t = 0 the block's forward base.
//             A step without a head is one select.  Then clip, transpose and store as above.
static_assert((kSegBits + kCumsumWaves * kSegGroups) * sizeof(u32) + kCumsumBlocks * (2u * sizeof(u64) + sizeof(u32)) <= 160u * 1024u,
              "one workgroup fits a CU's LDS");

__global__ __launch_bounds__(kCumsumWaves * 64) void total_parts_records_kernel(const BsiTotalPartsArgs ta) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kCumsumWaves][kSegGroups];
    __shared__ u64 s_head[kCumsumWaves];
    __shared__ u64 s_tail[kCumsumWaves];
    __shared__ u32 s_bound[2];
    const BsiCumsumPartsArgs &a = ta.p;
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    const u32 *sel = s_acc[kCumsumSliceWaves];
    u32 w_lo, w_hi;
    slice_share(a.c.n_slices_val, wave, w_lo, w_hi);

#pragma nounroll
    for (u64 seg = blockIdx.x; seg < a.c.n_segments; seg += gridDim.x) { // (workgroup-uniform)
        const u32 nvalid = segment_groups(a.c.groups, seg);
        image_fill(acc, 0u, lane);
        if (wave == kCumsumSliceWaves) {
            const u32 rows = segment_rows(a.c.n_rows, seg);
            starts_walk(a, acc, seg, nvalid, rows, lane);
            u32 last = 0u; // 1 + the last start among the lane's groups, 0: none
            u32 near = 0u; // 32768 - the first start among them, 0: none
#pragma unroll
            for (u32 i = 0; i < kSegGroups / 64u; ++i) {
                const u32 g = 64u * i + lane, w = acc[g];
                if (w != 0u) {
                    last = 31u * g + 32u - (u32)__clz(w);
                    if (near == 0u) near = 32768u - (31u * g + (u32)__builtin_ctz(w));
                }
            }
            last = (u32)__builtin_amdgcn_readlane((int)wave_scan_max32(last), 63);
            near = (u32)__builtin_amdgcn_readlane((int)wave_scan_max32(near), 63);
            if (lane == 0) {
                ta.records[seg].has_start = last != 0u ? 1ull : 0ull;
                s_bound[0] = near != 0u ? 32768u - near : 31u * kSegGroups; // the rows in front of here are the segment's head
                s_bound[1] = last != 0u ? last - 1u : 0u;                   // the rows from here on are its tail
            }
            selection_preset(acc, a.c.n_rows, seg, nvalid, lane);
            selection_walk(a.c, acc, seg, nvalid, lane);
        }
        __syncthreads();

        const u32 head_to = s_bound[0], tail_from = s_bound[1];
        u64 sum_h = 0, sum_t = 0; // the lane's share of the wavefront's
        auto count = [&](u32 sig) { // the image's set bits among the selected rows of the head and of the tail, at weight 2^sig
            u32 ch = 0, ct = 0;
#pragma unroll
            for (u32 i = 0; i < kSegGroups / 64u; ++i) {
                const u32 g = 64u * i + lane;
                const u32 m = (wave < kCumsumSliceWaves ? acc[g] : kOnes31) & sel[g];
                ch += (u32)__popc(m & (g < head_to / 31u ? kOnes31 : g == head_to / 31u ? (1u << (head_to % 31u)) - 1u : 0u));
                ct += (u32)__popc(m & (g < tail_from / 31u ? 0u : g == tail_from / 31u ? (kOnes31 << (tail_from % 31u)) & kOnes31 : kOnes31));
            }
            sum_h += (u64)ch << sig;
            sum_t += (u64)ct << sig;
        };
        if (wave < kCumsumSliceWaves) {
            if (w_lo < w_hi) walk_slices(a.c, w_lo, w_hi, seg, nvalid, acc, lane, count); // (wave-uniform)
        } else if (a.c.n_slices_val == 0u) {
            count(0u);
        }
        sum_h = wave_sum(sum_h);
        sum_t = wave_sum(sum_t);
        if (lane == 0) {
            s_head[wave] = sum_h;
            s_tail[wave] = sum_t;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 head = 0, tail = 0;
#pragma unroll
            for (u32 w = 0; w < kCumsumWaves; ++w) {
                head += s_head[w];
                tail += s_tail[w];
            }
            ta.records[seg].head = head;
            ta.records[seg].tail = tail;
        }
        // (no third barrier, as above: the bounds were read behind the first barrier, wavefront 7 writes the next ones behind this one)
    }
}

// One direction of the scan.  kBack false: records[i].tail becomes the fold of (has_start, tail) of records[0 .. i); true: entry k
// is record n - 1 - k, and records[i].head becomes the fold of (has_start, head) of the records behind i, the nearest last.
template <bool kBack>
__device__ __forceinline__ void total_parts_scan_pass(BsiTotalPartsRecord *records, u64 n, u64 *s_wave_s, u32 *s_wave_f, u32 wave, u32 lane) {
    PartsPair carry = {0ull, 0u}; // the fold of the rounds done (workgroup-uniform)
#pragma nounroll
    for (u64 i0 = 0; i0 < n; i0 += (u64)kScanWaves * 64u * kScanPer) {
        const u64 first = i0 + (u64)threadIdx.x * kScanPer;
        PartsPair v[kScanPer], mine = {0ull, 0u};
#pragma unroll
        for (u32 i = 0; i < kScanPer; ++i) {
            v[i] = {0ull, 0u};
            if (first + i < n) {
                const BsiTotalPartsRecord &r = records[kBack ? n - 1u - (first + i) : first + i];
                v[i] = {kBack ? r.head : r.tail, (u32)r.has_start};
            }
            mine = parts_fold(mine, v[i]);
        }
        PartsPair incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const PartsPair t = {__shfl_up(incl.s, off), (u32)__shfl_up((int)incl.f, off)};
            if (lane >= (u32)off) incl = parts_fold(t, incl);
        }
        if (lane == 63u) {
            s_wave_s[wave] = incl.s;
            s_wave_f[wave] = incl.f;
        }
        PartsPair excl = {__shfl_up(incl.s, 1), (u32)__shfl_up((int)incl.f, 1)};
        if (lane == 0u) excl = {0ull, 0u};
        __syncthreads();
        PartsPair before = carry, all = carry;
#pragma unroll
        for (u32 w = 0; w < kScanWaves; ++w) {
            const PartsPair x = {s_wave_s[w], s_wave_f[w]};
            if (w < wave) before = parts_fold(before, x);
            all = parts_fold(all, x);
        }
        PartsPair run = parts_fold(before, excl);
#pragma unroll
        for (u32 i = 0; i < kScanPer; ++i) {
            if (first + i < n) {
                BsiTotalPartsRecord &r = records[kBack ? n - 1u - (first + i) : first + i];
                if (kBack)
                    r.head = run.s;
                else
                    r.tail = run.s;
            }
            run = parts_fold(run, v[i]);
        }
        carry = all;
        __syncthreads(); // the next round's wave totals
    }
}

__global__ __launch_bounds__(kScanWaves * 64) void total_parts_scan_kernel(BsiTotalPartsRecord *records, u64 n) {
    __shared__ u64 s_wave_s[kScanWaves];
    __shared__ u32 s_wave_f[kScanWaves];
    const u32 wave = wave_id(), lane = lane_id();
    total_parts_scan_pass<false>(records, n, s_wave_s, s_wave_f, wave, lane);
    total_parts_scan_pass<true>(records, n, s_wave_s, s_wave_f, wave, lane); // (other fields: a thread reads what it wrote itself or nobody wrote)
}

struct TotalTriple {
    u64 head, tail;
    u32 f;
};

// block blk's triple (wave-uniform): whether it holds a start, the sum of its selected values in front of its first one and at or
// behind its last one
template <u32 kSteps>
__device__ __forceinline__ TotalTriple block_triple(const u32 *s_rows, const u32 *sel, const u32 *st, u32 n_slices_val, u32 blk, u32 lane) {
    u32 v[kSteps], heads;
    load_block_parts<kSteps>(s_rows, sel, st, n_slices_val, blk, lane, v, heads);
    u32 last = heads != 0u ? 64u * (31u - (u32)__clz(heads)) + lane + 1u : 0u;         // 1 + the block row of the lane's last start
    u32 near = heads != 0u ? 4096u - (64u * (u32)__builtin_ctz(heads) + lane) : 0u;    // 4096 - the block row of its first one
    last = (u32)__builtin_amdgcn_readlane((int)wave_scan_max32(last), 63);
    near = (u32)__builtin_amdgcn_readlane((int)wave_scan_max32(near), 63);
    const u32 tail_from = last != 0u ? last - 1u : 0u, head_to = near != 0u ? 4096u - near : 64u * kSteps;
    u64 head = 0, tail = 0;
#pragma unroll
    for (u32 t = 0; t < kSteps; ++t) {
        head += 64u * t + lane < head_to ? v[t] : 0u;
        tail += 64u * t + lane >= tail_from ? v[t] : 0u;
    }
    return {uniform64(wave_sum(head)), uniform64(wave_sum(tail)), last != 0u ? 1u : 0u};
}

// Block blk of segment seg: the totals of the partitions its rows lie in, stored as 2 kSteps words of every result row.  base: the
// running sum in front of the block since the last start; back: what flows into the block from behind.
template <u32 kSteps, bool kWide, bool kHigh>
__device__ __forceinline__ void total_block(const BsiCumsumArgs &a, const u32 *s_rows, const u32 *sel, const u32 *st, u64 seg, u32 rows, u32 blk, u32 lane,
                                            u64 base, u64 back) {
    u32 lo[kSteps], hi[kSteps];
    u32 picked, heads;
    const u64 le = ~0ull >> (63u - lane); // the lanes at or in front of this one
    u64 carry = base; // the sum in front of the step since the last start (wave-uniform)
    {
        // the forward pass: scan_block_parts' step, inclusive, for every row whether selected or not
        u32 v[kSteps];
        picked = load_block_parts<kSteps>(s_rows, sel, st, a.n_slices_val, blk, lane, v, heads);
#pragma unroll
        for (u32 t = 0; t < kSteps; ++t) {
            const u32 x = v[t];
            const u64 s = kWide ? (u64)wave_scan_incl32(x & 0xFFFFu) + ((u64)wave_scan_incl32(x >> 16) << 16) : (u64)wave_scan_incl32(x);
            const u64 hm = __ballot(((heads >> t) & 1u) != 0u);
            u64 r;
            if (hm == 0ull) { // (wave-uniform)
                r = carry + s;
                carry += ((u64)(kWide ? (u32)__builtin_amdgcn_readlane((int)(u32)(s >> 32), 63) : 0u) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)s, 63);
            } else {
                const u64 e = s - x; // the exclusive scan
                const u64 mine = hm & le;
                const u32 hl = 63u - (u32)__clzll((long long)(mine | 1ull)); // the lane's head lane (lane 0 where it has none: not used)
                const u64 eh = ((u64)(kWide ? (u32)__builtin_amdgcn_ds_bpermute((int)(4u * hl), (int)(u32)(e >> 32)) : 0u) << 32) |
                               (u32)__builtin_amdgcn_ds_bpermute((int)(4u * hl), (int)(u32)e);
                r = mine != 0ull ? s - eh : carry + s;
                const int hlast = 63 - (int)__clzll((long long)hm); // (scalar)
                const u64 s63 = ((u64)(kWide ? (u32)__builtin_amdgcn_readlane((int)(u32)(s >> 32), 63) : 0u) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)s, 63);
                const u64 el = ((u64)(kWide ? (u32)__builtin_amdgcn_readlane((int)(u32)(e >> 32), hlast) : 0u) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)e, hlast);
                carry = s63 - el;
            }
            lo[t] = (u32)r;
            hi[t] = (u32)(r >> 32);
        }
    }
    // the backward pass: `after` is the total of the partition that is open at the step's end (wave-uniform; the carry is now the
    // running sum at the block's last row)
    u64 after = carry + back;
    u32 have = 0u; // lane j: word j of the block's selection
    const u32 row0 = (u32)kCumsumBlockRows * blk + lane;
#pragma unroll
    for (u32 i = 0; i < kSteps; ++i) {
        const u32 t = kSteps - 1u - i;
        const u64 hm = __ballot(((heads >> t) & 1u) != 0u);
        u32 tl = (u32)after, th = (u32)(after >> 32);
        if (hm != 0ull) { // (wave-uniform)
            const u64 behind = hm & ~le; // the heads behind this lane
            const u32 src = behind != 0ull ? (u32)__builtin_ctzll(behind) - 1u : lane; // the lane in front of the next one
            const u32 gl = (u32)__builtin_amdgcn_ds_bpermute((int)(4u * src), (int)lo[t]);
            const u32 gh = kHigh ? (u32)__builtin_amdgcn_ds_bpermute((int)(4u * src), (int)hi[t]) : 0u;
            if (behind != 0ull) {
                tl = gl;
                th = gh;
            }
            const int f = (int)__builtin_ctzll(hm); // the step's first head (scalar)
            if (f > 0)
                after = ((u64)(kHigh ? (u32)__builtin_amdgcn_readlane((int)hi[t], f - 1) : 0u) << 32) | (u32)__builtin_amdgcn_readlane((int)lo[t], f - 1);
            else if (t > 0u)
                after = ((u64)(kHigh ? (u32)__builtin_amdgcn_readlane((int)hi[t > 0u ? t - 1u : 0u], 63) : 0u) << 32) |
                        (u32)__builtin_amdgcn_readlane((int)lo[t > 0u ? t - 1u : 0u], 63);
            else
                after = base;
        }
        const bool on = ((picked >> t) & 1u) != 0u;
        if (!((on || a.all_rows != 0u) && row0 + 64u * t < rows)) tl = th = 0u;
        lo[t] = tl;
        hi[t] = th;
        const u64 m = __ballot(on);
        have = put_lane((u32)m, 2u * t, have);
        have = put_lane((u32)(m >> 32), 2u * t + 1u, have);
    }
    const bool store = lane < 2u * kSteps; // (the half block: 32 words)
    u32 *out = a.matrix + (seg * kSegWords + kCumsumBlockWords * blk + lane); // row 0 of the matrix; every row is n_words further
    u32 b = a.n_slices_out;
    if (kHigh) {
#pragma nounroll
        for (; b > 32u; --b) {
            const u32 w = slice_words(hi, 1u << (b - 33u));
            if (store) *out = w;
            out += a.n_words;
        }
    }
#pragma nounroll
    for (; b > 0u; --b) {
        const u32 w = slice_words(lo, 1u << (b - 1u));
        if (store) *out = w;
        out += a.n_words;
    }
    if (a.all_rows == 0u && store) *out = have;
}

template <bool kWide, bool kHigh>
__global__ __launch_bounds__(kCumsumWaves * 64) void total_parts_rows_kernel(const BsiTotalPartsArgs ta) {
    __shared__ __attribute__((aligned(16))) u32 s_rows[kSegBits];
    __shared__ __attribute__((aligned(16))) u32 s_acc[kCumsumWaves][kSegGroups];
    __shared__ u64 s_block[kCumsumBlocks];   // tails
    __shared__ u64 s_block_h[kCumsumBlocks]; // heads
    __shared__ u32 s_block_f[kCumsumBlocks];
    const BsiCumsumPartsArgs &pa = ta.p;
    const BsiCumsumArgs &a = pa.c;
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    const u32 *sel = s_acc[kCumsumSliceWaves];
    const u32 *st = s_acc[kPartsStartsWave];
    const u32 nv = a.n_slices_val;
    const u32 per = (nv + kPartsSliceWaves - 1u) / kPartsSliceWaves; // the value's slices shared among six wavefronts
    const u32 w_lo = min(wave * per, nv), w_hi = wave < kPartsSliceWaves ? min(w_lo + per, nv) : w_lo;
    const bool last_half = wave + kCumsumWaves == kCumsumBlocks - 1u; // (wave-uniform: the wavefront whose second block is the half one)

#pragma nounroll
    for (u64 seg = blockIdx.x; seg < a.n_segments; seg += gridDim.x) { // (workgroup-uniform)
        const u32 nvalid = segment_groups(a.groups, seg);
        const u32 rows = segment_rows(a.n_rows, seg);

        if (nv != 0u) // (without value slices the rows' words are never read)
            for (u32 p = threadIdx.x * 4u; p < kSegBits; p += kCumsumWaves * 64u * 4u) *reinterpret_cast<uint4 *>(s_rows + p) = make_uint4(0u, 0u, 0u, 0u);
        if (wave < kCumsumSliceWaves)
            image_fill(acc, 0u, lane);
        else
            selection_preset(acc, a.n_rows, seg, nvalid, lane);
        __syncthreads();

        if (wave < kPartsSliceWaves) {
            if (w_lo < w_hi) // (wave-uniform)
                walk_slices(a, w_lo, w_hi, seg, nvalid, acc, lane, [&](u32 sig) { fold_slice_bits(acc, s_rows, 0u, kSegGroups / 64u, sig, lane); });
        } else if (wave == kPartsStartsWave) {
            starts_walk(pa, acc, seg, nvalid, rows, lane);
        } else {
            selection_walk(a, acc, seg, nvalid, lane);
        }
        __syncthreads();

        {
            const TotalTriple t0 = block_triple<kCumsumBlockSteps>(s_rows, sel, st, nv, wave, lane);
            const TotalTriple t1 = last_half ? block_triple<kCumsumBlockSteps / 2u>(s_rows, sel, st, nv, kCumsumBlocks - 1u, lane)
                                             : block_triple<kCumsumBlockSteps>(s_rows, sel, st, nv, wave + kCumsumWaves, lane);
            if (lane == 0) {
                s_block[wave] = t0.tail;
                s_block_h[wave] = t0.head;
                s_block_f[wave] = t0.f;
                s_block[wave + kCumsumWaves] = t1.tail;
                s_block_h[wave + kCumsumWaves] = t1.head;
                s_block_f[wave + kCumsumWaves] = t1.f;
            }
        }
        __syncthreads();

        // what flows into the wavefront's two blocks from behind: the heads of the blocks behind up to the first with a start
        u64 back = ta.records[seg].head; // (scanned: what flows into the segment from behind)
#pragma nounroll
        for (u32 b = kCumsumBlocks - 1u; b > wave + kCumsumWaves; --b) back = s_block_f[b] != 0u ? s_block_h[b] : back + s_block_h[b];
        const u64 back1 = uniform64(back);
#pragma nounroll
        for (u32 b = wave + kCumsumWaves; b > wave; --b) back = s_block_f[b] != 0u ? s_block_h[b] : back + s_block_h[b];
        const u64 back0 = uniform64(back);

        u64 base = ta.records[seg].tail; // (scanned: what flows into the segment from the front)
#pragma nounroll
        for (u32 b = 0; b < wave; ++b) base = s_block_f[b] != 0u ? s_block[b] : base + s_block[b];
        base = uniform64(base);
        total_block<kCumsumBlockSteps, kWide, kHigh>(a, s_rows, sel, st, seg, rows, wave, lane, base, back0);
#pragma nounroll
        for (u32 b = wave; b < wave + kCumsumWaves; ++b) base = s_block_f[b] != 0u ? s_block[b] : base + s_block[b];
        base = uniform64(base);
        if (last_half)
            total_block<kCumsumBlockSteps / 2u, kWide, kHigh>(a, s_rows, sel, st, seg, rows, kCumsumBlocks - 1u, lane, base, back1);
        else
            total_block<kCumsumBlockSteps, kWide, kHigh>(a, s_rows, sel, st, seg, rows, wave + kCumsumWaves, lane, base, back1);
        __syncthreads(); // the next segment clears the rows and the images
    }
}

} // namespace

hipError_t launch_bsi_total_parts(const BsiTotalPartsArgs &a, hipStream_t s) {
    const BsiCumsumArgs &c = a.p.c;
    if (c.n_segments == 0) return hipSuccess;
    const dim3 grid((unsigned)(c.n_segments < kCumsumGridItems ? c.n_segments : kCumsumGridItems)), block(kCumsumWaves * 64);
    hipLaunchKernelGGL(total_parts_records_kernel, grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(total_parts_scan_kernel, dim3(1), dim3(kScanWaves * 64), 0, s, a.records, c.n_segments);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const bool wide = c.n_slices_val > kCumsumNarrowBits, high = c.n_slices_out > 32u;
    if (wide && high)
        hipLaunchKernelGGL((total_parts_rows_kernel<true, true>), grid, block, 0, s, a);
    else if (wide)
        hipLaunchKernelGGL((total_parts_rows_kernel<true, false>), grid, block, 0, s, a);
    else if (high)
        hipLaunchKernelGGL((total_parts_rows_kernel<false, true>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((total_parts_rows_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_bsi_cumsum_parts(const BsiCumsumPartsArgs &a, hipStream_t s) {
    if (a.c.n_segments == 0) return hipSuccess;
    const dim3 grid((unsigned)(a.c.n_segments < kCumsumGridItems ? a.c.n_segments : kCumsumGridItems)), block(kCumsumWaves * 64);
    hipLaunchKernelGGL(cumsum_parts_totals_kernel, grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cumsum_parts_scan_kernel, dim3(1), dim3(kScanWaves * 64), 0, s, a.records, a.c.n_segments);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const bool wide = a.c.n_slices_val > kCumsumNarrowBits, high = a.c.n_slices_out > 32u;
    if (wide && high)
        hipLaunchKernelGGL((cumsum_parts_rows_kernel<true, true>), grid, block, 0, s, a);
    else if (wide)
        hipLaunchKernelGGL((cumsum_parts_rows_kernel<true, false>), grid, block, 0, s, a);
    else if (high)
        hipLaunchKernelGGL((cumsum_parts_rows_kernel<false, true>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((cumsum_parts_rows_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_bsi_cumsum(const BsiCumsumArgs &a, hipStream_t s) {
    if (a.n_segments == 0) return hipSuccess;
    const dim3 grid((unsigned)(a.n_segments < kCumsumGridItems ? a.n_segments : kCumsumGridItems)), block(kCumsumWaves * 64);
    hipLaunchKernelGGL(cumsum_totals_kernel, grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cumsum_scan_kernel, dim3(1), dim3(kScanWaves * 64), 0, s, a.totals, a.n_segments);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const bool wide = a.n_slices_val > kCumsumNarrowBits, high = a.n_slices_out > 32u;
    if (wide && high)
        hipLaunchKernelGGL((cumsum_rows_kernel<true, true>), grid, block, 0, s, a);
    else if (wide)
        hipLaunchKernelGGL((cumsum_rows_kernel<true, false>), grid, block, 0, s, a);
    else if (high)
        hipLaunchKernelGGL((cumsum_rows_kernel<false, true>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((cumsum_rows_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

} // namespace wah
