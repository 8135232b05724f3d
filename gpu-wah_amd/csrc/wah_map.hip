// wah_map.hip -- wah_bsi_map_indexed_device: a BIT-SLICED key pushed through a lookup table key -> value in device memory, the
// looked-up value leaving as a NEW bit-sliced attribute: the star join's projection (`SELECT d.x FROM f JOIN d ON f.fk = d.rowid`
// as an attribute of f), a unary function of a small-domain key tabulated once, a dictionary recoding.  No value column is written
// and read again: what moves is the key's compressed slices in and the result's decoded slice matrix out, which the compress
// passes turn into the index as they do the builder's (wah_bsi_build.hip).
//
// bsi_map_segments_kernel: group_by_items_kernel's frame in its count-only layout (wah_group_by.hip) -- one WORKGROUP of eight
// wavefronts per segment, a grid of capped size striding over the segments, s_rows[kSegBits] plus eight images: 159 744 bytes of
// LDS, one workgroup per CU -- with bsi_slices_kernel's transpose (wah_slice_words.hpp) where that kernel adds into buckets.
//   fold      wavefronts 0 .. 6 walk their share of the key's slices with list_walk under OR, one row at a time in the zeroed
//             image, and fold it with fold_slice_bits into the key word of each of the segment's 31 744 rows in s_rows.
//             Wavefront 7 makes the SELECTION image: all ones clipped to segment_groups / segment_rows(n_rows), the key's
//             existence row walked into it under AND.
//   lookup    behind the barrier.  A segment's 31 744 rows are exactly 992 words of every result slice: 15 blocks of 2048 rows
//             (64 words) and one HALF block of 1024 rows (32 words).  Wavefront w takes blocks w and w + 8.  For a block, lane
//             l of step t (32 steps, 16 in the half block) owns row r = 2048 blk + 64 t + l: its key word is s_rows[r]
//             (consecutive lanes, consecutive banks), its selection bit is bit r % 31 of word r / 31 of wavefront 7's image.  THE
//             TABLE LOADS OF kMapChunk STEPS ARE ISSUED BEFORE THE FIRST ONE IS USED (resolve_buckets' shape): one bounds test and
//             one 4-byte load per selected row, nothing loaded for a row that is not selected, nothing read at or behind n_keys.
//             The block's values stay in statically indexed registers; a row without a value holds 0.
//   transpose a RUNTIME loop over the result's slices, most significant first: slice_words(v, 1u << b) -- the ballots of the
//             steps put by v_writelane into one accumulator -- and one store of 256 contiguous bytes (128 in the half block) to
//             matrix row i, word 992 seg + 64 blk + lane.  The ballots of "has a value" are the existence row.
// Every word of every result row is written exactly once: the matrix needs no clearing.  Nothing goes back to LDS behind the
// barrier -- the values are in the registers the ballots read, and an LDS image of the result would be written and read once for
// nothing -- and no register array is indexed by a runtime value.  Misses (an existing row whose key is at or behind n_keys or
// whose entry is kMapNull; refused unless the call is partial) and entries with a bit at or above n_slices_out are ORed into one
// register and reported once per wavefront at the end, by one lane, with the atomicOr the builder uses.
#include "wah_fold_bits.hpp"
#include "wah_slice_words.hpp"

namespace wah {
namespace {

constexpr u32 kMapGridItems = 512;  // workgroups of bsi_map_segments_kernel at the most (two per CU: one resident, one waiting)
constexpr u32 kMapWaves = 8;        // wavefronts of a workgroup
constexpr u32 kMapSliceWaves = kMapWaves - 1u;  // ... that walk slices; the last one walks the existence row
constexpr u32 kMapChunk = 8;        // steps whose table loads are in flight together
constexpr u32 kMapNull = 0xFFFFFFFFu; // WAH_MAP_NULL: an entry without a value, and what a row that loads nothing holds
constexpr u32 kMapBlockWords = 64; // slice words per block: one per lane (bsi_slices_kernel's block)
constexpr u32 kMapBlockSteps = 32; // steps of 64 rows per block
constexpr u32 kMapBlockRows = 2048; // 32 * kMapBlockWords
constexpr u32 kMapBlocks = 16;      // blocks of a segment: 15 of kMapBlockRows rows and a half one
static_assert((kSegBits + kMapWaves * kSegGroups) * sizeof(u32) <= 160u * 1024u, "one workgroup fits a CU's LDS");
static_assert((kMapBlocks - 1u) * kMapBlockRows + kMapBlockRows / 2u == kSegBits && (kMapBlocks - 1u) * kMapBlockWords + kMapBlockWords / 2u == kSegWords,
              "a segment: fifteen blocks and a half");
static_assert(kMapBlocks == 2u * kMapWaves && kMapBlockSteps % kMapChunk == 0u && (kMapBlockSteps / 2u) % kMapChunk == 0u, "two blocks per wavefront, whole chunks");

// Block blk of segment seg: kSteps steps of 64 rows (32, or 16 in the half block) looked up and stored as 2 kSteps words of every
// result row.  bad: the wavefront's register of refusals.
template <u32 kSteps>
__device__ __forceinline__ void map_block(const BsiMapArgs &a, const u32 *s_rows, const u32 *sel, u64 seg, u32 blk, u32 lane, u32 &bad) {
    const ListGlobalU32 map = (ListGlobalU32)(uintptr_t)a.map;
    const u32 over = a.n_slices_out >= 32u ? 0u : ~0u << a.n_slices_out; // bits of an entry that the result has no room for
    u32 row0 = (u32)kMapBlockRows * blk + lane;
    // (opaque: the 32 steps' selection words and shifts depend on lane and block alone, and hoisted out of the loop over the
    //  segments they would take two hundred registers)
    asm volatile("" : "+v"(row0));
    u32 v[kSteps];
    u32 have = 0u; // lane j: word j of the block's existence row
#pragma unroll
    for (u32 c = 0; c < kSteps; c += kMapChunk) {
        u32 raw[kMapChunk];
        u32 picked = 0u; // bit i: row i of the chunk is selected (one register, not a lane mask per row, across the loads)
#pragma unroll
        for (u32 i = 0; i < kMapChunk; ++i) {
            const u32 r = row0 + 64u * (c + i);
            const u32 k = s_rows[r];
            const u32 bit = (sel[r / 31u] >> (r % 31u)) & 1u;
            picked |= bit << i;
            raw[i] = bit != 0u && (u64)k < a.n_keys ? map[k] : kMapNull; // (nothing is read behind n_keys)
        }
        if (a.partial != 0u) picked = 0u; // (wave-uniform: a miss is no refusal)
#pragma unroll
        for (u32 i = 0; i < kMapChunk; ++i) {
            const bool has = raw[i] != kMapNull;
            bad |= (has ? raw[i] & over : (picked >> i) & 1u);
            v[c + i] = has ? raw[i] : 0u;
            const u64 m = __ballot(has);
            have = put_lane((u32)m, 2u * (c + i), have);
            have = put_lane((u32)(m >> 32), 2u * (c + i) + 1u, have);
        }
    }
    const bool store = lane < 2u * kSteps; // (the half block: 32 words)
    u32 *out = a.matrix + (seg * kSegWords + kMapBlockWords * blk + lane); // row 0 of the matrix; every row is n_words further
#pragma nounroll
    for (u32 b = a.n_slices_out; b > 0u; --b) {
        const u32 w = slice_words(v, 1u << (b - 1u));
        if (store) *out = w;
        out += a.n_words;
    }
    if (a.out_exists != 0u && store) *out = have;
}

__global__ __launch_bounds__(kMapWaves * 64) void bsi_map_segments_kernel(const BsiMapArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_rows[kSegBits];
    __shared__ __attribute__((aligned(16))) u32 s_acc[kMapWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    const ListOp m_or = list_op(1u), m_and = list_op(0u); // a slice is ORed into the zeroed image, the existence row ANDed into the preset one
    const u32 nk = a.n_slices_key;
    // the key's slices are shared out over wavefronts 0 .. 6
    const u32 per = (nk + kMapSliceWaves - 1u) / kMapSliceWaves;
    const u32 w_lo = min(wave * per, nk), w_hi = wave < kMapSliceWaves ? min(w_lo + per, nk) : w_lo;
    u32 bad = 0u;

#pragma nounroll
    for (u64 seg = blockIdx.x; seg < a.n_segments; seg += gridDim.x) { // (workgroup-uniform)
        const u32 nvalid = segment_groups(a.groups, seg);

        for (u32 p = threadIdx.x * 4u; p < kSegBits; p += kMapWaves * 64u * 4u) *reinterpret_cast<uint4 *>(s_rows + p) = make_uint4(0u, 0u, 0u, 0u);
        if (wave < kMapSliceWaves) {
            image_fill(acc, 0u, lane);
        } else { // the selection image: every row of the segment that lies in front of n_rows
            const u32 rows = segment_rows(a.n_rows, seg), full = rows / 31u, rest = rows % 31u;
#pragma unroll
            for (u32 i = 0; i < kSegGroups / 64u; ++i) {
                const u32 g = 64u * i + lane;
                acc[g] = g >= nvalid ? 0u : g < full ? kOnes31 : g == full ? (1u << rest) - 1u : 0u;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        __syncthreads();

        if (wave < kMapSliceWaves) {
            if (w_lo < w_hi) { // (wave-uniform) table rows [w_lo, w_hi) of the key, the first of significance nk - 1 - w_lo
                u32 cur = 0;       // the table row the image holds (wave-uniform)
                bool open = false; // ... if it holds one: rows settled in the gather never get there
                auto fold = [&]() {
                    fold_slice_bits(acc, s_rows, 0u, kSegGroups / 64u, nk - 1u - w_lo - cur, lane);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    image_fill(acc, 0u, lane);
                };
                const bool ok = list_walk(a.key + w_lo, w_hi - w_lo, seg, nvalid, m_or.fill, acc, lane, [&](u32) -> const ListOp & { return m_or; }, [&](u32 j) {
                    if (open) fold(); // this row's words begin: the one in the image is complete
                    cur = j;
                    open = true;
                });
                if (open) fold();
                // (no early return: the workgroup's barriers are for all its wavefronts; the output of a refused call is unspecified)
                if (!ok) report_stream_error(a.ctrl, lane);
            }
        } else if (a.has_exists) { // the key table's last row
            const bool ok = list_walk(a.key + nk, 1u, seg, nvalid, m_and.fill, acc, lane, [&](u32) -> const ListOp & { return m_and; }, [](u32) {});
            if (!ok) report_stream_error(a.ctrl, lane);
        }
        __syncthreads();

        const u32 *sel = s_acc[kMapSliceWaves];
        map_block<kMapBlockSteps>(a, s_rows, sel, seg, wave, lane, bad);
        if (wave + kMapWaves < kMapBlocks - 1u) // (wave-uniform)
            map_block<kMapBlockSteps>(a, s_rows, sel, seg, wave + kMapWaves, lane, bad);
        else
            map_block<kMapBlockSteps / 2u>(a, s_rows, sel, seg, kMapBlocks - 1u, lane, bad);
        __syncthreads(); // the next segment clears the rows and the images
    }
    if (__ballot(bad != 0u) != 0ull && lane == 0) atomicOr(a.ctrl + kCtlError, kErrStream);
}

} // namespace

hipError_t launch_bsi_map(const BsiMapArgs &a, hipStream_t s) {
    if (a.n_segments == 0) return hipSuccess;
    const dim3 grid((unsigned)(a.n_segments < kMapGridItems ? a.n_segments : kMapGridItems)), block(kMapWaves * 64);
    hipLaunchKernelGGL(bsi_map_segments_kernel, grid, block, 0, s, a);
    return hipGetLastError();
}

} // namespace wah
