// wah_member.hip -- wah_bsi_member_indexed_device: `value IN (set)` / `NOT IN` over a bit-sliced attribute, the set a sorted list
// of 64-bit values or a bit array over the value domain (a decoded bitmap: the semi-join of a foreign key against the filter of
// its dimension table).  The result is one decoded bitmap in the scratch, which the compress passes take from there
// (combine_then_compress, wah_api.hip) -- the road of the range call.
//
// member_items_kernel: values_items_kernel's frame (wah_values.hip) -- one WORKGROUP of eight wavefronts per item, a grid of
// capped size striding over the items -- with a probe where that kernel stores values:
//   up to 32 slices   an item is a segment; one u32 per row in LDS (31 744 rows: 124 KiB);
//   more than 32      the whole value is needed per row, so an item is a segment and a HALF OF ITS GROUPS (512 groups = 15 872
//                     rows of two u32 each: the same 124 KiB; the low halves of the values lie in front, the high halves behind
//                     them, so that both are read at stride 31).  The walk covers the segment, the fold takes the item's half
//                     of the image only: one LDS atomic per set bit position and slice, on the half the slice belongs to.
// The table's rows (slices, then the existence bitmap) are shared out over the wavefronts in contiguous runs; a wavefront walks
// its run with list_walk under OR, one row at a time in its zeroed image, and folds a slice into the rows' words when the walk
// crosses to the next row (fold_slice_bits, wah_fold_bits.hpp -- the fold of values_items_kernel).  The existence bitmap is the
// table's LAST row, so the wavefront that holds the end of the table simply does not fold it: it stays in that wavefront's image
// (a row settled in the gather leaves the zeroed image: no row exists), where the probe finds it behind the barrier.  No bit of
// the values is spent on it, so 32 and 64 slices need no other layout.
//
// Behind the barrier, the probe: wavefront w takes the steps s = w, w + 8 of the segment (w of the item's eight steps above 32
// slices), a lane group 64 s + lane: it reads the group's 31 rows (stride 31: conflict-free, wah_fold_bits.hpp), probes the set
// per row, assembles the group's word, applies NEGATE and the existence group, and hands the word to seg_store in the register
// it is in -- the lanes of a step are the 64 groups seg_store repacks into 62 words, so no image of the result is needed.
//   list       a branch-free search for the last entry <= value over `count` entries (wave-uniform: every lane runs the same
//              number of steps), then one compare; eight rows' searches are interleaved so that eight loads are in flight;
//   bit array  one bounds test and one 4-byte load per row, 31 loads in flight.
// A half-segment item owns 8 of the 16 steps: 512 groups are exactly 496 words, so no two items write one word.
//
// member_check_kernel: the list's order and count, a capped grid striding over the set.  Both kernels clamp the count to the
// capacity before anything is read through it.
#include "wah_fold_bits.hpp"

namespace wah {
namespace {

constexpr u32 kMemberGridItems = 512;  // workgroups of member_items_kernel at the most (two per CU: one resident, one waiting)
constexpr u32 kMemberWaves = 8;        // wavefronts of a workgroup
constexpr u32 kMemberHalfGroups = kSegGroups / 2u;        // groups of an item above 32 slices
constexpr u32 kMemberHalfRows = 31u * kMemberHalfGroups;  // ... and its rows: where the high halves of the values begin
constexpr u32 kMemberCheckGrid = 1024; // workgroups of member_check_kernel at the most
constexpr u32 kMemberChunk = 8;        // rows whose list searches run interleaved
static_assert((kSegBits + kMemberWaves * kSegGroups) * sizeof(u32) <= 160u * 1024u, "one workgroup fits a CU's LDS");
static_assert(2u * kMemberHalfRows == kSegBits && kMemberHalfGroups == 64u * kMemberWaves, "a half item: one step per wavefront");

// the entries of the list that count (wave-uniform); the check kernel reports a count above the capacity
__device__ __forceinline__ u64 member_count(const MemberArgs &a) {
    const u64 n = a.set_count ? *(ListGlobalU64)(uintptr_t)a.set_count : a.set_capacity;
    return n < a.set_capacity ? n : a.set_capacity;
}

// bit i of the result: rows' value v[i] is in the list.  The search keeps `base`, the last entry <= v among those looked at (or 0).
__device__ __forceinline__ u32 probe_list(ListGlobalU64 set, u64 count, const u64 (&v)[kMemberChunk]) {
    u64 base[kMemberChunk];
#pragma unroll
    for (u32 i = 0; i < kMemberChunk; ++i) base[i] = 0;
#pragma nounroll
    for (u64 n = count; n > 1u;) { // (wave-uniform)
        const u64 half = n >> 1;
        u64 e[kMemberChunk];
#pragma unroll
        for (u32 i = 0; i < kMemberChunk; ++i) e[i] = set[base[i] + half];
#pragma unroll
        for (u32 i = 0; i < kMemberChunk; ++i) base[i] += e[i] <= v[i] ? half : 0ull;
        n -= half;
    }
    u32 bits = 0;
    if (count != 0u) {
        u64 e[kMemberChunk];
#pragma unroll
        for (u32 i = 0; i < kMemberChunk; ++i) e[i] = set[base[i]];
#pragma unroll
        for (u32 i = 0; i < kMemberChunk; ++i) bits |= (e[i] == v[i] ? 1u : 0u) << i;
    }
    return bits;
}

// the same for the bit array of set_bits bits
__device__ __forceinline__ u32 probe_bitset(ListGlobalU32 words, u64 set_bits, const u64 (&v)[kMemberChunk]) {
    u32 w[kMemberChunk];
#pragma unroll
    for (u32 i = 0; i < kMemberChunk; ++i) w[i] = v[i] < set_bits ? words[v[i] >> 5] : 0u;
    u32 bits = 0;
#pragma unroll
    for (u32 i = 0; i < kMemberChunk; ++i) bits |= ((w[i] >> ((u32)v[i] & 31u)) & 1u) << i;
    return bits;
}

// The 31 rows of one group, lo[b] (and hi[b] above 32 slices) at stride 1 from `lo` / `hi` on: the group's word of the rows
// whose value is in the set.  Chunks of kMemberChunk rows; the last chunk's row 31 does not exist: row 30 is probed twice and the
// bit is cut off.
template <bool kWide, bool kBitset>
__device__ __forceinline__ u32 probe_group(const MemberArgs &a, u64 count, const u32 *lo, const u32 *hi) {
    u32 word = 0;
#pragma unroll
    for (u32 c = 0; c < 32u; c += kMemberChunk) {
        u64 v[kMemberChunk];
#pragma unroll
        for (u32 i = 0; i < kMemberChunk; ++i) {
            const u32 b = c + i < 31u ? c + i : 30u;
            v[i] = kWide ? ((u64)hi[b] << 32) | lo[b] : (u64)lo[b];
        }
        const u32 bits = kBitset ? probe_bitset((ListGlobalU32)(uintptr_t)a.set, a.set_capacity, v) : probe_list((ListGlobalU64)(uintptr_t)a.set, count, v);
        word |= bits << c;
    }
    return word & kOnes31;
}

template <bool kWide, bool kBitset>
__global__ __launch_bounds__(kMemberWaves * 64) void member_items_kernel(const MemberArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_rows[kSegBits];
    __shared__ __attribute__((aligned(16))) u32 s_acc[kMemberWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    const ListOp m = list_op(1u); // a table row is ORed into the zeroed image
    const u32 ns = a.n_slices, n_rows = a.n_slices + a.has_exists;
    // the table's rows are shared out over the wavefronts; wave_e holds the table's last row
    const u32 per = (n_rows + kMemberWaves - 1u) / kMemberWaves;
    const u32 w_lo = min(wave * per, n_rows), w_hi = min(w_lo + per, n_rows);
    const u32 wave_e = (n_rows - 1u) / per;
    const u32 halves = kWide ? 2u : 1u;
    const u64 count = kBitset ? 0ull : member_count(a);
    const u32 flip = a.negate ? kOnes31 : 0u;

#pragma nounroll
    for (u64 t = blockIdx.x; t < a.n_items; t += gridDim.x) { // (workgroup-uniform)
        const u64 seg = t / halves;
        const u32 half = (u32)(t % halves);
        const u32 nvalid = segment_groups(a.g.groups, seg);

        for (u32 p = threadIdx.x * 4u; p < kSegBits; p += kMemberWaves * 64u * 4u) *reinterpret_cast<uint4 *>(s_rows + p) = make_uint4(0u, 0u, 0u, 0u);
        image_fill(acc, 0u, lane); // (the last item may have left the existence bitmap here)
        __syncthreads();

        if (w_lo < w_hi) { // (wave-uniform)
            u32 cur = 0;       // the table row the image holds, counted from w_lo (wave-uniform)
            bool open = false; // ... if it holds one: rows settled in the gather never get there
            auto fold = [&]() {
                const u32 sig = ns - 1u - (w_lo + cur);
                if (kWide)
                    fold_slice_bits(acc, s_rows + (sig >= 32u ? kMemberHalfRows : 0u), kMemberWaves * half, kMemberWaves, sig & 31u, lane);
                else
                    fold_slice_bits(acc, s_rows, 0u, kSegGroups / 64u, sig, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                image_fill(acc, 0u, lane);
            };
            const bool ok = list_walk(a.table + w_lo, w_hi - w_lo, seg, nvalid, m.fill, acc, lane, [&](u32) -> const ListOp & { return m; }, [&](u32 j) {
                if (open) fold(); // this row's words begin: the one in the image is complete
                cur = j;
                open = true;
            });
            if (open && w_lo + cur < ns) fold(); // (the existence bitmap stays in the image)
            // (no early return: the workgroup's barriers are for all its wavefronts; the output of a refused call is unspecified)
            if (!ok) report_stream_error(a.g.ctrl, lane);
        }
        __syncthreads();

        const SegStore st = seg_store_setup(a.g.out, a.g.out_words, seg, seg, lane);
        const u32 *have = s_acc[wave_e];
        if (kWide) {
            const u32 s = kMemberWaves * half + wave, g = 64u * s + lane, r = 31u * (64u * wave + lane);
            u32 word = probe_group<kWide, kBitset>(a, count, s_rows + r, s_rows + kMemberHalfRows + r) ^ flip;
            if (a.has_exists) word &= have[g];
            seg_store(st, (int)s, g < nvalid ? word : 0u);
        } else {
#pragma nounroll
            for (u32 s = wave; s < kSteps; s += kMemberWaves) {
                const u32 g = 64u * s + lane;
                u32 word = probe_group<kWide, kBitset>(a, count, s_rows + 31u * g, nullptr) ^ flip;
                if (a.has_exists) word &= have[g];
                seg_store(st, (int)s, g < nvalid ? word : 0u);
            }
        }
        __syncthreads(); // the next item clears the rows and the images
    }
}

// the list as the call wants it: a count within the capacity, non-decreasing entries within the count
__global__ __launch_bounds__(256) void member_check_kernel(const MemberArgs a) {
    const u64 given = a.set_count ? *(ListGlobalU64)(uintptr_t)a.set_count : a.set_capacity;
    const u64 count = member_count(a);
    const ListGlobalU64 set = (ListGlobalU64)(uintptr_t)a.set;
    bool bad = given > a.set_capacity;
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i + 1u < count; i += (u64)gridDim.x * 256u) bad |= set[i] > set[i + 1u];
    if (__ballot(bad) != 0ull) report_stream_error(a.g.ctrl, lane_id());
}

} // namespace

hipError_t launch_member(const MemberArgs &a, hipStream_t s) {
    if (!a.bitset) {
        const u64 blocks = (a.set_capacity + 255u) / 256u;
        const dim3 grid((unsigned)(blocks < 1u ? 1u : blocks < kMemberCheckGrid ? blocks : kMemberCheckGrid)), block(256);
        hipLaunchKernelGGL(member_check_kernel, grid, block, 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.n_items == 0) return hipSuccess;
    const dim3 grid((unsigned)(a.n_items < kMemberGridItems ? a.n_items : kMemberGridItems)), block(kMemberWaves * 64);
    const bool wide = a.n_slices > 32u;
    if (wide && a.bitset)
        hipLaunchKernelGGL((member_items_kernel<true, true>), grid, block, 0, s, a);
    else if (wide)
        hipLaunchKernelGGL((member_items_kernel<true, false>), grid, block, 0, s, a);
    else if (a.bitset)
        hipLaunchKernelGGL((member_items_kernel<false, true>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((member_items_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

} // namespace wah
