// wah_values.hip -- wah_values_indexed_device: a whole attribute read back out of the index, the values of the row range
// [first_row, first_row + n_rows) -- the inverse of wah_bsi_build_device (WAH_FETCH_BITS) and of an equality index built by
// wah_from_positions_device (WAH_FETCH_FIRST).  d_out[i] is what wah_fetch_indexed_device gives for the listed row first_row + i;
// where that call walks a segment once per 64 listed rows, this one walks it once (twice for an attribute of more than 32 slices).
//
// One launch, values_items_kernel, none of whose workgroups waits for another.  One WORKGROUP per item:
//   WAH_FETCH_BITS   an item is a segment of the window and a HALF of the value: the table rows of significance 0 .. 31 (the last
//                    min(32, n) rows: row 0 is the most significant) or of significance 32 .. 63 (the rows in front of them).  An
//                    attribute of at most 32 rows has one item per segment, which stores whole 8-byte elements; a wider one has
//                    two, and each stores the 4-byte half it owns of every element -- no two items touch one byte of d_out.
//   WAH_FETCH_FIRST  an item is a segment of the window; column numbers are below 2^24, so the value fits the same u32.
// The workgroup keeps one u32 per row of the segment in LDS (31 744 rows: 124 KiB) and every wavefront an image of the segment's
// 1024 groups beside it (4 KiB).  The item's table rows are shared out over the wavefronts in contiguous runs; a wavefront walks
// its run as fetch_items_kernel walks the table -- list_walk under OR, one row at a time in the zeroed image -- and folds the row
// in the image into the per-row words when the walk crosses to the next one.  Row p of the segment is bit p % 31 of group p / 31:
//   BITS   a lane takes group 64 k + lane and the bit number runs wave-uniform from 0 to 30, so the 64 lanes of one LDS `or` are
//          the rows 31 (64 k + lane) + b: 31 is odd, so they lie on different banks (one per lane of a 32-lane half).  A block of 64
//          groups that is all zero is skipped.
//   FIRST  a lane visits the set bits of its groups only (an LDS `min` each), so a column costs its words and its set bits, not
//          31 744 rows: an index of thousands of columns has a handful of set bits per column and segment.
// Several wavefronts fold at once, so the folds are LDS atomics (`or` of disjoint bits, `min`); no atomic ever touches global
// memory.  A row that is settled in the gather (one zero fill over the segment) never reaches the image and costs its gather
// only.  Behind a barrier the rows leave LDS, 64 consecutive rows per wavefront store, clipped to the window: every element of
// d_out[0 .. n_rows) is written exactly once, and nothing else is.
//
// Wavefronts per workgroup: 124 KiB of row words leave 36 KiB of the CU's 160 KiB, so at most nine images and one workgroup per
// CU either way.  EIGHT wavefronts (156 KiB): two per SIMD, so that one can fold while the other waits for its words, and a
// power of two for the run split.
//
// The grid is capped (kValuesGridItems workgroups, two per CU: one resident, one waiting for its LDS) and strides over the items:
// a bitmap may have 2^40 words.
#include "wah_fold_bits.hpp"

namespace wah {
namespace {

constexpr u32 kValuesGridItems = 512; // workgroups of values_items_kernel at the most
constexpr u32 kValuesWaves = 8;       // wavefronts of a workgroup
constexpr u32 kValuesNone = 0xFFFFFFFFu; // WAH_FETCH_FIRST: no column has the row (stored as UINT64_MAX)
static_assert((kSegBits + kValuesWaves * kSegGroups) * sizeof(u32) <= 160u * 1024u, "one workgroup fits a CU's LDS");

template <u32 kMode>
__global__ __launch_bounds__(kValuesWaves * 64) void values_items_kernel(const ValuesArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_rows[kSegBits];
    __shared__ __attribute__((aligned(16))) u32 s_acc[kValuesWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    const ListOp m = list_op(1u); // a table row is ORed into the zeroed image
    const u32 halves = kMode == kFetchBits && a.n_operands > 32u ? 2u : 1u;
    const u32 low_rows = a.n_operands < 32u ? a.n_operands : 32u; // BITS: the table rows of the low half, the table's last
    const u64 end_row = a.first_row + a.n_rows;
    image_fill(acc, 0u, lane);

#pragma nounroll
    for (u64 t = blockIdx.x; t < a.n_items; t += gridDim.x) { // (workgroup-uniform)
        const u64 seg = a.first_segment + t / halves;
        const u32 half = (u32)(t % halves);
        const u32 nvalid = segment_groups(a.groups, seg);
        // the item's table rows [j_lo, j_hi), and this wavefront's run of them
        u32 j_lo = 0, j_hi = a.n_operands;
        if (kMode == kFetchBits) {
            if (half == 0u) j_lo = a.n_operands - low_rows; else j_hi = a.n_operands - 32u;
        }
        const u32 per = (j_hi - j_lo + kValuesWaves - 1u) / kValuesWaves;
        const u32 w_lo = min(j_lo + wave * per, j_hi), w_hi = min(w_lo + per, j_hi);

        for (u32 p = threadIdx.x * 4u; p < kSegBits; p += kValuesWaves * 64u * 4u) {
            const u32 v = kMode == kFetchFirst ? kValuesNone : 0u;
            *reinterpret_cast<uint4 *>(s_rows + p) = make_uint4(v, v, v, v);
        }
        __syncthreads();

        if (w_lo < w_hi) { // (wave-uniform)
            u32 cur = 0;       // the table row the image holds, counted from w_lo (wave-uniform)
            bool open = false; // ... if it holds one: rows settled in the gather never get there
            auto fold = [&]() {
                const u32 j = w_lo + cur;
                if (kMode == kFetchBits) {
                    const u32 sig = (a.n_operands - 1u - j) & 31u; // (significance s lies in half s / 32 at bit s % 32)
                    fold_slice_bits(acc, s_rows, 0u, kSegGroups / 64u, sig, lane); // (wah_fold_bits.hpp: shared with wah_member.hip)
                } else {
#pragma nounroll
                    for (u32 k = 0; k < kSegGroups / 64u; ++k) {
                        const u32 g = 64u * k + lane;
                        u32 w = acc[g] & kOnes31;
                        u32 *row = s_rows + 31u * g;
                        while (w != 0u) {
                            const u32 b = (u32)__builtin_ctz(w);
                            w &= w - 1u;
                            __hip_atomic_fetch_min(row + b, j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                image_fill(acc, 0u, lane);
            };
            const bool ok = list_walk(a.table + w_lo, w_hi - w_lo, seg, nvalid, m.fill, acc, lane, [&](u32) -> const ListOp & { return m; }, [&](u32 j) {
                if (open) fold(); // this row's words begin: the one in the image is complete
                cur = j;
                open = true;
            });
            if (open) fold();
            // (no early return: the workgroup's barriers are for all its wavefronts; the output of a refused call is unspecified)
            if (!ok) report_stream_error(a.ctrl, lane);
        }
        __syncthreads();

        // the segment's rows that lie in the window leave, 64 consecutive rows per wavefront store
        const u64 seg_row0 = seg * (u64)kSegBits;
        const u32 lo = a.first_row > seg_row0 ? (u32)(a.first_row - seg_row0) : 0u;
        const u32 hi = end_row - seg_row0 < kSegBits ? (u32)(end_row - seg_row0) : kSegBits;
        for (u32 r = lo + threadIdx.x; r < hi; r += kValuesWaves * 64u) {
            const u32 v = s_rows[r];
            u64 *out = a.out + (seg_row0 + r - a.first_row); // (r >= lo: at or behind the window's first row)
            if (kMode == kFetchFirst)
                *out = v == kValuesNone ? ~0ull : (u64)v;
            else if (halves == 1u)
                *out = (u64)v;
            else
                reinterpret_cast<u32 *>(out)[half] = v; // (little endian: the low half first)
        }
        __syncthreads(); // the next item clears the rows
    }
}

} // namespace

hipError_t launch_values_items(const ValuesArgs &a, u32 mode, hipStream_t s) {
    if (a.n_items == 0) return hipSuccess;
    const dim3 grid((unsigned)(a.n_items < kValuesGridItems ? a.n_items : kValuesGridItems)), block(kValuesWaves * 64);
    if (mode == kFetchFirst)
        hipLaunchKernelGGL(values_items_kernel<kFetchFirst>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(values_items_kernel<kFetchBits>, grid, block, 0, s, a);
    return hipGetLastError();
}

} // namespace wah
