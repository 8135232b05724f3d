// wah_group_by.hip -- wah_bsi_group_by_indexed_device: `SELECT key, COUNT(*), SUM(value) WHERE <filters> GROUP BY key` over a
// BIT-SLICED key of up to 32 slices -- an attribute of many values, where a bitmap per group does not exist -- with an optional
// lookup table from key to bucket in front of the add: the star join's GROUP BY (`GROUP BY d.year` for a fact table's foreign
// key, the dimension's filter riding in the table as dropped keys).  No value column, no decoded filter and no row list is
// written: what leaves the kernel is the histogram.
//
// group_by_items_kernel: member_items_kernel's frame (wah_member.hip) -- one WORKGROUP of eight wavefronts per item, a grid of
// capped size striding over the items, fold_slice_bits (wah_fold_bits.hpp) unchanged -- with an add into an array of buckets
// where that kernel probes a set:
//   count only     an item is a segment; the key word of each of its 31 744 rows in s_rows (124 KiB);
//   with a value   an item is a segment and a HALF OF ITS GROUPS, the member kernel's layout above 32 slices: the key words of
//                  the half's 15 872 rows lie in front, the value words behind them, both read at stride 31.  The walk covers
//                  the whole segment either way, so A VALUE ATTRIBUTE DOUBLES THE OPERAND READS: every slice's words of a
//                  segment are loaded by both of its items, and each folds its half of the image only.
// The slices (the key's, then the value's) are shared out over wavefronts 0 .. 6 in contiguous runs, walked with list_walk under
// OR one row at a time in the zeroed image and folded when the walk crosses to the next row.  Wavefront 7 makes the SELECTION
// image: its image is preset to all ones, clipped to segment_groups / segment_rows (rows at or behind n_rows and pad bits are
// zero from the start), and the key's existence bitmap and the filter rows are walked into it under AND.  No LDS beyond the
// frame's 159 744 bytes.
//
// Behind the barrier, the scatter: wavefront w takes the steps s = w, w + 8 of the segment (step 8 half + w of a half item), a
// lane group 64 s + lane.  It reads the group's selection word and visits its up to 31 rows IN ORDER, eight at a time:
//   * the eight rows' key words are read from LDS, and THE MAP LOADS OF ALL EIGHT ARE ISSUED BEFORE THE FIRST ONE IS USED
//     (resolve_buckets: one bounds test and one 4-byte load per selected row, eight loads in flight per lane -- the shape of
//     probe_bitset in wah_member.hip); a row that is not selected loads nothing;
//   * runs of equal consecutive buckets are merged in registers into one (count, sum) pair before anything is added, so sorted
//     and clustered keys cost one add a run.
// Two routes, chosen by n_buckets alone (host-known, wave-uniform: a template parameter):
//   n_buckets + 1 <= kGroupByLdsBuckets   the adds are LDS atomics into u32 counts and u64 sums (24 KiB) that lie in the images
//                  of wavefronts 0 .. 5 -- a wavefront that has finished folding leaves its image zeroed, so the buckets need no
//                  clearing of their own; at the item's end every non-zero bucket leaves with one global 64-bit atomic for the
//                  count and one for the low sum word, plus the carry;
//   more buckets   global 64-bit atomics per run; the low sum word is added with the returning form, and `old + x < old` adds
//                  one to the high word.
// A run's sum is below 31 x 2^32 and an item's below 2^47: neither the registers nor the LDS sums can wrap.
#include "wah_fold_bits.hpp"

namespace wah {
namespace {

constexpr u32 kGroupByGridItems = 512;    // workgroups of group_by_items_kernel at the most (two per CU: one resident, one waiting)
constexpr u32 kGroupByLdsBuckets = 2048;  // buckets, "other" included, up to which an item adds in LDS
constexpr u32 kGroupByWaves = 8;          // wavefronts of a workgroup
constexpr u32 kGroupBySliceWaves = kGroupByWaves - 1u;     // ... that walk slices; the last one walks the selection rows
constexpr u32 kGroupByHalfGroups = kSegGroups / 2u;        // groups of an item with a value attribute
constexpr u32 kGroupByHalfRows = 31u * kGroupByHalfGroups; // ... and its rows: where the value words begin
constexpr u32 kGroupByChunk = 8;          // rows whose map loads are in flight together
constexpr u32 kGroupBySkip = 0xFFFFFFFFu; // a row that is not selected (a bucket is at most 2^30)
static_assert((kSegBits + kGroupByWaves * kSegGroups) * sizeof(u32) <= 160u * 1024u, "one workgroup fits a CU's LDS");
static_assert(2u * kGroupByHalfRows == kSegBits && kGroupByHalfGroups == 64u * kGroupByWaves, "a half item: one step per wavefront");
static_assert(kGroupByLdsBuckets * (sizeof(u32) + sizeof(u64)) <= (kGroupByWaves - 2u) * kSegGroups * sizeof(u32),
              "the LDS buckets fit the images of wavefronts 0 .. 5: the selection image and one more stay free");

// The buckets of rows c .. c + 7 of one group (row 31 does not exist: row 30 is read again, and its selection bit is clear):
// kGroupBySkip for a row that is not selected, else the row's bucket, "other" (n_buckets) included.
__device__ __forceinline__ void resolve_buckets(const GroupByArgs &a, const u32 *keys, u32 sel, u32 c, u32 (&bucket)[kGroupByChunk]) {
    const ListGlobalU32 map = (ListGlobalU32)(uintptr_t)a.map;
    u32 raw[kGroupByChunk];
    if (map != nullptr) { // (wave-uniform)
#pragma unroll
        for (u32 i = 0; i < kGroupByChunk; ++i) {
            const u32 k = keys[c + i < 31u ? c + i : 30u];
            raw[i] = ((sel >> (c + i)) & 1u) != 0u && (u64)k < a.n_keys ? map[k] : kGroupBySkip; // (nothing is read behind n_keys)
        }
    } else {
#pragma unroll
        for (u32 i = 0; i < kGroupByChunk; ++i) raw[i] = keys[c + i < 31u ? c + i : 30u];
    }
#pragma unroll
    for (u32 i = 0; i < kGroupByChunk; ++i)
        bucket[i] = ((sel >> (c + i)) & 1u) == 0u ? kGroupBySkip : raw[i] < a.n_buckets ? raw[i] : a.n_buckets;
}

// one run of a lane: `count` rows of bucket b whose values add up to `sum`
template <bool kVal, bool kLds>
__device__ __forceinline__ void add_run(const GroupByArgs &a, u32 *lds_counts, u64 *lds_sums, u32 b, u32 count, u64 sum) {
    if (kLds) {
        __hip_atomic_fetch_add(lds_counts + b, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (kVal && sum != 0ull) __hip_atomic_fetch_add(lds_sums + b, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
        __hip_atomic_fetch_add(a.counts + b, (u64)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (kVal && sum != 0ull) {
            const u64 old = __hip_atomic_fetch_add(a.sums + 2ull * b, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old + sum < old) __hip_atomic_fetch_add(a.sums + 2ull * b + 1ull, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The up to 31 selected rows of one group, keys[b] (and vals[b]) at stride 1: visited in order, runs of one bucket merged.
template <bool kVal, bool kLds>
__device__ __forceinline__ void scatter_group(const GroupByArgs &a, u32 *lds_counts, u64 *lds_sums, u32 sel, const u32 *keys, const u32 *vals) {
    if (sel == 0u) return;
    u32 cur = kGroupBySkip, count = 0; // the open run
    u64 sum = 0;
#pragma unroll
    for (u32 c = 0; c < 32u; c += kGroupByChunk) {
        u32 bucket[kGroupByChunk], v[kGroupByChunk];
        resolve_buckets(a, keys, sel, c, bucket);
#pragma unroll
        for (u32 i = 0; i < kGroupByChunk; ++i) v[i] = kVal ? vals[c + i < 31u ? c + i : 30u] : 0u;
#pragma unroll
        for (u32 i = 0; i < kGroupByChunk; ++i) {
            if (bucket[i] == kGroupBySkip) continue;
            if (bucket[i] != cur) {
                if (count != 0u) add_run<kVal, kLds>(a, lds_counts, lds_sums, cur, count, sum);
                cur = bucket[i];
                count = 0u;
                sum = 0ull;
            }
            ++count;
            sum += v[i];
        }
    }
    if (count != 0u) add_run<kVal, kLds>(a, lds_counts, lds_sums, cur, count, sum); // the lane's last run
}

template <bool kVal, bool kLds>
__global__ __launch_bounds__(kGroupByWaves * 64) void group_by_items_kernel(const GroupByArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_rows[kSegBits];
    __shared__ __attribute__((aligned(16))) u32 s_acc[kGroupByWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    const ListOp m_or = list_op(1u), m_and = list_op(0u); // a slice is ORed into the zeroed image, a selection row ANDed into the preset one
    const u32 nk = a.n_slices_key, total = a.n_slices_key + (kVal ? a.n_slices_val : 0u);
    // the slices (the key's, then the value's) are shared out over wavefronts 0 .. 6
    const u32 per = (total + kGroupBySliceWaves - 1u) / kGroupBySliceWaves;
    const u32 w_lo = min(wave * per, total), w_hi = wave < kGroupBySliceWaves ? min(w_lo + per, total) : w_lo;
    const u32 halves = kVal ? 2u : 1u;
    u32 *lds_counts = s_acc[0];                          // kLds: kGroupByLdsBuckets u32 in the images of wavefronts 0, 1
    u64 *lds_sums = reinterpret_cast<u64 *>(s_acc[2]);   // ... and as many u64 in those of wavefronts 2 .. 5

#pragma nounroll
    for (u64 t = blockIdx.x; t < a.n_items; t += gridDim.x) { // (workgroup-uniform)
        const u64 seg = t / halves;
        const u32 half = (u32)(t % halves);
        const u32 nvalid = segment_groups(a.groups, seg);

        for (u32 p = threadIdx.x * 4u; p < kSegBits; p += kGroupByWaves * 64u * 4u) *reinterpret_cast<uint4 *>(s_rows + p) = make_uint4(0u, 0u, 0u, 0u);
        if (wave < kGroupBySliceWaves) {
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

        if (wave < kGroupBySliceWaves) {
            // rows [lo, lo + n) of one attribute's table, the first of significance sig_top, folded into the words at `rows`
            auto walk_fold = [&](const BitopListOperand *table, u32 n, u32 sig_top, u32 *rows) {
                u32 cur = 0;       // the table row the image holds (wave-uniform)
                bool open = false; // ... if it holds one: rows settled in the gather never get there
                auto fold = [&]() {
                    fold_slice_bits(acc, rows, kVal ? kGroupByWaves * half : 0u, kVal ? kGroupByWaves : kSegGroups / 64u, sig_top - cur, lane);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    image_fill(acc, 0u, lane);
                };
                const bool ok = list_walk(table, n, seg, nvalid, m_or.fill, acc, lane, [&](u32) -> const ListOp & { return m_or; }, [&](u32 j) {
                    if (open) fold(); // this row's words begin: the one in the image is complete
                    cur = j;
                    open = true;
                });
                if (open) fold();
                // (no early return: the workgroup's barriers are for all its wavefronts; the output of a refused call is unspecified)
                if (!ok) report_stream_error(a.ctrl, lane);
            };
            const u32 k_hi = min(w_hi, nk);
            if (w_lo < k_hi) walk_fold(a.key + w_lo, k_hi - w_lo, nk - 1u - w_lo, s_rows); // (wave-uniform)
            if (kVal) {
                const u32 v_lo = max(w_lo, nk) - nk, v_hi = max(w_hi, nk) - nk;
                if (v_lo < v_hi) walk_fold(a.val + v_lo, v_hi - v_lo, a.n_slices_val - 1u - v_lo, s_rows + kGroupByHalfRows);
            }
        } else {
            bool ok = true;
            if (a.has_exists) // the key table's last row
                ok = list_walk(a.key + nk, 1u, seg, nvalid, m_and.fill, acc, lane, [&](u32) -> const ListOp & { return m_and; }, [](u32) {});
            if (a.n_filters != 0u)
                ok = list_walk(a.filters, a.n_filters, seg, nvalid, m_and.fill, acc, lane, [&](u32) -> const ListOp & { return m_and; }, [](u32) {}) && ok;
            if (!ok) report_stream_error(a.ctrl, lane);
        }
        __syncthreads(); // (the images of wavefronts 0 .. 6 are zero again: the LDS buckets begin empty)

        const u32 *sel = s_acc[kGroupBySliceWaves];
        if (kVal) {
            const u32 g = 64u * (kGroupByWaves * half + wave) + lane, r = 31u * (64u * wave + lane);
            scatter_group<kVal, kLds>(a, lds_counts, lds_sums, sel[g] & kOnes31, s_rows + r, s_rows + kGroupByHalfRows + r);
        } else {
#pragma nounroll
            for (u32 s = wave; s < kSteps; s += kGroupByWaves) {
                const u32 g = 64u * s + lane;
                scatter_group<kVal, kLds>(a, lds_counts, lds_sums, sel[g] & kOnes31, s_rows + 31u * g, nullptr);
            }
        }
        if (kLds) { // the item's non-zero buckets leave
            __syncthreads();
            for (u32 b = threadIdx.x; b <= a.n_buckets; b += kGroupByWaves * 64u) {
                const u32 count = lds_counts[b];
                if (count != 0u) add_run<kVal, false>(a, nullptr, nullptr, b, count, kVal ? lds_sums[b] : 0ull);
            }
        }
        __syncthreads(); // the next item clears the rows and the images
    }
}

} // namespace

hipError_t launch_group_by(const GroupByArgs &a, hipStream_t s) {
    if (a.n_items == 0) return hipSuccess;
    const dim3 grid((unsigned)(a.n_items < kGroupByGridItems ? a.n_items : kGroupByGridItems)), block(kGroupByWaves * 64);
    const bool val = a.n_slices_val != 0u, lds = a.n_buckets + 1u <= kGroupByLdsBuckets;
    if (val && lds)
        hipLaunchKernelGGL((group_by_items_kernel<true, true>), grid, block, 0, s, a);
    else if (val)
        hipLaunchKernelGGL((group_by_items_kernel<true, false>), grid, block, 0, s, a);
    else if (lds)
        hipLaunchKernelGGL((group_by_items_kernel<false, true>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((group_by_items_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

} // namespace wah
