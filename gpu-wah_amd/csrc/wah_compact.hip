// wah_compact.hip -- wah_compact_indexed_device: the rows that a mask bitmap selects (or, under WAH_COMPACT_DELETE, does not
// select) of every column of an index, moved together into new indexed bitmaps -- DELETE FROM t WHERE ..., CREATE TABLE s AS
// SELECT * FROM t WHERE ..., a sample, the drop of tomb-stoned rows.  The output is written as wah_splice_indexed_device writes
// it: the columns' compress() streams back to back and the index of the whole.  No decoded bitmap exists at any point.
//
// Only positions below n_rows are rows: what the mask or a column holds at or behind n_rows -- the pad bits of the last group, set
// pad bits of a foreign stream among them -- is never selected and never carried.  Ranks, rows and offsets are 64-bit throughout.
//
// The launches, none of whose workgroups waits for another:
//   compact_rank_kernel      one wavefront per mask segment (a capped grid, every wavefront a contiguous run of segments): the
//                            mask segment walked into an image of its 1024 groups in LDS (list_walk), ANDed with the row range,
//                            complemented under DELETE, popcounted.  The counts go to starts[segment].  EVERY mask segment is
//                            checked here, whatever it selects.  A mask segment that is one fill word selecting nothing -- zeros,
//                            or ones under DELETE -- is settled in the walk's gather and costs no image: the walk is under OR
//                            into a zeroed image, under DELETE under AND into an image of ones, so that such a fill is the walk's
//                            identity, and an image no word touched is not read.
//   (launch_select_rank_scan turns the counts into running ranks in place: starts[s] = selected rows in front of source segment
//   s, starts[S_src] = T.)
//   compact_total_kernel     one lane: *out_rows = T; T > 32 n_words_out is refused.  With a stream error in the control block
//                            the later launches return at once: after a refused mask no column is read.
//   compact_segments_kernel<false>  (column, output segment) items shared out over the launch's wavefronts in contiguous runs, as
//                            splice_segments_kernel shares them out (item_run, wah_count_emit.hpp).  A wavefront
//                            binary-searches the ranks for the first source segment that ends behind its bit range
//                            [31744 s, 31744 (s + 1)) ∩ [0, T) (first_end_behind, wah_device.hpp) and walks forward.  A
//                            source segment with no selected row is skipped without touching the column.  For the others the mask
//                            segment and the column segment are walked into two images, and 64 groups per step: the lane's
//                            selected mask bits, their popcount, a wave prefix sum with a carry across steps, the column group's
//                            bits under the mask moved together (compact_extract: gfx950 has no PEXT), and those <= 31 bits
//                            deposited at destination bit rank(segment) + prefix - base of a third image, clipped to the item's
//                            range.  A deposit meets at most two destination groups; neighbouring lanes may meet the same one, so
//                            it is an LDS atomic OR.  The image becomes words (image_words), the count goes to offsets[item].  An
//                            output segment at or behind T is one zero-fill with no image.
//   (launch_select_rank_scan turns the counts into the index in place.)
//   compact_segments_kernel<true>   the same items again; the words are staged in the column image's LDS and leave it 64
//                            consecutive words per store instruction, clipped by the room the count pass found and by the capacity.
// Per pass and column a source segment that holds a selected row is walked at most twice: its <= 31 744 survivors lie in at most
// two output segments.  The mask segment is walked once more per column; that is accepted.
// Three images of 4 KiB per wavefront, 48 KiB per workgroup of four: three workgroups per CU (160 KiB of LDS).
#include "wah_count_emit.hpp"
#include "wah_list_walk.hpp"

namespace wah {
namespace {

constexpr int kCompactWavesPerSimd = 3;

// the selected bits of group g of a source segment with seg_rows rows: the mask image's group, complemented under DELETE, below
// the row limit
__device__ __forceinline__ u32 compact_selected(u32 image_group, u32 del, u32 g, u32 seg_rows) {
    return (del ? ~image_group : image_group) & group_row_bits(g, seg_rows);
}
// the mask segment walked into its image: under OR into zeros, under DELETE under AND into ones (above).  touched: a word was
// applied -- the image may differ from what it was filled with
__device__ __forceinline__ bool compact_walk_mask(const CompactArgs &a, u64 seg, u32 nvalid, u32 *img, u32 lane, bool &touched) {
    const ListOp m = list_op(a.del ? 0u : 1u);
    return list_walk(a.mask, 1u, seg, nvalid, m.fill, img, lane, [&](u32) -> const ListOp & { return m; }, [&](u32) { touched = true; });
}

__global__ __launch_bounds__(kSegDecodeWaves * 64, 8) void compact_rank_kernel(const CompactArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_img[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    u32 *img = s_img[wave];
    const u32 identity = a.del ? kOnes31 : 0u;
    const ItemRun run = item_run(a.src_segments, kSegDecodeWaves, wave);
    image_fill(img, identity, lane);
    bool bad = false;
#pragma nounroll
    for (u64 seg = run.begin; seg < run.end; ++seg) {
        const u32 nvalid = segment_groups(a.src_groups, seg), seg_rows = segment_rows(a.src_rows, seg);
        bool touched = false;
        bad |= !compact_walk_mask(a, seg, nvalid, img, lane, touched);
        u32 count = 0;
        if (touched) { // (wave-uniform)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (u32 s = 0; s < kSteps; ++s) count += (u32)__builtin_popcount(compact_selected(img[64u * s + lane], a.del, 64u * s + lane, seg_rows));
            count = wave_total32(count);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            image_fill(img, identity, lane);
        }
        if (lane == 0) a.starts[seg] = (u64)count;
    }
    if (bad) report_stream_error(a.ctrl, lane); // (wave-uniform: list_walk's verdict)
}

__global__ __launch_bounds__(64) void compact_total_kernel(const CompactArgs a) {
    if (threadIdx.x != 0) return;
    const u64 total = a.starts[a.src_segments];
    *a.out_rows = total;
    if (total > a.n_bits) atomicOr(a.ctrl + kCtlError, kErrStream);
}

// The bits of x at the set bits of m moved together, lowest first (PEXT): bit k of the result is x's bit at the k-th set bit of
// m.  One step per set bit of x & m, or per clear one among m's where those are fewer (the result is then the complement within
// popcount(m) bits): at most 15 steps, none for a column group that is empty under the mask.
__device__ __forceinline__ u32 compact_extract(u32 x, u32 m, u32 cnt) {
    if (m == kOnes31) return x & kOnes31; // the group goes through unchanged
    u32 t = x & m;
    const bool flip = 2u * (u32)__builtin_popcount(t) > cnt;
    if (flip) t ^= m;
    u32 v = 0;
    while (t) {
        const u32 b = (u32)__builtin_ctz(t);
        t &= t - 1u;
        v |= 1u << (u32)__builtin_popcount(m & ((1u << b) - 1u));
    }
    return flip ? v ^ ((1u << cnt) - 1u) : v; // (cnt <= 30 here)
}

template <bool kEmit>
__global__ __launch_bounds__(kSegDecodeWaves * 64, kCompactWavesPerSimd) void compact_segments_kernel(const CompactArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_mask[kSegDecodeWaves][kSegGroups];
    __shared__ __attribute__((aligned(16))) u32 s_col[kSegDecodeWaves][kSegGroups];
    __shared__ __attribute__((aligned(16))) u32 s_dst[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    if ((a.ctrl[kCtlError] & kErrStream) != 0u) return; // a refused mask, too many rows (or, in the emit pass, a refused column): no stream is read
    u32 *msk = s_mask[wave], *col = s_col[wave], *dst = s_dst[wave];
    u32 *stage = col; // (the emit pass: the column image is free once the bits are deposited)
    const u64 n_items = a.n_columns * a.n_segments;
    const ItemRun run = item_run(n_items, kSegDecodeWaves, wave);
    emit_total<kEmit>(a, a.offsets, n_items, run, lane);
    const u64 all_rows = uniform64(a.starts[a.src_segments]); // T: at most 32 n_words_out (compact_total_kernel)
    const u32 identity = a.del ? kOnes31 : 0u;
    const ListOp m_or = list_op(1u); // a column segment is ORed into the zeroed image
#pragma nounroll
    for (u64 item = run.begin; item < run.end; ++item) {
        const u64 c = item / a.n_segments, seg = item - c * a.n_segments;
        const u64 base = seg * (u64)kSegBits;
        const u32 ngroups = seg + 1 == a.n_segments ? (u32)(a.groups - seg * kSegGroups) : kSegGroups;
        u32 total;
        if (base >= all_rows) { // behind the last selected row
            total = lone_zero_fill<kEmit>(ngroups, stage, lane);
        } else {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            image_fill(dst, 0u, lane);
            const u64 limit = base + kSegBits < all_rows ? base + kSegBits : all_rows;
            const u32 room = (u32)(limit - base); // the item's bits: 1 .. 31 744
            // from the first source segment whose selected rows end behind `base` (there is one: base < T)
#pragma nounroll
            for (u64 ss = first_end_behind(a.starts, a.src_segments, base); ss < a.src_segments; ++ss) {
                const u64 st = uniform64(a.starts[ss]), en = uniform64(a.starts[ss + 1]);
                if (st >= limit) break;
                if (en <= st) continue; // no selected row: neither mask nor column is touched
                const u32 nvalid = segment_groups(a.src_groups, ss), seg_rows = segment_rows(a.src_rows, ss);
                image_fill(msk, identity, lane);
                image_fill(col, 0u, lane);
                bool touched = false;
                const bool ok = compact_walk_mask(a, ss, nvalid, msk, lane, touched) &&
                                list_walk(a.table + c, 1u, ss, nvalid, m_or.fill, col, lane, [&](u32) -> const ListOp & { return m_or; }, [](u32) {});
                if (!ok) return report_stream_error(a.ctrl, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                // where this segment's first selected row lies in the item: negative when it belongs to the segment in front
                const long long first = (long long)st - (long long)base;
                u32 carry = 0;
#pragma nounroll
                for (u32 s = 0; s < kSteps; ++s) {
                    const u32 g = 64u * s + lane;
                    const u32 sel = compact_selected(msk[g], a.del, g, seg_rows);
                    const u32 cnt = (u32)__builtin_popcount(sel);
                    const u32 incl = wave_scan_incl32(cnt);
                    const u32 step_total = (u32)__builtin_amdgcn_readlane((int)incl, 63);
                    if (step_total != 0u) { // (wave-uniform) mask groups of zero: nothing is deposited
                        long long d = first + (long long)(carry + incl - cnt);
                        u32 n = cnt;
                        if (n != 0u && d < (long long)room && d + (long long)n > 0) {
                            u32 v = compact_extract(col[g], sel, cnt);
                            if (d < 0) { // the bits in front of the item belong to the output segment before
                                v >>= (u32)(-d);
                                n -= (u32)(-d);
                                d = 0;
                            }
                            if ((u32)d + n > room) n = room - (u32)d; // ... and those behind it to the next
                            v &= (1u << n) - 1u;                      // (n <= 31)
                            const u32 dg = (u32)d / 31u, off = (u32)d - 31u * dg; // dg <= 1023, and dg + 1 <= 1023 where off + n > 31
                            const u32 low = (v << off) & kOnes31;
                            if (low) atomicOr(dst + dg, low);
                            if (off + n > 31u) {
                                const u32 high = v >> (31u - off);
                                if (high) atomicOr(dst + dg + 1u, high);
                            }
                        }
                        carry += step_total;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the next walk fills the two source images
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            total = image_words<kEmit>(dst, ngroups, stage, lane);
        }
        item_tail<kEmit>(a, a.offsets, item, total, stage, lane);
    }
}

} // namespace

// the rank pass over the mask, its scan, and the one lane that writes T and judges it
hipError_t launch_compact_check(const CompactArgs &a, hipStream_t s) {
    const u64 want = (a.src_segments + kSegDecodeWaves - 1) / kSegDecodeWaves;
    constexpr u64 most = 256u * 8u; // CUs x resident workgroups of four wavefronts at eight waves per SIMD
    hipLaunchKernelGGL(compact_rank_kernel, dim3((unsigned)(want < 1 ? 1 : want > most ? most : want)), dim3(kSegDecodeWaves * 64), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_select_rank_scan(a.starts, a.src_segments, a.level1, a.level2, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(compact_total_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

// count pass (emit = false: every item's words to a.offsets) or emit pass (a.offsets scanned: the words to their place)
hipError_t launch_compact_segments(const CompactArgs &a, bool emit, hipStream_t s) {
    constexpr u64 most = 256u * 3u; // CUs x resident workgroups of four wavefronts at 48 KiB of LDS each
    return launch_count_or_emit(compact_segments_kernel<false>, compact_segments_kernel<true>, emit, a.n_columns * a.n_segments, kSegDecodeWaves, most, a, s);
}

} // namespace wah
