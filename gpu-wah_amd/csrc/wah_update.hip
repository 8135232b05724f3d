// wah_update.hip -- wah_update_indexed_device: the rows a mask bitmap selects of every column of an index take a new value, all
// other rows keep theirs -- UPDATE t SET x = 5 WHERE ..., the MERGE of a corrected batch, CASE WHEN p THEN a ELSE b END.  Output
// column c is then_c where the mask selects a row and else_c everywhere else, written as wah_compact_indexed_device writes its
// output: the columns' compress() streams back to back and the index of the whole.  No decoded bitmap exists at any point.
//
// No rows move, so segment s of an output column depends only on segment s of the mask, of the else column and of the then
// column: the (column, segment) item of compact_segments_kernel without ranks, searches, extraction or deposits, and a call with
// no check launch.  Only positions below n_rows are selected; the pad bits of the bitmap's last group are zero in the output
// whatever the sources hold there.
//
// The launches, none of whose workgroups waits for another:
//   update_segments_kernel<false>  (segment, column) items shared out over the launch's wavefronts in contiguous runs, enumerated
//                            SEGMENT-major (j = seg * n_columns + c, index entry c * S + seg): the mask segment is walked into its
//                            image of 1024 groups in LDS once per (wavefront, segment), clipped there to the rows below n_rows,
//                            and kept across the columns.  The walk is under OR into zeros, so a mask segment that is one zero
//                            fill is the walk's identity and costs no image pass.  Per column the else entry is walked into the
//                            destination image (a constant fills it); where the clipped mask selects a row of the segment the
//                            then entry is walked into a third image (a constant needs none) and every lane blends its groups,
//                            dst = (dst & ~sel) | (then & sel), 64 groups per step.  The pad bits are cleared, the image becomes
//                            words (image_words), the count goes to offsets[c * S + seg].
//   (launch_select_rank_scan turns the counts into the index in place.)
//   update_segments_kernel<true>   the same items again; the words are staged in the then image's LDS, which is free once the
//                            blend is done, and leave it 64 consecutive words per store instruction, clipped by the room the
//                            count pass found and by the capacity.
// The mask and every else entry that is no constant are read and checked in every segment, a then entry only in the segments
// where the clipped mask selects a row.  After a refused mask segment the wavefront reads no column.
// Three images of 4 KiB per wavefront, 48 KiB per workgroup of four: three workgroups per CU (160 KiB of LDS).
#include "wah_count_emit.hpp"
#include "wah_list_walk.hpp"

namespace wah {
namespace {

constexpr int kUpdateWavesPerSimd = 3;

// what a row of the else or the then table names
constexpr u32 kUpdateZeros = 0, kUpdateOnes = 1, kUpdateStream = 2, kUpdateBad = 3;
// Both pointers null: a constant, stream_words its bit (more than 1: refused).  Anything else is a stream for list_walk, which
// refuses a row with exactly one null pointer.  (wave-uniform: every lane reads the same three words)
__device__ __forceinline__ u32 update_kind(const BitopListOperand *row) {
    const u64 *e = reinterpret_cast<const u64 *>(row);
    const u64 comp = uniform64(e[0]), words = uniform64(e[1]), offs = uniform64(e[2]);
    if (comp != 0ull || offs != 0ull) return kUpdateStream;
    return words == 0ull ? kUpdateZeros : words == 1ull ? kUpdateOnes : kUpdateBad;
}

template <bool kEmit>
__global__ __launch_bounds__(kSegDecodeWaves * 64, kUpdateWavesPerSimd) void update_segments_kernel(const UpdateArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_mask[kSegDecodeWaves][kSegGroups];
    __shared__ __attribute__((aligned(16))) u32 s_then[kSegDecodeWaves][kSegGroups];
    __shared__ __attribute__((aligned(16))) u32 s_dst[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    if ((a.ctrl[kCtlError] & kErrStream) != 0u) return; // a refused stream (in the emit pass: the index is not one): nothing more is read
    u32 *msk = s_mask[wave], *thn = s_then[wave], *dst = s_dst[wave];
    u32 *stage = thn; // (the emit pass: the then image is free once the blend is done)
    const u64 n_items = a.n_columns * a.n_segments;
    const ItemRun run = item_run(n_items, kSegDecodeWaves, wave);
    const u64 begin = run.begin, end = run.end;
    emit_total<kEmit>(a, a.offsets, n_items, run, lane);
    const ListOp m_or = list_op(1u); // a segment is ORed into the zeroed image
    const u32 last_bits = (u32)(a.n_bits - 31ull * (a.groups - 1)); // the bits of the bitmap's last group that are positions: 1 .. 31
    u64 seg_in_image = ~0ull; // the segment whose clipped mask the mask image holds
    bool touched = false;     // a word was applied to the mask image: it may differ from zeros
    bool selects = false;     // the clipped mask selects a row of that segment
    image_fill(msk, 0u, lane);
    u64 seg = begin / a.n_columns, c = begin - seg * a.n_columns;
#pragma nounroll
    for (u64 j = begin; j < end; ++j, ++c) {
        if (c == a.n_columns) {
            c = 0;
            ++seg;
        }
        const u32 nvalid = segment_groups(a.groups, seg);
        if (seg != seg_in_image) { // (wave-uniform) the mask segment: once per wavefront and segment
            if (touched) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                image_fill(msk, 0u, lane);
            }
            touched = false;
            selects = false;
            seg_in_image = seg;
            const bool ok = list_walk(a.mask, 1u, seg, nvalid, m_or.fill, msk, lane, [&](u32) -> const ListOp & { return m_or; }, [&](u32) { touched = true; });
            if (!ok) return report_stream_error(a.ctrl, lane); // no column is read behind a refused mask segment
            if (touched) {
                const u32 seg_rows = segment_rows(a.n_rows, seg);
                u32 any = 0;
#pragma unroll
                for (u32 s = 0; s < kSteps; ++s) {
                    const u32 g = 64u * s + lane;
                    const u32 sel = msk[g] & group_row_bits(g, seg_rows);
                    msk[g] = sel;
                    any |= sel;
                }
                selects = __ballot(any != 0u) != 0ull;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
        }
        // the else entry into the destination image
        const u32 else_kind = update_kind(a.else_table + c);
        if (else_kind == kUpdateBad) return report_stream_error(a.ctrl, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        image_fill(dst, else_kind == kUpdateOnes ? kOnes31 : 0u, lane);
        if (else_kind == kUpdateStream &&
            !list_walk(a.else_table + c, 1u, seg, nvalid, m_or.fill, dst, lane, [&](u32) -> const ListOp & { return m_or; }, [](u32) {}))
            return report_stream_error(a.ctrl, lane);
        const u32 then_kind = update_kind(a.then_table + c);
        if (then_kind == kUpdateBad) return report_stream_error(a.ctrl, lane);
        if (selects) { // (wave-uniform) the then entry, and the blend
            if (then_kind == kUpdateStream) {
                image_fill(thn, 0u, lane);
                if (!list_walk(a.then_table + c, 1u, seg, nvalid, m_or.fill, thn, lane, [&](u32) -> const ListOp & { return m_or; }, [](u32) {}))
                    return report_stream_error(a.ctrl, lane);
            }
            const u32 then_const = then_kind == kUpdateOnes ? kOnes31 : 0u;
#pragma unroll
            for (u32 s = 0; s < kSteps; ++s) {
                const u32 g = 64u * s + lane;
                const u32 sel = msk[g];
                const u32 t = then_kind == kUpdateStream ? thn[g] : then_const;
                dst[g] = (dst[g] & ~sel) | (t & sel);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (seg + 1 == a.n_segments && lane == 0) dst[nvalid - 1u] &= (1u << last_bits) - 1u; // the pad bits of the bitmap's last group
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const u32 total = image_words<kEmit>(dst, nvalid, stage, lane);
        const u64 item = c * a.n_segments + seg;
        item_tail<kEmit>(a, a.offsets, item, total, stage, lane);
    }
}

} // namespace

// the call has nothing to find out before its items run
hipError_t launch_update_check(const UpdateArgs &, hipStream_t) { return hipSuccess; }

// count pass (emit = false: every item's words to a.offsets) or emit pass (a.offsets scanned: the words to their place)
hipError_t launch_update_segments(const UpdateArgs &a, bool emit, hipStream_t s) {
    constexpr u64 most = 256u * 3u; // CUs x resident workgroups of four wavefronts at 48 KiB of LDS each
    return launch_count_or_emit(update_segments_kernel<false>, update_segments_kernel<true>, emit, a.n_columns * a.n_segments, kSegDecodeWaves, most, a, s);
}

} // namespace wah
