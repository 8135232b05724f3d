// wah_splice.hip -- wah_splice_indexed_device: row ranges ("pieces") of indexed bitmaps concatenated into new indexed bitmaps, at any bit offset,
// for all columns of an index at once -- INSERT of a batch, a window of rows, the rollover of a partition.  The output is written
// as wah_from_positions_device writes it: the columns' compress() streams back to back and the index of the whole.
//
// Like the fetch call, ONLY the source segments that hold a spliced row are walked.  Three kinds of launches, and no workgroup of
// any of them waits for another:
//   splice_check_kernel      one workgroup: every piece is checked (rows inside its operands, no more rows than the output
//                            holds, without wrapping) and the running starts start(0 .. n_pieces) are left in the scratch; a
//                            refused piece counts as no rows.  Nothing is read through a piece unless EVERY piece was accepted:
//                            with a stream error in the control block the other launches return at once.
//   splice_segments_kernel<false>  (column, output segment) items shared out over the launch's wavefronts in contiguous runs,
//                            as from_positions_kernel shares its items out (item_run, wah_count_emit.hpp).  A wavefront
//                            searches the starts (first_end_behind, wah_device.hpp) for the pieces
//                            that overlap its bit range [31744 s, 31744 (s + 1)), and for every one of them and every source
//                            segment the piece's range touches here -- 31 744 bits lie in at most two -- walks the ONE table
//                            entry (piece, column) for that source segment into a zeroed source image (list_walk under OR),
//                            then moves the bits onto the destination's group grid (splice_move) and ORs them into the
//                            destination image.  The image becomes words as in from_positions_kernel (image_words); the
//                            count goes to offsets[item].
//   (launch_select_rank_scan turns the counts into the index in place.)
//   splice_segments_kernel<true>   the same items again; the words are staged in the source image's LDS and leave it 64
//                            consecutive words per store instruction, clipped by the room the count pass found and by the capacity.
// Two images of 4 KiB per wavefront, 32 KiB per workgroup of four: five workgroups per CU.
#include "wah_count_emit.hpp"
#include "wah_list_walk.hpp"

namespace wah {
namespace {

constexpr u32 kSpliceCheckThreads = 256;
constexpr int kSpliceWavesPerSimd = 5;

// the rows piece p adds to the output: n_rows, or 0 for a refused piece (bad is set).  A piece of no rows is legal whatever else it says.
__device__ __forceinline__ u64 splice_piece_rows(const SpliceArgs &a, u64 p, bool &bad) {
    const SplicePiece pc = a.pieces[p];
    if (pc.n_rows == 0ull) return 0ull;
    // (in this order nothing wraps: 32 n_words < 2^45, and first_row is below it before it is subtracted)
    const bool ok = pc.n_words != 0ull && pc.n_words < (1ull << 40) && pc.n_rows <= a.n_bits && pc.first_row <= 32ull * pc.n_words &&
                    pc.n_rows <= 32ull * pc.n_words - pc.first_row;
    bad |= !ok;
    return ok ? pc.n_rows : 0ull;
}

__global__ __launch_bounds__(256) void splice_check_kernel(const SpliceArgs a) {
    __shared__ u64 s_sum[kSpliceCheckThreads];
    const u32 t = threadIdx.x;
    const u64 per = (a.n_pieces + kSpliceCheckThreads - 1u) / kSpliceCheckThreads;
    const u64 begin = t * per < a.n_pieces ? t * per : a.n_pieces, end = begin + per < a.n_pieces ? begin + per : a.n_pieces;
    bool bad = false;
    u64 sum = 0; // (at most 2^16 pieces of at most 2^45 rows each)
    for (u64 p = begin; p < end; ++p) sum += splice_piece_rows(a, p, bad);
    s_sum[t] = sum;
    __syncthreads();
    u64 at = 0;
    for (u32 i = 0; i < t; ++i) at += s_sum[i];
    for (u64 p = begin; p < end; ++p) {
        a.starts[p] = at;
        at += splice_piece_rows(a, p, bad);
    }
    if (t == kSpliceCheckThreads - 1u) { // (its run ends at n_pieces: `at` is the total)
        a.starts[a.n_pieces] = at;
        bad |= at > a.n_bits;
    }
    if (__ballot(bad) != 0ull) report_stream_error(a.ctrl, lane_id());
}

// `len` >= 1 bits of the source image from bit sb on, ORed into the destination image from bit db on (both below 31 744, the
// ranges inside their images).  With delta = sb - db = 31 q + r, 0 <= r < 31: bit j of destination group d is bit j + r of
// source group d + q, or bit j + r - 31 of the group behind it.  Groups outside the image read as zero; what a source holds
// outside [sb, sb + len) -- set pad bits of a foreign stream among it -- dies in the mask.  A lane writes only groups 64 k +
// lane of the destination, its own in every call, and reads other lanes' groups of the source: the caller fences in front.
__device__ __forceinline__ void splice_move(const u32 *src, u32 *dst, u32 sb, u32 db, u32 len, u32 lane) {
    const int delta = (int)sb - (int)db;
    const int q = delta >= 0 ? delta / 31 : -((30 - delta) / 31);
    const u32 r = (u32)(delta - 31 * q);
    const u32 g_first = db / 31u, g_last = (db + len - 1u) / 31u;
#pragma nounroll
    for (u32 k = g_first / 64u; k <= g_last / 64u; ++k) {
        const u32 d = 64u * k + lane;
        if (d >= g_first && d <= g_last) {
            const int i = (int)d + q;
            const u32 x = i >= 0 && i < (int)kSegGroups ? src[i] : 0u;
            const u32 y = i + 1 >= 0 && i + 1 < (int)kSegGroups ? src[i + 1] : 0u;
            const u32 v = ((x >> r) | (y << (31u - r))) & kOnes31;
            const int lo = max((int)db - 31 * (int)d, 0), hi = min((int)(db + len) - 31 * (int)d, 31); // (0 <= lo < hi <= 31)
            dst[d] |= v & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the next walk zeroes the source image
}

template <bool kEmit>
__global__ __launch_bounds__(kSegDecodeWaves * 64, kSpliceWavesPerSimd) void splice_segments_kernel(const SpliceArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_src[kSegDecodeWaves][kSegGroups];
    __shared__ __attribute__((aligned(16))) u32 s_dst[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    if ((a.ctrl[kCtlError] & kErrStream) != 0u) return; // a refused piece (or, in the emit pass, stream): no stream is read
    u32 *src = s_src[wave], *dst = s_dst[wave];
    u32 *stage = src; // (the emit pass: the source image is free once the bits are moved)
    const u64 n_items = a.n_columns * a.n_segments;
    const ItemRun run = item_run(n_items, kSegDecodeWaves, wave);
    emit_total<kEmit>(a, a.offsets, n_items, run, lane);
    const u64 all_rows = uniform64(a.starts[a.n_pieces]); // T: at most 32 n_words_out (the check launch)
    const ListOp m = list_op(1u);                         // a source segment is ORed into the zeroed image
#pragma nounroll
    for (u64 item = run.begin; item < run.end; ++item) {
        const u64 c = item / a.n_segments, seg = item - c * a.n_segments;
        const u64 base = seg * (u64)kSegBits;
        const u32 ngroups = seg + 1 == a.n_segments ? (u32)(a.groups - seg * kSegGroups) : kSegGroups;
        u32 total;
        if (base >= all_rows) { // behind the last piece
            total = lone_zero_fill<kEmit>(ngroups, stage, lane);
        } else {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            image_fill(dst, 0u, lane);
            const u64 limit = base + kSegBits < all_rows ? base + kSegBits : all_rows;
            // from the first piece that ends behind `base` (there is one: base < T)
#pragma nounroll
            for (u64 p = first_end_behind(a.starts, a.n_pieces, base); p < a.n_pieces; ++p) {
                const u64 st = uniform64(a.starts[p]), en = uniform64(a.starts[p + 1]);
                if (st >= limit) break;
                if (en <= st || en <= base) continue; // (no rows; en <= base only for pieces of no rows at `base`)
                const u64 d0 = st > base ? st : base, d1 = en < limit ? en : limit;
                const u64 n_words = uniform64(a.pieces[p].n_words), first_row = uniform64(a.pieces[p].first_row);
                const u64 s0 = first_row + (d0 - st), s1 = s0 + (d1 - d0); // (accepted: s1 <= 32 n_words)
                const u64 src_groups = (32ull * n_words + 30ull) / 31ull;
                const BitopListOperand *entry = a.table + (p * a.n_columns + c);
#pragma nounroll
                for (u64 ss = s0 / kSegBits; ss * kSegBits < s1; ++ss) {
                    const u64 sbase = ss * kSegBits;
                    const u64 t0 = s0 > sbase ? s0 : sbase, t1 = s1 < sbase + kSegBits ? s1 : sbase + kSegBits;
                    if (ss * kSegGroups >= src_groups) break; // (never for an accepted piece)
                    const u32 nvalid = segment_groups(src_groups, ss);
                    image_fill(src, 0u, lane);
                    const bool ok = list_walk(entry, 1u, ss, nvalid, m.fill, src, lane, [&](u32) -> const ListOp & { return m; }, [](u32) {});
                    if (!ok) return report_stream_error(a.ctrl, lane);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    splice_move(src, dst, (u32)(t0 - sbase), (u32)(d0 + (t0 - s0) - base), (u32)(t1 - t0), lane);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            total = image_words<kEmit>(dst, ngroups, stage, lane);
        }
        item_tail<kEmit>(a, a.offsets, item, total, stage, lane);
    }
}

} // namespace

hipError_t launch_splice_check(const SpliceArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(splice_check_kernel, dim3(1), dim3(kSpliceCheckThreads), 0, s, a);
    return hipGetLastError();
}

// count pass (emit = false: every item's words to a.offsets) or emit pass (a.offsets scanned: the words to their place)
hipError_t launch_splice_segments(const SpliceArgs &a, bool emit, hipStream_t s) {
    constexpr u64 most = 256u * 5u; // CUs x resident workgroups of four wavefronts at 32 KiB of LDS each
    return launch_count_or_emit(splice_segments_kernel<false>, splice_segments_kernel<true>, emit, a.n_columns * a.n_segments, kSegDecodeWaves, most, a, s);
}

} // namespace wah
