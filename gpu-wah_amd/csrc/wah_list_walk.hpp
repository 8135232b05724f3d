// wah_list_walk.hpp -- the walk over a table of indexed compressed bitmaps (wah_bitop_operand, include/wah.h) by one wavefront, for
// one segment: every row's words of that segment applied to an image of the segment's 1024 groups in LDS (list_walk), the sweep
// that keeps one row at a time in the zeroed image (row_sweep), the segment a wavefront owns (wave_segment), image_fill and
// report_stream_error.  Written once for the kernels that read such a table: the queries of wah_bitop_list.hip, the
// (column, segment) items of wah_splice.hip, wah_compact.hip and wah_update.hip, and the (segment, half) items of wah_values.hip and
// wah_member.hip.
//
// One wavefront owns one output segment; its accumulator is the segment's 1024 groups in LDS (4 KiB per wavefront, 16 KiB per
// workgroup: bitop_many_segments_kernel holds 20).  An operand's segment is never expanded: its words are loaded in batches of
// 128 (two per lane, through a descriptor clipped to the segment's range, as seg_load_words loads them), one wave scan per
// batch gives every word the group it starts at (the clamps and the "exactly nvalid groups, no empty word" check of
// seg_mark), and every word is applied where it lies --
//   a literal            combines into its one group;
//   a fill that is the operation's identity (zeros under OR / XOR / ANDNOT, ones under AND: most of a sparse or clustered
//                        operand) costs nothing beyond its load and its share of the scan;
//   a fill with an effect (ones under OR: set, XOR: flip, ANDNOT: clear; zeros under AND: clear) of up to kListShortFill groups
//                        is applied by its own lane, a longer one by the whole wave, 64 groups per step, the long fills of a
//                        batch one after the other off a ballot mask.
// Every group of the segment is covered by exactly one word of an operand (the scan's positions are disjoint whatever the words
// say), so no two lanes touch one accumulator group for one operand: no atomics.  A segment's cost goes with the words the
// operands hold there plus the length of the fills that change the result, not with n_operands x 1024 groups.
#ifndef WAH_LIST_WALK_HPP_
#define WAH_LIST_WALK_HPP_
#include "wah_segdecode.hpp"

namespace wah {
namespace {

constexpr u32 kListShortFill = 8; // groups of a fill up to which its own lane applies it
#ifndef WAH_LIST_DEPTH
#define WAH_LIST_DEPTH 4
#endif
constexpr int kListDepth = WAH_LIST_DEPTH; // batches of 128 words in flight per wave

// the operation on the accumulator (runs_op(), wah_device.hpp), and the kind of fill that changes it
struct ListOp {
    RunsOp m;
    u32 fill;     // kFillOne or kFillZero
    u32 fill_val; // its 31 bits
};
__device__ __forceinline__ ListOp list_op(u32 op) {
    ListOp o;
    o.m = runs_op(op);
    o.fill = op == 0u ? kFillZero : kFillOne;
    o.fill_val = op == 0u ? 0u : kOnes31;
    return o;
}
__device__ __forceinline__ u32 list_combine(u32 r, u32 v, const ListOp &o) { return runs_combine(r, v, o.m); }

typedef const __attribute__((address_space(1))) u64 *ListGlobalU64;
typedef const __attribute__((address_space(1))) u32 *ListGlobalU32;
// 64 operands of the table, one per lane: where each one's words of segment `seg` lie
struct ListChunk {
    u32 addr_lo, addr_hi; // the segment's first word
    u32 cnt;              // its words; 0: no such operand, one that is refused (bad), or one that is settled (list_gather)
    bool bad;
};
__device__ __forceinline__ ListChunk list_gather(const BitopListOperand *table, u32 j0, u32 n, u64 seg, u32 nvalid, u32 fill_with_effect, u32 lane) {
    const u32 j = j0 + lane;
    const bool has = j < n;
    u64 comp = 0, c_words = 0, offs = 0;
    if (has) {
        const u64 *e = reinterpret_cast<const u64 *>(table + j);
        comp = e[0];
        c_words = e[1];
        offs = e[2];
    }
    // an entry is checked before a pointer of it is followed ...
    const bool entry_ok = has && offs != 0ull && (offs & 7ull) == 0ull && comp != 0ull && (comp & 3ull) == 0ull && c_words < (1ull << 40);
    u64 w0 = 0, w1 = 0;
    if (entry_ok) {
        const ListGlobalU64 p = (ListGlobalU64)(uintptr_t)offs + seg; // (global, not generic: no aperture test)
        w0 = p[0];
        w1 = p[1];
    }
    // ... and a range before the stream is read through it: inside the stream, in order, at least one word (the segment has
    // groups) and at most one per group
    ListChunk c;
    c.bad = has && (!entry_ok || w1 <= w0 || w1 > c_words || w1 - w0 > nvalid);
    c.cnt = has && !c.bad ? (u32)(w1 - w0) : 0u;
    const u64 addr = comp + 4ull * w0;
    // A segment that is ONE fill of all its groups and the operation's identity (a bin of a clustered index: nearly all of its
    // segments) is complete and changes nothing: it is settled here, 64 operands at a time, and never becomes a batch.  (Its word
    // is read inside the range just checked; anything else of one word -- a fill with an effect, a wrong count -- goes the
    // general way and is applied or refused there.)
    if (c.cnt == 1u) {
        const u32 only = *(ListGlobalU32)(uintptr_t)addr;
        if (only >= kFillZero && (only & kCountMask) == nvalid && (only & kFillOne) != fill_with_effect) c.cnt = 0u;
    }
    c.addr_lo = (u32)addr;
    c.addr_hi = (u32)(addr >> 32);
    return c;
}

// a place in the chunk's sequence of batches: batch b of the operand in lane j (64: behind the last one)
struct ListCursor {
    u32 j, b;
};
__device__ __forceinline__ ListCursor list_first(u64 live) {
    ListCursor c;
    c.j = live ? (u32)__builtin_ctzll(live) : 64u;
    c.b = 0;
    return c;
}
__device__ __forceinline__ void list_advance(ListCursor &c, const ListChunk &ch, u64 live) {
    if (c.j >= 64u) return;
    const u32 cnt = (u32)__builtin_amdgcn_readlane((int)ch.cnt, (int)c.j);
    if (128u * (c.b + 1u) < cnt) {
        ++c.b;
    } else {
        const u64 m = c.j >= 63u ? 0ull : live & (~0ull << (c.j + 1u)); // the next operand that has words
        c.j = m ? (u32)__builtin_ctzll(m) : 64u;
        c.b = 0;
    }
}
// the batch's words, two per lane (reads past the range return 0; behind the last batch: a descriptor of no bytes, nothing is read)
// (ONE 8-byte load into a register pair that stays a pair: two 4-byte loads are merged by the compiler and taken apart again with
//  moves, which wait for the load -- and nothing would be in flight)
typedef u32 ListPair __attribute__((__vector_size__(8)));
__device__ __forceinline__ void list_issue(ListPair &q, const ListCursor &c, const ListChunk &ch, u32 lane) {
    const int jj = (int)min(c.j, 63u);
    const u32 cnt = c.j < 64u ? (u32)__builtin_amdgcn_readlane((int)ch.cnt, jj) : 0u;
    const u64 addr = ((u64)(u32)__builtin_amdgcn_readlane((int)ch.addr_hi, jj) << 32) | (u32)__builtin_amdgcn_readlane((int)ch.addr_lo, jj);
    const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(reinterpret_cast<const void *>(addr), cnt * 4u);
    const u32 off = (128u * c.b + 2u * lane) * 4u;
    q = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0);
}

// what a word's own lane applies: n groups of v from p on -- a literal (n = 1) or a short fill with an effect; the first group, and,
// where a batch has such fills at all, the rest
__device__ __forceinline__ void list_put_first(u32 *acc, u32 p, u32 n, u32 v, const ListOp &m) {
    if (n) acc[p] = list_combine(acc[p], v, m);
}
__device__ __forceinline__ void list_put_rest(u32 *acc, u32 p, u32 n, u32 v, const ListOp &m) {
    u32 t[kListShortFill];
#pragma unroll
    for (u32 i = 1; i < kListShortFill; ++i)
        if (i < n) t[i] = acc[p + i];
#pragma unroll
    for (u32 i = 1; i < kListShortFill; ++i)
        if (i < n) acc[p + i] = list_combine(t[i], v, m);
}
// the long fills with an effect of one batch (mask: the lanes that hold one; p, n: where each lies), by the whole wave
__device__ __forceinline__ void list_put_long(u32 *acc, u64 mask, u32 p, u32 n, const ListOp &m, u32 lane) {
    while (mask) {
        const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask));
        mask &= mask - 1ull;
        const u32 g0 = (u32)__builtin_amdgcn_readlane((int)p, l), g1 = g0 + (u32)__builtin_amdgcn_readlane((int)n, l);
        for (u32 g = g0 + lane; g < g1; g += 64u) acc[g] = list_combine(acc[g], m.fill_val, m);
    }
}

// One batch (words wi .. wi + 127 of an operand's `cnt`, w0 / w1 two per lane) applied to the accumulator; pos: the groups the
// operand's batches have covered so far.  Nothing is put outside the accumulator whatever the words say.
__device__ __forceinline__ void list_apply_batch(u32 *acc, u32 w0, u32 w1, u32 wi, u32 cnt, u32 &pos, bool &empty_word, const ListOp &m, u32 lane) {
    // a full batch of literals (dense data: all of its batches) is 128 consecutive groups: no scan, no fills to look for
    if (wi + 128u <= cnt && pos + 128u <= kSegGroups && __ballot((int)(w0 | w1) < 0) == 0ull) { // wave-uniform
        const u32 p = pos + 2u * lane;
        const u32 r0 = acc[p], r1 = acc[p + 1u];
        acc[p] = list_combine(r0, w0, m);
        acc[p + 1u] = list_combine(r1, w1, m);
        pos += 128u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        return;
    }
    const u32 i0 = wi + 2u * lane;
    const bool in0 = i0 < cnt, in1 = i0 + 1u < cnt;
    // counts are clamped so that a corrupt word cannot wrap the 32-bit sums; anything above 1024 fails the total
    const u32 n0 = in0 ? min(word_groups(w0), 2u * kSegGroups) : 0u, n1 = in1 ? min(word_groups(w1), 2u * kSegGroups) : 0u;
    empty_word |= (in0 && n0 == 0u) || (in1 && n1 == 0u);
    const u32 incl = wave_scan_incl32(n0 + n1);
    const u32 p1 = pos + incl - n1, p0 = p1 - n0;
    const bool a0 = in0 && p0 + n0 <= kSegGroups, a1 = in1 && p1 + n1 <= kSegGroups;
    const bool lit0 = (int)w0 >= 0, lit1 = (int)w1 >= 0;
    const bool eff0 = a0 && (w0 & kFillOne) == m.fill, eff1 = a1 && (w1 & kFillOne) == m.fill; // (bits 31, 30: a fill of that kind)
    const u32 v0 = lit0 ? w0 : m.fill_val, v1 = lit1 ? w1 : m.fill_val;
    // what the lane applies itself: its literals (one group) and its short fills with an effect
    const u32 s0 = a0 && lit0 ? 1u : (eff0 && n0 <= kListShortFill ? n0 : 0u);
    const u32 s1 = a1 && lit1 ? 1u : (eff1 && n1 <= kListShortFill ? n1 : 0u);
    list_put_first(acc, p0, s0, v0, m);
    list_put_first(acc, p1, s1, v1, m);
    if (__ballot(s0 > 1u || s1 > 1u) != 0ull) {
        list_put_rest(acc, p0, s0, v0, m);
        list_put_rest(acc, p1, s1, v1, m);
    }
    list_put_long(acc, __ballot(eff0 && n0 > kListShortFill), p0, n0, m, lane);
    list_put_long(acc, __ballot(eff1 && n1 > kListShortFill), p1, n1, m, lane);
    pos += (u32)__builtin_amdgcn_readlane((int)incl, 63);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the next batch's (the next operand's) lanes touch other groups than these
}

// The walk over the first n_rows rows of a table, for segment `seg` of nvalid groups: every row's words of that segment applied to
// the accumulator in the table's order.  op_of(j): the operation row j is applied with (fill_with_effect: the kind of fill that
// changes the accumulator under it, kFillOne or kFillZero -- one kind for the whole walk); begin_row(j) is called, wave-uniform,
// before the first batch of row j is applied -- where a kernel that keeps one row at a time in the accumulator folds the rows in
// front of j.  Returns the verdict, wave-uniform: no row refused, no empty word, every row's words exactly nvalid groups.
//
// What such a wave waits for is memory, not instructions: an index bin of a few words per segment is two dependent round
// trips (table entry -> index pair -> words) for a hundred instructions.  With the next operand's words in flight while the
// current one is applied (the x / y rotation of bitop_many_segments_kernel, table entries and index pairs by scalar loads) every
// operand still costs a whole round trip: 256 clustered operands of 32 MiB took 0.75 ms, 0.013 of the roofline.  So the
// pipeline is not by operand:
//   * the table is walked 64 rows at a time, one row per LANE: entry, check, index pair, range check -- two round trips
//     per 64 rows, by vector loads (an entry is checked before its index pointer is followed, a range before the stream is
//     read through it);
//   * the unit in flight is a BATCH of 128 words, whatever row it belongs to: kListDepth batches are always on their way
//     (a producer cursor runs that far ahead of the consumer's over the 64 rows' batches), in registers of their own --
//     the loop is unrolled by the depth, so no batch is ever moved -- eight registers instead of the thirty-two of two whole
//     segments, which lets eight waves per SIMD stay resident.
// ... and it is instructions: with memory out of the way the walk is bound by what it issues per batch (about 125 wave
// instructions: 256 random bins of 221 words per segment 0.89 ms).  Two cases therefore never reach the general batch code: a
// segment that is ONE fill of all its groups and the operation's identity -- nearly every segment of a clustered bin -- is
// settled while the chunk is gathered, 64 rows at a time (list_gather); a full batch of literals -- every batch of a
// dense operand -- is 128 consecutive groups, combined without scan or fill tests (list_apply_batch).
// A settled row never becomes a batch, so begin_row is not called for it: a caller finds the rows it has to fold from the row
// NUMBERS it is given, and folds the rows behind the last one that had words after the walk.
template <class OpOf, class BeginRow>
__device__ __forceinline__ bool list_walk(const BitopListOperand *table, u32 n_rows, u64 seg, u32 nvalid, u32 fill_with_effect, u32 *acc, u32 lane,
                                          OpOf op_of, BeginRow begin_row) {
    bool lane_bad = false, empty_word = false; // per lane: a refused row of mine; an empty word among mine
    bool sums_ok = true;                       // wave-uniform: every row's words made up exactly nvalid groups
#pragma nounroll
    for (u32 j0 = 0; j0 < n_rows; j0 += 64u) {
        const ListChunk ch = list_gather(table, j0, n_rows, seg, nvalid, fill_with_effect, lane);
        lane_bad |= ch.bad;
        const u64 live = __ballot(ch.cnt != 0u);
        ListCursor prod = list_first(live), cons = prod;
        ListPair q[kListDepth];
#pragma unroll
        for (int i = 0; i < kListDepth; ++i) {
            list_issue(q[i], prod, ch, lane);
            list_advance(prod, ch, live);
        }
        u32 pos = 0;
#pragma nounroll
        while (cons.j < 64u) {
#pragma unroll
            for (int i = 0; i < kListDepth; ++i) {
                if (cons.j < 64u) { // wave-uniform
                    const u32 cnt = (u32)__builtin_amdgcn_readlane((int)ch.cnt, (int)cons.j);
                    const u32 wi = 128u * cons.b;
                    if (cons.b == 0u) {
                        pos = 0u;
                        begin_row(j0 + cons.j);
                    }
                    list_apply_batch(acc, q[i][0], q[i][1], wi, cnt, pos, empty_word, op_of(j0 + cons.j), lane);
                    if (wi + 128u >= cnt) sums_ok = sums_ok && pos == nvalid; // the row's last batch
                }
                list_advance(cons, ch, live);
                list_issue(q[i], prod, ch, lane); // (into the registers just used: no batch is ever moved)
                list_advance(prod, ch, live);
            }
        }
    }
    return sums_ok && __ballot(lane_bad || empty_word) == 0ull;
}

// the segment a wavefront owns: number k of the launch's, `seg` of the bitmap, nvalid groups (1024 but for the bitmap's last)
struct WaveSegment {
    u64 k, seg;
    u32 nvalid;
};
// false: the launch has no segment for this wave
__device__ __forceinline__ bool wave_segment(WaveSegment &w, u64 first_segment, u64 n_segments, u64 groups, u32 wave) {
    w.k = (u64)blockIdx.x * kSegDecodeWaves + wave;
    if (w.k >= n_segments) return false;
    w.seg = first_segment + w.k;
    w.nvalid = segment_groups(groups, w.seg);
    return true;
}

// all 1024 groups of a wave's LDS image set to v, fenced: the wave's other lanes read and write them next
__device__ __forceinline__ void image_fill(u32 *acc, u32 v, u32 lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) reinterpret_cast<uint4 *>(acc)[64 * i + (int)lane] = make_uint4(v, v, v, v);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// The sweep of a kernel that keeps ONE row of the table at a time in the image: the walk under OR into the zeroed image `acc`,
// and fold_row(cur), wave-uniform, once for every row cur = 0 .. n_fold - 1 in order, while the image holds exactly that row.
// Returns the walk's verdict.
//   * The crossing to another row is found from row NUMBERS: a row settled in the gather never reaches begin_row, so when
//     row j's words begin every row in front of j is folded -- the settled ones as the zeros they are, out of the image that
//     the fold before them left zeroed.
//   * Two fences frame the zeroing: the first keeps fold_row's reads of the image, which are other lanes' groups than the
//     lane's own 16-byte stores cover, in front of those stores; the second (image_fill's) keeps the stores in front of the
//     next row's words.
//   * The tail: begin_row is only ever called by a row that has words, so the last row, and the settled ones in front of it,
//     are folded behind the walk.  n_fold is n_rows, or n_rows - 1 for a caller that wants the last row left in the image.
template <class FoldRow>
__device__ __forceinline__ bool row_sweep(const BitopListOperand *table, u32 n_rows, u32 n_fold, const WaveSegment &w, u32 *acc, u32 lane,
                                          FoldRow fold_row) {
    u32 cur = 0; // the row the image holds
    auto fold = [&]() {
        fold_row(cur);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        image_fill(acc, 0u, lane);
        ++cur;
    };
    const ListOp m = list_op(1u);
    const bool ok = list_walk(table, n_rows, w.seg, w.nvalid, m.fill, acc, lane, [&](u32) -> const ListOp & { return m; }, [&](u32 j) {
#pragma nounroll
        while (cur < j) fold();
    });
#pragma nounroll
    while (cur < n_fold) fold();
    return ok;
}

// a wave that refused something: the launch reports kErrStream (and a walk kernel's wave returns without storing)
__device__ __forceinline__ void report_stream_error(u32 *ctrl, u32 lane) {
    if (lane == 0) atomicOr(ctrl + kCtlError, kErrStream);
}

} // namespace
} // namespace wah
#endif // WAH_LIST_WALK_HPP_
