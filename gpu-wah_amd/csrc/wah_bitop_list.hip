// wah_bitop_list.hip -- the queries that walk a table of indexed compressed bitmaps, one wavefront per output segment:
//   bitop_list_segments_kernel     one bit operation over ANY number of operands (wah_bitop_list_indexed_device): `value IN (...)`
//                                  and `lo <= value <= hi` on an equality-encoded bitmap index are the OR of as many bitmaps as the
//                                  list or the range has bins (the reference has no counterpart: its README.md:10 only names such
//                                  operations)
//   bitop_clauses_segments_kernel  AND over clauses of (negated) ORs (wah_bitop_clauses_indexed_device)
//   bsi_range_segments_kernel      lo <= value <= hi over a bit-sliced attribute (wah_bsi_range_indexed_device)
//   bsi_compare_segments_kernel    A op B row by row over two bit-sliced attributes (wah_bsi_compare_indexed_device)
//   bsi_arith_segments_kernel      A + B, A - B row by row as a new bit-sliced attribute (wah_bsi_arith_indexed_device)
//   bsi_mul_segments_kernel        A * B row by row as a new bit-sliced attribute (wah_bsi_mul_indexed_device)
//   bsi_kth_pass_kernel            one pass of the radix select over such an attribute (wah_bsi_kth_indexed_device)
//   bsi_kth_group_pass_kernel      the same pass for every (group, query) pair of a GROUP BY at once (wah_bsi_kth_grouped_indexed_device)
//   fetch_items_kernel             the values of listed rows, one wavefront per 64 listed rows of a segment (wah_fetch_indexed_device)
//   splice_segments_kernel         row ranges of indexed bitmaps concatenated into new ones, one wavefront per (column, output
//                                  segment) (wah_splice_indexed_device)
// The walk itself is written once (list_walk), and so is the sweep that keeps one row at a time in the zeroed image (row_sweep);
// a kernel adds the state it keeps per segment, how a row is folded into it, and what it stores or counts.
//
// The rows are named by a table in DEVICE memory (wah_bitop_operand, include/wah.h) that only these kernels read: the host
// never sees it, so a captured launch replayed over a rewritten table combines the new selection.  Nothing is decided from the
// rows' lengths on the host -- one route, whatever they hold.
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
#include "wah_image_words.hpp"
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
    const u64 g0 = w.seg * kSegGroups;
    w.nvalid = groups - g0 < kSegGroups ? (u32)(groups - g0) : kSegGroups;
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

// wah_compact.hip, a translation unit of its own, includes this file for the walk above and nothing else: the walk is stated
// once, here, where its callers and the tests that read its constants look for it.
#ifdef WAH_LIST_WALK_ONLY
} // namespace
} // namespace wah
#else

// the wave's result, value_of_step(s) for group 64 s + lane, as the segment's decoded words (seg_store: 31 -> 32 repack); groups at
// and behind nvalid are written as zero
template <class ValueOfStep>
__device__ __forceinline__ void store_segment(const SegmentsArgs &g, const WaveSegment &w, u32 lane, ValueOfStep value_of_step) {
    const SegStore st = seg_store_setup(g.out, g.out_words, w.seg, w.k, lane);
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) seg_store(st, s, (u32)(64 * s) + lane < w.nvalid ? value_of_step(s) : 0u);
}

// wah_bitop_list_indexed_device. The first operand is the same code on a preset accumulator (all ones for AND, zero otherwise;
// the first operand of ANDNOT applied as OR).  The accumulated segment is written as decoded words into the scratch's bitmap
// area (seg_store: 31 -> 32 repack), and the compress passes run over that -- the road of wah_bitop_many_indexed_device, one
// bitmap-sized intermediate.
__global__ __launch_bounds__(kSegDecodeWaves * 64, 8) void bitop_list_segments_kernel(const BitopListArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    WaveSegment w;
    if (!wave_segment(w, a.g.first_segment, a.g.n_segments, a.g.groups, wave)) return;
    u32 *acc = s_acc[wave];
    image_fill(acc, a.op == 0u ? kOnes31 : 0u, lane);

    const ListOp m_first = list_op(a.op == 3u ? 1u : a.op), m_rest = list_op(a.op);
    const bool ok = list_walk(a.table, a.n, w.seg, w.nvalid, m_rest.fill, acc, lane,
                              [&](u32 j) -> const ListOp & { return j == 0u ? m_first : m_rest; }, [](u32) {});
    if (!ok) return report_stream_error(a.g.ctrl, lane);
    store_segment(a.g, w, lane, [&](int s) { return acc[64 * s + (int)lane]; });
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_bitop_clauses_indexed_device: AND over clauses of (negate ? NOT : ) OR of the clause's operands -- a whole WHERE clause
// of IN / NOT IN lists over a bitmap index.  The operand table is the list call's, flattened over the clauses; a second
// table in device memory holds one 64-bit word per clause: the index one past its last operand, bit 63 = negate.
//
// The inner level is list_walk under OR: the LDS accumulator holds the CURRENT clause's OR, and the table is walked whatever
// the clauses are.  The outer level is sixteen
// registers per lane: the result's group 64 s + lane (the layout seg_store wants; an LDS row per step, no bank conflicts),
// preset to all ones.  When the walk reaches an operand at or behind the current clause's end the clause is FOLDED --
// result &= clause ^ (negate ? all ones : 0), accumulator zeroed -- and the next clause begins; the crossing is found from
// operand numbers, so a clause whose operands were all settled in the gather (its OR is the zeroed accumulator) is folded like
// any other, by the next operand that has words or behind the last chunk.  Nothing looks at the result before the end: a
// result that has become all zeros skips nothing, every operand's every segment is checked as in the list kernel.
//
// Clause ends reach the wave 64 at a time, one per lane, and are checked where they are loaded, before one of them steers a
// fold: strictly increasing, at most n_operands (which also refuses every bit besides the index and bit 63), the last one
// equal to n_operands.  After a bad window nothing folds any more and the launch reports kErrStream.
constexpr u32 kClauseNever = 0x7FFFFFFFu; // an end no operand number reaches

struct ClauseWindow {
    u32 v; // clause base + lane: its end (at most 2^24) | negate << 31; kClauseNever: no such clause, or a refused table
    bool bad;
};
__device__ __forceinline__ ClauseWindow clause_window(const u64 *ends, u32 base, u32 n_clauses, u32 n, u32 lane) {
    const u32 i = base + lane;
    const bool has = i < n_clauses;
    u64 e = 0, before = 0;
    if (has) {
        const ListGlobalU64 p = (ListGlobalU64)(uintptr_t)ends + i;
        e = p[0];
        if (i) before = p[-1];
    }
    const u64 end = e & ~kClauseNegate, prev = before & ~kClauseNegate;
    const bool bad = has && (end > (u64)n || end <= prev || (i + 1u == n_clauses && end != (u64)n));
    ClauseWindow w;
    w.bad = __ballot(bad) != 0ull; // wave-uniform
    w.v = has && !w.bad ? (u32)end | ((e & kClauseNegate) ? 0x80000000u : 0u) : kClauseNever;
    return w;
}

__global__ __launch_bounds__(kSegDecodeWaves * 64, 8) void bitop_clauses_segments_kernel(const BitopClausesArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    WaveSegment w;
    if (!wave_segment(w, a.g.first_segment, a.g.n_segments, a.g.groups, wave)) return;
    u32 *acc = s_acc[wave];
    // (image_fill written out: this kernel fills its 64 VGPRs, and with the helper HERE it compiles to 8 bytes of scratch per lane)
#pragma unroll
    for (int i = 0; i < 4; ++i) reinterpret_cast<uint4 *>(acc)[64 * i + (int)lane] = make_uint4(0u, 0u, 0u, 0u);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    u32 res[kSteps]; // the AND over the clauses folded so far: group 64 s + lane
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) res[s] = kOnes31;
    // the current clause (wave-uniform): its number, its window's first clause, its end and flag
    ClauseWindow win = clause_window(a.clause_ends, 0u, a.n_clauses, a.n, lane);
    bool table_bad = win.bad;
    u32 ci = 0, cbase = 0;
    u32 cur = (u32)__builtin_amdgcn_readlane((int)win.v, 0);
    // fold the current clause into the result and begin the next one
    auto fold = [&]() {
        const u32 flip = (int)cur < 0 ? kOnes31 : 0u;
#pragma unroll
        for (int s = 0; s < (int)kSteps; ++s) res[s] &= acc[64 * s + (int)lane] ^ flip;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        image_fill(acc, 0u, lane);
        ++ci;
        if (ci - cbase == 64u) {
            cbase = ci;
            win = clause_window(a.clause_ends, cbase, a.n_clauses, a.n, lane);
            table_bad |= win.bad;
        }
        cur = (u32)__builtin_amdgcn_readlane((int)win.v, (int)(ci - cbase));
    };

    const ListOp m = list_op(1u); // a clause is an OR
    const bool ok = list_walk(a.table, a.n, w.seg, w.nvalid, m.fill, acc, lane, [&](u32) -> const ListOp & { return m; }, [&](u32 j) {
#pragma nounroll
        while ((cur & kClauseNever) <= j) fold(); // this operand begins another clause (or a later one)
    });
    // behind the last operand: the last clause, and in front of it those whose operands had no words to apply
#pragma nounroll
    while ((cur & kClauseNever) <= a.n) fold();
    if (!ok || table_bad) return report_stream_error(a.g.ctrl, lane);
    store_segment(a.g, w, lane, [&](int s) { return res[s]; });
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_bsi_range_indexed_device: lo <= value <= hi over a bit-sliced attribute (O'Neil & Quass) -- one bitmap per BIT of the
// value, most significant first, and a range predicate is one sweep over them (row_sweep): every slice in turn is FOLDED into
// the sweep's state, which lives in registers, group 64 s + lane.  A slice whose segment was settled in the gather (one zero
// fill) is folded like any other: a zero slice under a bound bit of 1 moves every still-equal row to "below".
//
// The fold is the O'Neil step for both bounds in one sweep.  With the slice's bits B and the bounds' bits l, h at this
// significance (wave-uniform scalars):  GT |= EQlo & B if l == 0;  EQlo &= l ? B : ~B;  LT |= EQhi & ~B if h == 1;
// EQhi &= h ? B : ~B;  result = (GT | EQlo) & (LT | EQhi).  Four arrays of sixteen are cut to three: while the bounds' bits
// agree EQlo == EQhi and neither GT nor LT decides anything; at the first bit where they differ (l = 0, h = 1 for lo < hi)
// the still-equal rows split into those that follow lo, all of them below hi already, and those that follow hi, all above
// lo already.  From there on GT only grows inside the first set and LT inside the second, both mean "strictly inside", and
// they share one array:  result = IN | EQlo | EQhi.  An empty range (lo > hi, or lo beyond the slices' width) walks and
// checks everything all the same and stores zeros: the verdict depends neither on the data nor on the bounds.
// The existence row, where there is one, is the last row and is folded as a plain AND.
//
// 48 registers of state do not fit beside the walk in the 64 that eight waves per SIMD allow: the kernel asks for four
// (128 registers; its 16 KiB of LDS per workgroup would allow more).
constexpr int kBsiWavesPerSimd = 4;

__global__ __launch_bounds__(kSegDecodeWaves * 64, kBsiWavesPerSimd) void bsi_range_segments_kernel(const BsiRangeArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    WaveSegment w;
    if (!wave_segment(w, a.g.first_segment, a.g.n_segments, a.g.groups, wave)) return;
    u32 *acc = s_acc[wave];
    image_fill(acc, 0u, lane);

    // the bounds (wave-uniform, read here and nowhere on the host), clamped to the slices' width
    const u32 ns = a.n_slices, n_rows = a.n_slices + a.has_exists;
    const u64 vmax = ns >= 64u ? ~0ull : (1ull << ns) - 1ull;
    const u64 lo = a.bounds[0], hi_given = a.bounds[1];
    const bool none = lo > hi_given || lo > vmax; // an empty range
    const u64 hi = hi_given < vmax ? hi_given : vmax;

    u32 eq_lo[kSteps], eq_hi[kSteps], in[kSteps]; // rows equal to lo / to hi so far; rows strictly inside: group 64 s + lane
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) {
        eq_lo[s] = kOnes31;
        eq_hi[s] = kOnes31;
        in[s] = 0u;
    }
    bool diverged = false; // a more significant bit of the bounds differed
    const bool ok = row_sweep(a.table, n_rows, n_rows, w, acc, lane, [&](u32 cur) {
        if (cur < ns) {
            const u32 sig = ns - 1u - cur;
            const bool l = (lo >> sig) & 1ull, h = (hi >> sig) & 1ull;
            const u32 gt = diverged && !l ? kOnes31 : 0u, lt = diverged && h ? kOnes31 : 0u;
            const u32 flip_lo = l ? 0u : kOnes31, flip_hi = h ? 0u : kOnes31;
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) {
                const u32 b = acc[64 * s + (int)lane];
                in[s] |= (eq_lo[s] & b & gt) | (eq_hi[s] & ~b & lt);
                eq_lo[s] &= b ^ flip_lo;
                eq_hi[s] &= b ^ flip_hi;
            }
            diverged = diverged || l != h;
        } else { // the existence bitmap
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) {
                const u32 b = acc[64 * s + (int)lane];
                in[s] &= b;
                eq_lo[s] &= b;
                eq_hi[s] &= b;
            }
        }
    });
    if (!ok) return report_stream_error(a.g.ctrl, lane);
    store_segment(a.g, w, lane, [&](int s) { return none ? 0u : in[s] | eq_lo[s] | eq_hi[s]; });
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_bsi_compare_indexed_device: A op B row by row over TWO bit-sliced attributes of ka and kb slices -- the range kernel's
// sweep with the constant's bit replaced by the other attribute's slice.  row_sweep keeps one row at a time in the
// image, so the table is interleaved by significance, most significant first: for sig = max(ka, kb) - 1 .. 0 A's slice
// of that significance (if sig < ka), then B's (if sig < kb); then A's existence row, then B's, where they have one.  With
// d = |ka - kb| and kmin = min(ka, kb) that is d rows of the wider attribute alone, then kmin pairs (A, B): attribute and
// significance of row j follow from ka, kb and the two flags by wave-uniform arithmetic, and nothing else describes the table.
//
// The state, group 64 s + lane: eq (rows whose more significant bits agree, preset to all ones), gt (rows where A is already
// above B, preset to zero) and hold (A's slice of the current pair).  The fold:
//   a row of the wider attribute alone   the other attribute's bit is 0:  gt |= eq & acc (only if the row is A's);  eq &= ~acc
//   A's slice of a pair                  hold = acc
//   B's slice of a pair                  gt |= eq & hold & ~acc;  eq &= ~(hold ^ acc)
//   an existence row                     ex &= acc
// The negated operators (NE, LE, LT) set every row that gt / eq do not, so the existence rows cannot be folded into gt and eq
// alone: a mask ex is needed.  It costs no register: behind the last slice `hold` is dead, so it is preset to all ones there and
// becomes ex -- gt and eq are left as they are and every operator's result is ANDed with ex once, at the store (GT gt, GE
// gt | eq, EQ eq, NE ~eq, LE ~gt, LT ~(gt | eq)).  48 registers of state, the range kernel's budget and its launch bound.
// Nothing looks at the operator or the state before the store: every row's every segment is walked and checked.
__global__ __launch_bounds__(kSegDecodeWaves * 64, kBsiWavesPerSimd) void bsi_compare_segments_kernel(const BsiCompareArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    WaveSegment w;
    if (!wave_segment(w, a.g.first_segment, a.g.n_segments, a.g.groups, wave)) return;
    u32 *acc = s_acc[wave];
    image_fill(acc, 0u, lane);

    // the table's shape (wave-uniform): `alone` rows of the wider attribute, then pairs up to n_slice_rows, then existence rows
    const u32 ka = a.n_slices_a, kb = a.n_slices_b;
    const bool a_wider = ka > kb;
    const u32 alone = a_wider ? ka - kb : kb - ka;
    const u32 n_slice_rows = ka + kb, n_rows = n_slice_rows + a.exists_a + a.exists_b;

    u32 eq[kSteps], gt[kSteps], hold[kSteps]; // group 64 s + lane; hold: A's slice of the current pair, behind the slices ex
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) {
        eq[s] = kOnes31;
        gt[s] = 0u;
        hold[s] = 0u;
    }
    const bool ok = row_sweep(a.table, n_rows, n_rows, w, acc, lane, [&](u32 cur) {
        if (cur < alone) { // the narrower attribute has a 0 here
            const u32 a_mask = a_wider ? kOnes31 : 0u;
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) {
                const u32 v = acc[64 * s + (int)lane];
                gt[s] |= eq[s] & v & a_mask;
                eq[s] &= ~v;
            }
        } else if (cur < n_slice_rows) {
            if (((cur - alone) & 1u) == 0u) { // A's slice of a pair
#pragma unroll
                for (int s = 0; s < (int)kSteps; ++s) hold[s] = acc[64 * s + (int)lane];
            } else { // B's
#pragma unroll
                for (int s = 0; s < (int)kSteps; ++s) {
                    const u32 b = acc[64 * s + (int)lane];
                    gt[s] |= eq[s] & hold[s] & ~b;
                    eq[s] &= ~(hold[s] ^ b);
                }
            }
        } else { // an existence row; the first one turns hold into ex
            const u32 keep = cur == n_slice_rows ? 0u : kOnes31;
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) hold[s] = (hold[s] | ~keep) & acc[64 * s + (int)lane];
        }
    });
    if (!ok) return report_stream_error(a.g.ctrl, lane);
    // result = ((gt & use_gt) | (eq & use_eq)) ^ flip, over the rows that exist in both
    const u32 op = a.op;
    const u32 use_gt = op == kCmpEQ || op == kCmpNE ? 0u : kOnes31;
    const u32 use_eq = op == kCmpGT || op == kCmpLE ? 0u : kOnes31;
    const u32 flip = op == kCmpNE || op == kCmpLE || op == kCmpLT ? kOnes31 : 0u;
    const u32 no_ex = n_rows == n_slice_rows ? kOnes31 : 0u; // no existence row: hold is still a slice
    store_segment(a.g, w, lane, [&](int s) { return (((gt[s] & use_gt) | (eq[s] & use_eq)) ^ flip) & (hold[s] | no_ex) & kOnes31; });
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_bsi_arith_indexed_device: A + B or A - B row by row over two bit-sliced attributes of ka and kb slices, as a NEW bit-sliced
// attribute of n_out slices -- a ripple carry over the slices.  The carry runs from the least significant slice up, so this
// table is interleaved the other way round: A's existence row, then B's, where they have one (the first sum slice leaves the
// wave before the sweep ends, and it leaves ANDed with them); then for sig = 0 .. max(ka, kb) - 1 A's slice of that significance
// (if sig < ka), then B's (if sig < kb).  With kmin = min(ka, kb) that is kmin pairs (A, B), then |ka - kb| rows of the wider
// attribute alone: attribute and significance of row j follow from ka, kb and the two flags by wave-uniform arithmetic.
//
// The state, group 64 s + lane: ex (preset to all ones), carry (preset to 0 for ADD and to all ones for SUB: A - B = A + ~B + 1)
// and hold (A's slice of the current pair).  The fold:
//   an existence row                     ex &= acc
//   A's slice of a pair                  hold = acc
//   the closing row of a significance    a, b = (hold, acc) for B's slice of a pair, (acc, 0) for A's alone, (0, acc) for B's alone;
//                                        b ^= flip (all ones for SUB);  sum = a ^ b ^ carry;  carry = (a & b) | (carry & (a ^ b));
//                                        sum & ex leaves as the segment's 992 decoded words of matrix row n_out - 1 - sig
// which row is which comes down to three wave-uniform masks (what of hold and of the image is a, what of the image is b), so the
// closing fold is one piece of code.  A closing row at or above n_out (a truncating call) is folded like any other -- the
// verdict depends neither on the data nor on n_out -- and stored through a descriptor of no bytes: the hardware drops it.
// Behind the sweep the slices sig = max(ka, kb) .. n_out - 1 come from the carry alone (ADD: carry & ex, then carry = 0 -- a zero
// extension; SUB: ~carry & ex, carry unchanged -- the borrow, that is the sign, extended), then the ex row where there is one.
// The matrix is the builder's: [n_out (+ 1), n_words], most significant slice first, n_words a multiple of 992, so every
// segment is whole (1024 groups) and every word of the matrix is written by exactly one wave: it needs no clearing.
// A slice settled in the gather is folded out of the zeroed image like any other row: it still advances the carry and still
// emits its slice.  The walk's verdict is known only behind its last row: a wave that refuses something reports and stores
// nothing more -- the slices it stored on the way are its own words of a matrix whose call is refused as a whole.
// 48 registers of state, the compare kernel's budget and its launch bound; the sixteen stores of a closing fold need the lane
// constants of the repack and four scalars for the descriptor on top, which still fit: no scratch (Makefile: asm).
__global__ __launch_bounds__(kSegDecodeWaves * 64, kBsiWavesPerSimd) void bsi_arith_segments_kernel(const BsiArithArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    WaveSegment w;
    if (!wave_segment(w, 0ull, a.n_segments, a.groups, wave)) return;
    u32 *acc = s_acc[wave];
    image_fill(acc, 0u, lane);

    // the table's shape (wave-uniform): the existence rows, then `pairs` rows in pairs, then rows of the wider attribute alone
    const u32 ka = a.n_slices_a, kb = a.n_slices_b, n_out = a.n_slices_out;
    const bool a_wider = ka > kb;
    const u32 kmin = a_wider ? kb : ka, kmax = a_wider ? ka : kb;
    const u32 n_ex = a.exists_a + a.exists_b, pairs = 2u * kmin, n_rows = n_ex + ka + kb;
    const u32 flip = a.sub ? kOnes31 : 0u;

    // matrix row `row` of this wave's segment; live == false: a descriptor of no bytes, every store through it is dropped
    auto row_store = [&](u32 row, bool live) {
        return seg_store_setup(a.matrix + (u64)row * a.n_words, live ? a.n_words : 0ull, w.seg, w.k, lane);
    };

    u32 ex[kSteps], carry[kSteps], hold[kSteps]; // group 64 s + lane; hold: A's slice of the current pair
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) {
        ex[s] = kOnes31;
        carry[s] = flip;
        hold[s] = 0u;
    }
    const bool ok = row_sweep(a.table, n_rows, n_rows, w, acc, lane, [&](u32 cur) {
        if (cur < n_ex) {
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) ex[s] &= acc[64 * s + (int)lane];
            return;
        }
        const u32 r = cur - n_ex;
        const bool paired = r < pairs;
        if (paired && (r & 1u) == 0u) { // A's slice of a pair
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) hold[s] = acc[64 * s + (int)lane];
            return;
        }
        // the closing row of significance sig
        const u32 sig = paired ? r >> 1 : r - kmin;
        const u32 a_held = paired ? kOnes31 : 0u, a_here = !paired && a_wider ? kOnes31 : 0u, b_here = paired || !a_wider ? kOnes31 : 0u;
        const bool live = sig < n_out;
        const SegStore st = row_store(live ? n_out - 1u - sig : 0u, live);
#pragma unroll
        for (int s = 0; s < (int)kSteps; ++s) {
            const u32 v = acc[64 * s + (int)lane];
            const u32 x = (hold[s] & a_held) | (v & a_here), y = (v & b_here) ^ flip;
            const u32 t = x ^ y;
            seg_store(st, s, (t ^ carry[s]) & ex[s]);
            carry[s] = (x & y) | (carry[s] & t);
        }
    });
    if (!ok) return report_stream_error(a.ctrl, lane);
    // the slices above both attributes, least significant first: the carry, or the borrow, and its extension
#pragma nounroll
    for (u32 sig = kmax; sig < n_out; ++sig) {
        const SegStore st = row_store(n_out - 1u - sig, true);
#pragma unroll
        for (int s = 0; s < (int)kSteps; ++s) {
            seg_store(st, s, (carry[s] ^ flip) & ex[s]);
            carry[s] &= flip;
        }
    }
    if (n_ex != 0u) {
        const SegStore st = row_store(n_out, true);
#pragma unroll
        for (int s = 0; s < (int)kSteps; ++s) seg_store(st, s, ex[s]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_bsi_mul_indexed_device: A * B row by row over two bit-sliced attributes of ka and kb slices, as a NEW bit-sliced attribute
// of n_out slices -- schoolbook shift-and-add over the slices.  Every slice of B meets every slice of A, so this table is not
// interleaved: A's existence row, then B's, where they have one; then ALL of A's slices, least significant first; then ALL of
// B's, least significant first.  A is complete before the first slice of B arrives.
//
// What does not fit into registers lies in the wave's own area of the scratch (BsiMulArgs.work), in GROUP form, 31-bit groups in
// 32-bit words, no repack: ka slices of A's image, then the accumulator P of n_out slices, 4 KiB each.  A slice is four
// quarters of 64 quads: quad 64 q + lane holds the lane's groups 64 (4 q + t) + lane, t = 0 .. 3 -- the groups the lane owns
// everywhere in this file -- so a lane moves a slice as four 16-byte accesses, a wave's access is 1 KiB without a gap, and a lane
// only ever writes and later reads ITS OWN sixteen groups: program order is all the ordering there is, no fence, no atomics.
// The state beside the walk is ex (preset to all ones); b and carry live inside one fold.  The fold:
//   an existence row      ex &= acc
//   A's slice i           the image's groups leave into slice i of the wave's area
//   B's slice j           b = the image's groups; carry = 0; for i = 0 .. ka - 1 while i + j < n_out:
//                             x = A_i & b;  p = P[i + j];  t = p ^ x;  P[i + j] = t ^ carry;  carry = (p & x) | (carry & t)
//                         then P[ka + j] = carry where ka + j < n_out
//   B's slice 0           reads no P: P[i] = A_i & b, P[ka] = 0
// After j partial products P < 2^(ka + j): every slice step j reads has been written (by induction P[0 .. ka + j - 1], below
// n_out), and its carry goes out into a slice nobody has written yet -- no clearing launch, and the carry never ripples further.
// A slice of B that is all zero in this segment (wave-uniform: one ballot; a settled row is folded as the zeros it is) skips the
// loop and writes P[ka + j] = 0 alone -- sparse slices and the zero bits of a constant cost next to nothing.  The skip is inside
// the fold: the walk and its checks are untouched, every row's every segment is walked whatever the data and whatever n_out.
// The fold runs quarter by quarter: b, carry, x, p and the next step's x and p are one quad each, so the loads of step i + 1 are
// in flight behind the stores of step i within the launch bound.
// Behind the sweep P[sig] & ex leaves through seg_store into matrix row n_out - 1 - sig for every sig < n_out, zeros at and above
// ka + kb, then the ex row where there is one.  Every word of the matrix is written by exactly one wave.  A wave that refuses
// something has written its own area of the scratch only; it reports and stores nothing.
typedef u32 MulQuad __attribute__((ext_vector_type(4)));
constexpr u32 kSliceQuads = kSegGroups / 4u; // 256: the quads of one slice of a wave's area
__global__ __launch_bounds__(kSegDecodeWaves * 64, kBsiWavesPerSimd) void bsi_mul_segments_kernel(const BsiMulArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    WaveSegment w;
    if (!wave_segment(w, 0ull, a.n_segments, a.groups, wave)) return;
    u32 *acc = s_acc[wave];
    image_fill(acc, 0u, lane);

    const u32 ka = a.n_slices_a, kb = a.n_slices_b, n_out = a.n_slices_out;
    const u32 n_ex = a.exists_a + a.exists_b, n_rows = n_ex + ka + kb;
    const u32 n_acc = ka + kb < n_out ? ka + kb : n_out; // the accumulator's slices that are ever written
    // the lane's quad of quarter 0 of A's slice 0, and of P[0]
    MulQuad *const image = reinterpret_cast<MulQuad *>(a.work) + w.k * (u64)(ka + n_out) * kSliceQuads + lane;
    MulQuad *const prod = image + (u64)ka * kSliceQuads;

    u32 ex[kSteps]; // group 64 s + lane
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) ex[s] = kOnes31;
    const bool ok = row_sweep(a.table, n_rows, n_rows, w, acc, lane, [&](u32 cur) {
        if (cur < n_ex) {
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) ex[s] &= acc[64 * s + (int)lane];
            return;
        }
        const u32 r = cur - n_ex;
        if (r < ka) { // A's slice r
            MulQuad *const dst = image + (u64)r * kSliceQuads;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                MulQuad v;
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = acc[64 * (4 * q + t) + (int)lane];
                dst[64 * q] = v;
            }
            return;
        }
        // B's slice j
        const u32 j = r - ka;
        const u32 n_i = j >= n_out ? 0u : (ka < n_out - j ? ka : n_out - j); // the steps that land below n_out
        const bool top = ka + j < n_out;                                     // the carry's slice exists
        u32 any = 0u;
#pragma unroll
        for (int s = 0; s < (int)kSteps; ++s) any |= acc[64 * s + (int)lane];
        if (j != 0u && __ballot(any != 0u) == 0ull) { // nothing to add: the carry slot alone
            if (top) {
#pragma unroll
                for (int q = 0; q < 4; ++q) prod[(u64)(ka + j) * kSliceQuads + 64 * q] = MulQuad(0u);
            }
            return;
        }
#pragma nounroll
        for (u32 q = 0; q < 4u; ++q) {
            MulQuad b;
#pragma unroll
            for (int t = 0; t < 4; ++t) b[t] = acc[64u * (4u * q + (u32)t) + lane];
            const MulQuad *const A = image + 64u * q;
            MulQuad *const P = prod + (u64)j * kSliceQuads + 64u * q;
            MulQuad carry = MulQuad(0u);
            if (j == 0u) {
#pragma unroll 2
                for (u32 i = 0; i < n_i; ++i) P[(u64)i * kSliceQuads] = A[(u64)i * kSliceQuads] & b;
            } else if (n_i != 0u) {
                MulQuad x = A[0], p = P[0];
#pragma nounroll
                for (u32 i = 0; i < n_i; ++i) {
                    MulQuad xn = x, pn = p;
                    if (i + 1u < n_i) { // (wave-uniform) step i + 1's loads, in front of step i's store
                        xn = A[(u64)(i + 1u) * kSliceQuads];
                        pn = P[(u64)(i + 1u) * kSliceQuads];
                    }
                    x &= b;
                    const MulQuad t = p ^ x;
                    P[(u64)i * kSliceQuads] = t ^ carry;
                    carry = (p & x) | (carry & t);
                    x = xn;
                    p = pn;
                }
            }
            if (top) P[(u64)ka * kSliceQuads] = carry;
        }
    });
    if (!ok) return report_stream_error(a.ctrl, lane);
    // the product's slices, least significant first; at and above ka + kb there is nothing but zeros
#pragma nounroll
    for (u32 sig = 0; sig < n_out; ++sig) {
        const SegStore st = seg_store_setup(a.matrix + (u64)(n_out - 1u - sig) * a.n_words, a.n_words, w.seg, w.k, lane);
        MulQuad v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = sig < n_acc ? prod[(u64)sig * kSliceQuads + 64 * q] : MulQuad(0u);
#pragma unroll
        for (int s = 0; s < (int)kSteps; ++s) seg_store(st, s, v[s / 4][s % 4] & ex[s]);
    }
    if (n_ex != 0u) {
        const SegStore st = seg_store_setup(a.matrix + (u64)n_out * a.n_words, a.n_words, w.seg, w.k, lane);
#pragma unroll
        for (int s = 0; s < (int)kSteps; ++s) seg_store(st, s, ex[s]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_bsi_kth_indexed_device: the value of a given rank (MIN, MAX, a quantile, the k-th largest) among the rows that a set of
// filter bitmaps selects, over the same bit-sliced attribute -- a radix select over the slices, most significant first.  The
// value is resolved in DIGITS of kBsiKthDigitBits slices: pass p counts, for every pattern of digit p, the selected rows whose
// more significant bits equal the prefix decided so far and whose digit is that pattern; a one-wave kernel behind it picks the
// bucket that holds the rank and extends the prefix.  The order of the launches on the stream is the only synchronisation.
//
// A pass is the range kernel's walk over the filter rows and the slices up to the end of its digit, one wavefront per segment.
// `eq` -- the rows still in the running -- lives in registers, group 64 s + lane, as eq_lo does there: it starts as the
// segment's valid bits (the pad bits of the bitmap's last group cleared), is ANDed with every filter row, and with B or ~B of
// every slice above the digit according to the prefix's bit (wave-uniform, read from the scratch).  The digit's own slices are
// kept as they are: the last one never leaves the LDS image -- the last row of a walk is only ever folded behind the loop, and
// there the counting takes its place --, the two in front of it go into registers of their own, and the first slice of a digit
// of four into a second LDS image (eq and THREE arrays of sixteen beside the walk spill five registers at the 128 that four
// waves per SIMD allow; eq and two are the range kernel's 48, and 32 KiB of LDS per workgroup still allow five workgroups).  Every
// lane counts popcount(eq & pattern) for the 2^digit patterns, sixteen DPP sums make them the wave's, and lane b adds bucket b
// with one 64-bit atomic if it is not zero.  Nothing of bitmap size is written, and nothing is kept per segment between the
// passes: the next pass walks the filters and the slices above its digit again, which costs their words once more but needs
// no state that goes with n_words -- sixteen words per lane and segment written and read back would be as many bytes as two
// incompressible slices, per pass.
//
// A short last digit (n_slices no multiple of the width) is right-aligned: the slices it does not have read as zero, so only
// the buckets below 2^(its width) are counted into.  Every pass walks and checks all of its rows whatever the prefix, the
// query or the counts are, and the last pass walks every row of the table.
constexpr int kBsiKthWavesPerSimd = 4;
constexpr int kBsiKthInRegs = kBsiKthDigitBits >= 3u ? 2 : (int)kBsiKthDigitBits - 1; // slices of a digit held in registers
constexpr bool kBsiKthInLds = kBsiKthDigitBits == 4u;                                  // ... and one more in an LDS image
static_assert(kBsiKthDigitBits >= 1u && kBsiKthDigitBits <= 4u, "a digit is one to four slices");

__global__ __launch_bounds__(kSegDecodeWaves * 64, kBsiKthWavesPerSimd) void bsi_kth_pass_kernel(const BsiKthArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kSegDecodeWaves][kSegGroups];
    __shared__ __attribute__((aligned(16))) u32 s_top[kBsiKthInLds ? kSegDecodeWaves : 1][kSegGroups]; // the slice of bucket bit 3
    const u32 wave = wave_id(), lane = lane_id();
    WaveSegment w;
    if (!wave_segment(w, 0ull, a.n_segments, a.groups, wave)) return;
    u32 *acc = s_acc[wave];
    u32 *top = s_top[kBsiKthInLds ? wave : 0u];
    image_fill(acc, 0u, lane);
    if (kBsiKthInLds) image_fill(top, 0u, lane); // (a short digit has no such slice)

    // the rows of this pass (wave-uniform): the filters, then the slices up to the end of digit `pass`
    const u32 nf = a.n_filters, ns = a.n_slices;
    const u32 digit_first = a.pass * kBsiKthDigitBits;
    const u32 digit_end = min(digit_first + kBsiKthDigitBits, ns);
    const u32 n_rows = nf + digit_end;
    const u64 prefix = a.state[kKthPrefix]; // what the passes in front of this one decided

    u32 eq[kSteps];                           // selected rows whose bits above the digit equal the prefix: group 64 s + lane
    u32 dg[kBsiKthInRegs ? kBsiKthInRegs : 1][kSteps]; // the digit's slices in front of its last: dg[j] is bit j + 1 of the bucket number
    const u64 last_group = a.groups - 1ull - w.seg * kSegGroups; // (beyond nvalid in every segment but the bitmap's last)
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) {
        const u32 g = (u32)(64 * s) + lane;
        eq[s] = g >= w.nvalid ? 0u : (u64)g == last_group ? kOnes31 >> a.pad_bits : kOnes31;
#pragma unroll
        for (int j = 0; j < kBsiKthInRegs; ++j) dg[j][s] = 0u;
    }
    // every row but the pass's last is folded: that one stays in the image and is counted
    const bool ok = row_sweep(a.table, n_rows, n_rows - 1u, w, acc, lane, [&](u32 cur) {
        if (cur < nf + digit_first) {
            // a filter: AND; a slice above the digit: AND with B or ~B by the prefix's bit
            const u32 sig = ns - 1u - (cur - nf); // (not used for a filter)
            const u32 flip = cur < nf || ((prefix >> (sig & 63u)) & 1ull) ? 0u : kOnes31;
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) eq[s] &= acc[64 * s + (int)lane] ^ flip;
        } else {
            const u32 j = digit_end - 2u - (cur - nf); // 0 .. digit - 2
#pragma unroll
            for (int jj = 0; jj < kBsiKthInRegs; ++jj)
                if (j == (u32)jj) {
#pragma unroll
                    for (int s = 0; s < (int)kSteps; ++s) dg[jj][s] = acc[64 * s + (int)lane];
                }
            if (kBsiKthInLds && j == (u32)kBsiKthInRegs) {
#pragma unroll
                for (int s = 0; s < (int)kSteps; ++s) top[64 * s + (int)lane] = acc[64 * s + (int)lane];
            }
        }
    });
    if (!ok) return report_stream_error(a.ctrl, lane);
    // bucket b: the rows of eq whose digit is b -- bit 0 the image's slice, bit j + 1 dg[j], bit 3 the second image's
    u32 count[kBsiKthBuckets];
#pragma unroll
    for (int b = 0; b < (int)kBsiKthBuckets; ++b) count[b] = 0u;
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) {
        const u32 low = acc[64 * s + (int)lane];
        const u32 high = kBsiKthInLds ? top[64 * s + (int)lane] : 0u;
#pragma unroll
        for (int hi = 0; hi < (int)(kBsiKthBuckets / 2u); ++hi) {
            u32 e = eq[s];
#pragma unroll
            for (int j = 0; j < kBsiKthInRegs; ++j) e &= (hi >> j) & 1 ? dg[j][s] : ~dg[j][s];
            if (kBsiKthInLds) e &= (hi >> kBsiKthInRegs) & 1 ? high : ~high;
            count[2 * hi + 1] += (u32)__builtin_popcount(e & low);
            count[2 * hi] += (u32)__builtin_popcount(e & ~low);
        }
    }
    u32 mine = 0; // lane b: bucket b of the wave
#pragma unroll
    for (int b = 0; b < (int)kBsiKthBuckets; ++b) {
        const u32 t = wave_total32(count[b]);
        if (lane == (u32)b) mine = t;
    }
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(a.hist) + ((u64)a.pass * kBsiKthCopies + blockIdx.x % kBsiKthCopies) * kBsiKthBuckets;
    if (lane < kBsiKthBuckets && mine != 0u) atomicAdd(hist + lane, (unsigned long long)mine);
}

// floor(x * y / d) for x <= d, d > 0: the 128-bit product by shift and subtract (one lane, once per call)
__device__ __forceinline__ u64 kth_muldiv(u64 x, u64 y, u64 d) {
    const u64 hi = __umul64hi(x, y), lo = x * y;
    u64 rem = 0, quot = 0; // (the quotient is at most y: it fits)
#pragma nounroll
    for (int i = 127; i >= 0; --i) {
        const u64 bit = i >= 64 ? (hi >> (i - 64)) & 1ull : (lo >> i) & 1ull;
        const bool carry = rem >> 63;
        rem = (rem << 1) | bit;
        quot <<= 1;
        if (carry || rem >= d) {
            rem -= d;
            quot |= 1ull;
        }
    }
    return quot;
}

// One wave behind every pass: sums the copies of the pass's histogram (lane b: bucket b), and lane 0 decides.  Pass 0 turns
// the query into a rank from the bottom (total = the sum of the first histogram; a rank from the top is total - 1 - rank); every
// pass picks the bucket that holds the rank, adds the buckets below it to `less`, and puts its number into the prefix; the last
// one writes the result.  A query that names no row (found = 0) changes nothing of what is walked.
__global__ __launch_bounds__(64) void bsi_kth_decide_kernel(const BsiKthArgs a) {
    __shared__ u64 s_hist[kBsiKthBuckets];
    const u32 lane = lane_id();
    if (lane < kBsiKthBuckets) {
        u64 sum = 0;
        for (u32 c = 0; c < kBsiKthCopies; ++c) sum += a.hist[((u64)a.pass * kBsiKthCopies + c) * kBsiKthBuckets + lane];
        s_hist[lane] = sum;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const u32 ns = a.n_slices;
    const u32 digit_end = min((a.pass + 1u) * kBsiKthDigitBits, ns);
    const bool last = digit_end == ns;
    u64 rank = a.state[kKthRank], less = a.state[kKthLess], total = a.state[kKthTotal];
    bool found = a.state[kKthFound] != 0ull;
    if (a.pass == 0u) {
        total = 0;
        for (u32 b = 0; b < kBsiKthBuckets; ++b) total += s_hist[b];
        const u64 kind = a.query[0], qa = a.query[1], qb = a.query[2];
        found = false;
        if (total != 0ull) {
            if (kind == 0ull || kind == 1ull) { // WAH_BSI_KTH_ASCENDING, WAH_BSI_KTH_DESCENDING
                found = qa < total;
                rank = kind == 0ull ? qa : total - 1ull - qa;
            } else if (kind == 2ull && qb != 0ull && qa <= qb) { // WAH_BSI_KTH_QUANTILE
                found = true;
                rank = kth_muldiv(qa, total - 1ull, qb);
            }
        }
        less = 0;
        a.state[kKthTotal] = total;
        a.state[kKthFound] = found ? 1ull : 0ull;
    }
    u64 equal = 0, bucket = 0;
    if (found) {
        u64 below = 0;
        for (u32 b = 0; b < kBsiKthBuckets; ++b) {
            const u64 h = s_hist[b];
            if (rank < below + h) {
                bucket = b;
                equal = h;
                break;
            }
            below += h;
        }
        rank -= below;
        less += below;
    }
    const u64 prefix = a.state[kKthPrefix] | (bucket << (ns - digit_end));
    a.state[kKthPrefix] = prefix;
    a.state[kKthRank] = rank;
    a.state[kKthLess] = less;
    if (last) {
        a.result[0] = found ? 1ull : 0ull;
        a.result[1] = found ? prefix : 0ull;
        a.result[2] = total;
        a.result[3] = found ? less : 0ull;
        a.result[4] = found ? equal : 0ull;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_bsi_kth_grouped_indexed_device: the same radix select for L = n_groups x n_queries selects at once -- `SELECT g, MIN(x),
// MAX(x), median(x) ... GROUP BY g`.  Select l = g * n_queries + q asks query q of the rows that the filters AND the R rows of
// group g select; it has a state block and, per pass, kBsiKthGroupCopies histograms of its own in the scratch.  A pass is ONE
// launch for all selects and the decision behind it another, so a call is as many launches as the ungrouped one's.
//
// The ITEMS of a pass are (segment, select) pairs, the select running fastest: item i is select i % L of segment i / L.  The grid
// is capped at what the chip holds at once and a wavefront takes item after item, a whole grid apart, so the wavefronts
// that run at one time hold consecutive items: the L walks of one segment's slice words are neighbours in time and find them
// in the L2 / the memory-side cache and not in HBM (WAH_BSI_KTH_GROUP_SEGMENT_FASTEST builds the other order, for the
// measurement in DESIGN.md alone).
//
// An item is bsi_kth_pass_kernel's work for its segment with the select's own prefix, in three sweeps, because list_walk wants
// a contiguous table and the three tables are contiguous each: the filter rows (none: no sweep), the group's R rows -- both
// folded into eq as plain ANDs --, then the slices down to the digit's end, the last one left in the image and counted.  One
// loop runs the three (one instance of the walk in the code, not three).
//
// The short cut that makes clustered keys cheap: behind the second sweep eq is the selection of this segment.  If no lane holds
// a bit of it the item has nothing to count and skips its slice sweep -- with keys sorted by group that is all but one select of
// most segments.  What is CHECKED does not depend on it: the filter rows and the group's rows are walked, and so checked, by
// every item in every pass, in front of the short cut; and the items of select 0 in the LAST pass, which walks every slice,
// take no short cut, so every segment of every slice is checked once per call whatever the data and the queries are.
// The body of an item: bsi_kth_pass_kernel's, restated as functions -- the state beside the walk, how it begins, how a row is folded
// into it, and the count behind the sweep.  It is a COPY: with bsi_kth_pass_kernel itself written over these functions its device
// code does not come out as it was (DESIGN.md 5.14.1 has the figures), so that kernel and bsi_kth_decide_kernel stay as they are.
typedef u32 KthEq[kSteps];                                    // selected rows whose bits above the digit equal the prefix: group 64 s + lane
typedef u32 KthDigit[kBsiKthInRegs ? kBsiKthInRegs : 1][kSteps]; // the digit's slices in front of its last: dg[j] is bit j + 1 of the bucket number
// eq: the segment's valid bits, the pad bits of the bitmap's last group cleared; no slice of the digit yet
__device__ __forceinline__ void kth_pass_begin(KthEq &eq, KthDigit &dg, const WaveSegment &w, u64 groups, u32 pad_bits, u32 lane) {
    // (in 32 bits: the group numbers are lane constants that an item loop keeps; as 64-bit pairs they are thirty-two registers)
    const u64 behind = groups - 1ull - w.seg * kSegGroups;
    const u32 last_group = behind < kSegGroups ? (u32)behind : kSegGroups; // (the bitmap's last group: in its last segment only)
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) {
        const u32 g = (u32)(64 * s) + lane;
        eq[s] = g >= w.nvalid ? 0u : g == last_group ? kOnes31 >> pad_bits : kOnes31;
#pragma unroll
        for (int j = 0; j < kBsiKthInRegs; ++j) dg[j][s] = 0u;
    }
}
// row `cur` of a sweep over nf filter rows and then the slices down to digit_end, while the image holds it
__device__ __forceinline__ void kth_pass_fold(KthEq &eq, KthDigit &dg, u32 cur, u32 nf, u32 ns, u32 digit_first, u32 digit_end, u64 prefix, const u32 *acc,
                                              u32 *top, u32 lane) {
    if (cur < nf + digit_first) {
        // a filter: AND; a slice above the digit: AND with B or ~B by the prefix's bit
        const u32 sig = ns - 1u - (cur - nf); // (not used for a filter)
        const u32 flip = cur < nf || ((prefix >> (sig & 63u)) & 1ull) ? 0u : kOnes31;
#pragma unroll
        for (int s = 0; s < (int)kSteps; ++s) eq[s] &= acc[64 * s + (int)lane] ^ flip;
    } else {
        const u32 j = digit_end - 2u - (cur - nf); // 0 .. digit - 2
#pragma unroll
        for (int jj = 0; jj < kBsiKthInRegs; ++jj)
            if (j == (u32)jj) {
#pragma unroll
                for (int s = 0; s < (int)kSteps; ++s) dg[jj][s] = acc[64 * s + (int)lane];
            }
        if (kBsiKthInLds && j == (u32)kBsiKthInRegs) {
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) top[64 * s + (int)lane] = acc[64 * s + (int)lane];
        }
    }
}
// behind the sweep: the rows of eq whose digit is b are counted into bucket b -- bit 0 the image's slice, bit j + 1 dg[j], bit 3
// the second image's -- and lane b's return value is the wave's bucket b.  (The counters are the caller's: declared in here they cost
// bsi_kth_pass_kernel, when it was tried over this function, fifteen spilled registers.)
__device__ __forceinline__ u32 kth_pass_count(u32 (&count)[kBsiKthBuckets], const KthEq &eq, const KthDigit &dg, const u32 *acc, const u32 *top, u32 lane) {
#pragma unroll
    for (int b = 0; b < (int)kBsiKthBuckets; ++b) count[b] = 0u;
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) {
        const u32 low = acc[64 * s + (int)lane];
        const u32 high = kBsiKthInLds ? top[64 * s + (int)lane] : 0u;
#pragma unroll
        for (int hi = 0; hi < (int)(kBsiKthBuckets / 2u); ++hi) {
            u32 e = eq[s];
#pragma unroll
            for (int j = 0; j < kBsiKthInRegs; ++j) e &= (hi >> j) & 1 ? dg[j][s] : ~dg[j][s];
            if (kBsiKthInLds) e &= (hi >> kBsiKthInRegs) & 1 ? high : ~high;
            count[2 * hi + 1] += (u32)__builtin_popcount(e & low);
            count[2 * hi] += (u32)__builtin_popcount(e & ~low);
        }
    }
    u32 mine = 0; // lane b: bucket b of the wave
#pragma unroll
    for (int b = 0; b < (int)kBsiKthBuckets; ++b) {
        const u32 tot = wave_total32(count[b]);
        if (lane == (u32)b) mine = tot;
    }
    return mine;
}

// The decision behind a pass, bsi_kth_decide_kernel's lane 0 restated as a function (a copy, as above), run by ONE thread: hist
// holds the pass's sixteen counts, state / query / result are the select's own.  Pass 0 turns
// the query into a rank from the bottom (total = the sum of the first histogram; a rank from the top is total - 1 - rank); every
// pass picks the bucket that holds the rank, adds the buckets below it to `less`, and puts its number into the prefix; the last
// one writes the result.  A query that names no row (found = 0) changes nothing of what is walked.
__device__ __forceinline__ void kth_decide(const u64 *hist, u64 *state, const u64 *query, u64 *result, u32 pass, u32 ns) {
    const u32 digit_end = min((pass + 1u) * kBsiKthDigitBits, ns);
    const bool last = digit_end == ns;
    u64 rank = state[kKthRank], less = state[kKthLess], total = state[kKthTotal];
    bool found = state[kKthFound] != 0ull;
    if (pass == 0u) {
        total = 0;
        for (u32 b = 0; b < kBsiKthBuckets; ++b) total += hist[b];
        const u64 kind = query[0], qa = query[1], qb = query[2];
        found = false;
        if (total != 0ull) {
            if (kind == 0ull || kind == 1ull) { // WAH_BSI_KTH_ASCENDING, WAH_BSI_KTH_DESCENDING
                found = qa < total;
                rank = kind == 0ull ? qa : total - 1ull - qa;
            } else if (kind == 2ull && qb != 0ull && qa <= qb) { // WAH_BSI_KTH_QUANTILE
                found = true;
                rank = kth_muldiv(qa, total - 1ull, qb);
            }
        }
        less = 0;
        state[kKthTotal] = total;
        state[kKthFound] = found ? 1ull : 0ull;
    }
    u64 equal = 0, bucket = 0;
    if (found) {
        u64 below = 0;
        for (u32 b = 0; b < kBsiKthBuckets; ++b) {
            const u64 h = hist[b];
            if (rank < below + h) {
                bucket = b;
                equal = h;
                break;
            }
            below += h;
        }
        rank -= below;
        less += below;
    }
    const u64 prefix = state[kKthPrefix] | (bucket << (ns - digit_end));
    state[kKthPrefix] = prefix;
    state[kKthRank] = rank;
    state[kKthLess] = less;
    if (last) {
        result[0] = found ? 1ull : 0ull;
        result[1] = found ? prefix : 0ull;
        result[2] = total;
        result[3] = found ? less : 0ull;
        result[4] = found ? equal : 0ull;
    }
}

constexpr int kBsiKthGroupWavesPerSimd = 4;
#ifdef WAH_BSI_KTH_GROUP_SEGMENT_FASTEST
constexpr bool kBsiKthGroupSelectFastest = false;
#else
constexpr bool kBsiKthGroupSelectFastest = true;
#endif

__global__ __launch_bounds__(kSegDecodeWaves * 64, kBsiKthGroupWavesPerSimd) void bsi_kth_group_pass_kernel(const BsiKthGroupArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kSegDecodeWaves][kSegGroups];
    __shared__ __attribute__((aligned(16))) u32 s_top[kBsiKthInLds ? kSegDecodeWaves : 1][kSegGroups]; // the slice of bucket bit 3
    const u32 wave = wave_id(), lane = lane_id();
    u32 *acc = s_acc[wave];
    u32 *top = s_top[kBsiKthInLds ? wave : 0u];
    // (a pass's digit has a slice for the second image in every item that counts, or in none: zeroed once)
    if (kBsiKthInLds) image_fill(top, 0u, lane);

    const u32 nf = a.n_filters, ns = a.n_slices, rows_per_group = a.rows_per_group;
    const u32 digit_first = a.pass * kBsiKthDigitBits;
    const u32 digit_end = min(digit_first + kBsiKthDigitBits, ns);
    const bool last_pass = digit_end == ns;
    // An item is a pair (slow, fast) of item number i = slow * n_fast + fast; a wavefront's next item is a whole grid further on.
    // Both numbers are kept and stepped, so the loop divides nothing.  (Wave-uniform, and said so: they stay scalars.)
    const u32 n_selects = a.n_groups * a.n_queries;
    const u64 n_fast = kBsiKthGroupSelectFastest ? (u64)n_selects : a.n_segments, n_slow = kBsiKthGroupSelectFastest ? a.n_segments : (u64)n_selects;
    const u64 first = (u64)blockIdx.x * kSegDecodeWaves + uniform32(wave), stride = (u64)gridDim.x * kSegDecodeWaves;
    const u64 step_slow = stride / n_fast, step_fast = stride % n_fast;
    u64 slow = uniform64(first / n_fast), fast = uniform64(first % n_fast);
    // With the select running fastest, segment s holds select l at place (l + s / R) % L and not at place l, R = the segments one
    // trip of the grid covers.  Without that turn, and with L a divisor of the grid's wavefronts, a wavefront has ONE select in all
    // its items: the few wavefronts of select 0 then walk all slices of all their segments one after the other in the last pass
    // (they are the items that check, below), and those of a select whose rows are one run of segments (clustered keys) do all
    // of its work, while the rest of the chip has finished (64 sorted groups x {MIN, MAX}, 20 slices: 1.45 ms; DESIGN.md 5.14.1
    // has what the turn makes of it).  The turn depends on the segment alone, so a segment's L items are still its L selects; it is
    // stepped like the item itself: turn = (slow / R) % L, left = slow % R.
    const u64 per_trip = step_slow ? step_slow : 1ull;
    u64 left = uniform64(slow % per_trip);
    u32 turn = uniform32((u32)((slow / per_trip) % n_selects));
    auto turn_on = [&]() {
        if (++turn == n_selects) turn = 0u;
    };

#pragma nounroll
    for (; slow < n_slow; slow += step_slow, fast += step_fast, turn_on()) { // (step_slow is R, or 0 where the grid holds every item)
        if (fast >= n_fast) { // (at most once: both summands were below n_fast)
            fast -= n_fast;
            if (++left == per_trip) {
                left = 0ull;
                turn_on();
            }
            if (++slow >= n_slow) break;
        }
        const u64 seg = kBsiKthGroupSelectFastest ? slow : fast;
        const u32 sel = kBsiKthGroupSelectFastest ? ((u32)fast >= turn ? (u32)fast - turn : (u32)fast + n_selects - turn) : (u32)slow;
        const u32 group = sel / a.n_queries;
        WaveSegment w;
        w.k = seg;
        w.seg = seg;
        w.nvalid = a.groups - seg * kSegGroups < kSegGroups ? (u32)(a.groups - seg * kSegGroups) : kSegGroups;
        const u64 prefix = uniform64(a.state[(u64)sel * kBsiKthStateWords + kKthPrefix]); // what the passes in front of this one decided for this select
        image_fill(acc, 0u, lane); // (the item before left its last slice there)

        KthEq eq;
        KthDigit dg;
        kth_pass_begin(eq, dg, w, a.groups, a.pad_bits, lane);
        bool ok = true, counts = true;
#pragma nounroll
        for (u32 sweep = 0; sweep < 3u; ++sweep) {
            // the sweep's table, its rows, how many of them are plain ANDs, and the digit as kth_pass_fold wants it
            const BitopListOperand *table = sweep == 0u ? a.filters : sweep == 1u ? a.keys + (u64)group * rows_per_group : a.slices;
            const u32 n_rows = sweep == 0u ? nf : sweep == 1u ? rows_per_group : digit_end;
            const u32 n_and = sweep == 2u ? 0u : n_rows;
            const u32 above = sweep == 2u ? digit_first : 0u; // slices above the digit: ANDed by the prefix
            if (n_rows == 0u) continue; // (no filter)
            if (sweep == 2u) {
                u32 any = 0u;
#pragma unroll
                for (int s = 0; s < (int)kSteps; ++s) any |= eq[s];
                // nothing selected here: nothing to count -- unless this item is the one that checks the slices
                if (__ballot(any != 0u) == 0ull && !(last_pass && sel == 0u)) {
                    counts = false;
                    break;
                }
            }
            // every row of an AND sweep is folded; the slices' last stays in the image and is counted
            ok = row_sweep(table, n_rows, sweep == 2u ? n_rows - 1u : n_rows, w, acc, lane,
                           [&](u32 cur) { kth_pass_fold(eq, dg, cur, n_and, ns, above, digit_end, prefix, acc, top, lane); }) && ok;
        }
        if (!ok) return report_stream_error(a.ctrl, lane);
        if (!counts) continue;
        u32 count[kBsiKthBuckets];
    const u32 mine = kth_pass_count(count, eq, dg, acc, top, lane);
        unsigned long long *hist = reinterpret_cast<unsigned long long *>(a.hist) +
                                   (((u64)a.pass * n_selects + sel) * kBsiKthGroupCopies + blockIdx.x % kBsiKthGroupCopies) * kBsiKthBuckets;
        if (lane < kBsiKthBuckets && mine != 0u) atomicAdd(hist + lane, (unsigned long long)mine);
    }
}

// One THREAD per select behind every pass: it sums the copies of its select's histogram of the pass into its own row of the
// LDS table and decides as bsi_kth_decide_kernel's lane 0 does; every group is asked the same queries, so select l reads query
// l % n_queries.
constexpr u32 kBsiKthGroupDecideThreads = 64;
__global__ __launch_bounds__(kBsiKthGroupDecideThreads) void bsi_kth_group_decide_kernel(const BsiKthGroupArgs a) {
    __shared__ u64 s_hist[kBsiKthGroupDecideThreads][kBsiKthBuckets + 1u]; // (+ 1: the threads' rows on different banks)
    const u64 n_selects = (u64)a.n_groups * a.n_queries;
    const u64 sel = (u64)blockIdx.x * kBsiKthGroupDecideThreads + threadIdx.x;
    if (sel >= n_selects) return;
    u64 *mine = s_hist[threadIdx.x];
    const u64 *hist = a.hist + ((u64)a.pass * n_selects + sel) * kBsiKthGroupCopies * kBsiKthBuckets;
    for (u32 b = 0; b < kBsiKthBuckets; ++b) {
        u64 sum = 0;
        for (u32 c = 0; c < kBsiKthGroupCopies; ++c) sum += hist[c * kBsiKthBuckets + b];
        mine[b] = sum;
    }
    kth_decide(mine, a.state + sel * kBsiKthStateWords, a.queries + (sel % a.n_queries) * 3ull, a.results + sel * 5ull, a.pass, a.n_slices);
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_fetch_indexed_device: the values of LISTED rows -- `SELECT price, city ... LIMIT 100` behind the row numbers.  The walk is
// the range kernel's, one table row at a time ORed into the zeroed image; what is kept beside it is not per group but per
// LISTED ROW: lane l owns one listed row of the segment, and when the walk crosses to another table row it reads the ONE bit
// its row has in the image -- group p / 31 of the segment, bit p % 31 -- and the image is zeroed again.
//   WAH_FETCH_BITS   the bit goes to significance n_operands - 1 - row (row 0 most significant: a bit-sliced attribute);
//   WAH_FETCH_FIRST  the first table row whose bit is set is the value (the key of an equality-encoded attribute).
// A table row that was settled in the gather (one zero fill) has no bit anywhere and is not folded at all: only rows that had
// words are, so a clustered index of thousands of bins costs a listed segment its gather and the few bins that live there.
//
// Unlike every other caller of list_walk, ONLY the segments that hold a listed row are walked.  Two launches:
//   fetch_check_kernel  one listed row per thread: below 32 n_words, not smaller than its predecessor.  Row i is the HEAD of an
//                       item when i % 64 == 0 or its segment differs from row i - 1's, so an item is at most 64 consecutive
//                       listed rows of one segment; the heads' list indices are appended to the item list -- a ballot, one
//                       vector atomic add per wave -- in no particular order.
//   fetch_items_kernel  the host cannot know how many items there are, so the grid has a fixed size (at most kFetchGridWaves
//                       wavefronts) and its waves stride over the item list.  The launch order is the only synchronisation.
//                       Nothing is read through a listed row unless the check pass accepted EVERY row: with an error in the
//                       control block the kernel returns at once.
// One wave owns its listed rows across all table rows: no atomics on the output.  A segment with R listed rows is walked
// ceil(R / 64) times (more where items are cut at multiples of 64 of the LIST): the call is for lists that are short beside the
// bitmap.
constexpr u32 kFetchGridWaves = 8192; // wavefronts of fetch_items_kernel at the most: 256 CUs x 4 SIMDs x 8 waves
constexpr u32 kFetchSegBits = kSegGroups * 31u;
static_assert(kFetchGridWaves % kSegDecodeWaves == 0, "whole workgroups");

__global__ __launch_bounds__(256) void fetch_check_kernel(const FetchArgs a) {
    const u32 lane = lane_id();
    const u64 n_waves = (u64)gridDim.x * 4u;
    unsigned long long *counter = reinterpret_cast<unsigned long long *>(a.ctrl + kCtlFetchItems);
    bool bad = false;
#pragma nounroll
    for (u64 base = ((u64)blockIdx.x * 4u + wave_id()) * 64u; base < a.n_rows; base += n_waves * 64u) { // (wave-uniform)
        const u64 i = base + lane;
        const bool has = i < a.n_rows;
        u64 p = 0, before = 0;
        if (has) {
            p = a.rows[i];
            if (i) before = a.rows[i - 1];
        }
        bad |= has && (p >= a.n_bits || p < before);
        const bool head = has && (lane == 0u || p / kFetchSegBits != before / kFetchSegBits); // (base is a multiple of 64)
        const u64 heads = __ballot(head);                                                    // (lane 0 has a row: never 0)
        u64 first = 0;
        if (lane == 0u) first = atomicAdd(counter, (unsigned long long)__popcll(heads));
        first = uniform64(first);
        // a list that does not ascend can have more heads than the list has room for: it is refused, and nothing is put outside
        const u64 slot = first + (u64)__popcll(heads & ((1ull << lane) - 1ull));
        if (head && slot < a.capacity) a.items[slot] = i;
    }
    if (__ballot(bad) != 0ull) report_stream_error(a.ctrl, lane);
}

template <u32 kMode>
__global__ __launch_bounds__(kSegDecodeWaves * 64, 8) void fetch_items_kernel(const FetchArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    if (a.ctrl[kCtlError] != 0u) return; // a refused row: no stream is read
    const u64 counted = *reinterpret_cast<const u64 *>(a.ctrl + kCtlFetchItems);
    const u64 n_items = counted < a.capacity ? counted : a.capacity;
    const u64 stride = (u64)gridDim.x * kSegDecodeWaves;
    u32 *acc = s_acc[wave];
    image_fill(acc, 0u, lane);
    const ListOp m = list_op(1u); // a table row is ORed into the zeroed image

#pragma nounroll
    for (u64 t = (u64)blockIdx.x * kSegDecodeWaves + wave; t < n_items; t += stride) {
        // the item: the listed rows from its head up to the next multiple of 64 of the list that lie in the head's segment (the
        // list ascends: they are the first ones)
        const u64 i0 = uniform64(a.items[t]);
        if (i0 >= a.n_rows) continue;
        const u64 behind = (i0 | 63ull) + 1ull;
        const u64 i = i0 + lane;
        const bool has = i < (behind < a.n_rows ? behind : a.n_rows);
        const u64 p = has ? a.rows[i] : 0ull;
        const u64 group = p / 31u;
        const u64 seg = uniform64(group / kSegGroups);
        const u64 g0 = seg * kSegGroups;
        if (g0 >= a.groups) continue; // (no accepted row lies there)
        const bool mine = has && group / kSegGroups == seg;
        const u32 g = mine ? (u32)(group - g0) : 0u, bit = (u32)(p - group * 31u);
        const u32 nvalid = a.groups - g0 < kSegGroups ? (u32)(a.groups - g0) : kSegGroups;

        u64 v = kMode == kFetchFirst ? ~0ull : 0ull;
        u32 cur = 0;       // the table row the image holds (wave-uniform)
        bool open = false; // ... if it holds one: rows settled in the gather never get there
        // fold the image's row into the listed rows' values and zero the image for the next one (not row_sweep: only the rows
        // that had words are folded, so the crossing is begin_row itself and no row number is counted up to)
        auto fold = [&]() {
            const u32 b = (acc[g] >> bit) & 1u;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            image_fill(acc, 0u, lane);
            if (kMode == kFetchBits)
                v |= (u64)b << ((a.n_operands - 1u - cur) & 63u); // (at most 64 table rows: 0 .. 63, never a shift by 64)
            else if (b != 0u && v == ~0ull)
                v = cur;
        };
        const bool ok = list_walk(a.table, a.n_operands, seg, nvalid, m.fill, acc, lane, [&](u32) -> const ListOp & { return m; }, [&](u32 j) {
            if (open) fold(); // this row's words begin: the one in the image is complete
            cur = j;
            open = true;
        });
        if (open) fold();
        if (!ok) return report_stream_error(a.ctrl, lane);
        if (mine) a.out[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// wah_splice_indexed_device: row ranges ("pieces") of indexed bitmaps concatenated into new indexed bitmaps, at any bit offset,
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
//                            as from_positions_kernel shares its items out.  A wavefront searches the starts for the pieces
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
constexpr u32 kSpliceSegBits = kSegGroups * 31u; // 31 744
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
    const u64 n_waves = (u64)gridDim.x * kSegDecodeWaves;
    const u64 per = (n_items + n_waves - 1) / n_waves;
    const u64 w = (u64)blockIdx.x * kSegDecodeWaves + wave;
    const u64 begin = w * per < n_items ? w * per : n_items, end = begin + per < n_items ? begin + per : n_items;
    if (kEmit && w == 0 && lane == 0) {
        const u64 total = a.offsets[n_items];
        *a.out_words = total;
        if (total > a.out_capacity) atomicOr(a.ctrl + kCtlError, kErrCapacity);
    }
    const u64 all_rows = uniform64(a.starts[a.n_pieces]); // T: at most 32 n_words_out (the check launch)
    const ListOp m = list_op(1u);                         // a source segment is ORed into the zeroed image
#pragma nounroll
    for (u64 item = begin; item < end; ++item) {
        const u64 c = item / a.n_segments, seg = item - c * a.n_segments;
        const u64 base = seg * (u64)kSpliceSegBits;
        const u32 ngroups = seg + 1 == a.n_segments ? (u32)(a.groups - seg * kSegGroups) : kSegGroups;
        u32 total;
        if (base >= all_rows) {
            // behind the last piece: one zero-fill of the segment's groups; no LDS image, no load
            total = 1u;
            if (kEmit && lane == 0) stage[0] = fill_word(kTypeZero, ngroups);
        } else {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            image_fill(dst, 0u, lane);
            const u64 limit = base + kSpliceSegBits < all_rows ? base + kSpliceSegBits : all_rows;
            // the first piece that ends behind `base` (there is one: base < T)
            u64 lo = 0, hi = a.n_pieces - 1;
            while (lo < hi) {
                const u64 mid = lo + (hi - lo) / 2;
                if (uniform64(a.starts[mid + 1]) > base) hi = mid; else lo = mid + 1;
            }
#pragma nounroll
            for (u64 p = lo; p < a.n_pieces; ++p) {
                const u64 st = uniform64(a.starts[p]), en = uniform64(a.starts[p + 1]);
                if (st >= limit) break;
                if (en <= st || en <= base) continue; // (no rows; en <= base only for pieces of no rows at `base`)
                const u64 d0 = st > base ? st : base, d1 = en < limit ? en : limit;
                const u64 n_words = uniform64(a.pieces[p].n_words), first_row = uniform64(a.pieces[p].first_row);
                const u64 s0 = first_row + (d0 - st), s1 = s0 + (d1 - d0); // (accepted: s1 <= 32 n_words)
                const u64 src_groups = (32ull * n_words + 30ull) / 31ull;
                const BitopListOperand *entry = a.table + (p * a.n_columns + c);
#pragma nounroll
                for (u64 ss = s0 / kSpliceSegBits; ss * kSpliceSegBits < s1; ++ss) {
                    const u64 sbase = ss * kSpliceSegBits;
                    const u64 t0 = s0 > sbase ? s0 : sbase, t1 = s1 < sbase + kSpliceSegBits ? s1 : sbase + kSpliceSegBits;
                    if (ss * kSegGroups >= src_groups) break; // (never for an accepted piece)
                    const u32 nvalid = src_groups - ss * kSegGroups < kSegGroups ? (u32)(src_groups - ss * kSegGroups) : kSegGroups;
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
        if (kEmit) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const u64 at = a.offsets[item], room = a.offsets[item + 1] - at; // what the count pass found
            const u32 words = (u64)total < room ? total : (u32)room;
            for (u32 i = lane; i < words; i += 64u)
                if (at + i < a.out_capacity) a.out[at + i] = stage[i];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the next item stages over these words
        } else if (lane == 0) {
            a.offsets[item] = (u64)total;
        }
    }
}

// one wavefront per segment, kSegDecodeWaves of them per workgroup
template <class Args>
hipError_t launch_per_segment(void (*kernel)(const Args), u64 n_segments, const Args &a, hipStream_t s) {
    if (n_segments == 0) return hipSuccess;
    const u64 grid = (n_segments + kSegDecodeWaves - 1) / kSegDecodeWaves;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kSegDecodeWaves * 64), 0, s, a);
    return hipGetLastError();
}

} // namespace

hipError_t launch_bitop_list_segments(const BitopListArgs &a, hipStream_t s) { return launch_per_segment(bitop_list_segments_kernel, a.g.n_segments, a, s); }
hipError_t launch_bitop_clauses_segments(const BitopClausesArgs &a, hipStream_t s) { return launch_per_segment(bitop_clauses_segments_kernel, a.g.n_segments, a, s); }
hipError_t launch_bsi_range_segments(const BsiRangeArgs &a, hipStream_t s) { return launch_per_segment(bsi_range_segments_kernel, a.g.n_segments, a, s); }
hipError_t launch_bsi_compare_segments(const BsiCompareArgs &a, hipStream_t s) { return launch_per_segment(bsi_compare_segments_kernel, a.g.n_segments, a, s); }
hipError_t launch_bsi_arith_segments(const BsiArithArgs &a, hipStream_t s) { return launch_per_segment(bsi_arith_segments_kernel, a.n_segments, a, s); }
hipError_t launch_bsi_mul_segments(const BsiMulArgs &a, hipStream_t s) { return launch_per_segment(bsi_mul_segments_kernel, a.n_segments, a, s); }
hipError_t launch_bsi_kth_pass(const BsiKthArgs &a, hipStream_t s) { return launch_per_segment(bsi_kth_pass_kernel, a.n_segments, a, s); }

hipError_t launch_fetch_check(const FetchArgs &a, hipStream_t s) {
    if (a.n_rows == 0) return hipSuccess;
    const u64 want = (a.n_rows + 255) / 256;
    constexpr u64 most = 256u * 8u;
    hipLaunchKernelGGL(fetch_check_kernel, dim3((unsigned)(want > most ? most : want)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// a grid of fixed size -- the item count is known to the device only --, smaller only where the item list has no room for more
hipError_t launch_fetch_items(const FetchArgs &a, u32 mode, hipStream_t s) {
    if (a.n_rows == 0) return hipSuccess;
    const u64 waves = a.capacity < kFetchGridWaves ? a.capacity : kFetchGridWaves;
    const dim3 grid((unsigned)((waves + kSegDecodeWaves - 1) / kSegDecodeWaves)), block(kSegDecodeWaves * 64);
    if (mode == kFetchFirst)
        hipLaunchKernelGGL(fetch_items_kernel<kFetchFirst>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(fetch_items_kernel<kFetchBits>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_splice_check(const SpliceArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(splice_check_kernel, dim3(1), dim3(kSpliceCheckThreads), 0, s, a);
    return hipGetLastError();
}

// count pass (emit = false: every item's words to a.offsets) or emit pass (a.offsets scanned: the words to their place)
hipError_t launch_splice_segments(const SpliceArgs &a, bool emit, hipStream_t s) {
    const u64 n_items = a.n_columns * a.n_segments;
    const u64 want = (n_items + kSegDecodeWaves - 1) / kSegDecodeWaves;
    constexpr u64 most = 256u * 5u; // CUs x resident workgroups of four wavefronts at 32 KiB of LDS each
    const dim3 grid((unsigned)(want < 1 ? 1 : want > most ? most : want)), block(kSegDecodeWaves * 64);
    if (emit)
        hipLaunchKernelGGL(splice_segments_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(splice_segments_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_bsi_kth_decide(const BsiKthArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(bsi_kth_decide_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

// one wavefront per (segment, select) item while the chip holds them all at once; beyond that a wavefront takes several
hipError_t launch_bsi_kth_group_pass(const BsiKthGroupArgs &a, hipStream_t s) {
    const u64 n_items = a.n_segments * a.n_groups * a.n_queries;
    if (n_items == 0) return hipSuccess;
    const u64 want = (n_items + kSegDecodeWaves - 1) / kSegDecodeWaves;
    constexpr u64 most = 256u * 4u; // CUs x resident workgroups of four wavefronts at four waves per SIMD
    hipLaunchKernelGGL(bsi_kth_group_pass_kernel, dim3((unsigned)(want > most ? most : want)), dim3(kSegDecodeWaves * 64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_bsi_kth_group_decide(const BsiKthGroupArgs &a, hipStream_t s) {
    const u32 n_selects = a.n_groups * a.n_queries;
    hipLaunchKernelGGL(bsi_kth_group_decide_kernel, dim3((n_selects + kBsiKthGroupDecideThreads - 1u) / kBsiKthGroupDecideThreads),
                       dim3(kBsiKthGroupDecideThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace wah
#endif // WAH_LIST_WALK_ONLY
