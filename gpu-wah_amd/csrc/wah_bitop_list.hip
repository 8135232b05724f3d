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
//   bsi_div_segments_kernel        A / B, A % B row by row as a new bit-sliced attribute (wah_bsi_div_indexed_device)
//   bsi_kth_pass_kernel            one pass of the radix select over such an attribute (wah_bsi_kth_indexed_device)
//   bsi_kth_group_pass_kernel      the same pass for every (group, query) pair of a GROUP BY at once (wah_bsi_kth_grouped_indexed_device)
//   fetch_items_kernel             the values of listed rows, one wavefront per 64 listed rows of a segment (wah_fetch_indexed_device)
// The walk itself is written once (list_walk, wah_list_walk.hpp), and so is the sweep that keeps one row at a time in the zeroed
// image (row_sweep); a kernel adds the state it keeps per segment, how a row is folded into it, and what it stores or counts.
//
// The rows are named by a table in DEVICE memory (wah_bitop_operand, include/wah.h) that only these kernels read: the host
// never sees it, so a captured launch replayed over a rewritten table combines the new selection.  Nothing is decided from the
// rows' lengths on the host -- one route, whatever they hold.
#include "wah_list_walk.hpp"

namespace wah {
namespace {

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
// wah_bsi_div_indexed_device: floor(A / B) or A mod B row by row over two bit-sliced attributes of ka and kb slices, as a NEW
// bit-sliced attribute of n_out slices -- restoring long division over the slices, the multiplication kernel's machine run the
// other way.  The dividend is consumed from the top and the divisor has to be whole before the first quotient slice leaves, so
// the table is: A's existence row, then B's, where they have one; then ALL of B's slices, LEAST significant first; then ALL of
// A's, MOST significant first.  A row with B = 0 has no result: the existence row of the output, which is ALWAYS there, is the
// AND of the bitmaps present and of (B != 0).
//
// The wave's own area of the scratch (BsiDivArgs.work), in the multiplication kernel's group form (quad 64 q + lane, a lane only
// ever reads back what it wrote itself): kb slices of B's image, then R and T of kb + 1 slices each -- 3 kb + 2 slices of 4 KiB.
// R is the remainder shifted up by one with the dividend's next bit below it, T = R - B, and which of the two is the remainder
// is the quotient bit q: nobody moves anything, the next step blends while it reads.  The state beside the walk is ex (preset
// to all ones) and, while B arrives, nz (the OR of B's slices, preset to zero).  The fold:
//   an existence row      ex &= acc
//   B's slice s           the image's groups leave into slice s of the wave's area;  nz |= acc;  at s = kb - 1:  ex &= nz
//   A's slice i           Rn = the image's groups (the dividend's bit);  borrow = 0;  for s = 0 .. kb, with b = B_s (0 at s = kb):
//                             Tn = Rn ^ b ^ borrow;  borrow = (~Rn & b) | (~(Rn ^ b) & borrow);
//                             Re = q ? T[s] : R[s]  (s < kb: the remainder the step before left, read in front of the stores);
//                             R[s] = Rn;  T[s] = Tn;  Rn = Re  (the shift: slice s of the old remainder is slice s + 1 of R)
//                         then q = ~borrow;  q & ex leaves as matrix row n_out - 1 - i of the quotient
// The ripple runs over kb + 1 slices: the shifted remainder reaches 2^(kb + 1) - 1 where B's top slice is set.  Slice kb of the
// remainder itself is always zero (it is below B), so nothing reads R[kb] or T[kb], and step kb needs only its borrow: it
// stores neither.  q lives in the slot of T[kb]: the fold runs quarter by quarter in a loop, as the multiplication fold does,
// and sixteen registers picked by the quarter's number would become an array in private memory (Makefile: asm -- with q
// in registers the kernel spills, rolled or unrolled); a quarter reads its quad of q in front of its steps and writes it behind.
// While every slice of A seen so far was all zero in this segment (wave-uniform: one ballot over the image; a settled row is
// folded as the zeros it is) the remainder is still zero and every row that exists has B >= 1: the step stores a zero quotient
// slice and touches nothing.  The first step that runs takes Re as zeros without reading the area -- which is why nothing needs
// clearing, as j == 0 in the multiplication fold -- and from then on no zero slice is skipped: values far below their declared
// width cost their real width.  So do divisors: B's slices above its last one that is not all zero in this segment (kb_run of
// them remain, wave-uniform, known when B is complete) are zeros in every row, the remainder stays below 2^kb_run, and the
// ripple of every step runs over kb_run + 1 slices instead of kb + 1.  Both skips are inside the fold: every row's every
// segment is walked and checked whatever the data, the mode and n_out.  A quotient slice at or above n_out, and every one in
// REMAINDER mode, is stored through a descriptor of no bytes.  In a quarter b, borrow, Rn, Re and the next step's b, R and T are one quad each, so the loads of step s + 1 are in
// flight behind the stores of step s within the launch bound.
// Behind the sweep: QUOTIENT zeros for the slices at and above ka; REMAINDER Re[sig] & ex for sig < min(kb, n_out) (zeros where
// no step ran) and zeros above; then the ex row.  Every word of the matrix is written by exactly one wave.  A wave that refuses
// something reports and stores nothing more.
__global__ __launch_bounds__(kSegDecodeWaves * 64, kBsiWavesPerSimd) void bsi_div_segments_kernel(const BsiDivArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_acc[kSegDecodeWaves][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    WaveSegment w;
    if (!wave_segment(w, 0ull, a.n_segments, a.groups, wave)) return;
    u32 *acc = s_acc[wave];
    image_fill(acc, 0u, lane);

    const u32 ka = a.n_slices_a, kb = a.n_slices_b, n_out = a.n_slices_out;
    const u32 n_ex = a.exists_a + a.exists_b, n_rows = n_ex + kb + ka;
    const bool quotient = a.remainder == 0u;
    // (wave-uniform) quad 0 of B's slice 0, of R[0] and of T[0]; the lane's quad of quarter qd is 64 qd + lane behind them
    MulQuad *const divisor = reinterpret_cast<MulQuad *>(a.work) + w.k * (u64)(3u * kb + 2u) * kSliceQuads;
    MulQuad *const rem = divisor + (u64)kb * kSliceQuads;
    MulQuad *const tri = rem + (u64)(kb + 1u) * kSliceQuads;
    // the lane's quad of quarter qd of slice s behind one of them
    auto quad = [&](MulQuad *base, u32 s, u32 qd) -> MulQuad & { return base[(u64)s * kSliceQuads + 64u * qd + lane]; };

    // matrix row `row` of this wave's segment; live == false: a descriptor of no bytes, every store through it is dropped
    auto row_store = [&](u32 row, bool live) {
        return seg_store_setup(a.matrix + (u64)row * a.n_words, live ? a.n_words : 0ull, w.seg, w.k, lane);
    };

    u32 ex[kSteps], nz[kSteps]; // group 64 s + lane
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) {
        ex[s] = kOnes31;
        nz[s] = 0u;
    }
    bool started = false; // (wave-uniform) a slice of A that is not all zero has been seen: R and T hold a step's result
    u32 kb_run = 1u;      // (wave-uniform) B's slices up to its last one that is not all zero in this segment, at least one
    const bool ok = row_sweep(a.table, n_rows, n_rows, w, acc, lane, [&](u32 cur) {
        if (cur < n_ex) {
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) ex[s] &= acc[64 * s + (int)lane];
            return;
        }
        const u32 r = cur - n_ex;
        if (r < kb) { // B's slice r
            u32 any = 0u;
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                MulQuad v;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    v[t] = acc[64 * (4 * qd + t) + (int)lane];
                    nz[4 * qd + t] |= v[t];
                    any |= v[t];
                }
                quad(divisor, r, (u32)qd) = v;
            }
            if (__ballot(any != 0u) != 0ull) kb_run = r + 1u;
            if (r + 1u == kb) {
#pragma unroll
                for (int s = 0; s < (int)kSteps; ++s) ex[s] &= nz[s];
            }
            return;
        }
        // A's slice i
        const u32 i = ka - 1u - (r - kb);
        const bool live = quotient && i < n_out;
        const SegStore st = row_store(live ? n_out - 1u - i : 0u, live);
        const bool first = !started;
        if (first) {
            u32 any = 0u;
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) any |= acc[64 * s + (int)lane];
            if (__ballot(any != 0u) == 0ull) { // the remainder is still zero: a zero quotient slice, nothing else
#pragma unroll
                for (int s = 0; s < (int)kSteps; ++s) seg_store(st, s, 0u);
                return;
            }
            started = true;
        }
#pragma nounroll
        for (u32 qd = 0; qd < 4u; ++qd) {
            MulQuad rn;
#pragma unroll
            for (int t = 0; t < 4; ++t) rn[t] = acc[64u * (4u * qd + (u32)t) + lane];
            MulQuad qm = MulQuad(0u), re = MulQuad(0u); // re: Re[s], which becomes slice s + 1 of the next R
            if (!first) {
                qm = quad(tri, kb, qd);
                re = (quad(tri, 0u, qd) & qm) | (quad(rem, 0u, qd) & ~qm);
            }
            MulQuad borrow = MulQuad(0u), b = quad(divisor, 0u, qd);
#pragma nounroll
            for (u32 s = 0; s < kb_run; ++s) {
                MulQuad bn = MulQuad(0u), rx = MulQuad(0u), tx = MulQuad(0u);
                if (s + 1u < kb_run) { // (wave-uniform) step s + 1's loads, in front of step s's stores
                    bn = quad(divisor, s + 1u, qd);
                    if (!first) {
                        rx = quad(rem, s + 1u, qd);
                        tx = quad(tri, s + 1u, qd);
                    }
                }
                const MulQuad x = rn ^ b;
                quad(rem, s, qd) = rn;
                quad(tri, s, qd) = x ^ borrow;
                borrow = (~rn & b) | (~x & borrow);
                rn = re;
                b = bn;
                re = (tx & qm) | (rx & ~qm);
            }
            // the last step, where b = 0, stores nothing: the borrow goes on where that slice of R is clear, and q = ~borrow
            quad(tri, kb, qd) = rn | ~borrow;
        }
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            const MulQuad qn = quad(tri, kb, (u32)qd);
#pragma unroll
            for (int t = 0; t < 4; ++t) seg_store(st, 4 * qd + t, qn[t] & ex[4 * qd + t]);
        }
    });
    if (!ok) return report_stream_error(a.ctrl, lane);
    if (quotient) { // at and above ka there is nothing but zeros
#pragma nounroll
        for (u32 sig = ka; sig < n_out; ++sig) {
            const SegStore st = row_store(n_out - 1u - sig, true);
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) seg_store(st, s, 0u);
        }
    } else { // the remainder the last step left, least significant first; at and above kb zeros
        const u32 n_rem = started ? (kb_run < n_out ? kb_run : n_out) : 0u;
        MulQuad qm[4];
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) qm[qd] = started ? quad(tri, kb, (u32)qd) : MulQuad(0u);
#pragma nounroll
        for (u32 sig = 0; sig < n_out; ++sig) {
            const SegStore st = row_store(n_out - 1u - sig, true);
            MulQuad v[4];
#pragma unroll
            for (int qd = 0; qd < 4; ++qd)
                v[qd] = sig < n_rem ? (quad(tri, sig, (u32)qd) & qm[qd]) | (quad(rem, sig, (u32)qd) & ~qm[qd]) : MulQuad(0u);
#pragma unroll
            for (int s = 0; s < (int)kSteps; ++s) seg_store(st, s, v[s / 4][s % 4] & ex[s]);
        }
    }
    const SegStore st = row_store(n_out, true);
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) seg_store(st, s, ex[s]);
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
        const bool head = has && (lane == 0u || p / kSegBits != before / kSegBits); // (base is a multiple of 64)
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
        const u32 nvalid = segment_groups(a.groups, seg);

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
hipError_t launch_bsi_div_segments(const BsiDivArgs &a, hipStream_t s) { return launch_per_segment(bsi_div_segments_kernel, a.n_segments, a, s); }
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
