// wah_select.hip -- what a query wants from a result bitmap, without decoding it: how many bits it has set
// (wah_count_list_indexed_device: one count per operand of a table -- COUNT(*), or the GROUP BY histogram of an
// equality-encoded attribute) and which ones (wah_positions_indexed_device: the positions of the set bits of a window of ranks,
// in ascending order -- SELECT rowid ... LIMIT / OFFSET).  The reference has no counterpart.
//
// and how many bits it shares with each of many others (wah_count_masked_indexed_device: the popcount of mask AND operand for every
// pair of two tables -- GROUP BY under a WHERE filter, the cross-tab of two attributes; wah_group_sum_indexed_device: the same under
// the AND of several rows per group, with the group's own count and the sums of bit-sliced attributes -- SELECT g, h, COUNT(*),
// SUM(x) WHERE ... GROUP BY g, h).
//
// Five kinds of launches, and no workgroup of any of them waits for another.  The three counting kernels share their frame, and
// every shared piece is written once, by the helper named here:
//   the items             shared out over the launch's wavefronts in contiguous runs (item_run, wah_device.hpp).  A table row is
//                         checked before its index pointer is followed, the index range (seg_range) before the stream is read
//                         through it (select_range); the segment's words are loaded two per lane per batch of 128 (seg_load_words)
//                         and the next item's row and range are on their way while this one's words are counted.
//   where they lie        an operand's words are counted without decoding a group (count_where_they_lie): a literal is its
//                         popcount, a one-fill 31 bits per group, a zero-fill nothing.  The words' groups are summed beside the
//                         bits, and a segment whose words do not make up exactly its groups, or that holds an empty fill, is
//                         refused (kErrStream) and counts nothing.
//   the run ends          a wavefront sums its run and adds into global memory with 64-bit vector atomics only when the counter
//                         it counts for changes; what the workgroup's four wavefronts hold at their runs' ends is merged in LDS
//                         first (merge_run_ends; select_count_kernel: its own scalar form of it).
//   select_count_kernel   (operand, segment) pairs, one counter per operand; the positions call stores every segment's count
//                         into its rank table instead.  The cost goes with the operands' words.
//   count_masked_kernel   (mask, chunk of up to 64 operands, segment) items (ChunkCursor).  The mask's segment is decoded (seg_mark /
//                         seg_group) into a per-wavefront LDS image M[1024] of its groups, pad bits cleared, beside P[1024], the
//                         exclusive prefix sum of their popcounts (image_prefix); the words of the chunk's operands are counted
//                         against it (count_against_image), lane l keeping the l-th operand's count (count_under_mask): a literal
//                         at group lo is popcount(x & M[lo]), a one-fill of n groups P[lo + n] - P[lo], a zero-fill nothing.  A
//                         mask segment of one fill word needs no image: zeros count nothing, under ones the words count where
//                         they lie.  LDS: 10 KiB per wavefront, 40 960 B per workgroup: four workgroups per CU.
//   group_count_kernel /  count_masked_kernel's items, LDS and run ends with an image that is the AND of the call's filter rows and
//   group_fold_kernel     the group's own: made conjunct by conjunct, the first one stored, the later ones ANDed in place, P and the
//                         pad bits in one pass behind the last; a conjunct of one one-fill is skipped, one zero-fill leaves nothing
//                         to count, and the conjunction's own bits are counted once per (group, segment).  The fold: one thread per
//                         (group, attribute) adds the counts of the attribute's slices, shifted, in 128 bits.
//   rank_reduce_kernel /  the exclusive prefix sum of the rank table (one u64 per segment, + 1 for the total): chunks of 4096
//   rank_scan_kernel      entries, their totals one level up (two levels up for more than 2^24 segments), scanned there, then
//                         every chunk scans itself in place on top of what lies in front of it.  The top level is at most
//                         4096 entries whatever the bitmap's length (n_words < 2^40: 2^30 segments, 2^18 chunks, 67 chunks of
//                         chunks).
//   select_emit_kernel    one wavefront per segment.  A segment whose ranks miss the window has read two table entries and
//                         is done.  Otherwise seg_mark / seg_group give lane l the group 64 s + l of step s; popcount, a wave
//                         scan and the running rank give every set bit its rank.  The bits' in-segment positions (15 bits) are
//                         staged in LDS, one 16-bit slot per bit, 64 x 31 slots: a step's worth -- and flushed by lane i taking
//                         slot i + 64 j, so that the 8-byte stores of a wave go to consecutive addresses (a lane that stored its
//                         own bits would issue up to 31 stores at a stride of its neighbours' popcounts).  The window is a
//                         compare per store.  A step without a set bit, or with its ranks outside the window, stages nothing.
//                         LDS: 5 KiB for the mark phase + 3968 B staging per wavefront, 36 352 B per workgroup: four workgroups
//                         (sixteen wavefronts) per CU.
// The pad rule (include/wah.h): the last group of the bitmap has 31 G - 32 n_words bits that lie behind the bitmap; whatever
// the stream says there -- a literal with those bits set, a one-fill over the group -- they are neither counted nor listed.
#include "wah_segdecode.hpp"

namespace wah {
namespace {

// the table and the indexes are read-only for a launch and every address below is the same in all lanes: through the scalar cache
typedef const __attribute__((address_space(4))) u64 *SelConstU64;

// one row of the operand table, or the call's one operand
struct SelectRow {
    u64 comp, c_words, offs;
};
template <bool kTable>
__device__ __forceinline__ SelectRow select_row(const SelectCountArgs &a, u64 j) {
    SelectRow r;
    if (kTable) {
        const SelConstU64 e = (SelConstU64)(uintptr_t)(a.table + j);
        r.comp = e[0];
        r.c_words = e[1];
        r.offs = e[2];
    } else {
        r.comp = (u64)(uintptr_t)a.one.comp;
        r.c_words = a.one.c_words;
        r.offs = (u64)(uintptr_t)a.one.offs;
    }
    return r;
}
// the operand's words of segment `seg`: the entry is checked, then the index pair read and checked (bad: refused, no words)
__device__ __forceinline__ SegRange select_range(const SelectRow &r, u64 groups, u64 seg) {
    const bool entry_ok = r.offs != 0ull && (r.offs & 7ull) == 0ull && r.comp != 0ull && (r.comp & 3ull) == 0ull && r.c_words < (1ull << 40);
    u64 w0 = 0, w1 = 0;
    if (entry_ok) {
        const SelConstU64 p = (SelConstU64)(uintptr_t)r.offs + seg;
        w0 = p[0];
        w1 = p[1];
    }
    SegmentsArgs sa = {};
    sa.c_words = r.c_words;
    sa.groups = groups;
    SegRange rg = seg_range(sa, seg, w0, w1);
    if (!entry_ok) {
        rg.bad = 1u;
        rg.cnt = 0u;
        rg.w0 = 0;
    }
    return rg;
}

// what a lane's words of a segment count: their bits, their groups, and whether one of them is a fill of no groups
struct SegCount {
    u32 bits, grps;
    bool empty_word;
};
// the verdict on a segment whose words make up `grps` groups in all, as seg_mark gives it: exactly its groups, no word empty
__device__ __forceinline__ bool segment_ok(const SegRange &rg, u32 grps, bool empty_word) {
    return !rg.bad && grps == rg.nvalid && __ballot(empty_word) == 0ull;
}
// A segment's words counted where they lie.  count_bits: a literal counts its popcount and a one-fill 31 bits per group (otherwise
// only the groups are counted); the bitmap's last word -- the last word of its last segment -- loses the pad bits.
__device__ __forceinline__ SegCount count_where_they_lie(const SegRange &rg, const u32 (&x0)[kSegBatches], const u32 (&x1)[kSegBatches], bool count_bits,
                                                         bool last_seg, u32 pad_bits, u32 pad_mask, u32 lane) {
    bool empty_word = false;
    u32 grps = 0, bits = 0;
#pragma unroll
    for (int b = 0; b < kSegBatches; ++b) {
        if (128u * b < rg.cnt) { // wave-uniform
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const u32 x = h ? x1[b] : x0[b];
                const u32 i = 128u * b + 2u * lane + h;
                const bool in = i < rg.cnt;
                // counts are clamped so that a corrupt word cannot wrap the 32-bit sums; anything above 1024 fails the total
                const u32 n = in ? min(word_groups(x), 2u * kSegGroups) : 0u;
                empty_word |= in && n == 0u;
                const bool lit = (int)x >= 0, ones = (x & kFillOne) == kFillOne;
                const bool last_word = last_seg && i == rg.cnt - 1u; // of the bitmap
                const u32 pad = last_word ? pad_bits : 0u;
                const u32 fill_bits = ones && n ? 31u * n - pad : 0u;
                bits += !(in && count_bits) ? 0u : lit ? (u32)__builtin_popcount(x & (last_word ? pad_mask : kOnes31)) : fill_bits;
                grps += n;
            }
        }
    }
    return {bits, grps, empty_word};
}

// kTable: one count per table row, added up over its segments; otherwise the one operand `one`, one count per segment.
// Why the runs are CONTIGUOUS and their ends merged: an atomic per segment would be 270 000 of them on ONE address for a 1 GiB
// operand, 11.6 ns each (3.2 ms, measured; the words themselves take a tenth of that).
template <bool kTable>
__global__ __launch_bounds__(kSegDecodeWaves * 64, 8) void select_count_kernel(const SelectCountArgs a) {
    __shared__ u64 s_j[kSegDecodeWaves], s_acc[kSegDecodeWaves];
    const u32 wave = wave_id(), lane = lane_id();
    const u64 n_items = kTable ? (u64)a.n_operands * a.n_segments : a.n_segments;
    const ItemRun run = item_run(n_items, kSegDecodeWaves, wave);
    const u64 begin = run.begin, end = run.end;
    const u32 pad_mask = kOnes31 >> a.pad_bits;
    u64 j = kTable ? begin / a.n_segments : 0ull;
    u64 seg = begin - j * a.n_segments;
    u64 acc = 0;
    bool refused = false;
    SelectRow row = {}, next_row = {};
    SegRange next = {};
    if (begin < end) {
        next_row = select_row<kTable>(a, j);
        next = select_range(next_row, a.groups, seg);
    }
#pragma nounroll
    for (u64 item = begin; item < end; ++item) {
        const SegRange rg = next;
        row = next_row;
        SegmentsArgs sa = {};
        sa.comp = reinterpret_cast<const u32 *>((uintptr_t)row.comp);
        u32 x0[kSegBatches], x1[kSegBatches];
        seg_load_words(sa, rg, x0, x1, lane);
        // the pair behind this one
        const bool last_of_operand = seg + 1 == a.n_segments;
        const u64 j_next = last_of_operand ? j + 1 : j, seg_next = last_of_operand ? 0ull : seg + 1;
        if (item + 1 < end) {
            if (kTable && last_of_operand) next_row = select_row<kTable>(a, j_next);
            next = select_range(next_row, a.groups, seg_next);
        }
        const SegCount n = count_where_they_lie(rg, x0, x1, true, last_of_operand, a.pad_bits, pad_mask, lane);
        const u32 total_grps = wave_total32(n.grps), total_bits = wave_total32(n.bits);
        const bool ok = segment_ok(rg, total_grps, n.empty_word);
        refused |= !ok;
        if (kTable) {
            acc += ok ? (u64)total_bits : 0ull;
            if (last_of_operand && item + 1 < end) { // the run goes on with another operand
                if (lane == 0 && acc) atomicAdd(reinterpret_cast<unsigned long long *>(a.counts + j), (unsigned long long)acc);
                acc = 0;
            }
        } else if (lane == 0) {
            a.counts[seg] = ok ? (u64)total_bits : 0ull;
        }
        if (item + 1 < end) {
            j = j_next;
            seg = seg_next;
        }
    }
    if (refused && lane == 0) atomicOr(a.ctrl + kCtlError, kErrStream);
    if (kTable) {
        // what the workgroup's wavefronts hold for the operands their runs end in: consecutive runs, so equal operands are neighbours
        if (lane == 0) {
            s_j[wave] = begin < end ? j : ~0ull;
            s_acc[wave] = acc;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 at = ~0ull, sum = 0;
            for (int v = 0; v < kSegDecodeWaves; ++v) {
                if (s_j[v] != at) {
                    if (at != ~0ull && sum) atomicAdd(reinterpret_cast<unsigned long long *>(a.counts + at), (unsigned long long)sum);
                    at = s_j[v];
                    sum = 0;
                }
                sum += s_acc[v];
            }
            if (at != ~0ull && sum) atomicAdd(reinterpret_cast<unsigned long long *>(a.counts + at), (unsigned long long)sum);
        }
    }
}

// ---- counts under a mask, and under a conjunction: what the two chunked kernels share ------------------------------------------
__device__ __forceinline__ SelectRow table_row(const BitopListOperand *table, u64 j) {
    const SelConstU64 e = (SelConstU64)(uintptr_t)(table + j);
    SelectRow r;
    r.comp = e[0];
    r.c_words = e[1];
    r.offs = e[2];
    return r;
}

// what a wavefront knows of the mask segment it holds
constexpr u32 kMaskNone = 0, kMaskZeros = 1, kMaskOnes = 2, kMaskImage = 3, kMaskBad = 4;
// LDS of one wavefront: P (2 KiB; its first KiB are the mark phase's flags, which are in registers before P is written), the mark
// phase's words (4 KiB), M (4 KiB).  Four wavefronts: 40 960 B, a quarter of a CU's 160 KiB to the byte -- which is why P has no
// entry 1024 (the total is a scalar) and the workgroup's merge at the end borrows wavefront 0's M.
constexpr u32 kMaskedP = 0, kMaskedWords = 2048, kMaskedM = 2048 + 4096, kMaskedWaveLds = 2048 + 4096 + 4096;

// P and the pad rule of a new image: M[g] = group g of the image (group_of_step(s, g) for g = 64 s + lane; m_is_new: M does not
// hold it yet), the bitmap's last group without its pad bits; P[g] = the set bits of the groups in front of g.  Returns their
// total.  (P goes over the mark phase's flags: they are in registers, or no longer needed, when this is called.)
template <class GroupOfStep>
__device__ __forceinline__ u32 image_prefix(u32 *M, unsigned short *P, bool m_is_new, bool last_seg, u32 nvalid, u32 pad_mask, u32 lane,
                                            GroupOfStep group_of_step) {
    const u32 pad_group = last_seg ? nvalid - 1u : 0xFFFFFFFFu;
    u32 run = 0;
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) {
        const u32 g = (u32)(64 * s) + lane;
        u32 grp = group_of_step(s, g);
        if (g == pad_group) grp &= pad_mask;
        if (m_is_new || g == pad_group) M[g] = grp;
        const u32 cnt = (u32)__builtin_popcount(grp);
        const u32 incl = wave_scan_incl32(cnt);
        P[g] = (unsigned short)(run + incl - cnt); // at most 31 744
        run += (u32)__builtin_amdgcn_readlane((int)incl, 63);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    return run;
}

// the bits an operand word of n groups at group lo shares with the mask image
__device__ __forceinline__ u32 image_bits(u32 x, u32 n, u32 lo, const u32 *M, const unsigned short *P, u32 p_total) {
    if (n == 0u) return 0u; // (no word here, or an empty fill: refused)
    if ((int)x >= 0) return (u32)__builtin_popcount(x & M[min(lo, kSegGroups - 1u)]);
    if ((x & kFillOne) != kFillOne) return 0u;
    // (a corrupt stream's positions may lie behind the segment: it is refused, and nothing is read out of bounds)
    const u32 hi = lo + n;
    const u32 p_hi = hi >= kSegGroups ? p_total : (u32)P[hi], p_lo = lo >= kSegGroups ? p_total : (u32)P[lo];
    return p_hi - p_lo;
}
// a segment's words counted against the image, where they lie (batch_places); grps: the segment's, in every lane
__device__ __forceinline__ SegCount count_against_image(const SegRange &rg, const u32 (&x0)[kSegBatches], const u32 (&x1)[kSegBatches], const u32 *M,
                                                        const unsigned short *P, u32 p_total, u32 lane) {
    u32 bits = 0, pos = 0; // pos: groups covered by the batches so far
    bool empty_word = false;
#pragma unroll
    for (int b = 0; b < kSegBatches; ++b) {
        if (128u * b < rg.cnt) { // wave-uniform
            const BatchPlaces p = batch_places(x0[b], x1[b], 128u * b, rg.cnt, pos, lane);
            empty_word |= p.empty;
            bits += image_bits(x0[b], p.n0, p.lo0, M, P, p_total) + image_bits(x1[b], p.n1, p.lo1, M, P, p_total);
        }
    }
    return {bits, pos, empty_word};
}

// The end of an operand's segment under the mask segment the wavefront holds (kind; M, P, p_total under kMaskImage): its words
// counted -- against the image, where they lie under a mask of ones, not at all under one of zeros -- and judged under EVERY
// kind, so that the verdict does not depend on the data; lane jj, which keeps the count of the chunk's jj-th operand, adds the bits.
__device__ __forceinline__ void count_under_mask(u32 kind, const SegRange &org, const u32 (&x0)[kSegBatches], const u32 (&x1)[kSegBatches], const u32 *M,
                                                 const unsigned short *P, u32 p_total, bool last_seg, u32 pad_bits, u32 pad_mask, u32 jj, u32 lane, u64 &acc,
                                                 bool &refused) {
    SegCount n;
    if (kind == kMaskImage) { // wave-uniform
        n = count_against_image(org, x0, x1, M, P, p_total, lane);
    } else {
        n = count_where_they_lie(org, x0, x1, kind == kMaskOnes, last_seg, pad_bits, pad_mask, lane);
        n.grps = wave_total32(n.grps);
    }
    const u32 total_bits = wave_total32(n.bits);
    const bool ok = kind != kMaskBad && segment_ok(org, n.grps, n.empty_word);
    refused |= !ok;
    if (lane == jj && ok) acc += (u64)total_bits;
}

// Where a wavefront stands in its run of (row, chunk, segment) items -- row: a mask, or a group; chunk c: `chunk` <= 64
// consecutive operands that share the row's image of the segment, served one after the other (jj) --, ordered (row, chunk,
// segment).  q = row * n_chunks + c names the counters the wavefront counts for: lane l's is operand c * chunk + l under the row.
struct ChunkBehind {
    u64 j0; // the chunk's first operand
    u32 jn; // and how many it has
    bool last_jj, last_seg, last_c;
    u64 q, seg, row, c; // of the item behind this one
};
struct ChunkCursor {
    u32 n_operands, chunk;
    u64 n_segments, n_chunks;
    u64 item, end;
    u64 q, seg, row, c;
    u32 jj;
    __device__ __forceinline__ bool more() const { return item + 1 < end; } // the run goes on behind this item
    // what comes behind this operand's segment: the chunk's next operand (!last_jj), or the next item
    __device__ __forceinline__ ChunkBehind behind() const {
        ChunkBehind b;
        b.j0 = c * chunk;
        b.jn = n_operands - b.j0 < chunk ? (u32)(n_operands - b.j0) : chunk;
        b.last_jj = jj + 1u == b.jn;
        b.last_seg = seg + 1 == n_segments;
        b.last_c = c + 1 == n_chunks;
        b.seg = b.last_seg ? 0ull : seg + 1;
        b.q = b.last_seg ? q + 1 : q;
        b.c = !b.last_seg ? c : b.last_c ? 0ull : c + 1;
        b.row = b.last_seg && b.last_c ? row + 1 : row;
        return b;
    }
    __device__ __forceinline__ void advance(const ChunkBehind &b) {
        if (!b.last_jj) {
            ++jj;
        } else {
            if (more()) {
                q = b.q;
                seg = b.seg;
                row = b.row;
                c = b.c;
            }
            ++item;
            jj = 0;
        }
    }
};
__device__ __forceinline__ ChunkCursor chunk_cursor(u32 n_rows, u32 n_operands, u32 chunk, u64 n_segments, u32 wave) {
    ChunkCursor at;
    at.n_operands = n_operands;
    at.chunk = chunk;
    at.n_segments = n_segments;
    at.n_chunks = ((u64)n_operands + chunk - 1) / chunk;
    const ItemRun run = item_run((u64)n_rows * at.n_chunks * n_segments, kSegDecodeWaves, wave);
    at.item = run.begin;
    at.end = run.end;
    at.q = run.begin / n_segments;
    at.seg = run.begin - at.q * n_segments;
    at.row = at.q / at.n_chunks;
    at.c = at.q - at.row * at.n_chunks;
    at.jj = 0;
    return at;
}

// What the workgroup's wavefronts hold for the counters their runs end in (q: ~0 for a wavefront without a run; acc: lane l's
// count; kRows: the row's own counter `rows` with racc beside it), merged and added: consecutive runs, so equal q are neighbours.
// One wave instruction adds a chunk's consecutive counts.  (Every image is done with: the merge borrows them.)
template <bool kRows>
__device__ __forceinline__ void merge_run_ends(unsigned char (*lds)[kMaskedWaveLds], u64 q, u64 acc, u64 racc, u64 n_chunks, u64 *counts, u64 *rows,
                                               u32 n_operands, u32 chunk, u32 wave, u32 lane) {
    __syncthreads();
    u64 *s_q = reinterpret_cast<u64 *>(lds[0] + kMaskedWords), *s_r = s_q + kSegDecodeWaves;
    reinterpret_cast<u64 *>(lds[wave] + kMaskedM)[lane] = acc;
    if (lane == 0) {
        s_q[wave] = q;
        if (kRows) s_r[wave] = racc;
    }
    __syncthreads();
    if (wave == 0) {
        u64 at = ~0ull, sum = 0, rsum = 0;
        for (int v = 0; v <= kSegDecodeWaves; ++v) {
            const u64 qv = v < kSegDecodeWaves ? s_q[v] : ~0ull;
            if (qv != at) { // wave-uniform
                if (at != ~0ull) {
                    const u64 mr = at / n_chunks, mc = at - mr * n_chunks;
                    if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(counts + mr * n_operands + mc * chunk + lane), (unsigned long long)sum);
                    if (kRows && lane == 0 && rsum) atomicAdd(reinterpret_cast<unsigned long long *>(rows + mr), (unsigned long long)rsum);
                }
                at = qv;
                sum = 0;
                rsum = 0;
            }
            if (v < kSegDecodeWaves) {
                sum += reinterpret_cast<const u64 *>(lds[v] + kMaskedM)[lane];
                if (kRows) rsum += s_r[v];
            }
        }
    }
}

// ---- counts under a mask -----------------------------------------------------------------------------------------------------
// counts[i * n_operands + j] += the set bits of mask i AND operand j; the cursor's row is the mask i.  The mask segment's image is
// made once per item and serves the chunk's operands.  (The first version took (mask, operand, segment) triples in the order (i, j,
// segment) and made the image anew for every operand: 3.5 - 5 us per triple and wavefront, nearly all of it the image: DESIGN
// 5.11.)  Consecutive items share the mask segment only in bitmaps of one segment; then the image is kept.  The next mask row and
// range are fetched with the next operand's, and P is made inside the steps that make M.
__global__ __launch_bounds__(kSegDecodeWaves * 64) void count_masked_kernel(const CountMaskedArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_lds[kSegDecodeWaves][kMaskedWaveLds];
    const u32 wave = wave_id(), lane = lane_id();
    unsigned char *flag = s_lds[wave] + kMaskedP;
    unsigned short *P = reinterpret_cast<unsigned short *>(s_lds[wave] + kMaskedP);
    u32 *words = reinterpret_cast<u32 *>(s_lds[wave] + kMaskedWords);
    u32 *M = reinterpret_cast<u32 *>(s_lds[wave] + kMaskedM);
    ChunkCursor at = chunk_cursor(a.n_masks, a.n_operands, a.chunk, a.n_segments, wave);
    const bool has_run = at.item < at.end;
    const u32 pad_mask = kOnes31 >> a.pad_bits;
    u64 acc = 0; // lane l: operand c * chunk + l under mask i
    bool refused = false;
    u32 kind = kMaskNone, p_total = 0;
    u64 img_i = 0, img_seg = 0;
    SelectRow mrow = {}, orow = {}, next_mrow = {}, next_orow = {};
    SegRange next_m = {}, next_o = {};
    if (has_run) {
        next_mrow = table_row(a.masks, at.row);
        next_orow = table_row(a.operands, at.c * a.chunk);
        next_m = select_range(next_mrow, a.groups, at.seg);
        next_o = select_range(next_orow, a.groups, at.seg);
    }
#pragma nounroll
    while (at.item < at.end) {
        const SegRange mrg = next_m, org = next_o;
        mrow = next_mrow;
        orow = next_orow;
        const bool fresh = at.jj == 0u && (kind == kMaskNone || at.row != img_i || at.seg != img_seg); // wave-uniform
        SegmentsArgs msa = {}, osa = {};
        msa.comp = reinterpret_cast<const u32 *>((uintptr_t)mrow.comp);
        osa.comp = reinterpret_cast<const u32 *>((uintptr_t)orow.comp);
        u32 m0[kSegBatches], m1[kSegBatches], x0[kSegBatches], x1[kSegBatches];
        if (fresh) seg_load_words(msa, mrg, m0, m1, lane);
        seg_load_words(osa, org, x0, x1, lane);
        const ChunkBehind nx = at.behind();
        if (!nx.last_jj) {
            next_orow = table_row(a.operands, nx.j0 + at.jj + 1u);
            next_o = select_range(next_orow, a.groups, at.seg);
        } else if (at.more()) {
            next_orow = table_row(a.operands, nx.c * a.chunk);
            if (nx.row != at.row) next_mrow = table_row(a.masks, nx.row);
            next_m = select_range(next_mrow, a.groups, nx.seg);
            next_o = select_range(next_orow, a.groups, nx.seg);
        }
        if (fresh) {
            img_i = at.row;
            img_seg = at.seg;
            const u32 first = (u32)__builtin_amdgcn_readfirstlane((int)m0[0]); // lane 0 holds the segment's first word
            if (!mrg.bad && mrg.cnt == 1u && (first & kFillZero) && (first & kCountMask) == mrg.nvalid) {
                kind = (first & kFillOne) == kFillOne ? kMaskOnes : kMaskZeros; // one fill over the segment: no image
            } else if (!seg_mark(mrg, m0, m1, flag, words, lane)) {
                kind = kMaskBad;
            } else {
                kind = kMaskImage;
                const uint4 fq = reinterpret_cast<const uint4 *>(flag)[lane];
                const u32 f[4] = {fq.x, fq.y, fq.z, fq.w};
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // P goes over the flags
                u32 before = 0xFFFFFFFFu;
                p_total = image_prefix(M, P, true, nx.last_seg, mrg.nvalid, pad_mask, lane,
                                       [&](int s, u32) { return seg_group(s, f, before, words, mrg.cnt, mrg.nvalid, lane); });
            }
        }
        count_under_mask(kind, org, x0, x1, M, P, p_total, nx.last_seg, a.pad_bits, pad_mask, at.jj, lane, acc, refused);
        if (nx.last_jj && nx.last_seg && at.more()) { // the run goes on with another chunk or mask
            if (acc) atomicAdd(reinterpret_cast<unsigned long long *>(a.counts + at.row * a.n_operands + nx.j0 + lane), (unsigned long long)acc);
            acc = 0;
        }
        at.advance(nx);
    }
    if (refused && lane == 0) atomicOr(a.ctrl + kCtlError, kErrStream);
    merge_run_ends<false>(s_lds, has_run ? at.q : ~0ull, acc, 0ull, at.n_chunks, a.counts, nullptr, a.n_operands, a.chunk, wave, lane);
}

// ---- grouped counts under a conjunction, and their sums ----------------------------------------------------------------------
// conjunct t of group g: the call's filter rows first, then the group's own rows
__device__ __forceinline__ SelectRow conjunct_row(const GroupCountArgs &a, u64 g, u32 t) {
    return t < a.n_filters ? table_row(a.filters, t) : table_row(a.keys, g * a.rows_per_group + (t - a.n_filters));
}

// counts[g * n_operands + j] += the set bits of (filter 0 AND .. AND filter F-1 AND group g's R rows) AND operand j, and rows[g] +=
// the set bits of that conjunction itself; the cursor's row is the group g.  The image is made once per item, conjunct by conjunct:
// seg_load_words, seg_mark and the sixteen steps of seg_group each, the first one STORING M[g], every later one ANDing into it; P
// -- which lies over the mark phase's flags and so cannot be written while a conjunct is still to be marked -- and the pad bits in
// one pass over M behind the last conjunct.  A conjunct whose segment is one one-fill changes nothing and is not decoded; one
// zero-fill makes the item's mask zeros, and the conjuncts behind it are judged where their words lie instead of being marked; if
// all are one-fills the operands are counted as under kMaskOnes.  EVERY segment of every filter row, group row and operand is
// loaded and checked under every short cut.  Only the items of chunk 0 add the conjunction's own bits (p_total; 31 per group under
// ones, less the pad bits; nothing under zeros): once per (g, segment).
__global__ __launch_bounds__(kSegDecodeWaves * 64) void group_count_kernel(const GroupCountArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_lds[kSegDecodeWaves][kMaskedWaveLds];
    const u32 wave = wave_id(), lane = lane_id();
    unsigned char *flag = s_lds[wave] + kMaskedP;
    unsigned short *P = reinterpret_cast<unsigned short *>(s_lds[wave] + kMaskedP);
    u32 *words = reinterpret_cast<u32 *>(s_lds[wave] + kMaskedWords);
    u32 *M = reinterpret_cast<u32 *>(s_lds[wave] + kMaskedM);
    const u32 n_conjuncts = a.n_filters + a.rows_per_group;
    ChunkCursor at = chunk_cursor(a.n_groups, a.n_operands, a.chunk, a.n_segments, wave);
    const bool has_run = at.item < at.end;
    const u32 pad_mask = kOnes31 >> a.pad_bits;
    u64 acc = 0;   // lane l: operand c * chunk + l under group g's conjunction
    u64 racc = 0;  // the conjunction's own bits (chunk 0 only), wave-uniform
    bool refused = false;
    u32 kind = kMaskNone, p_total = 0;
    u64 img_g = 0, img_seg = 0;
    SelectRow orow = {}, next_orow = {};
    SegRange next_o = {};
    if (has_run) {
        next_orow = table_row(a.operands, at.c * a.chunk);
        next_o = select_range(next_orow, a.groups, at.seg);
    }
#pragma nounroll
    while (at.item < at.end) {
        const SegRange org = next_o;
        orow = next_orow;
        const bool fresh = at.jj == 0u && (kind == kMaskNone || at.row != img_g || at.seg != img_seg); // wave-uniform
        SegmentsArgs osa = {};
        osa.comp = reinterpret_cast<const u32 *>((uintptr_t)orow.comp);
        u32 x0[kSegBatches], x1[kSegBatches];
        if (!fresh) seg_load_words(osa, org, x0, x1, lane); // (under a new image: behind its last conjunct, the registers are the conjuncts' till then)
        const ChunkBehind nx = at.behind();
        if (!nx.last_jj) {
            next_orow = table_row(a.operands, nx.j0 + at.jj + 1u);
            next_o = select_range(next_orow, a.groups, at.seg);
        } else if (at.more()) {
            next_orow = table_row(a.operands, nx.c * a.chunk);
            next_o = select_range(next_orow, a.groups, nx.seg);
        }
        if (fresh) {
            img_g = at.row;
            img_seg = at.seg;
            bool zeros = false, bad = false, image = false; // wave-uniform, all three
            SelectRow crow = conjunct_row(a, at.row, 0);
            SegRange next_c = select_range(crow, a.groups, at.seg);
#pragma nounroll
            for (u32 t = 0; t < n_conjuncts; ++t) {
                const SegRange crg = next_c;
                SegmentsArgs csa = {};
                csa.comp = reinterpret_cast<const u32 *>((uintptr_t)crow.comp);
                u32 m0[kSegBatches], m1[kSegBatches];
                seg_load_words(csa, crg, m0, m1, lane);
                if (t + 1u < n_conjuncts) { // the conjunct behind this one is on its way while this one is marked
                    crow = conjunct_row(a, at.row, t + 1u);
                    next_c = select_range(crow, a.groups, at.seg);
                }
                const u32 first = (u32)__builtin_amdgcn_readfirstlane((int)m0[0]); // lane 0 holds the segment's first word
                if (!crg.bad && crg.cnt == 1u && (first & kFillZero) && (first & kCountMask) == crg.nvalid) {
                    zeros |= (first & kFillOne) != kFillOne; // one fill over the segment: ones change nothing, zeros leave nothing
                } else if (zeros || bad) {
                    const SegCount n = count_where_they_lie(crg, m0, m1, false, false, 0u, 0u, lane); // no image will be read: judged, not decoded
                    bad |= !segment_ok(crg, wave_total32(n.grps), n.empty_word);
                } else if (!seg_mark(crg, m0, m1, flag, words, lane)) {
                    bad = true;
                } else {
                    const uint4 fq = reinterpret_cast<const uint4 *>(flag)[lane];
                    const u32 f[4] = {fq.x, fq.y, fq.z, fq.w};
                    u32 before = 0xFFFFFFFFu;
#pragma unroll
                    for (int s = 0; s < (int)kSteps; ++s) {
                        u32 grp = seg_group(s, f, before, words, crg.cnt, crg.nvalid, lane);
                        const u32 k = (u32)(64 * s) + lane; // (this lane's own entry, in every conjunct)
                        if (image) grp &= M[k];
                        M[k] = grp;
                    }
                    image = true;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the next conjunct is marked over these flags and words
                }
            }
            kind = bad ? kMaskBad : zeros ? kMaskZeros : image ? kMaskImage : kMaskOnes;
            seg_load_words(osa, org, x0, x1, lane);
            if (kind == kMaskImage) // no conjunct is left to be marked
                p_total = image_prefix(M, P, false, nx.last_seg, org.nvalid, pad_mask, lane, [&](int, u32 k) { return M[k]; });
        }
        count_under_mask(kind, org, x0, x1, M, P, p_total, nx.last_seg, a.pad_bits, pad_mask, at.jj, lane, acc, refused);
        // COUNT(*) of the group: the conjunction's own bits in this segment, once per (g, segment)
        if (at.jj == 0u && at.c == 0)
            racc += kind == kMaskImage ? (u64)p_total : kind == kMaskOnes ? (u64)(31u * org.nvalid - (nx.last_seg ? a.pad_bits : 0u)) : 0ull;
        if (nx.last_jj && nx.last_seg && at.more()) { // the run goes on with another chunk or group
            if (acc) atomicAdd(reinterpret_cast<unsigned long long *>(a.counts + at.row * a.n_operands + nx.j0 + lane), (unsigned long long)acc);
            if (lane == 0 && racc) atomicAdd(reinterpret_cast<unsigned long long *>(a.rows + at.row), (unsigned long long)racc);
            acc = 0;
            racc = 0;
        }
        at.advance(nx);
    }
    if (refused && lane == 0) atomicOr(a.ctrl + kCtlError, kErrStream);
    merge_run_ends<true>(s_lds, has_run ? at.q : ~0ull, acc, racc, at.n_chunks, a.counts, a.rows, a.n_operands, a.chunk, wave, lane);
}

// sums[g][t] = the counts of attribute t's slices under group g, slice i of bits[t] weighing 2^(bits[t] - 1 - i): one thread per
// (group, attribute).  A count is below 2^45 and an attribute has at most 64 slices: below 2^109, in 128 bits
constexpr u32 kFoldThreads = 256;
__global__ __launch_bounds__(kFoldThreads) void group_fold_kernel(const GroupFoldArgs a) {
    const u64 t = (u64)blockIdx.x * kFoldThreads + threadIdx.x;
    if (t >= (u64)a.n_groups * a.n_attrs) return;
    const u64 g = t / a.n_attrs;
    const u32 at = (u32)(t - g * a.n_attrs);
    u32 first = 0;
    for (u32 i = 0; i < at; ++i) first += a.bits[i];
    const u32 n_bits = a.bits[at];
    const u64 *counts = a.counts + g * a.n_operands + first;
    unsigned __int128 sum = 0;
    for (u32 i = 0; i < n_bits; ++i) sum += (unsigned __int128)counts[i] << (n_bits - 1u - i);
    a.sums[2 * t] = (u64)sum;
    a.sums[2 * t + 1] = (u64)(sum >> 64);
}

// ---- the rank scan -----------------------------------------------------------------------------------------------------------
constexpr u32 kRankThreads = 256;
constexpr u32 kRankPerThread = kRankChunk / kRankThreads; // 16

// out[b] = the sum of chunk b of in[0 .. n)
__global__ __launch_bounds__(kRankThreads) void rank_reduce_kernel(const u64 *in, u64 n, u64 *out) {
    __shared__ u64 s_wave[kRankThreads / 64];
    const u64 base = (u64)blockIdx.x * kRankChunk;
    u64 v = 0;
#pragma unroll 4
    for (u32 i = threadIdx.x; i < kRankChunk; i += kRankThreads)
        if (base + i < n) v += in[base + i];
    v = wave_sum(v);
    if (lane_id() == 0) s_wave[wave_id()] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
        for (u32 w = 0; w < kRankThreads / 64; ++w) t += s_wave[w];
        out[blockIdx.x] = t;
    }
}

// chunk b of v[0 .. n_out) becomes its exclusive prefix sum, on top of front[b] (null: of nothing); entries at and behind n_in
// are read as 0 -- the entry behind the last segment's receives the total
__global__ __launch_bounds__(kRankThreads) void rank_scan_kernel(u64 *v, u64 n_in, u64 n_out, const u64 *front) {
    __shared__ u64 s_wave[kRankThreads / 64];
    const u32 lane = lane_id(), wave = wave_id();
    const u64 t0 = (u64)blockIdx.x * kRankChunk + (u64)threadIdx.x * kRankPerThread;
    u64 x[kRankPerThread];
    u64 mine = 0;
#pragma unroll
    for (u32 i = 0; i < kRankPerThread; ++i) {
        x[i] = t0 + i < n_in ? v[t0 + i] : 0ull;
        mine += x[i];
    }
    const u64 incl = wave_scan_incl(mine, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    u64 run = front ? front[blockIdx.x] : 0ull;
    for (u32 w = 0; w < wave; ++w) run += s_wave[w];
    run += incl - mine;
#pragma unroll
    for (u32 i = 0; i < kRankPerThread; ++i) {
        if (t0 + i < n_out) v[t0 + i] = run;
        run += x[i];
    }
}

// ---- the positions -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSegDecodeWaves * 64) void select_emit_kernel(const SelectEmitArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_flag[kSegDecodeWaves][kSegGroups];
    __shared__ __attribute__((aligned(16))) u32 s_seg[kSegDecodeWaves][kSegGroups];
    __shared__ __attribute__((aligned(16))) unsigned short s_stage[kSegDecodeWaves][kSelectStageSlots];
    const u32 wave = wave_id(), lane = lane_id();
    const u64 k = (u64)blockIdx.x * kSegDecodeWaves + wave;
    // the count pass is complete: its verdict on every segment is in.  A refused stream lists nothing.
    const u32 err = uniform32(__hip_atomic_load(a.g.ctrl + kCtlError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (k == 0 && lane == 0) {
        const u64 total = err ? 0ull : a.ranks[a.g.n_segments];
        const u64 left = total > a.first ? total - a.first : 0ull;
        a.info[0] = total;
        a.info[1] = left < a.capacity ? left : a.capacity;
    }
    if (err || k >= a.g.n_segments) return;
    const u64 seg = k;
    typedef const __attribute__((address_space(4))) u64 *const_u64_ptr;
    const const_u64_ptr ranks = (const_u64_ptr)(uintptr_t)(a.ranks + seg);
    const u64 r0 = ranks[0], r1 = ranks[1];
    if (r1 <= a.first || r0 >= a.end || r0 == r1) return;

    const const_u64_ptr offs = (const_u64_ptr)(uintptr_t)(a.g.seg_offsets + seg);
    const SegRange rg = seg_range(a.g, seg, offs[0], offs[1]);
    u32 x0[kSegBatches], x1[kSegBatches];
    seg_load_words(a.g, rg, x0, x1, lane);
    unsigned char *flag = s_flag[wave];
    u32 *words = s_seg[wave];
    unsigned short *stage = s_stage[wave];
    if (!seg_mark(rg, x0, x1, flag, words, lane)) { // (the count pass accepted it: only a stream that changes under the call)
        if (lane == 0) atomicOr(a.g.ctrl + kCtlError, kErrStream);
        return;
    }
    const uint4 fq = reinterpret_cast<const uint4 *>(flag)[lane];
    const u32 f[4] = {fq.x, fq.y, fq.z, fq.w};
    u32 before = 0xFFFFFFFFu;
    // the bitmap's last group loses its pad bits
    const u32 pad_group = seg + 1 == a.g.n_segments ? rg.nvalid - 1u : 0xFFFFFFFFu;
    const u64 base_pos = seg * (u64)kSegBits;
    u64 run = r0; // the rank of the step's first set bit
#pragma unroll
    for (int s = 0; s < (int)kSteps; ++s) {
        u32 grp = seg_group(s, f, before, words, rg.cnt, rg.nvalid, lane);
        const u32 g = (u32)(64 * s) + lane;
        if (g == pad_group) grp &= kOnes31 >> a.pad_bits;
        const u32 c = (u32)__builtin_popcount(grp);
        const u32 incl = wave_scan_incl32(c);
        const u32 tot = (u32)__builtin_amdgcn_readlane((int)incl, 63);
        if (tot != 0u && run + tot > a.first && run < a.end) { // wave-uniform
            u32 o = incl - c;
            const u32 p0 = g * 31u;
            while (grp) {
                stage[o++] = (unsigned short)(p0 + (u32)__builtin_ctz(grp));
                grp &= grp - 1u;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (u32 i = lane; i < tot; i += 64u) {
                const u64 rank = run + i;
                if (rank >= a.first && rank < a.end) a.out[rank - a.first] = base_pos + stage[i];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the next step stages over these slots
        }
        run += tot;
    }
}

} // namespace

// how many workgroups a count launch gets: what the chip holds at once (every wavefront takes one contiguous run), no more
static unsigned select_count_grid(u64 n_items) {
    const u64 want = (n_items + kSegDecodeWaves - 1) / kSegDecodeWaves;
    constexpr u64 most = 256u * 8u; // CUs x resident workgroups of four wavefronts at eight waves per SIMD
    return (unsigned)(want < 1 ? 1 : want > most ? most : want);
}

hipError_t launch_select_count(const SelectCountArgs &a, hipStream_t s) {
    if (a.n_segments == 0) return hipSuccess;
    if (a.table) {
        hipLaunchKernelGGL(select_count_kernel<true>, dim3(select_count_grid((u64)a.n_operands * a.n_segments)), dim3(kSegDecodeWaves * 64), 0, s, a);
    } else {
        hipLaunchKernelGGL(select_count_kernel<false>, dim3(select_count_grid(a.n_segments)), dim3(kSegDecodeWaves * 64), 0, s, a);
    }
    return hipGetLastError();
}

// ... of the two chunked kernels (rows: masks, or groups): their 40 960 B of LDS let four workgroups onto a CU.  The chunk: as many
// operands per image as leave every wavefront of a full grid eight items or more, 64 at the most
struct ChunkedGrid {
    u32 chunk;
    unsigned workgroups;
};
static ChunkedGrid chunked_count_grid(u64 rows, u64 operands, u64 segments) {
    constexpr u64 most = 256u * 4u;
    u64 chunk = 64;
    auto items = [&](u64 by) { return rows * ((operands + by - 1) / by) * segments; };
    while (chunk > 1 && items(chunk) < 8 * most * kSegDecodeWaves) chunk /= 2;
    const u64 want = (items(chunk) + kSegDecodeWaves - 1) / kSegDecodeWaves;
    return {(u32)chunk, (unsigned)(want > most ? most : want)};
}

hipError_t launch_count_masked(const CountMaskedArgs &a, hipStream_t s) {
    if (a.n_segments == 0) return hipSuccess;
    const ChunkedGrid g = chunked_count_grid(a.n_masks, a.n_operands, a.n_segments);
    CountMaskedArgs b = a;
    b.chunk = g.chunk;
    hipLaunchKernelGGL(count_masked_kernel, dim3(g.workgroups), dim3(kSegDecodeWaves * 64), 0, s, b);
    return hipGetLastError();
}

// ... of the grouped count, then the fold on the same stream (it runs for an empty bitmap too: every sum is stored)
hipError_t launch_group_sum(const GroupCountArgs &a, const GroupFoldArgs &f, hipStream_t s) {
    if (a.n_segments != 0) {
        const ChunkedGrid g = chunked_count_grid(a.n_groups, a.n_operands, a.n_segments);
        GroupCountArgs b = a;
        b.chunk = g.chunk;
        hipLaunchKernelGGL(group_count_kernel, dim3(g.workgroups), dim3(kSegDecodeWaves * 64), 0, s, b);
    }
    const u64 n_sums = (u64)f.n_groups * f.n_attrs;
    hipLaunchKernelGGL(group_fold_kernel, dim3((unsigned)((n_sums + kFoldThreads - 1) / kFoldThreads)), dim3(kFoldThreads), 0, s, f);
    return hipGetLastError();
}

// ranks[0 .. n_segments] <- exclusive prefix sum of ranks[0 .. n_segments) (the last entry: the total); level1 / level2: room
// for one entry per chunk of the level below (select_rank_levels)
hipError_t launch_select_rank_scan(u64 *ranks, u64 n_segments, u64 *level1, u64 *level2, hipStream_t s) {
    const u64 n0 = n_segments + 1;
    const u64 n1 = (n0 + kRankChunk - 1) / kRankChunk, n2 = (n1 + kRankChunk - 1) / kRankChunk;
    if (n2 > kRankChunk) return hipErrorInvalidValue; // (more than 2^36 segments: no bitmap of fewer than 2^40 words has them)
    if (n1 > 1) {
        hipLaunchKernelGGL(rank_reduce_kernel, dim3((unsigned)n1), dim3(kRankThreads), 0, s, ranks, n_segments, level1);
        if (n2 > 1) {
            hipLaunchKernelGGL(rank_reduce_kernel, dim3((unsigned)n2), dim3(kRankThreads), 0, s, level1, n1, level2);
            hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(kRankThreads), 0, s, level2, n2, n2, (const u64 *)nullptr);
        }
        hipLaunchKernelGGL(rank_scan_kernel, dim3((unsigned)n2), dim3(kRankThreads), 0, s, level1, n1, n1, n2 > 1 ? (const u64 *)level2 : (const u64 *)nullptr);
    }
    hipLaunchKernelGGL(rank_scan_kernel, dim3((unsigned)n1), dim3(kRankThreads), 0, s, ranks, n_segments, n0, n1 > 1 ? (const u64 *)level1 : (const u64 *)nullptr);
    return hipGetLastError();
}

hipError_t launch_select_emit(const SelectEmitArgs &a, hipStream_t s) {
    const u64 grid = a.g.n_segments ? (a.g.n_segments + kSegDecodeWaves - 1) / kSegDecodeWaves : 1; // (no segment: one workgroup writes the two totals)
    hipLaunchKernelGGL(select_emit_kernel, dim3((unsigned)grid), dim3(kSegDecodeWaves * 64), 0, s, a);
    return hipGetLastError();
}

} // namespace wah
