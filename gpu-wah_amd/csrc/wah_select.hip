// wah_select.hip -- what a query wants from a result bitmap, without decoding it: how many bits it has set
// (wah_count_list_indexed_device: one count per operand of a table -- COUNT(*), or the GROUP BY histogram of an
// equality-encoded attribute) and which ones (wah_positions_indexed_device: the positions of the set bits of a window of ranks,
// in ascending order -- SELECT rowid ... LIMIT / OFFSET).  The reference has no counterpart.
//
// Three kinds of launches, and no workgroup of any of them waits for another:
//   select_count_kernel   (operand, segment) pairs shared out over the launch's wavefronts in contiguous runs.  The table row is checked before its index pointer
//                         is followed, the index range (seg_range) before the stream is read through it; the segment's words
//                         are loaded two per lane per batch of 128 (seg_load_words) and counted where they lie -- a literal is
//                         its popcount, a one-fill 31 bits per group, a zero-fill nothing: no group is ever decoded.  The
//                         words' groups are summed beside the bits, and a segment whose words do not make up exactly its
//                         groups, or that holds an empty fill, is refused (kErrStream) and counts nothing.  A wavefront sums
//                         its run and adds into the operand's count with a 64-bit vector atomic when the operand changes, a
//                         workgroup merges its four runs' ends first; the positions call stores every segment's count into its
//                         rank table instead.  The cost goes with the operands' words.
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

// kTable: one count per table row, added up over its segments; otherwise the one operand `one`, one count per segment.
// The (operand, segment) pairs are shared out in CONTIGUOUS runs, one per wavefront: a wavefront adds its segments' counts up
// and issues one atomic when the operand changes, and what the four wavefronts of a workgroup hold at their ends is merged in
// LDS first -- an atomic per segment would be 270 000 of them on ONE address for a 1 GiB operand, 11.6 ns each (3.2 ms, measured;
// the words themselves take a tenth of that).  While a segment's words are counted the next segment's index pair is on its way.
template <bool kTable>
__global__ __launch_bounds__(kSegDecodeWaves * 64, 8) void select_count_kernel(const SelectCountArgs a) {
    __shared__ u64 s_j[kSegDecodeWaves], s_acc[kSegDecodeWaves];
    const u32 wave = wave_id(), lane = lane_id();
    const u64 n_items = kTable ? (u64)a.n_operands * a.n_segments : a.n_segments;
    const u64 n_waves = (u64)gridDim.x * kSegDecodeWaves;
    const u64 per = (n_items + n_waves - 1) / n_waves;
    const u64 w = (u64)blockIdx.x * kSegDecodeWaves + wave;
    const u64 begin = w * per < n_items ? w * per : n_items, end = begin + per < n_items ? begin + per : n_items;
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
        // the bitmap's last word (the last word of its last segment) loses the pad bits
        const u32 last = last_of_operand ? rg.cnt - 1u : 0xFFFFFFFFu;
        u32 bits = 0, grps = 0;
        bool empty_word = false;
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
                    const u32 pad = i == last ? a.pad_bits : 0u;
                    const u32 fill_bits = ones && n ? 31u * n - pad : 0u;
                    bits += !in ? 0u : lit ? (u32)__builtin_popcount(x & (i == last ? pad_mask : kOnes31)) : fill_bits;
                    grps += n;
                }
            }
        }
        const u32 total_grps = wave_total32(grps), total_bits = wave_total32(bits);
        const bool ok = !rg.bad && total_grps == rg.nvalid && __ballot(empty_word) == 0ull;
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
    const u64 base_pos = seg * (u64)(kSegGroups * 31u);
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
