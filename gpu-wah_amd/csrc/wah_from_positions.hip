// wah_from_positions.hip -- compressed bitmaps straight from sorted lists of row numbers (wah_from_positions_device): the way
// into the index that does not go through a decoded bitmap.  Any number of lists in one call; for every list the words that
// compress() emits for the bitmap of n_words words that has exactly those bits set, all streams back to back, and beside them
// the segment index of the whole (n_lists x S + 1 entries), which is what every indexed call reads.  The reference has no
// counterpart: its compress() takes the decoded bitmap (compress.cu:41-209).
//
// Three kinds of launches, and no workgroup of any of them waits for another:
//   from_positions_check_kernel  a grid-stride pass over the ends and the rows.  An end is refused when it is smaller than the
//                         one before it, larger than n_rows, or the last one and not n_rows; a row when it is at or behind
//                         32 n_words; a descent rows[i - 1] >= rows[i] when i is not an entry of the ends (a binary search
//                         of the ends: a valid call has fewer descents than lists).  Every end and every row is looked at.
//   from_positions_kernel<false>  (list, segment) items shared out over the launch's wavefronts in contiguous runs, as
//                         select_count_kernel shares its pairs out.  A wavefront finds the item's slice of the list by two
//                         64-way searches for the segment's bit range [31744 s, 31744 (s + 1)) -- the first one is the slice
//                         end the item before it found, the list's own ends bound segment 0 and the last segment -- and
//                         counts the words of the segment by one of three routes:
//                           no row          one zero-fill of the segment's groups; no LDS, no load
//                           1 .. 64 rows    in registers: lane l holds row l, a ballot of "another group than my left
//                                           neighbour" gives the group heads, a segmented OR scan over the lanes of a group its
//                                           31 bits; the last lane of every group speaks for it: a zero-fill for the gap in
//                                           front of it (if any), then a literal, or a one-fill that swallows the all-ones group
//                                           that touches it on the left (31 + 31 rows: at most two fit), and one zero-fill
//                                           behind the last group
//                           more rows       ds_or of every row's bit into an image of the segment's 1024 groups in LDS, then
//                                           64 groups per step: zero / all ones / literal per lane, the last lane of every
//                                           run emits its word (ballots give its place, the run's length comes from the
//                                           nearest break on the left and, across a step's edge, from a carried length)
//                         and stores the count at offsets[list * S + segment].
//   (launch_select_rank_scan turns the counts into the index in place.)
//   from_positions_kernel<true>  the same items, the same classification -- the rows of a segment are a few hundred bytes where a
//                         temporary stream per segment would be written and read again --; the words go into an LDS staging area
//                         of the wavefront and leave it 64 consecutive words per store instruction, clipped by the capacity.
// What the check pass refuses is not trusted by the other two: ends are clamped to n_rows and to each other before they bound
// a read of the rows, a row's place in its segment is clamped to the segment, a segment's words are clipped to the room the
// count pass gave it, and every store to the output is compared with the capacity.
#include "wah_count_emit.hpp"

namespace wah {
namespace {

typedef const __attribute__((address_space(4))) u64 *FpConstU64;

constexpr u32 kFpWaves = 4;

__global__ __launch_bounds__(256) void from_positions_check_kernel(const FromPositionsArgs a) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    for (u64 j = t; j < a.n_lists; j += stride) {
        const u64 e = a.list_ends[j], before = j ? a.list_ends[j - 1] : 0ull;
        bad |= e < before || e > a.n_rows || (j + 1 == a.n_lists && e != a.n_rows);
    }
    for (u64 i = t; i < a.n_rows; i += stride) {
        const u64 r = a.rows[i];
        bad |= r >= a.n_bits;
        if (i && a.rows[i - 1] >= r) {
            // legal only where a list ends: the first end that is not below i must be i
            u64 lo = 0, hi = a.n_lists;
            while (lo < hi) {
                const u64 mid = lo + (hi - lo) / 2;
                if (a.list_ends[mid] < i) lo = mid + 1; else hi = mid;
            }
            bad |= lo == a.n_lists || a.list_ends[lo] != i;
        }
    }
    if (__ballot(bad) != 0ull && lane_id() == 0) atomicOr(a.ctrl + kCtlError, kErrStream);
}

// the first index in [b, e) whose row is not below key (e if none), by the whole wavefront: 64 probes per round.  Wave-uniform
// in, wave-uniform out; on rows that do not ascend it returns some index in [b, e]
__device__ __forceinline__ u64 fp_lower_bound(const u64 *rows, u64 b, u64 e, u64 key, u32 lane) {
    while (e - b > 64) {
        const u64 len = e - b, step = (len + 63) / 64;
        const u64 behind = (u64)(lane + 1u) * step; // one past chunk `lane`
        const u64 probe = b + (behind < len ? behind : len) - 1;
        const u32 k = (u32)__popcll(__ballot(rows[probe] < key)); // chunks whose last row is below the key
        if (k == 64u) return e;
        const u64 nb = b + k * step, ne = nb + step;
        b = nb < e ? nb : e;
        e = ne < e ? ne : e;
    }
    const bool below = lane < e - b && rows[b + lane] < key;
    return b + (u64)__popcll(__ballot(below));
}

template <bool kEmit>
__global__ __launch_bounds__(kFpWaves * 64) void from_positions_kernel(const FromPositionsArgs a) {
    __shared__ __attribute__((aligned(16))) u32 s_img[kFpWaves][kSegGroups];
    __shared__ __attribute__((aligned(16))) u32 s_stage[kEmit ? kFpWaves : 1][kSegGroups];
    const u32 wave = wave_id(), lane = lane_id();
    u32 *img = s_img[wave];
    u32 *stage = s_stage[kEmit ? wave : 0];
    const u64 n_items = a.n_lists * a.n_segments;
    const ItemRun run = item_run(n_items, kFpWaves, wave);
    const u64 begin = run.begin, end = run.end;
    const FpConstU64 ends = (FpConstU64)(uintptr_t)a.list_ends;
    const FpConstU64 offs = (FpConstU64)(uintptr_t)a.offsets;
    emit_total<kEmit>(a, offs, n_items, run, lane);
    u64 c = begin / a.n_segments;
    u64 seg = begin - c * a.n_segments;
    u64 lb = 0, le = 0, slice_end = 0; // the list's rows; where the segment before this one ended in them
    bool have_list = false;
#pragma nounroll
    for (u64 item = begin; item < end; ++item) {
        if (!have_list) {
            // an end is clamped before it bounds a read (the check pass refuses what is clamped here)
            const u64 e0 = c ? ends[c - 1] : 0ull, e1 = ends[c];
            lb = e0 < a.n_rows ? e0 : a.n_rows;
            le = e1 < a.n_rows ? e1 : a.n_rows;
            le = le < lb ? lb : le;
            have_list = true;
        }
        const u64 base = seg * (u64)kSegBits;
        const bool last = seg + 1 == a.n_segments;
        const u32 ngroups = last ? (u32)(a.groups - seg * kSegGroups) : kSegGroups;
        const u64 lo = seg == 0 ? lb : item == begin ? fp_lower_bound(a.rows, lb, le, base, lane) : slice_end;
        const u64 hi = last ? le : fp_lower_bound(a.rows, lo, le, base + kSegBits, lane);
        slice_end = hi;
        const u64 n = hi - lo;
        u32 total;
        if (n == 0) {
            total = lone_zero_fill<kEmit>(ngroups, stage, lane);
        } else if (n <= 64) {
            // ---- in registers: lane l holds row l ----
            const u32 cnt = (u32)n;
            const bool act = lane < cnt;
            const u64 row = act ? a.rows[lo + lane] : 0ull;
            const u64 rel = row - base;
            const u32 p = rel < (u64)ngroups * 31u ? (u32)rel : ngroups * 31u - 1u; // (a refused row: clamped into the segment)
            const u32 g = p / 31u, bit = p - 31u * g;
            const u32 g_left = (u32)__shfl_up((int)g, 1);
            const u64 heads = __ballot(act && (lane == 0 || g != g_left));
            const u64 tails = ((heads >> 1) | (1ull << (cnt - 1u))) & (cnt == 64u ? ~0ull : lanes_below(cnt));
            const u32 headpos = 63u - (u32)__builtin_clzll((heads | 1ull) & (~0ull >> (63u - lane)));
            u32 v = 1u << bit;
#pragma unroll
            for (u32 off = 1; off < 64u; off <<= 1) {
                const u32 t = (u32)__shfl_up((int)v, (int)off);
                if (lane >= off && lane - off >= headpos) v |= t;
            }
            const bool tail = (tails >> lane) & 1ull;
            const bool ones = v == kOnes31;
            // the group on my group's left: its last lane is the one in front of my group's head
            const u32 left = (headpos - 1u) & 63u;
            const u32 left_g = (u32)__shfl((int)g, (int)left);
            const bool left_ones = __shfl((int)ones, (int)left) != 0;
            const u32 gap = headpos ? g - left_g - 1u : g;
            const bool joins = tail && ones && headpos && left_ones && gap == 0u; // one fill with the all-ones group on the left
            const u64 joiners = __ballot(joins);
            // an all-ones group whose right neighbour joins it leaves the word to that one
            const u64 tails_right = lane == 63u ? 0ull : tails >> (lane + 1u);
            const u32 right = tails_right ? lane + 1u + (u32)__builtin_ctzll(tails_right) : 63u;
            const bool joined = tails_right && ((joiners >> right) & 1ull);
            const bool gap_word = tail && gap != 0u;
            const bool own_word = tail && !(ones && joined);
            const u32 nw = (gap_word ? 1u : 0u) + (own_word ? 1u : 0u);
            const u32 incl = wave_scan_incl32(nw);
            const u32 g_last = (u32)__builtin_amdgcn_readlane((int)g, (int)(cnt - 1u));
            const u32 behind = ngroups - 1u - g_last;
            total = (u32)__builtin_amdgcn_readlane((int)incl, 63) + (behind ? 1u : 0u);
            if (kEmit) {
                u32 at = incl - nw;
                if (gap_word) stage[at++] = fill_word(kTypeZero, gap);
                if (own_word) stage[at] = ones ? fill_word(kTypeOnes, joins ? 2u : 1u) : v;
                if (behind && lane == 0) stage[total - 1u] = fill_word(kTypeZero, behind);
            }
        } else {
            // ---- through an image of the segment's groups in LDS ----
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (u32 k = 0; k < kSegGroups / 256u; ++k) reinterpret_cast<uint4 *>(img)[64u * k + lane] = make_uint4(0u, 0u, 0u, 0u);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (u64 i = lo + lane; i < hi; i += 64u) {
                const u64 rel = a.rows[i] - base;
                const u32 p = rel < (u64)ngroups * 31u ? (u32)rel : ngroups * 31u - 1u;
                const u32 g = p / 31u;
                atomicOr(img + g, 1u << (p - 31u * g));
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            total = image_words<kEmit>(img, ngroups, stage, lane); // (wah_image_words.hpp)
        }
        item_tail<kEmit>(a, offs, item, total, stage, lane);
        if (last) {
            ++c;
            seg = 0;
            have_list = false;
        } else {
            ++seg;
        }
    }
}

} // namespace

hipError_t launch_from_positions_check(const FromPositionsArgs &a, hipStream_t s) {
    const u64 n = a.n_rows > a.n_lists ? a.n_rows : a.n_lists;
    const u64 want = (n + 255) / 256;
    constexpr u64 most = 256u * 8u;
    hipLaunchKernelGGL(from_positions_check_kernel, dim3((unsigned)(want > most ? most : want)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// count pass (emit = false: every item's words to a.offsets) or emit pass (a.offsets scanned: the words to their place)
hipError_t launch_from_positions_segments(const FromPositionsArgs &a, bool emit, hipStream_t s) {
    constexpr u64 most = 256u * 8u; // CUs x resident workgroups of four wavefronts at eight waves per SIMD
    return launch_count_or_emit(from_positions_kernel<false>, from_positions_kernel<true>, emit, a.n_lists * a.n_segments, kFpWaves, most, a, s);
}

} // namespace wah
