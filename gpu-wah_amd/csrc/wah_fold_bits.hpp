// wah_fold_bits.hpp -- the fold of the kernels that keep one word per ROW of a segment in LDS (values_items_kernel of
// wah_values.hip, member_items_kernel of wah_member.hip): the table row a wavefront's image holds -- one slice of a bit-sliced
// attribute -- ORed into the rows' words at one bit.  Written once for both.
#ifndef WAH_FOLD_BITS_HPP_
#define WAH_FOLD_BITS_HPP_
#include "wah_list_walk.hpp"

namespace wah {
namespace {

// Blocks k_lo .. k_lo + k_n - 1 of 64 groups of the image `acc`; row p of them (bit p % 31 of their group p / 31) is rows[p],
// and gets bit `sig` where the image has the row's bit.  A lane takes group 64 k + lane and the bit number runs wave-uniform
// from 0 to 30, so the 64 lanes of one LDS `or` are the rows 31 (64 k + lane) + b: 31 is odd, so they lie on different banks
// (one per lane of a 32-lane half).  A block of 64 groups that is all zero is skipped.  Several wavefronts fold at once into
// the same words, at other bits: LDS atomics.
__device__ __forceinline__ void fold_slice_bits(const u32 *acc, u32 *rows, u32 k_lo, u32 k_n, u32 sig, u32 lane) {
#pragma nounroll
    for (u32 k = 0; k < k_n; ++k) {
        const u32 w = acc[64u * (k_lo + k) + lane];
        if (__ballot(w != 0u) == 0ull) continue;
        u32 *row = rows + 31u * (64u * k + lane);
        // (every lane ORs, a zero where its bit is clear: two instructions a bit and no branch on the lanes)
#pragma unroll
        for (u32 b = 0; b < 31u; ++b)
            __hip_atomic_fetch_or(row + b, ((w >> b) & 1u) << sig, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

} // namespace
} // namespace wah
#endif // WAH_FOLD_BITS_HPP_
