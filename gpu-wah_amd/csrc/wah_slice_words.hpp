// wah_slice_words.hpp -- the bit transpose of the kernels that hold a block of values in registers and write slice words
// (bsi_slices_kernel of wah_bsi_build.hip, bsi_map_segments_kernel of wah_map.hip): lane l of step t owns row 64 t + l of the
// block, the ballot of "my value has this bit" is words 2t and 2t + 1 of the slice, and v_writelane puts them into lanes 2t and
// 2t + 1 of ONE accumulator -- after the steps lane j holds word j, and one store instruction writes the block's words of the
// slice's row.  Written once for both.
#ifndef WAH_SLICE_WORDS_HPP_
#define WAH_SLICE_WORDS_HPP_
#include "wah_device.hpp"

// v_writelane_b32: `into` with lane `lane` replaced by the wave-uniform `value`.  This compiler has no builtin of that name, so
// the LLVM intrinsic is named directly: the compiler still knows what it does and schedules around it.
extern "C" __device__ int wah_writelane(int value, int lane, int into) __asm("llvm.amdgcn.writelane.i32");

namespace wah {
namespace {

__device__ __forceinline__ u32 put_lane(u32 value, u32 lane, u32 into) { return (u32)wah_writelane((int)value, (int)lane, (int)into); }

// lane j: word j of the block's bitmap of "half & mask is not zero", half[t] of lane l belonging to row 64 t + l (a block cut
// short has fewer steps: the lanes at and behind 2 kSteps hold zeros)
template <u32 kSteps>
__device__ __forceinline__ u32 slice_words(const u32 (&half)[kSteps], u32 mask) {
    u32 acc = 0u;
#pragma unroll
    for (u32 t = 0; t < kSteps; ++t) {
        const u64 m = __ballot((half[t] & mask) != 0u);
        acc = put_lane((u32)m, 2u * t, acc);
        acc = put_lane((u32)(m >> 32), 2u * t + 1u, acc);
    }
    return acc;
}

} // namespace
} // namespace wah
#endif // WAH_SLICE_WORDS_HPP_
