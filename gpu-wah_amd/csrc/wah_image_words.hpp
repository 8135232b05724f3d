// wah_image_words.hpp -- an image of one segment's 31-bit groups in LDS turned into the words compress() emits for them, by one
// wavefront.  Written once for the kernels that build a segment as such an image: from_positions_kernel
// (wah_from_positions.hip: the rows of a list ORed into it), splice_segments_kernel (wah_splice.hip: bits of source
// segments moved into it), compact_segments_kernel (wah_compact.hip: the bits a mask selects deposited into it) and
// update_segments_kernel (wah_update.hip: two sources blended in it under a mask).  The frame those four kernels put around it is
// wah_count_emit.hpp.
#ifndef WAH_IMAGE_WORDS_HPP_
#define WAH_IMAGE_WORDS_HPP_
#include "wah_device.hpp"

namespace wah {

constexpr u32 kTypeZero = 0, kTypeOnes = 1, kTypeLit = 2, kTypeNone = 3;

__device__ __forceinline__ u32 group_type(u32 v) { return v == 0u ? kTypeZero : v == kOnes31 ? kTypeOnes : kTypeLit; }
__device__ __forceinline__ u32 fill_word(u32 type, u32 count) { return kFillZero | (type == kTypeOnes ? 0x40000000u : 0u) | count; }
__device__ __forceinline__ u64 lanes_below(u32 lane) { return (1ull << lane) - 1ull; }

// The words of the first ngroups (1 .. 1024) groups of img, counted (the return value, wave-uniform) and, with kEmit, written to
// stage[0 ..) in order.  64 groups per step: zero / all ones / literal per lane, the last lane of every run emits its word
// (ballots give its place, the run's length comes from the nearest break on the left and, across a step's edge, from a carried
// length).  The caller fences between its last write to img and this, and behind this before stage is read by other lanes.
template <bool kEmit>
__device__ __forceinline__ u32 image_words(const u32 *img, u32 ngroups, u32 *stage, u32 lane) {
    const u32 n_steps = (ngroups + 63u) / 64u;
    u32 run = 0, carry_type = kTypeNone, carry_len = 0;
#pragma nounroll
    for (u32 s = 0; s < n_steps; ++s) {
        const u32 g = 64u * s + lane;
        const bool valid = g < ngroups;
        const u32 v = valid ? img[g] : 0u;
        const u32 t = valid ? group_type(v) : kTypeNone;
        u32 t_left = (u32)__shfl_up((int)t, 1), t_right = (u32)__shfl_down((int)t, 1);
        if (lane == 0) t_left = carry_type;
        if (lane == 63u) t_right = g + 1u < ngroups ? group_type(img[g + 1u]) : kTypeNone;
        const bool brk = valid && (t == kTypeLit || t != t_left);   // a word begins here
        const bool tail = valid && (t == kTypeLit || t != t_right); // ... and ends here
        const u64 brks = __ballot(brk), tls = __ballot(tail);
        const u32 headpos = 63u - (u32)__builtin_clzll((brks | 1ull) & (~0ull >> (63u - lane)));
        const u32 len = lane - headpos + 1u + (headpos == 0u && !(brks & 1ull) ? carry_len : 0u);
        if (kEmit && tail) stage[run + (u32)__popcll(tls & lanes_below(lane))] = t == kTypeLit ? v : fill_word(t, len);
        run += (u32)__popcll(tls);
        // the run that lane 63 is in goes on in the next step
        const bool open = (__ballot(valid && !tail) >> 63) & 1ull;
        carry_type = open ? (u32)__builtin_amdgcn_readlane((int)t, 63) : kTypeNone;
        carry_len = open ? (u32)__builtin_amdgcn_readlane((int)len, 63) : 0u;
    }
    return run;
}

} // namespace wah
#endif // WAH_IMAGE_WORDS_HPP_
