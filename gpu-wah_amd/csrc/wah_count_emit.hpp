// wah_count_emit.hpp -- the device half of count_scan_emit (wah_api.hip): the frame of a kernel that builds compress() streams
// item by item, one wavefront per item, in two passes over the same items -- the count pass leaves every item's words in
// offsets[item], launch_select_rank_scan turns the counts into the index in place, the emit pass writes every item's words where
// the index says.  Written once for from_positions_kernel (wah_from_positions.hip), splice_segments_kernel (wah_splice.hip),
// compact_segments_kernel (wah_compact.hip) and update_segments_kernel (wah_update.hip):
//   item_run        the share-out of the items over the launch's wavefronts (wah_device.hpp: the counting kernels of
//                   wah_select.hip share their items out the same way)
//   emit_total      the emit pass's one lane that reports the total and judges the capacity
//   lone_zero_fill  the item that holds no set bit
//   item_tail       what ends every item: its count stored, or its staged words clipped and stored
//   launch_count_or_emit  the launcher of either pass
// A kernel keeps its own loop over its run and its own body.  The frame is templated on the kernel's args and reads out,
// out_capacity, out_words, offsets and ctrl of them, under these names.
#ifndef WAH_COUNT_EMIT_HPP_
#define WAH_COUNT_EMIT_HPP_
#include "wah_image_words.hpp"

namespace wah {
namespace {

// the emit pass: one lane of the launch writes the words of all items and raises kErrCapacity where they do not fit.  offsets:
// a.offsets, through whatever pointer type the kernel reads the scanned index with
template <bool kEmit, class Args, class Offsets>
__device__ __forceinline__ void emit_total(const Args &a, Offsets offsets, u64 n_items, const ItemRun &r, u32 lane) {
    if (kEmit && r.first && lane == 0) {
        const u64 total = offsets[n_items];
        *a.out_words = total;
        if (total > a.out_capacity) atomicOr(a.ctrl + kCtlError, kErrCapacity);
    }
}

// an item without a set bit: one zero-fill of the segment's groups; no LDS image, no load.  Returns its words
template <bool kEmit>
__device__ __forceinline__ u32 lone_zero_fill(u32 ngroups, u32 *stage, u32 lane) {
    if (kEmit && lane == 0) stage[0] = fill_word(kTypeZero, ngroups);
    return 1u;
}

// The end of an item of `total` words (wave-uniform).  Count pass: the count to offsets[item].  Emit pass: the words lie in
// stage[0 .. total) (LDS, written by any lanes); they go to their place in the output, 64 consecutive words per store
// instruction, clipped by the room the count pass found -- the same, unless the sources changed under the call -- and by the
// capacity.  The second fence: the next item stages over these words.
template <bool kEmit, class Args, class Offsets>
__device__ __forceinline__ void item_tail(const Args &a, Offsets offsets, u64 item, u32 total, const u32 *stage, u32 lane) {
    if (kEmit) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const u64 at = offsets[item], room = offsets[item + 1] - at;
        const u32 words = (u64)total < room ? total : (u32)room;
        for (u32 i = lane; i < words; i += 64u)
            if (at + i < a.out_capacity) a.out[at + i] = stage[i];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    } else if (lane == 0) {
        a.offsets[item] = (u64)total;
    }
}

// count pass (emit = false: every item's words to a.offsets) or emit pass (a.offsets scanned: the words to their place) over
// n_items items: `waves` wavefronts per workgroup, at most `most` workgroups, at least one
template <class Args>
hipError_t launch_count_or_emit(void (*count)(const Args), void (*emit_kernel)(const Args), bool emit, u64 n_items, u32 waves, u64 most,
                                const Args &a, hipStream_t s) {
    const u64 want = (n_items + waves - 1) / waves;
    const dim3 grid((unsigned)(want < 1 ? 1 : want > most ? most : want)), block(waves * 64);
    hipLaunchKernelGGL(emit ? emit_kernel : count, grid, block, 0, s, a);
    return hipGetLastError();
}

} // namespace
} // namespace wah
#endif // WAH_COUNT_EMIT_HPP_
