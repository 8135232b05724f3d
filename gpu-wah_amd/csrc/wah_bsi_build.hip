// wah_bsi_build.hip -- the decoded slice matrix of a bit-sliced index straight from a column of 64-bit values
// (wah_bsi_build_device): a bit transpose.  Row i of the matrix [n_slices, n_words] holds bit n_bits - 1 - i of every value (row 0:
// the most significant bit), the existence bitmap is the last row when there is one; table row p is word p / 32, bit p % 32 of
// every matrix row.  The one-launch compressor turns the matrix into the index (slices are mostly incompressible: its own road).
// The reference has no counterpart: its compress() takes one decoded bitmap (compress.cu:41-209).
//
// One launch, bsi_slices_kernel, and no workgroup of it waits for another.  A wavefront owns a block of 2048 consecutive rows --
// 64 words of every slice, 16 KiB of values -- and takes blocks in a grid-stride loop:
//   load     32 steps of 64 rows, lane l taking row 64 t + l: 512 contiguous bytes per load instruction, each value read once and
//            kept as two statically indexed 32-bit halves (64 registers).  The loads go through buffer descriptors that end with
//            the column, so a row at or beyond n_rows is not loaded: value 0, not existing.  Every loaded value's bits at and above n_bits are ORed into one register BEFORE its existence byte is
//            looked at (the verdict does not depend on which rows exist); a row whose existence byte is 0 becomes value 0.  The
//            ballot of the existence bytes of step t is words 2t and 2t + 1 of the existence row.
//   slices   a RUNTIME loop over the bits, most significant first (the upper halves, then the lower ones: a 32-bit AND and a
//            compare per step instead of a 64-bit shift).  For slice b and each of the 32 unrolled steps, the ballot of "bit b of
//            my value" is words 2t and 2t + 1 of the slice; two v_writelane put them into lanes 2t and 2t + 1 of ONE accumulator,
//            so after 32 steps lane j holds word j and one store instruction writes 256 contiguous bytes of the slice's row,
//            masked by n_words in the last block.  No LDS, no register array indexed by the slice.
// Every word of every row is written, the zeros behind the last row up to n_words included: the matrix needs no clearing.  The
// only atomic is the one OR into the sticky error word, by one lane of a wavefront that saw a value at or above 2^n_bits.
#include "wah_slice_words.hpp" // put_lane and slice_words: shared with wah_map.hip

namespace wah {
namespace {

constexpr u32 kBsiBuildWaves = 4;    // wavefronts of a workgroup (nothing is shared between them)
constexpr u32 kBsiBlockWords = 64;   // slice words per block: one per lane
constexpr u32 kBsiBlockSteps = 32;   // loads of 64 rows per block
constexpr u64 kBsiBlockRows = 2048;  // 32 * kBsiBlockWords

template <bool kExists>
__global__ __launch_bounds__(kBsiBuildWaves * 64, 4) void bsi_slices_kernel(const BsiBuildArgs a) {
    const u32 lane = lane_id();
    const u64 n_blocks = (a.n_words + kBsiBlockWords - 1) / kBsiBlockWords;
    const u64 n_waves = (u64)gridDim.x * kBsiBuildWaves;
    // bits of a value's halves that a width of n_bits has no room for
    const u32 over_lo = a.n_bits >= 32u ? 0u : ~0u << a.n_bits;
    const u32 over_hi = a.n_bits >= 64u ? 0u : a.n_bits > 32u ? ~0u << (a.n_bits - 32u) : ~0u;
    u32 over = 0u;
#pragma nounroll
    for (u64 blk = (u64)blockIdx.x * kBsiBuildWaves + wave_id(); blk < n_blocks; blk += n_waves) {
        // the block's rows through descriptors that end with the column: a row at or beyond n_rows is not loaded and reads as 0,
        // value and existence byte alike, without a branch (a descriptor of 0 bytes over a null pointer loads nothing at all)
        const u64 row0 = blk * kBsiBlockRows;
        const u64 left = row0 < a.n_rows ? a.n_rows - row0 : 0ull;
        const u32 rows = (u32)(left < kBsiBlockRows ? left : kBsiBlockRows);
        const __amdgpu_buffer_rsrc_t rv = make_rsrc(a.values + row0, rows * 8u);
        u32 lo[kBsiBlockSteps], hi[kBsiBlockSteps];
#pragma unroll
        for (u32 t = 0; t < kBsiBlockSteps; ++t) {
            const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rv, lane * 8u + 512u * t, 0, 0);
            lo[t] = v.x;
            hi[t] = v.y;
        }
        u32 have = 0u; // lane j: word j of the existence row
        if (kExists) {
            const __amdgpu_buffer_rsrc_t re = make_rsrc(a.exists + row0, rows);
            u32 e[kBsiBlockSteps];
#pragma unroll
            for (u32 t = 0; t < kBsiBlockSteps; ++t) e[t] = __builtin_amdgcn_raw_buffer_load_b8(re, lane + 64u * t, 0, 0);
#pragma unroll
            for (u32 t = 0; t < kBsiBlockSteps; ++t) {
                over |= (lo[t] & over_lo) | (hi[t] & over_hi); // (before the existence byte has its say)
                const bool has = e[t] != 0u;
                lo[t] = has ? lo[t] : 0u;
                hi[t] = has ? hi[t] : 0u;
                const u64 m = __ballot(has);
                have = put_lane((u32)m, 2u * t, have);
                have = put_lane((u32)(m >> 32), 2u * t + 1u, have);
            }
        } else {
#pragma unroll
            for (u32 t = 0; t < kBsiBlockSteps; ++t) over |= (lo[t] & over_lo) | (hi[t] & over_hi);
        }
        const u64 word = blk * kBsiBlockWords + lane;
        const bool store = word < a.n_words;
        u32 *out = a.out + word; // row 0 of the matrix; every row is n_words further
#pragma nounroll
        for (u32 b = a.n_bits; b > 32u; --b) {
            const u32 w = slice_words(hi, 1u << (b - 33u));
            if (store) *out = w;
            out += a.n_words;
        }
#pragma nounroll
        for (u32 b = a.n_bits < 32u ? a.n_bits : 32u; b > 0u; --b) {
            const u32 w = slice_words(lo, 1u << (b - 1u));
            if (store) *out = w;
            out += a.n_words;
        }
        if (kExists && store) *out = have;
    }
    if (__ballot(over != 0u) != 0ull && lane == 0) atomicOr(a.ctrl + kCtlError, kErrStream);
}

} // namespace

hipError_t launch_bsi_slices(const BsiBuildArgs &a, hipStream_t s) {
    const u64 n_blocks = (a.n_words + kBsiBlockWords - 1) / kBsiBlockWords;
    const u64 want = (n_blocks + kBsiBuildWaves - 1) / kBsiBuildWaves;
    constexpr u64 most = 256u * 8u; // CUs x workgroups of four wavefronts: more than are ever resident at once
    const dim3 grid((unsigned)(want < 1 ? 1 : want > most ? most : want));
    if (a.exists) {
        hipLaunchKernelGGL(bsi_slices_kernel<true>, grid, dim3(kBsiBuildWaves * 64), 0, s, a);
    } else {
        hipLaunchKernelGGL(bsi_slices_kernel<false>, grid, dim3(kBsiBuildWaves * 64), 0, s, a);
    }
    return hipGetLastError();
}

} // namespace wah
