// wah_device.hpp -- wavefront / LDS / scan helpers shared by the kernel files (gfx950, wave64).
// Everything lives in an anonymous namespace: every translation unit gets its own copy, nothing is exported.
#ifndef WAH_DEVICE_HPP_
#define WAH_DEVICE_HPP_

#include "wah_internal.hpp"

namespace wah {
namespace {

using u32 = uint32_t;
using u64 = uint64_t;

// Diagnostic build only (make diag): per-phase cycle totals of each workgroup's thread 0, added into the unused
// tail of the control block.  The product build contains no stamps.
#ifdef WAH_DIAG
#define WAH_STAMP_DECL u64 dg_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; u64 dg_big[8] = {0, 0, 0, 0, 0, 0, 0, 0}; u64 dg_prev = __builtin_readcyclecounter();
#define WAH_STAMP(i)                                      \
    do {                                                  \
        const u64 dg_now = __builtin_readcyclecounter();  \
        dg_acc[i] += dg_now - dg_prev;                    \
        dg_big[i] += (dg_now - dg_prev) > 4000u;          \
        dg_prev = dg_now;                                 \
    } while (0)
#define WAH_STAMP_FLUSH(ctrl)                                                                      \
    do {                                                                                           \
        if (threadIdx.x == 0)                                                                      \
            for (int i = 0; i < 8; ++i) {                                                          \
                atomicAdd(reinterpret_cast<unsigned long long *>(ctrl + 192) + i, (unsigned long long)dg_acc[i]); \
                atomicAdd(reinterpret_cast<unsigned long long *>(ctrl + 192) + 16 + i, (unsigned long long)dg_big[i]); \
            }                                                                                      \
    } while (0)
#else
#define WAH_STAMP_DECL
#define WAH_STAMP(i) asm volatile("; WAH_MARK " #i ::: "memory")
#define WAH_STAMP_FLUSH(ctrl)
#endif

constexpr u32 kMaxSpins = 1u << 21; // bound of every in-kernel wait (polls with a sleep in between: seconds)

__device__ __forceinline__ u32 lane_id() { return threadIdx.x & 63u; }
// wave-uniform by construction; readfirstlane tells the compiler so (keeps masks and offsets in SGPRs)
__device__ __forceinline__ u32 wave_id() { return (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ u32 wave_sum32(u32 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// inclusive prefix sum across the 64 lanes
__device__ __forceinline__ u64 wave_scan_incl(u64 v, u32 lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 t = __shfl_up(v, off);
        if (lane >= (u32)off) v += t;
    }
    return v;
}

// inclusive prefix sum of a u32 across the 64 lanes with DPP only (no LDS crossbar): Hillis-Steele inside each
// row of 16 lanes (row_shr 1,2,4,8, zero fill), then row_bcast:15 into rows 1 and 3, then row_bcast:31 into rows 2-3
__device__ __forceinline__ u32 wave_scan_incl32(u32 v) {
    v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false);
    return v;
}

// sum of a u32 over the 64 lanes as a wave-uniform value, DPP only (wave_sum32's six trips through the LDS crossbar are
// a chain of six LDS latencies)
__device__ __forceinline__ u32 wave_total32(u32 v) { return (u32)__builtin_amdgcn_readlane((int)wave_scan_incl32(v), 63); }

// inclusive prefix MAXIMUM of a u32 across the 64 lanes, same DPP pattern (missing sources read as 0)
__device__ __forceinline__ u32 wave_scan_max32(u32 v) {
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, true));
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, true));
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, true));
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, true));
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false));
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false));
    return v;
}

// Values read back from LDS are wave-uniform here by construction; readfirstlane tells the compiler so, which
// keeps everything derived from them (segment numbers, masks, offsets, branches) on the scalar unit.
__device__ __forceinline__ u32 uniform32(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 uniform64(u64 v) {
    return ((u64)uniform32((u32)(v >> 32)) << 32) | uniform32((u32)v);
}


typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32 u32x2 __attribute__((ext_vector_type(2)));

using lds_u32_ptr = __attribute__((address_space(3))) u32 *;
using lds_u64_ptr = __attribute__((address_space(3))) u64 *;
using lds_u16_ptr = __attribute__((address_space(3))) unsigned short *;
using lds_u8_ptr = __attribute__((address_space(3))) unsigned char *;


// Buffer descriptor over `bytes` bytes at p (raw, stride 0): loads past the end return 0, stores past the end are
// dropped -- the hardware does the tail padding (F5) and the capacity clipping, and addresses become
// descriptor + 32-bit lane offset + immediate, with no 64-bit vector arithmetic per access.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, u32 bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x27000);
}

// ---------------------------------------------------------------------------
// Launch epochs: how the scan areas of the tile kernels (compress_tile_body, decode_sums_kernel) get by without
// being cleared.  Everything a launch publishes is stamped with the launch epoch kept in the control block: read by
// every workgroup at its start, advanced by the LAST tile once its scan is complete -- by then every other tile has
// published, hence started.  A zeroed workspace is epoch 0 = "nothing valid".  When the epoch space is used up, the
// next launch has tile 0 clear the scan area while the others wait for it (tile 0 has the smallest blockIdx: it is
// running).  Called by ALL threads of the workgroup (it contains barriers in the wrap case).
// ---------------------------------------------------------------------------
struct LaunchEpoch {
    u32 epoch;
    bool wrap, bad;
};

// Tile number of a workgroup of a tile kernel = the order in which workgroups START RUNNING (one agent-scope atomic per
// workgroup), never blockIdx: a tile only ever waits for tiles with smaller numbers, and those have been drawn, so they
// are running (or done) -- whatever else shares the GPU.  With tile = blockIdx two such kernels running side by side
// (two streams, two processes) can starve each other for good: the XCDs dispatch their shares of a grid independently,
// so kernel A's waiting tiles can fill one XCD while its lowest tile needs a slot on another that kernel B's waiting
// tiles fill, and vice versa (seen: multi-second stalls with two ranks on one card).  Called by ALL threads.
__device__ __forceinline__ u32 draw_tile(u32 *ctrl, u32 *s_tile) {
    if (threadIdx.x == 0) *s_tile = __hip_atomic_fetch_add(ctrl + kCtlStart, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return uniform32(*s_tile);
}

// A workgroup's prologue is ASK, TICKET, DECIDE.  What launch_epoch_begin needs of the control block does not depend on the
// tile number, so it is asked for BEFORE the ticket is drawn: the three loads and thread 0's ticket atomic are in flight together,
// one round trip instead of two in front of the tile's first data load (which needs the ticket and nothing else: the callers issue
// it right behind draw_tile, under tile < n_tiles, and call launch_epoch_begin with it in flight).  Reading early is allowed: the
// words are written by launch_epoch_end alone, by the LAST tile once every other tile has published -- hence started, hence asked
// -- and the protocol wants no more of a workgroup than that it has read the epoch before it publishes.  Relaxed atomic loads
// (wavefront scope: the plain global_load they were, no cache bits -- nothing of THIS launch writes the words while they are
// read): the compiler moves no atomic across draw_tile's atomic and barrier, so they stay in front of s_barrier.  Vector loads,
// not scalar ones: the scalar cache is shared between CUs and is not what an earlier launch's agent-scope stores are ordered
// against.
struct EpochAsk {
    u32 stored, magic, wraps;
};
__device__ __forceinline__ EpochAsk launch_epoch_ask(u32 *ctrl) {
    EpochAsk q;
    q.stored = __hip_atomic_load(ctrl + kCtlEpoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    q.magic = __hip_atomic_load(ctrl + kCtlMagic, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    q.wraps = __hip_atomic_load(ctrl + kCtlWraps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); // (used when the epoch space wraps; the epoch's line)
    return q;
}
// TICKET, with the answers taken behind its barrier (scalar registers from here on).  They have had the ticket's round trip and
// the barrier to arrive, so this wait is over before it begins -- and it is the last one for them: the wait counters count in
// order, and a wait for the answers placed BEHIND the tile's data loads waits, wherever a branch lies between, for the data too
// (seen: s_waitcnt vmcnt(1) behind the eight loads of a pair, in front of the decision).
__device__ __forceinline__ u32 draw_tile(u32 *ctrl, u32 *s_tile, EpochAsk &ask) {
    const u32 tile = draw_tile(ctrl, s_tile);
    ask.stored = uniform32(ask.stored);
    ask.magic = uniform32(ask.magic);
    ask.wraps = uniform32(ask.wraps);
    return tile;
}

// DECIDE, behind the ticket's barrier, from what launch_epoch_ask brought (the caller's data loads may be in flight: on le.bad it
// waits for them before it returns; the wrap path's wait happens with them in flight)
__device__ __forceinline__ LaunchEpoch launch_epoch_begin(u32 *ctrl, const EpochAsk &ask, u32 tile, u32 n_tiles, u32 *scan_area, u64 scan_words, int keep_error) {
    LaunchEpoch le;
    const u32 stored = ask.stored, magic = ask.magic; // (draw_tile has made them scalar)
    // neither a zeroed nor a used workspace: a foreign magic word, an epoch no launch can have left, or a ticket counter
    // that did not start at zero -- a tile number outside the grid, checked BEFORE anything is indexed with it (recycled
    // memory often reads as magic == 0 with garbage elsewhere)
    le.bad = (magic != 0u && magic != kWorkspaceMagic) || stored > kEpochWrap || tile >= n_tiles;
    le.wrap = stored >= kEpochWrap;
    le.epoch = (stored == 0u || le.wrap) ? 1u : stored;
    if (le.bad) {
        if (threadIdx.x == 0) atomicOr(ctrl + kCtlError, kErrWorkspace);
        return le;
    }
    if (le.wrap) {
        const u32 wraps = ask.wraps;
        if (tile == 0) {
            for (u64 k = threadIdx.x; k < scan_words; k += blockDim.x)
                __hip_atomic_store(scan_area + k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0) __hip_atomic_store(ctrl + kCtlClearDone, wraps + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (threadIdx.x == 0) {
                u32 spins = 0;
                while (__hip_atomic_load(ctrl + kCtlClearDone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != wraps + 1u) {
                    if (++spins > kMaxSpins) {
                        atomicOr(ctrl + kCtlError, kErrTimeout);
                        break;
                    }
                    __builtin_amdgcn_s_sleep(8);
                }
            }
            __syncthreads();
        }
    }
    if (tile == 0 && threadIdx.x == 0 && !keep_error) {
        // a new launch: forget the previous one's status.  Completed before this tile publishes anything, and every
        // error of this launch is raised by a tile that has seen something published.
        __hip_atomic_store(ctrl + kCtlError, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    return le;
}

// one lane of the last tile, after its scan: every other tile has published its granule, so it has read the epoch
__device__ __forceinline__ void launch_epoch_end(u32 *ctrl, const LaunchEpoch &le) {
    if (le.wrap) __hip_atomic_store(ctrl + kCtlWraps, ctrl[kCtlWraps] + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(ctrl + kCtlStart, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // every tile number has been drawn
    __hip_atomic_store(ctrl + kCtlMagic, kWorkspaceMagic, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(ctrl + kCtlEpoch, le.epoch + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int kAuxSc1 = 16; // buffer load cache policy: sc1 = agent scope (served past the XCD-private caches)

// groups a compressed word expands to
__device__ __forceinline__ u32 word_groups(u32 w) {
    return (w & kFillZero) ? (w & kCountMask) : 1u; // kernels.cu:298-304
}

// the combination of two group values (31 bits) by the minterms of `acc op operand` (include/wah.h: WAH_OP_AND 0, OR 1, XOR 2,
// ANDNOT 3: A and not B and not C ...): three masks, wave-uniform, made once -- no branch on the operation inside a step
// (the run merge of wah_bitop_runs.hip, the operand list of wah_bitop_list.hip)
struct RunsOp {
    u32 ab, a_nb, na_b;
};
__device__ __forceinline__ RunsOp runs_op(u32 op) {
    RunsOp m;
    m.ab = op <= 1u ? ~0u : 0u;
    m.a_nb = op == 0u ? 0u : ~0u;
    m.na_b = op == 1u || op == 2u ? ~0u : 0u;
    return m;
}
__device__ __forceinline__ u32 runs_combine(u32 r, u32 v, const RunsOp &m) {
    return ((r & v & m.ab) | (r & ~v & m.a_nb) | (~r & v & m.na_b)) & kOnes31;
}

// A bitmap's segments (1024 groups of 31 positions each) as the indexed kernels cut them
constexpr u32 kSegBits = kSegGroups * 31u; // 31 744
// the groups of segment `seg` of a bitmap of `groups`: 1024 but for the last
__device__ __forceinline__ u32 segment_groups(u64 groups, u64 seg) {
    const u64 g0 = seg * kSegGroups;
    return groups - g0 < kSegGroups ? (u32)(groups - g0) : kSegGroups;
}
// the positions of segment `seg` that are rows, of a bitmap of n_rows rows: the first `return value` of its 31 744 (0 .. 31 744)
__device__ __forceinline__ u32 segment_rows(u64 n_rows, u64 seg) {
    const u64 lo = seg * (u64)kSegBits;
    return n_rows <= lo ? 0u : n_rows - lo < kSegBits ? (u32)(n_rows - lo) : kSegBits;
}
// the bits of group g of a segment with seg_rows rows that are rows
__device__ __forceinline__ u32 group_row_bits(u32 g, u32 seg_rows) {
    const u32 first = 31u * g;
    const u32 nb = seg_rows <= first ? 0u : min(seg_rows - first, 31u);
    return (1u << nb) - 1u; // (nb <= 31: bit 31 is never a row)
}
// the first i of 0 .. n - 1 whose run [starts[i], starts[i + 1]) ends behind `base`, for ascending starts with starts[n] > base
// (wave-uniform)
__device__ __forceinline__ u64 first_end_behind(const u64 *starts, u64 n, u64 base) {
    u64 lo = 0, hi = n - 1;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (uniform64(starts[mid + 1]) > base) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the items begin .. end - 1 of n_items that this wavefront owns: contiguous runs of equal length over the launch's wavefronts
// (`waves` per workgroup), the last ones shorter or empty
struct ItemRun {
    u64 begin, end;
    bool first; // the launch's first wavefront
};
__device__ __forceinline__ ItemRun item_run(u64 n_items, u32 waves, u32 wave) {
    const u64 n_waves = (u64)gridDim.x * waves;
    const u64 per = (n_items + n_waves - 1) / n_waves;
    const u64 w = (u64)blockIdx.x * waves + wave;
    ItemRun r;
    r.begin = w * per < n_items ? w * per : n_items;
    r.end = r.begin + per < n_items ? r.begin + per : n_items;
    r.first = w == 0;
    return r;
}

// expand / checker / merge kernels: one workgroup of four wavefronts per 4096-word tile
constexpr int kExpandThreads = kExpandWaves * 64;                 // 256
constexpr int kExpandWordsPerThread = kScanTileWords / kExpandThreads; // 16
constexpr u32 kCoarse = kScanTileWords / 64;                      // coarse prefix: one entry per 64 words

} // namespace
} // namespace wah

#endif // WAH_DEVICE_HPP_
