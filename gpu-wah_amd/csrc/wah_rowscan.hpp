// wah_rowscan.hpp -- the one-hop ROW SCAN of the tile kernels, written once (included by wah_compress.hip, wah_decode.hip).
//
// Every one-launch route rests on it: a workgroup draws a tile number (draw_tile, wah_device.hpp), publishes its tile's
// total as an epoch-stamped GRANULE, and wave 0 resolves what lies in front of the tile.  It replaces
// thrust::exclusive_scan + the blocking 8-byte reads of compress.cu:133-157 and decompress.cu:66-80.
//   granule[t]           {epoch:16, total ...} of tile t, published as soon as the tile's total is known
//   slot[s][0]           u64 {epoch:16, value:48}: what lies in front of superrow s  (superrow = kSuperRows rows)
//   slot[s][1 + k]       u64 {epoch:16, value:48}: total of row k of superrow s      (row = kRowTiles tiles)
// (scan area = one block per superrow: its 64 x 256 granules, then its 65 slots -- every entry has the same address and
//  the same meaning whatever the size of the input, so a workspace can serve inputs of different sizes in turn)
// Three scans use it; they differ in what a granule is and in how four of them fold -- the scan's POLICY:
//   compress              u32 {epoch:16, words:16}                      TileScanPolicy  (wah_compress.hip)
//   unsegmented compress  u64 {epoch:16, words:16, T:1, L:17}, a second slot array for (T, L)   UnsegScanPolicy  (there)
//   decoder's sums        u64 {epoch:16, groups:48}, saturating at 2^47  SumScanPolicy   (wah_decode.hip)
// Tile (row r, index i) adds up, in ONE round trip of three loads per lane (parts a, b and c of the sweep):
//   granule[r][0 .. i)  +  granule[r-1][0 .. 256)  +  slot[s][1 ..] of rows s0 .. r-2  +  slot[s][0]
// The last tile of a row publishes the row's slot as soon as its own row is complete (no dependency on anything
// older), the last tile of a superrow publishes the next superrow's slot[.][0].  So every dependency is "published
// by a tile with a smaller number" and at most one hop old; rows r-2 and older had >= one whole row of time.
// Order: tile numbers are drawn in the order in which the workgroups start running, so a tile only ever waits for tiles
// that are running; every wait is bounded all the same (kMaxSpins, then WAH_ERR_TIMEOUT: never a hang).
// Epochs: the workspace is never cleared.  Every launch stamps what it publishes with the launch epoch kept in the
// control block (read by every workgroup at its start, advanced by the LAST tile once its scan is complete -- by
// then every other tile has published, hence started).  A zeroed workspace is epoch 0 = "nothing valid".  When
// the 16-bit epoch is used up, the next launch has tile 0 clear the scan area while the others wait for it.
#ifndef WAH_ROWSCAN_HPP_
#define WAH_ROWSCAN_HPP_

#include "wah_device.hpp"

namespace wah {
namespace {

constexpr u32 kRowTiles = 256;  // granules per row: one 16-byte load per lane (8-byte granules: two)
constexpr u32 kSuperRows = 64;  // rows per superrow: one 8-byte load per lane
constexpr u32 kSlotShift = 48;  // u64 slots and 8-byte granules: value in the low 48 bits, epoch above
constexpr u64 kSlotMask = (1ull << kSlotShift) - 1ull;
static_assert(kRowSlots == kSuperRows + 1, "slot layout");
static_assert(kScanBlockWords >= kSuperRows * kRowTiles + 2 * kRowSlots && kScanSlotsAt == kSuperRows * kRowTiles, "scan block layout");
static_assert(kUnsegBlockWords >= kUnsegSlotsBAt + 2 * kRowSlots && kUnsegSlotsBAt >= kUnsegSlotsAAt + 2 * kRowSlots &&
                  kUnsegSlotsAAt == 2 * kSuperRows * kRowTiles,
              "unsegmented scan block layout");
static_assert(kSumScanBlockWords >= 2 * kSuperRows * kRowTiles + 2 * kRowSlots && kSumScanSlotsAt == 2 * kSuperRows * kRowTiles,
              "sums scan block layout");

struct ScanGeom {
    u32 row, idx, sup, row0; // tile = row * kRowTiles + idx; superrow of the row and its first row
    u32 n_slots;             // slots to read: [0] and the rows row0 .. row - 2
    bool has_prev;           // the previous row belongs to the same superrow (else slot[0] covers it)
};

__device__ __forceinline__ ScanGeom scan_geom(u32 tile) {
    ScanGeom g;
    g.row = tile / kRowTiles;
    g.idx = tile % kRowTiles;
    g.sup = g.row / kSuperRows;
    g.row0 = g.sup * kSuperRows;
    g.has_prev = g.row > g.row0;
    g.n_slots = g.has_prev ? g.row - g.row0 : 1u;
    return g;
}

// The sweep's descriptors are made of values that ARE the same in every lane (the tile's number and what follows from it);
// they are passed through readfirstlane all the same: where the compiler cannot prove it (seen in decode_tile_kernel, where
// the call sits inside `if (wave == 0)` of a large unrolled body) it wraps every load in a "waterfall" loop over the distinct
// descriptors, and a re-read issued for SOME lanes then came back with the other lanes' earlier values zeroed (ROCm 7.2;
// tools/dbg_decode_tile.py: the base of a first-generation tile of row 2 = the entries of lanes 30..61 only).  For the same
// reason row_scan_wait re-issues a sweep from EVERY lane, never under a per-lane condition.
struct SweepAt {
    u32 *block;                     // my superrow's granules and slots
    u32 row_in_super, idx, n_slots; // of my tile (ScanGeom)
};
__device__ __forceinline__ SweepAt sweep_at(u32 *block, const ScanGeom &g) {
    return {reinterpret_cast<u32 *>(uniform64(reinterpret_cast<u64>(block))), uniform32(g.row - g.row0), uniform32(g.idx), uniform32(g.n_slots)};
}
__device__ __forceinline__ u64 sweep_slots(const SweepAt &s, u32 slots_at, u32 lane) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(make_rsrc(s.block + slots_at, s.n_slots * 8u), lane * 8u, 0, kAuxSc1);
    return ((u64)v.y << 32) | v.x;
}

// ---- the sweep over 8-byte granules (unsegmented compress: two slot arrays; the decoder's sums: one) -------------------------
template <u32 kSlotArrays>
struct Sweep8 {
    u32x4 a[2], b[2];   // granules of my row (entries below me; the descriptor cuts the rest off) and of the previous row: four per lane
    u64 c[kSlotArrays]; // slots of my superrow: lane 0 = what lies in front of it, lane 1 + k = its row k
};
__device__ __forceinline__ u64 granule8(const u32x4 (&q)[2], int k) { // entry k of a lane's four
    const u32x4 &v = q[k >> 1];
    return ((u64)(k & 1 ? v.w : v.y) << 32) | (k & 1 ? v.z : v.x);
}
template <u32... kSlotsAt> // where the block's slot arrays begin (32-bit words)
__device__ __forceinline__ void sweep8_issue(u32 *block, const ScanGeom &g, u32 lane, bool need_a, bool need_b, bool need_c,
                                             Sweep8<sizeof...(kSlotsAt)> &p) {
    constexpr u32 slots_at[] = {kSlotsAt...};
    const SweepAt s = sweep_at(block, g);
    if (need_a) {
        const __amdgpu_buffer_rsrc_t ra = make_rsrc(s.block + (u64)s.row_in_super * kRowTiles * 2u, s.idx * 8u);
        p.a[0] = __builtin_amdgcn_raw_buffer_load_b128(ra, lane * 32u, 0, kAuxSc1);
        p.a[1] = __builtin_amdgcn_raw_buffer_load_b128(ra, lane * 32u + 16u, 0, kAuxSc1);
    }
    if (need_b) {
        const __amdgpu_buffer_rsrc_t rb = make_rsrc(s.block + (u64)(s.row_in_super - 1u) * kRowTiles * 2u, kRowTiles * 8u);
        p.b[0] = __builtin_amdgcn_raw_buffer_load_b128(rb, lane * 32u, 0, kAuxSc1);
        p.b[1] = __builtin_amdgcn_raw_buffer_load_b128(rb, lane * 32u + 16u, 0, kAuxSc1);
    }
    if (need_c) {
#pragma unroll
        for (u32 i = 0; i < sizeof...(kSlotsAt); ++i) p.c[i] = sweep_slots(s, slots_at[i], lane);
    }
}
// which of a lane's four entries are wanted (sequence number below `below`) and not of this epoch yet
__device__ __forceinline__ u32 sweep8_missing(const u32x4 (&q)[2], u32 below, u32 lane, u32 epoch) {
    u32 bad = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4u * lane + k < below && (u32)(granule8(q, k) >> kSlotShift) != epoch) bad |= 1u << k;
    return bad;
}
// slot 0 of superrow 0 is never written: nothing lies in front of the first tile
__device__ __forceinline__ bool slot_wanted(const ScanGeom &g, u32 lane) { return lane < g.n_slots && !(g.sup == 0u && lane == 0u); }

__device__ __forceinline__ void row_scan_timeout(u32 *ctrl, u32 lane) {
    if (lane == 0) atomicOr(ctrl + kCtlError, kErrTimeout);
}

// ---- the wait: wave 0 of a tile, its sweep issued; returns when the policy has accepted all three parts (or on timeout) ---------
// The policy is a struct of a few inline members, all state in registers:
//   Word                   what an entry's epoch is read from (the granule, or the half of it that holds the epoch)
//   issue(lane, a, b, c)   the sweep's loads for the parts still needed -- always called by every lane (see sweep_at)
//   missing_a/_b/_c(lane)  mask of the lane's entries of that part that are wanted and not of this epoch yet
//   accept_a/_b/_c(lane)   the part is complete: fold it; accept_a also publishes the row's slot if the tile is its row's last
//   row_a(), row_b()       where entry 0 of the part lives; slot_word(lane, mask): the same for a missing slot
//   epoch_of(word)
// If a few entries of the sweep are still missing (the nearest predecessors), the sweep is simply read again.  If many are
// (a tile of an XCD that runs ahead of the others), the wave does NOT sweep again and again -- hundreds of waiting tiles
// re-reading 2.5 KB each every microsecond is traffic of the order of the bitmap's: it parks on ONE word, the missing entry
// with the highest tile number, the one that will be published last (row a before row b before the slots), and sweeps again
// when that one is there.
// kDirectLanes: up to this many lanes with missing entries (the nearest ~64 predecessors) are read again at once; 0 = always
// park.  Both compress scans take 16; the decoder's scan takes 0, measured: decode_tile_kernel on the 1 GiB bitmaps with 0 / 16 /
// 64 takes 0.3204 / 0.3208 / 0.3209 ms (sparse) and 0.4117 / 0.4115 / 0.4118 ms (dense), each +- 0.001 -- no difference, so it
// keeps the shorter code (profiles/critical_path_priority_time.txt).
// kDropPriority: the caller runs its scan at raised issue priority (s_setprio).  The first evaluation of the sweep
// runs raised; as soon as something is missing the wave drops to priority 0 and stays there -- no s_sleep and no polling load is
// ever issued at raised priority, where it would take issue slots from the waves it is waiting for.  The caller drops again
// (a no-op then) once it has used the result.
template <u32 kDirectLanes, bool kDropPriority = false, class Policy>
__device__ __forceinline__ void row_scan_wait(Policy &p, const ScanGeom &g, u32 *ctrl, u32 epoch, u32 lane, u32 *polls = nullptr) {
    (void)polls; // (WAH_DIAG: sweeps issued beyond the first)
    bool need_a = true, need_b = g.has_prev, need_c = true;
    u32 spins = 0;
    for (;;) {
        u32 bad_a = 0, bad_b = 0, bad_c = 0; // per lane: which of my entries are missing
        u64 ba = 0, bb = 0, bc = 0;
        if (need_a) {
            bad_a = p.missing_a(lane);
            ba = __ballot(bad_a != 0u);
            if (ba == 0) {
                p.accept_a(lane);
                need_a = false;
            }
        }
        if (need_b) {
            bad_b = p.missing_b(lane);
            bb = __ballot(bad_b != 0u);
            if (bb == 0) {
                p.accept_b(lane);
                need_b = false;
            }
        }
        if (need_c) {
            bad_c = p.missing_c(lane);
            bc = __ballot(bad_c != 0u);
            if (bc == 0) {
                p.accept_c(lane);
                need_c = false;
            }
        }
        if (!(need_a || need_b || need_c)) return;
        if (++spins > kMaxSpins) return row_scan_timeout(ctrl, lane);
        if (kDropPriority) __builtin_amdgcn_s_setprio(0); // something is missing: from here on the wave only waits, and waits at priority 0
        if (kDirectLanes != 0u && (u32)__builtin_popcountll(ba) + (u32)__builtin_popcountll(bb) + (u32)__builtin_popcountll(bc) <= kDirectLanes) {
            __builtin_amdgcn_s_sleep(4);
        } else {
            const typename Policy::Word *target;
            if (need_a) {
                const u32 hl = 63u - (u32)__builtin_clzll(ba);
                target = p.row_a() + 4u * hl + (31u - (u32)__builtin_clz((u32)__builtin_amdgcn_readlane((int)bad_a, (int)hl)));
            } else if (need_b) {
                const u32 hl = 63u - (u32)__builtin_clzll(bb);
                target = p.row_b() + 4u * hl + (31u - (u32)__builtin_clz((u32)__builtin_amdgcn_readlane((int)bad_b, (int)hl)));
            } else {
                const u32 hl = 63u - (u32)__builtin_clzll(bc);
                target = p.slot_word(hl, (u32)__builtin_amdgcn_readlane((int)bad_c, (int)hl));
            }
            for (;;) {
                __builtin_amdgcn_s_sleep(8);
                if (p.epoch_of(__hip_atomic_load(target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == epoch) break;
                if (++spins > kMaxSpins) return row_scan_timeout(ctrl, lane);
            }
        }
        p.issue(lane, need_a, need_b, need_c);
#ifdef WAH_DIAG
        if (polls) ++*polls;
#endif
    }
}

} // namespace
} // namespace wah

#endif // WAH_ROWSCAN_HPP_
