// wah_api.hip -- the C ABI of include/wah.h and the C++-linkage drop-ins of
// include/compress.h / include/decompress.h, on top of the kernels.
//
// Host orchestration replacing compress.cu:41-209 and decompress.cu:18-141:
// same phases and the same three timings, but the device phase is
// memset(control block) + kernel(s) with no allocation, no blocking 8-byte
// read-back in the middle and no library scan.
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <sys/mman.h>
#include <cstdlib>
#include <cstring>

// (-fvisibility=hidden: the reference's two entry points are exported like everything include/wah.h declares; their
//  headers stay the reference's text)
#pragma GCC visibility push(default)
#include "../../include/compress.h"
#include "../../include/decompress.h"
#pragma GCC visibility pop
#include "../../include/wah.h"
#include "wah_internal.hpp"

namespace {

thread_local char g_err[256] = "";

void set_err(const char *what, hipError_t e = hipSuccess) {
    if (e != hipSuccess)
        std::snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    else
        std::snprintf(g_err, sizeof g_err, "%s", what);
}

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
inline size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

// a call that is refused: the text wah_last_error() returns, and the code the call returns
int refuse(const char *what, int rc, hipError_t e = hipSuccess) {
    set_err(what, e);
    return rc;
}

// a bitmap of n_words words: its 31-bit groups, its segments of kSegGroups groups, and the bits of its last group that lie
// behind the bitmap (31 G - 32 n_words: 0 .. 30)
struct SegGeometry {
    uint64_t groups, n_segments;
    uint32_t pad_bits;
};
SegGeometry seg_geometry(uint64_t n_words) {
    SegGeometry g;
    g.groups = wah_max_compressed_words(n_words);
    g.n_segments = ceil_div(g.groups, (uint64_t)wah::kSegGroups);
    g.pad_bits = (uint32_t)(31u * g.groups - 32u * n_words);
    return g;
}

// what the indexed calls ask of their scratch, and of an operand table in device memory (wah_bitop_operand rows)
inline bool scratch_ok(const void *d_scratch) { return d_scratch && aligned(d_scratch, 255); }
inline bool table_ok(uint64_t n, const void *d_table, uint64_t n_words) {
    return n >= 1 && n <= wah::kMaxBitopListOperands && d_table && aligned(d_table, 7) && n_words < (1ull << 40);
}
constexpr const char *kBadTable = "between 1 and 2^24 operands in an 8-byte aligned table, fewer than 2^40 words";
// ... and of their output: the calls that leave ONE stream need its count, and its words unless the bitmap is empty (the index is
// optional); the calls that leave several streams back to back need all three, aligned
inline bool out_given(uint64_t n_words, const uint32_t *d_out, const uint64_t *d_out_words) { return d_out_words && (!n_words || d_out); }
inline bool out_triple_ok(const uint32_t *d_out, const uint64_t *d_out_words, const uint64_t *d_out_offsets) {
    return d_out && aligned(d_out, 3) && d_out_words && aligned(d_out_words, 7) && d_out_offsets && aligned(d_out_offsets, 7);
}

// Workspace layouts.  Everything a launch stamps with its epoch lives in areas whose PLACE depends on the workspace's size
// only, never on the size of the input: one workspace serves inputs of different sizes in turn (include/wah.h), and an
// area that moved with the input would let one call's data be read as another call's published entries.  Both layouts
// are [control block][first half][second half], the halves being (workspace_bytes - control block) / 2 each.
struct CompressLayout {
    uint64_t n_groups, n_segments, n_tiles;
    uint32_t wave_segs;
    size_t ctrl_off, desc_off, unseg_off, half, total; // total: what an input of this size needs
};

// first half: scan area of compress_pair_kernel / compress_tile_body (one block of kScanBlockWords per 64 x 256 tiles, +
// the block a full last superrow publishes into); second half: scan area of the unsegmented mode (blocks of
// kUnsegBlockWords), which the no-wait route borrows for its table of tile counts (offsets below 2^48: never a valid
// epoch stamp)
CompressLayout compress_layout(uint64_t n_words, size_t workspace_bytes = 0) {
    CompressLayout l;
    const SegGeometry g = seg_geometry(n_words);
    l.n_groups = g.groups;
    l.n_segments = g.n_segments;
    l.wave_segs = wah::compress_wave_segs(l.n_segments);
    l.n_tiles = ceil_div(l.n_segments, (uint64_t)wah::kCompressTileWaves * l.wave_segs);
    // sized for the shortest tiles: a workspace serves any smaller bitmap too
    const uint64_t blocks = ceil_div(l.n_segments, (uint64_t)wah::kCompressTileWaves) / wah::kScanBlockTiles + 1;
    static_assert(wah::kUnsegBlockWords >= wah::kScanBlockWords, "the halves are sized by the larger block");
    const size_t need_half = round256(blocks * wah::kUnsegBlockWords * sizeof(uint32_t));
    l.ctrl_off = 0;
    l.desc_off = wah::kCtlWords * sizeof(uint32_t);
    l.total = l.desc_off + 2 * need_half;
    const size_t w = workspace_bytes ? workspace_bytes : l.total;
    l.half = w > l.desc_off ? ((w - l.desc_off) / 2) & ~(size_t)255 : 0;
    l.unseg_off = l.desc_off + l.half;
    if (l.half < need_half) l.total = w + 1; // (does not fit: the callers compare workspace_bytes with total)
    return l;
}

struct DecodeLayout {
    uint64_t n_tiles;
    size_t ctrl_off, desc_off, base_off, flags_off, defer_off, bucket_off, half, total, scan_bytes;
};

// first half: scan area of the sums kernel / of the one-pass decoder (one block per 64 x 256 workgroup tiles, + the one a full
// last superrow publishes into; the one-pass decoder's workgroup tiles are the shorter ones: 8192 words); second half: tile
// bases, one flag byte per tile, the one-pass decoder's list of deferred tiles (rewritten by every call, no epochs)
DecodeLayout decode_layout(uint64_t c_words, size_t workspace_bytes = 0) {
    DecodeLayout l;
    l.n_tiles = ceil_div(c_words, (uint64_t)wah::kScanTileWords);
    const uint64_t wg_tiles = ceil_div(c_words, (uint64_t)wah::kDecodeTileWords);
    const uint64_t blocks = wg_tiles / wah::kSumScanBlockTiles + 1;
    const size_t scan_need = blocks * wah::kSumScanBlockWords * sizeof(uint32_t);
    const size_t base_bytes = round256((l.n_tiles + 4) * sizeof(uint64_t)); // (+ two words for wah_validate_device)
    const size_t flag_bytes = round256(l.n_tiles + 16);                       // one byte per tile: contains empty fills
    const size_t defer_bytes = round256((size_t)wah::decode_defer_capacity(l.n_tiles, c_words) * 2 * sizeof(uint64_t)); // the list of deferred / shared-out tiles
    const size_t bucket_bytes = round256((l.n_tiles + 1) * 64 * sizeof(uint32_t)); // ... and their sums of group counts per 64 words
    const size_t rest_need = base_bytes + flag_bytes + defer_bytes + bucket_bytes;
    const size_t need_half = round256(scan_need > rest_need ? scan_need : rest_need);
    l.ctrl_off = 0;
    l.desc_off = wah::kCtlWords * sizeof(uint32_t);
    l.total = l.desc_off + 2 * need_half;
    const size_t w = workspace_bytes ? workspace_bytes : l.total;
    l.half = w > l.desc_off ? ((w - l.desc_off) / 2) & ~(size_t)255 : 0;
    l.scan_bytes = l.half; // (the wrap-around clear covers the whole first half, whatever was launched into it)
    l.base_off = l.desc_off + l.half;
    l.flags_off = l.base_off + base_bytes;
    l.defer_off = l.flags_off + flag_bytes; // the list (its counters: kCtlDefer in the control block)
    l.bucket_off = l.defer_off + defer_bytes;
    if (l.half < need_half) l.total = w + 1;
    return l;
}

int status_from_bits(uint32_t err);

// status word of a launch, and optionally `n_vals` 64-bit results of it, in ONE round trip to the device
int read_status(void *d_workspace, void *stream, const uint64_t *d_vals = nullptr, uint64_t *vals = nullptr, int n_vals = 0) {
    uint32_t err = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(&err, static_cast<uint32_t *>(d_workspace) + wah::kCtlError, sizeof err,
                                  hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && n_vals) e = hipMemcpyAsync(vals, d_vals, n_vals * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_err("status read-back", e);
        return WAH_ERR_HIP;
    }
    return status_from_bits(err);
}

int status_from_bits(uint32_t err) {
    if (err & wah::kErrWorkspace) {
        set_err("compress workspace was not initialised (wah_workspace_init_device)");
        return WAH_ERR_WORKSPACE;
    }
    if (err & wah::kErrTimeout) {
        set_err("in-kernel bounded wait expired");
        return WAH_ERR_TIMEOUT;
    }
    if (err & wah::kErrStream) {
        set_err("malformed compressed stream");
        return WAH_ERR_STREAM;
    }
    if (err & wah::kErrCapacity) {
        set_err("output capacity too small");
        return WAH_ERR_CAPACITY;
    }
    return WAH_OK;
}

// The *_status of the indexed calls.  A call whose kernels share the control block at the head of the scratch reads that one; a
// call that ends in the compress passes reads its own block first (what its sweep refused in an operand), then the block of the
// compress workspace at `ws_c`.
int scratch_status(void *d_scratch, void *stream) {
    if (!d_scratch) return WAH_ERR_ARG;
    return read_status(d_scratch, stream);
}
int scratch_status_then(size_t ws_c, void *d_scratch, void *stream) {
    const int rc = scratch_status(d_scratch, stream);
    return rc != WAH_OK ? rc : read_status(static_cast<char *>(d_scratch) + ws_c, stream);
}

// Host-pointer entry points: the results of a launch (kCtlResult) lie beside its error word, so one 32-byte copy into
// page-locked memory + one stream synchronisation is the whole read-back (two pageable copies cost 2 x 15 us more).
int read_status_packed(void *d_workspace, uint32_t *pinned, uint64_t *vals, int n_vals) {
    hipError_t e = hipMemcpyAsync(pinned, static_cast<uint32_t *>(d_workspace) + wah::kCtlError, 8 * sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        set_err("status read-back", e);
        return WAH_ERR_HIP;
    }
    for (int i = 0; i < n_vals; ++i) std::memcpy(&vals[i], pinned + (wah::kCtlResult - wah::kCtlError) + 2 * i, sizeof(uint64_t));
    return status_from_bits(pinned[0]);
}

// ... or without any copy: the last tile of the launch wrote {1 | error bits << 32, results...} into page-locked host
// memory; wait for the stream and read them.  A launch that ended early (unusable workspace) leaves the mark unset.
int wait_host_result(volatile uint64_t *result, void *d_workspace, uint32_t *pinned, uint64_t *vals, int n_vals) {
    const hipError_t e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        set_err("waiting for the device", e);
        return WAH_ERR_HIP;
    }
    if (!(result[0] & 1ull)) return read_status_packed(d_workspace, pinned, vals, n_vals);
    for (int i = 0; i < n_vals; ++i) vals[i] = result[1 + i];
    return status_from_bits((uint32_t)(result[0] >> 32));
}

// Device buffers of the host-pointer entry points.  The reference allocates and frees them inside every call
// (compress.cu:57-114,177-202; decompress.cu:34-54,124-131), which puts hipMalloc/hipFree of up to two bitmap-sized
// buffers -- milliseconds, and cold address translations for the kernels that follow -- into the timings it
// reports.  Here the buffers are kept between calls: grow-only, one set per device, the call holds the set's
// mutex.  wah_host_cache_release() frees them; WAH_HOST_CACHE=0 in the environment restores allocate-and-free.
struct HostCache {
    static constexpr int kSlots = 6;
    std::mutex m;
    void *buf[kSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap[kSlots] = {0, 0, 0, 0, 0, 0};
    int device = -1; // the device the kept buffers live on
    uint32_t *pinned = nullptr; // 64 bytes of page-locked host memory: where status + sizes of a launch land (copied, or
                                // written by the kernel itself: CompressArgs::host_result)
    void release_locked() {
        for (int i = 0; i < kSlots; ++i) {
            if (buf[i]) (void)hipFree(buf[i]);
            buf[i] = nullptr;
            cap[i] = 0;
        }
    }
};
// one set per device: host threads that drive different GPUs (one host thread per GPU) neither
// share a mutex nor evict each other's buffers
constexpr int kMaxDevices = 64;
HostCache &host_cache(int device) {
    static HostCache *c = new HostCache[kMaxDevices]; // never destroyed: the HIP runtime may be gone before static destructors run
    return c[device >= 0 && device < kMaxDevices ? device : 0];
}
int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return dev;
}
bool host_cache_enabled() {
    static const bool on = [] {
        const char *e = std::getenv("WAH_HOST_CACHE");
        return !(e && e[0] == '0');
    }();
    return on;
}

// RAII bundle for the host-pointer paths: owns the timing events and the call's claim on the buffer set
// (or, without the cache, frees whatever was allocated, like the error exits of compress.cu:89-114).
struct HostCall {
    HostCache &cache = host_cache(current_device());
    std::unique_lock<std::mutex> lock{cache.m};
    const bool keep = host_cache_enabled();
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~HostCall() {
        release();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void release() {
        if (!keep) cache.release_locked();
    }
    // slot: which buffer of the set; a kept buffer that is large enough is handed out again as it is
    // (quiet: a failure is the caller's to handle -- no message, no error text)
    bool alloc(int slot, void **p, size_t bytes, const char *what, bool *fresh = nullptr, bool quiet = false) {
        if (bytes == 0) bytes = 16;
        if (fresh) *fresh = false;
        if (cache.buf[slot] && cache.cap[slot] >= bytes) {
            *p = cache.buf[slot];
            return true;
        }
        if (fresh) *fresh = true;
        if (cache.buf[slot]) (void)hipFree(cache.buf[slot]);
        cache.buf[slot] = nullptr;
        cache.cap[slot] = 0;
        hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) {
            if (quiet) {
                (void)hipGetLastError();
                return false;
            }
            set_err(what, e);
            std::fprintf(stderr, "wah: could not allocate %s (%zu bytes): %s\n", what, bytes, hipGetErrorString(e));
            return false;
        }
        cache.buf[slot] = *p;
        cache.cap[slot] = bytes;
        return true;
    }
    bool init() {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        cache.device = dev;
        if (!cache.pinned && hipHostMalloc(reinterpret_cast<void **>(&cache.pinned), 128, hipHostMallocDefault) != hipSuccess) {
            cache.pinned = nullptr;
            return false;
        }
        return hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    }
    void start() { (void)hipEventRecord(ev[0], nullptr); }
    // end of a phase that ends with device work: the event goes into the stream right behind the launch, so that it
    // carries the time at which the device finished, not the time at which the host noticed
    void mark() { (void)hipEventRecord(ev[1], nullptr); }
    float since_mark() {
        float ms = 0.f;
        (void)hipEventSynchronize(ev[1]);
        (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        return ms;
    }
    float stop() {
        float ms = 0.f;
        (void)hipEventRecord(ev[1], nullptr);
        (void)hipEventSynchronize(ev[1]);
        (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        return ms;
    }
};

// Result buffers of the host-pointer paths: free()-compatible like the reference's malloc (compress.cu:177,
// decompress.cu:127), but large ones are 2 MiB aligned and marked for transparent huge pages -- the copy back from the
// device is the first touch of this memory, and with 4 KiB pages its page faults, not PCIe, set the pace.
// *huge: the buffer is backed by huge pages on first touch (what copy_to_fresh_host() needs to know).
bool thp_available() {
    static const bool on = [] {
        char line[128] = "";
        if (FILE *f = std::fopen("/sys/kernel/mm/transparent_hugepage/enabled", "r")) {
            if (!std::fgets(line, sizeof line, f)) line[0] = 0;
            std::fclose(f);
        }
        return line[0] != 0 && std::strstr(line, "[never]") == nullptr;
    }();
    return on;
}
void *host_result_alloc(size_t bytes, bool *huge) {
    constexpr size_t kHuge = size_t(2) << 20;
    *huge = false;
    if (bytes >= 2 * kHuge && thp_available()) {
        const size_t rounded = (bytes + kHuge - 1) & ~(kHuge - 1);
        void *p = std::aligned_alloc(kHuge, rounded);
        if (p) {
            *huge = madvise(p, rounded, MADV_HUGEPAGE) == 0;
            return p;
        }
    }
    return std::malloc(bytes ? bytes : sizeof(uint32_t));
}

// WAH_FAULT_INJECT=timeout (include/wah.h; read per call): the host-pointer entry points treat their first launch as if one
// of its bounded waits had expired, which sends them down the no-wait route -- the only way to see that route taken by
// itself on a healthy GPU.
bool test_timeout_hook() {
    const char *e = std::getenv("WAH_FAULT_INJECT");
    return e && std::strcmp(e, "timeout") == 0;
}

thread_local int g_last_route = wah::kRouteNone; // which decoder the calling thread's last decode call launched
thread_local int g_last_bitop_route = 0;         // ... and which route its last indexed bit operation took (WAH_BITOP_ROUTE_*)

bool hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    set_err(what, e);
    std::fprintf(stderr, "wah: %s failed: %s\n", what, hipGetErrorString(e));
    return false;
}

// Device -> fresh host buffer.  Measured on the box (tools/scratch/d2h_probe.hip, 1 GiB): hipMemcpy into memory that
// has been touched runs at 56 GB/s, into untouched memory at 17-21 GB/s, because the copy takes the page faults one at
// a time.  With huge pages four threads fault 1 GiB in within 11 ms, so they run ahead of the copy, chunk by chunk, and
// the whole transfer reaches 47 GB/s.  (With 4 KiB pages concurrent faults contend and the plain copy is the faster
// one; MADV_POPULATE_WRITE does not scale over threads either.)
bool copy_to_fresh_host(void *host, const void *dev, size_t bytes, bool huge, const char *what) {
    constexpr size_t kChunk = size_t(16) << 20;
    const size_t n_chunks = (bytes + kChunk - 1) / kChunk;
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned n_threads = hw >= 8 ? 4 : hw >= 4 ? 2 : 1;
    if (!huge || n_chunks < 2) return hip_ok(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost), what);

    std::unique_ptr<std::atomic<uint8_t>[]> ready(new std::atomic<uint8_t>[n_chunks]);
    for (size_t i = 0; i < n_chunks; ++i) ready[i].store(0, std::memory_order_relaxed);
    std::atomic<bool> stop{false};
    auto fault_in = [&](unsigned t) {
        for (size_t i = t; i < n_chunks && !stop.load(std::memory_order_relaxed); i += n_threads) {
            volatile char *p = static_cast<char *>(host) + i * kChunk;
            const size_t len = std::min(kChunk, bytes - i * kChunk);
            for (size_t o = 0; o < len; o += 4096) p[o] = 0;
            ready[i].store(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> helpers;
    helpers.reserve(n_threads);
    try {
        for (unsigned t = 0; t < n_threads; ++t) helpers.emplace_back(fault_in, t);
    } catch (...) { // no threads to be had: whoever did start keeps going, the rest of the chunks are touched here
    }
    const unsigned started = (unsigned)helpers.size();
    bool ok = true;
    for (size_t i = 0; i < n_chunks && ok; ++i) {
        if (i % n_threads >= started) { // the helper that owns this chunk does not exist
            volatile char *p = static_cast<char *>(host) + i * kChunk;
            const size_t len = std::min(kChunk, bytes - i * kChunk);
            for (size_t o = 0; o < len; o += 4096) p[o] = 0;
            ready[i].store(1, std::memory_order_release);
        }
        while (!ready[i].load(std::memory_order_acquire)) std::this_thread::yield();
        const size_t len = std::min(kChunk, bytes - i * kChunk);
        ok = hip_ok(hipMemcpy(static_cast<char *>(host) + i * kChunk, static_cast<const char *>(dev) + i * kChunk, len,
                              hipMemcpyDeviceToHost), what);
    }
    stop.store(true, std::memory_order_relaxed);
    for (std::thread &h : helpers) h.join();
    return ok;
}

} // namespace

extern "C" {

const char *wah_last_error(void) { return g_err; }
const char *wah_version(void) { return "wah-mi355x 0.1 gfx950"; }
void wah_free(void *p) { std::free(p); }
void wah_host_cache_release(void) {
    for (int d = 0; d < kMaxDevices; ++d) {
        HostCache &c = host_cache(d);
        std::lock_guard<std::mutex> g(c.m);
        if (c.device < 0) continue; // never used
        int prev = 0;
        const bool switched = hipGetDevice(&prev) == hipSuccess && prev != c.device && hipSetDevice(c.device) == hipSuccess;
        c.release_locked();
        if (switched) (void)hipSetDevice(prev);
    }
}

uint64_t wah_max_compressed_words(uint64_t n_words) { return (32u * n_words + 30u) / 31u; }
uint64_t wah_decoded_words(uint64_t n_groups) { return (31u * n_groups + 31u) / 32u; }

size_t wah_compress_workspace_bytes(uint64_t n_words) { return compress_layout(n_words).total; }
size_t wah_decompress_workspace_bytes(uint64_t c_words, uint64_t out_capacity_words) {
    (void)out_capacity_words; // the workspace depends on the stream length only
    return decode_layout(c_words).total;
}

// clear_first: the caller's workspace is scratch of unknown content (the bitop paths): zero all of it in front of the
// launch, which makes it a fresh workspace every time -- and keep whatever error an upstream pass leaves in it.
static int compress_device_impl(const uint32_t *d_in, const uint32_t *d_in2, int op, const wah::PairCheck *check, uint64_t n_words,
                                uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_segment_offsets,
                                void *d_workspace, size_t workspace_bytes, void *stream, bool clear_first,
                                uint64_t *host_result = nullptr, const wah::BitopOperands *indexed = nullptr, bool unsegmented = false,
                                bool no_wait = false) {
    g_err[0] = 0;
    // WAH_FORCE_FALLBACK=1: every plain compress launch takes the no-wait route (tests; a GPU shared in ways that starve
    // the scan route's waits).  Read per call: it is a switch for a running process too.
    if (!no_wait) {
        const char *f = std::getenv("WAH_FORCE_FALLBACK");
        no_wait = f && f[0] == '1';
    }
    if (!d_out_words || !d_workspace || (n_words && ((!d_in && !indexed) || !d_out))) {
        set_err("null pointer");
        return WAH_ERR_ARG;
    }
    if (n_words >= (1ull << 40) || (reinterpret_cast<uintptr_t>(d_in) & 3u) || (reinterpret_cast<uintptr_t>(d_workspace) & 255u)) {
        set_err("size out of range or misaligned pointer");
        return WAH_ERR_ARG;
    }
    const CompressLayout l = compress_layout(n_words, workspace_bytes);
    if (workspace_bytes < l.total) {
        set_err("workspace too small");
        return WAH_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(d_workspace);
    hipError_t e = hipSuccess;
    if (clear_first) {
        e = wah::launch_clear(ws, l.desc_off + 2 * l.half, s);
        if (e != hipSuccess) {
            set_err("clearing the workspace", e);
            return WAH_ERR_HIP;
        }
    }
    if (n_words == 0) {
        e = wah::launch_clear(d_out_words, sizeof(uint64_t), s);
        if (e == hipSuccess && d_segment_offsets) e = wah::launch_clear(d_segment_offsets, sizeof(uint64_t), s);
        if (e == hipSuccess && !clear_first) e = wah::launch_clear(ws + wah::kCtlError * sizeof(uint32_t), sizeof(uint32_t), s);
        if (e != hipSuccess) {
            set_err("clearing the outputs", e);
            return WAH_ERR_HIP;
        }
        return WAH_OK;
    }
    wah::CompressArgs a{};
    a.in = d_in;
    a.n_words = n_words;
    a.n_segments = (uint32_t)l.n_segments;
    a.n_tiles = (uint32_t)l.n_tiles;
    a.wave_segs = l.wave_segs; // (pair mode: compress_tile_pair_kernel)
    // unsegmented: fills cross the segment cut (compress_unseg_pair_kernel), its own scan area
    a.unseg_desc = unsegmented ? reinterpret_cast<uint32_t *>(ws + l.unseg_off) : nullptr;
    if (no_wait) { // count / scan / place: nobody waits for anybody.  Its own tile shape (two segments per wave; the plain
                   // compress: two pairs); the table of tile counts lies in the workspace's second half
        a.wave_segs = (d_in2 || indexed) ? 2u : wah::compress_nowait_wave_segs(); // (plain and unsegmented: two PAIRS per wave)
        a.n_tiles = (uint32_t)ceil_div(l.n_segments, (uint64_t)wah::kCompressTileWaves * a.wave_segs);
        a.tile_counts = reinterpret_cast<uint64_t *>(ws + l.unseg_off);
    } else if (indexed) { // groups come from two indexed streams (bitop_tile_kernel): its own tile shape
        a.wave_segs = wah::kIndexedSegsPerWave;
        a.n_tiles = (uint32_t)ceil_div(l.n_segments, (uint64_t)wah::kCompressTileWaves * wah::kIndexedSegsPerWave);
    } else if (!d_in2) { // the plain compress and its unsegmented mode: pair-layout kernels, tiles of their own shapes
        const wah::TileShape shape = wah::compress_tile_shape(l.n_segments);
        a.wave_segs = 2 * shape.body_pairs;
        a.tail_pairs = shape.tail_pairs;
        a.big_tiles = shape.big_tiles;
        a.n_tiles = shape.n_tiles;
    }
    a.fast_segments = aligned16(d_in) ? 1u : 0u;
    a.full_segments = (uint32_t)(n_words / wah::kSegWords);
    a.tail_bytes = (uint32_t)(n_words % wah::kSegWords) * 4u;
    a.last_segment_groups = (uint32_t)(l.n_groups - (l.n_segments - 1) * wah::kSegGroups);
    a.out = d_out;
    a.out_capacity = out_capacity_words;
    a.out_words = d_out_words;
    a.seg_offsets = d_segment_offsets;
    a.ctrl = reinterpret_cast<uint32_t *>(ws + l.ctrl_off);
    a.gen_desc = reinterpret_cast<uint32_t *>(ws + l.desc_off);
    a.scan_words = 2 * l.half / sizeof(uint32_t); // both halves (the wrap-around clear covers them, whatever was launched into them)
    a.keep_error = clear_first ? 1 : 0;
    a.host_result = host_result;
#ifdef WAH_DIAG
    {
        static const uint32_t tune = [] { // diagnostic build only: 78 = compress_pair_kernel's per-tile time line (tools/pair_timeline.py)
            const char *e = std::getenv("WAH_TUNE"); // (this block exists in the diagnostic build only)
            return e ? (uint32_t)std::strtoul(e, nullptr, 0) : 0u;
        }();
        a.tune = tune;
    }
#endif
    a.in2 = d_in2;
    a.op = (uint32_t)op;
    if (d_in2) {
        if (!a.fast_segments || !aligned16(d_in2)) {
            set_err("pair mode needs 16-byte aligned bitmaps");
            return WAH_ERR_ARG;
        }
        if (check) e = wah::launch_bitop_check(check->info_a, check->info_b, check->ctrl_a, check->ctrl_b, check->groups, a.ctrl, s);
    }
    if (e == hipSuccess) e = indexed ? wah::launch_bitop_tiles(a, *indexed, s) : no_wait ? wah::launch_compress_nowait(a, s) : wah::launch_compress(a, s);
    if (e != hipSuccess) {
        set_err("compress kernel launch", e);
        return WAH_ERR_HIP;
    }
    return WAH_OK;
}

int wah_workspace_init_device(void *d_workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 255u)) {
        set_err("null or misaligned workspace");
        return WAH_ERR_ARG;
    }
    const hipError_t e = wah::launch_clear(d_workspace, workspace_bytes, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        set_err("clearing the workspace", e);
        return WAH_ERR_HIP;
    }
    return WAH_OK;
}

int wah_compress_device_indexed(const uint32_t *d_in, uint64_t n_words, uint32_t *d_out, uint64_t out_capacity_words,
                                uint64_t *d_out_words, uint64_t *d_segment_offsets, void *d_workspace,
                                size_t workspace_bytes, void *stream) {
    return compress_device_impl(d_in, nullptr, 0, nullptr, n_words, d_out, out_capacity_words, d_out_words, d_segment_offsets,
                                d_workspace, workspace_bytes, stream, false);
}

int wah_compress_device_ex(const uint32_t *d_in, uint64_t n_words, uint32_t *d_out, uint64_t out_capacity_words,
                           uint64_t *d_out_words, unsigned flags, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (flags & ~(unsigned)(WAH_UNSEGMENTED | WAH_NO_WAIT)) {
        g_err[0] = 0;
        set_err("unknown flag");
        return WAH_ERR_ARG;
    }
    return compress_device_impl(d_in, nullptr, 0, nullptr, n_words, d_out, out_capacity_words, d_out_words, nullptr, d_workspace,
                                workspace_bytes, stream, false, nullptr, nullptr, (flags & WAH_UNSEGMENTED) != 0, (flags & WAH_NO_WAIT) != 0);
}

int wah_compress_device(const uint32_t *d_in, uint64_t n_words, uint32_t *d_out, uint64_t out_capacity_words,
                        uint64_t *d_out_words, void *d_workspace, size_t workspace_bytes, void *stream) {
    return wah_compress_device_indexed(d_in, n_words, d_out, out_capacity_words, d_out_words, nullptr, d_workspace,
                                       workspace_bytes, stream);
}

int wah_compress_status(void *d_workspace, void *stream) { return read_status(d_workspace, stream); }

// One host thread per shard: its device made current, a stream of its own, one launch over the shard's column matrix, the
// status read back.  Nothing crosses between the threads but the join (columns are unrelated bitmaps).
int wah_compress_columns_multi_device(int n_shards, const wah_column_shard *shards, uint64_t n_words_per_column, int *status) {
    g_err[0] = 0;
    if (n_shards < 0 || (n_shards > 0 && !shards)) {
        set_err("null shard list");
        return WAH_ERR_ARG;
    }
    if (n_words_per_column % WAH_SEGMENT_WORDS != 0) {
        set_err("columns of a shard must be whole 992-word segments (a fill must not cross into the next column)");
        return WAH_ERR_ARG;
    }
    std::vector<int> rc((size_t)n_shards, WAH_OK);
    std::vector<std::string> msg((size_t)n_shards);
    auto work = [&](int i) {
        const wah_column_shard &sh = shards[i];
        hipStream_t s = nullptr;
        if (hipSetDevice(sh.device) != hipSuccess || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
            rc[i] = WAH_ERR_HIP;
            msg[i] = "could not make the shard's device current / create its stream";
            return;
        }
        rc[i] = wah_compress_device_indexed(sh.d_in, sh.n_columns * n_words_per_column, sh.d_out, sh.out_capacity_words, sh.d_out_words,
                                            sh.d_segment_offsets, sh.d_workspace, sh.workspace_bytes, s);
        if (rc[i] == WAH_OK) rc[i] = wah_compress_status(sh.d_workspace, s); // (synchronises the shard's stream)
        if (rc[i] != WAH_OK) msg[i] = g_err; // (this thread's own error text)
        (void)hipStreamDestroy(s);
    };
    std::vector<std::thread> threads;
    threads.reserve((size_t)n_shards);
    for (int i = 0; i < n_shards; ++i) {
        try {
            threads.emplace_back(work, i);
        } catch (...) { // no thread to be had: this shard on the caller's thread
            int prev = 0;
            const bool have_prev = hipGetDevice(&prev) == hipSuccess;
            work(i);
            if (have_prev) (void)hipSetDevice(prev);
        }
    }
    for (std::thread &t : threads) t.join();
    int first = WAH_OK;
    for (int i = 0; i < n_shards; ++i) {
        if (status) status[i] = rc[i];
        if (first == WAH_OK && rc[i] != WAH_OK) {
            first = rc[i];
            set_err(msg[i].c_str());
        }
    }
    return first;
}
int wah_decompress_status(void *d_workspace, void *stream) { return read_status(d_workspace, stream); }

// clear_first: the workspace is scratch of unknown content (the bitop paths): zero its control block and scan area in
// front of the launch, which makes it a fresh workspace every time.
static int decode_common(const uint32_t *d_comp, uint64_t c_words, uint32_t *d_out, uint64_t out_capacity_words,
                         uint64_t *d_out_info, void *d_workspace, size_t workspace_bytes, void *stream, bool do_scan,
                         bool do_expand, bool clear_first = false, uint64_t *host_result = nullptr, bool no_wait = false,
                         int route = 0 /* 0: by the rule below, 1: one pass, 2: two launches */) {
    g_err[0] = 0;
    g_last_route = wah::kRouteNone;
    // WAH_FORCE_FALLBACK=1: every sums pass takes the no-wait route (tests; a GPU shared in ways that starve the scan
    // route's waits).  Read per call: it is a switch for a running process too.
    if (!no_wait && do_scan) {
        const char *f = std::getenv("WAH_FORCE_FALLBACK");
        no_wait = f && f[0] == '1';
    }
    if (!d_out_info || !d_workspace || (c_words && !d_comp) || (do_expand && out_capacity_words && !d_out)) {
        set_err("null pointer");
        return WAH_ERR_ARG;
    }
    if (c_words >= (1ull << 40) || (reinterpret_cast<uintptr_t>(d_comp) & 3u) || (reinterpret_cast<uintptr_t>(d_workspace) & 255u)) {
        set_err("size out of range or misaligned pointer");
        return WAH_ERR_ARG;
    }
    const DecodeLayout l = decode_layout(c_words, workspace_bytes);
    if (workspace_bytes < l.total) {
        set_err("workspace too small");
        return WAH_ERR_WORKSPACE;
    }
    if (l.n_tiles >= (1ull << 31)) {
        set_err("stream too long");
        return WAH_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(d_workspace);
    hipError_t e = hipSuccess;
    // ONE pass over the stream (decode_tile_kernel + the launch over its list) is CORRECT for every 16-byte aligned stream: the
    // kernel decides tile by tile, from the tile's own words, whether it expands the tile itself (up to about 7 groups per word)
    // or puts it on the list that the launch behind it shares out over work items.  It is also the FASTER route for streams of
    // up to 7 groups per word (by 13-19 % against the two launches, which read the stream twice), as fast within 1.5 % from about
    // 32 groups per word on (every tile on the list: the list's launch is the expand kernel) and 3-6 % faster from about 200; in
    // between -- 8 to 30 groups per word -- the two launches win by about 20 % (tools/decode_density_time.py, 992 MiB, one bit in
    // 2^9: 0.338 ms against 0.282, 2^10: 0.280 / 0.243 -- a stream of 60-130 MB is 2000-4000 workgroups of the tile kernel, whose
    // tickets and list entries come out of one address each at 86 per microsecond: 98 us where the sums kernel takes 41).  The library cannot look at the stream without a pass over it, so the default goes by what the
    // CAPACITY allows the stream to be: at most 7 words of output per word of stream, or more than 40 -- one pass; between --
    // the two launches.  A caller who knows better says so (WAH_ONE_PASS / WAH_TWO_LAUNCHES); decompress(), which has the stream
    // in host memory, samples it and does.
    // (7 words of output per word of stream: the tile kernel expands up to 7.5 groups = 7.27 words per word itself)
    const bool prefer_one_pass = route == 1 || (route == 0 && (out_capacity_words <= 7 * c_words || out_capacity_words > 40 * c_words));
    const bool one_pass = do_scan && do_expand && !no_wait && prefer_one_pass && c_words != 0 && aligned16(d_comp);
    if (do_expand || do_scan) g_last_route = one_pass ? wah::kRouteOnePass : no_wait ? wah::kRouteNoWait : wah::kRouteTwoLaunches;
    if (one_pass) {
        if (clear_first) e = wah::launch_clear(ws, l.base_off, s); // (control block -- with the deferred tiles' counters -- and scan area)
        if (e != hipSuccess) {
            set_err("clearing the workspace", e);
            return WAH_ERR_HIP;
        }
        wah::ScanArgs a{};
        a.comp = d_comp;
        a.c_words = c_words;
        a.n_tiles = l.n_tiles;
        a.info = d_out_info;
        a.tile_base = reinterpret_cast<uint64_t *>(ws + l.base_off);
        a.ctrl = reinterpret_cast<uint32_t *>(ws + l.ctrl_off);
        a.gen_desc = reinterpret_cast<uint32_t *>(ws + l.desc_off);
        a.scan_words = l.scan_bytes / sizeof(uint32_t);
        a.tile_flags = reinterpret_cast<uint8_t *>(ws + l.flags_off);
        a.aligned16 = 1;
        a.host_result = host_result;
        a.no_wait = 0;
        wah::ExpandArgs x{};
        x.comp = d_comp;
        x.c_words = c_words;
        x.out = d_out;
        x.out_capacity = out_capacity_words;
        x.info = d_out_info;
        x.tile_base = a.tile_base;
        x.tile_flags = a.tile_flags;
        x.ctrl = a.ctrl;
        x.aligned16 = 1;
        x.parts = 1;
        x.tile_buckets = reinterpret_cast<const uint32_t *>(ws + l.bucket_off);
        e = wah::launch_decode_tiles(a, x, reinterpret_cast<uint64_t *>(ws + l.defer_off), s);
        if (e != hipSuccess) {
            set_err("decode tile kernel launch", e);
            return WAH_ERR_HIP;
        }
        return WAH_OK;
    }
    if (do_scan) {
        if (clear_first) e = wah::launch_clear(ws, l.base_off, s);
        if (e == hipSuccess && c_words == 0) {
            e = wah::launch_clear(d_out_info, 2 * sizeof(uint64_t), s);
            if (e == hipSuccess && !clear_first) e = wah::launch_clear(ws + wah::kCtlError * sizeof(uint32_t), sizeof(uint32_t), s);
        }
        if (e != hipSuccess) {
            set_err("clearing the workspace", e);
            return WAH_ERR_HIP;
        }
        if (c_words) {
            wah::ScanArgs a{};
            a.comp = d_comp;
            a.c_words = c_words;
            a.n_tiles = l.n_tiles;
            a.info = d_out_info;
            a.tile_base = reinterpret_cast<uint64_t *>(ws + l.base_off);
            a.ctrl = reinterpret_cast<uint32_t *>(ws + l.ctrl_off);
            a.gen_desc = reinterpret_cast<uint32_t *>(ws + l.desc_off);
            a.scan_words = l.scan_bytes / sizeof(uint32_t);
            a.tile_flags = reinterpret_cast<uint8_t *>(ws + l.flags_off);
            a.aligned16 = aligned16(d_comp) ? 1 : 0;
            a.host_result = host_result;
            a.no_wait = no_wait ? 1 : 0;
            a.defer_list = reinterpret_cast<uint64_t *>(ws + l.defer_off);
            a.defer_capacity = wah::decode_defer_capacity(l.n_tiles, c_words);
            e = wah::launch_decode_sums(a, s);
            if (e != hipSuccess) {
                set_err("decode sums kernel launch", e);
                return WAH_ERR_HIP;
            }
        }
    }
    if (c_words == 0) return WAH_OK;
    if (do_expand) {
        wah::ExpandArgs x{};
        x.comp = d_comp;
        x.c_words = c_words;
        x.out = d_out;
        x.out_capacity = out_capacity_words;
        x.info = d_out_info;
        x.tile_base = reinterpret_cast<const uint64_t *>(ws + l.base_off);
        x.tile_flags = reinterpret_cast<const uint8_t *>(ws + l.flags_off);
        x.ctrl = reinterpret_cast<uint32_t *>(ws + l.ctrl_off);
        x.aligned16 = aligned16(d_comp) ? 1 : 0;
        x.parts = 1; // the launcher decides
        x.defer_list = reinterpret_cast<const uint64_t *>(ws + l.defer_off);
        x.defer_count = reinterpret_cast<const uint32_t *>(ws + l.ctrl_off) + wah::kCtlDefer;
        x.defer_capacity = wah::decode_defer_capacity(l.n_tiles, c_words);
        e = wah::launch_decode_expand(x, l.n_tiles, s);
        if (e != hipSuccess) {
            set_err("decode expand kernel launch", e);
            return WAH_ERR_HIP;
        }
    }
    return WAH_OK;
}

int wah_decompress_device(const uint32_t *d_comp, uint64_t c_words, uint32_t *d_out, uint64_t out_capacity_words,
                          uint64_t *d_out_info, void *d_workspace, size_t workspace_bytes, void *stream) {
    return decode_common(d_comp, c_words, d_out, out_capacity_words, d_out_info, d_workspace, workspace_bytes, stream,
                         true, true);
}

int wah_decompress_device_ex(const uint32_t *d_comp, uint64_t c_words, uint32_t *d_out, uint64_t out_capacity_words,
                             uint64_t *d_out_info, unsigned flags, void *d_workspace, size_t workspace_bytes, void *stream) {
    if ((flags & ~(unsigned)(WAH_NO_WAIT | WAH_TWO_LAUNCHES | WAH_ONE_PASS)) || ((flags & WAH_TWO_LAUNCHES) && (flags & WAH_ONE_PASS))) {
        g_err[0] = 0;
        set_err("unknown flag, or both WAH_ONE_PASS and WAH_TWO_LAUNCHES");
        return WAH_ERR_ARG;
    }
    return decode_common(d_comp, c_words, d_out, out_capacity_words, d_out_info, d_workspace, workspace_bytes, stream,
                         true, true, false, nullptr, (flags & WAH_NO_WAIT) != 0, (flags & WAH_ONE_PASS) ? 1 : (flags & WAH_TWO_LAUNCHES) ? 2 : 0);
}

int wah_last_decode_route(void) { return g_last_route; }
int wah_last_bitop_route(void) { return g_last_bitop_route; }

int wah_decompress_scan_device(const uint32_t *d_comp, uint64_t c_words, uint64_t *d_out_info, void *d_workspace,
                               size_t workspace_bytes, void *stream) {
    return decode_common(d_comp, c_words, nullptr, 0, d_out_info, d_workspace, workspace_bytes, stream, true, false);
}

int wah_decompress_expand_device(const uint32_t *d_comp, uint64_t c_words, uint32_t *d_out,
                                 uint64_t out_capacity_words, uint64_t *d_out_info, void *d_workspace,
                                 size_t workspace_bytes, void *stream) {
    return decode_common(d_comp, c_words, d_out, out_capacity_words, d_out_info, d_workspace, workspace_bytes, stream,
                         false, true);
}

int wah_validate_device(const uint32_t *d_comp, uint64_t c_words, uint64_t *d_report, void *d_workspace,
                        size_t workspace_bytes, void *stream) {
    if (!d_report) {
        g_err[0] = 0;
        set_err("null pointer");
        return WAH_ERR_ARG;
    }
    // the sums pass gives the tile bases and the totals ([words, groups] land in d_report[0..1] for a moment)
    const int rc = decode_common(d_comp, c_words, nullptr, 0, d_report, d_workspace, workspace_bytes, stream, true, false);
    if (rc != WAH_OK) return rc;
    const DecodeLayout l = decode_layout(c_words, workspace_bytes);
    char *ws = static_cast<char *>(d_workspace);
    // keep the totals aside (behind the tile bases), then build the report
    uint64_t *info = reinterpret_cast<uint64_t *>(ws + l.base_off) + (l.n_tiles + 1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(info, d_report, 2 * sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess)
        e = wah::launch_validate(d_comp, c_words, reinterpret_cast<const uint64_t *>(ws + l.base_off), info, d_report, l.n_tiles, s);
    if (e != hipSuccess) {
        set_err("validate kernel launch", e);
        return WAH_ERR_HIP;
    }
    return WAH_OK;
}

int wah_build_index_device(const uint32_t *d_comp, uint64_t c_words, uint64_t *d_segment_offsets, uint64_t offsets_capacity,
                           uint64_t *d_out_info, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (!d_segment_offsets || !d_out_info || offsets_capacity == 0) {
        g_err[0] = 0;
        set_err("null pointer or empty index");
        return WAH_ERR_ARG;
    }
    // the sums pass: tile bases in the workspace, [decoded words, groups] in d_out_info
    const int rc = decode_common(d_comp, c_words, nullptr, 0, d_out_info, d_workspace, workspace_bytes, stream, true, false);
    if (rc != WAH_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (c_words == 0) { // no groups, no segments: the index is the single entry 0
        const hipError_t e = wah::launch_clear(d_segment_offsets, sizeof(uint64_t), s);
        if (e != hipSuccess) {
            set_err("clearing the index", e);
            return WAH_ERR_HIP;
        }
        return WAH_OK;
    }
    const DecodeLayout l = decode_layout(c_words, workspace_bytes);
    char *ws = static_cast<char *>(d_workspace);
    const hipError_t e = wah::launch_build_index(d_comp, c_words, reinterpret_cast<const uint64_t *>(ws + l.base_off), d_out_info,
                                                 d_segment_offsets, offsets_capacity, reinterpret_cast<uint32_t *>(ws + l.ctrl_off),
                                                 l.n_tiles, s);
    if (e != hipSuccess) {
        set_err("index kernel launch", e);
        return WAH_ERR_HIP;
    }
    return WAH_OK;
}

// ---- merged (unsegmented) form -------------------------------------------------------------------------------
namespace {
struct MergeLayout {
    size_t decode_bytes, kept_off, pos_off, info_off, total;
};
MergeLayout merge_layout(uint64_t c_words) {
    MergeLayout l;
    const DecodeLayout d = decode_layout(c_words);
    l.decode_bytes = round256(d.total);
    l.kept_off = l.decode_bytes;
    l.info_off = round256(l.kept_off + (d.n_tiles + 2) * sizeof(uint64_t));
    l.pos_off = l.info_off + 256;
    l.total = round256(l.pos_off + (d.n_tiles + 2) * sizeof(uint64_t)); // (one position per TILE: round 3 kept one per word)
    return l;
}
} // namespace

size_t wah_merge_fills_workspace_bytes(uint64_t c_words) { return merge_layout(c_words).total; }

int wah_merge_fills_device(const uint32_t *d_comp, uint64_t c_words, uint32_t *d_out, uint64_t out_capacity_words,
                           uint64_t *d_out_words, void *d_workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (!d_out_words || !d_workspace || (c_words && (!d_comp || !d_out))) {
        set_err("null pointer");
        return WAH_ERR_ARG;
    }
    const MergeLayout l = merge_layout(c_words);
    if (workspace_bytes < l.total) {
        set_err("workspace too small");
        return WAH_ERR_WORKSPACE;
    }
    char *ws = static_cast<char *>(d_workspace);
    uint64_t *info = reinterpret_cast<uint64_t *>(ws + l.info_off);
    // sums pass: tile bases and totals
    const int rc = decode_common(d_comp, c_words, nullptr, 0, info, d_workspace, l.decode_bytes, stream, true, false);
    if (rc != WAH_OK) return rc;
    const DecodeLayout d = decode_layout(c_words, l.decode_bytes);
    wah::MergeArgs a;
    a.comp = d_comp;
    a.c_words = c_words;
    a.n_tiles = d.n_tiles;
    a.tile_base = reinterpret_cast<const uint64_t *>(ws + d.base_off);
    a.info = info;
    a.tile_kept = reinterpret_cast<uint64_t *>(ws + l.kept_off);
    a.tile_first = reinterpret_cast<uint64_t *>(ws + l.pos_off);
    a.out = d_out;
    a.out_capacity = out_capacity_words;
    a.out_words = d_out_words;
    a.ctrl = reinterpret_cast<uint32_t *>(ws + d.ctrl_off);
    const hipError_t e = wah::launch_merge_fills(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        set_err("merge kernels launch", e);
        return WAH_ERR_HIP;
    }
    return WAH_OK;
}

// ---- bitwise operations on two compressed bitmaps -------------------------------------------------------------
namespace {
struct BitopLayout {
    size_t bitmap_a, bitmap_b, info_a, info_b, ws_a, ws_b, ws_c, total;
    size_t ws_a_bytes, ws_b_bytes, ws_c_bytes;
    uint64_t decoded_capacity;
};
BitopLayout bitop_layout(uint64_t n_words, uint64_t a_words, uint64_t b_words) {
    BitopLayout l;
    l.decoded_capacity = n_words + 1; // ceil(31 G / 32) is n_words or n_words + 1
    const size_t bm = round256(l.decoded_capacity * sizeof(uint32_t));
    l.ws_a_bytes = wah_decompress_workspace_bytes(a_words, l.decoded_capacity);
    l.ws_b_bytes = wah_decompress_workspace_bytes(b_words, l.decoded_capacity);
    l.ws_c_bytes = wah_compress_workspace_bytes(n_words);
    l.bitmap_a = 0;
    l.bitmap_b = bm;
    l.info_a = 2 * bm;
    l.info_b = l.info_a + 256;
    l.ws_a = l.info_b + 256;
    l.ws_b = l.ws_a + round256(l.ws_a_bytes);
    l.ws_c = l.ws_b + round256(l.ws_b_bytes);
    l.total = l.ws_c + round256(l.ws_c_bytes);
    return l;
}
} // namespace

size_t wah_bitop_scratch_bytes(uint64_t n_words, uint64_t a_words, uint64_t b_words) {
    return bitop_layout(n_words, a_words, b_words).total;
}

int wah_bitop_device(int op, uint64_t n_words, const uint32_t *d_a, uint64_t a_words, const uint32_t *d_b,
                     uint64_t b_words, uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words,
                     void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (op < WAH_OP_AND || op > WAH_OP_ANDNOT || !d_scratch || (reinterpret_cast<uintptr_t>(d_scratch) & 255u)) {
        set_err("bad operation or scratch pointer");
        return WAH_ERR_ARG;
    }
    const BitopLayout l = bitop_layout(n_words, a_words, b_words);
    if (scratch_bytes < l.total) {
        set_err("scratch too small");
        return WAH_ERR_WORKSPACE;
    }
    char *sc = static_cast<char *>(d_scratch);
    uint32_t *bm_a = reinterpret_cast<uint32_t *>(sc + l.bitmap_a), *bm_b = reinterpret_cast<uint32_t *>(sc + l.bitmap_b);
    uint64_t *info_a = reinterpret_cast<uint64_t *>(sc + l.info_a), *info_b = reinterpret_cast<uint64_t *>(sc + l.info_b);
    // (the decode workspaces inside the caller's scratch are cleared in front of every use: scratch needs no initialisation)
    int rc = decode_common(d_a, a_words, bm_a, l.decoded_capacity, info_a, sc + l.ws_a, l.ws_a_bytes, stream, true, true, true);
    if (rc == WAH_OK) rc = decode_common(d_b, b_words, bm_b, l.decoded_capacity, info_b, sc + l.ws_b, l.ws_b_bytes, stream, true, true, true);
    if (rc != WAH_OK) return rc;
    wah::PairCheck check;
    check.info_a = info_a;
    check.info_b = info_b;
    check.ctrl_a = reinterpret_cast<const uint32_t *>(sc + l.ws_a);
    check.ctrl_b = reinterpret_cast<const uint32_t *>(sc + l.ws_b);
    check.groups = wah_max_compressed_words(n_words);
    return compress_device_impl(bm_a, bm_b, op, &check, n_words, d_out, out_capacity_words, d_out_words, nullptr, sc + l.ws_c,
                                l.ws_c_bytes, stream, true);
}

int wah_bitop_status(void *d_scratch, uint64_t n_words, uint64_t a_words, uint64_t b_words, void *stream) {
    if (!d_scratch) return WAH_ERR_ARG;
    return read_status(static_cast<char *>(d_scratch) + bitop_layout(n_words, a_words, b_words).ws_c, stream);
}

int wah_gen_uniform_device(uint32_t *d_out, uint64_t n_words, uint64_t seed, uint64_t threshold, void *stream) {
    hipError_t e = wah::launch_gen_uniform(d_out, n_words, seed, threshold, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        set_err("generator launch", e);
        return WAH_ERR_HIP;
    }
    return WAH_OK;
}

int wah_gen_clustered_device(uint32_t *d_out, uint64_t n_words, uint64_t seed, uint64_t threshold, void *stream) {
    hipError_t e = wah::launch_gen_clustered(d_out, n_words, seed, threshold, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        set_err("generator launch", e);
        return WAH_ERR_HIP;
    }
    return WAH_OK;
}

int wah_copy_device(const uint32_t *d_in, uint32_t *d_out, uint64_t n_words, void *stream) {
    hipError_t e = wah::launch_copy(d_in, d_out, n_words, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        set_err("copy launch", e);
        return WAH_ERR_HIP;
    }
    return WAH_OK;
}

size_t wah_decompress_segments_workspace_bytes(void) { return round256(wah::kCtlWords * sizeof(uint32_t)); }

int wah_decompress_segments_device(const uint32_t *d_comp, uint64_t c_words, const uint64_t *d_segment_offsets, uint64_t n_words,
                                   uint64_t first_segment, uint64_t n_segments, uint32_t *d_out, uint64_t out_capacity_words,
                                   void *d_workspace, size_t workspace_bytes, void *stream) {
    g_err[0] = 0;
    if (!d_workspace || !d_segment_offsets || (c_words && !d_comp) || (n_segments && !d_out)) {
        set_err("null pointer");
        return WAH_ERR_ARG;
    }
    if (n_words >= (1ull << 40) || c_words >= (1ull << 40) || (reinterpret_cast<uintptr_t>(d_comp) & 3u) ||
        (reinterpret_cast<uintptr_t>(d_out) & 3u) || (reinterpret_cast<uintptr_t>(d_workspace) & 255u)) {
        set_err("size out of range or misaligned pointer");
        return WAH_ERR_ARG;
    }
    if (workspace_bytes < wah_decompress_segments_workspace_bytes()) {
        set_err("workspace too small");
        return WAH_ERR_WORKSPACE;
    }
    const uint64_t groups = seg_geometry(n_words).groups, all_segments = seg_geometry(n_words).n_segments; // G = ceil(32 n / 31)
    if (first_segment > all_segments || n_segments > all_segments - first_segment) {
        set_err("segment range outside the bitmap");
        return WAH_ERR_ARG;
    }
    const uint64_t out_words = wah_decoded_words(groups);
    const uint64_t range_end = (first_segment + n_segments) * wah::kSegWords < out_words ? (first_segment + n_segments) * wah::kSegWords : out_words;
    const uint64_t needed = n_segments ? range_end - first_segment * wah::kSegWords : 0;
    if (needed > out_capacity_words) {
        set_err("output capacity too small");
        return WAH_ERR_CAPACITY;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = wah::launch_clear(d_workspace, wah::kCtlWords * sizeof(uint32_t), s);
    if (e == hipSuccess) {
        wah::SegmentsArgs a = {};
        a.comp = d_comp;
        a.c_words = c_words;
        a.seg_offsets = d_segment_offsets;
        a.first_segment = first_segment;
        a.n_segments = n_segments;
        a.groups = groups;
        a.out_words = out_words;
        a.out = d_out;
        a.ctrl = static_cast<uint32_t *>(d_workspace);
        e = wah::launch_decode_segments(a, s);
    }
    if (e != hipSuccess) {
        set_err("segment decode launch", e);
        return WAH_ERR_HIP;
    }
    return WAH_OK;
}

namespace {
// scratch of wah_bitop_indexed_device: [control block of the combining pass][combined decoded bitmap][compress workspace]
constexpr uint64_t kRunsMaxWordsPerSeg = 112; // (bitop_runs_route below)
// (on the run-merge route the bitmap area holds the result's words per segment and per tile of segments instead)
struct BitopIndexedLayout {
    size_t bitmap, ws_c, total;
    size_t ws_c_bytes;
    uint64_t decoded_capacity;
    size_t runs_tiles, runs_temp; // run-merge route: the tile totals and the temporary, behind the segment counts at `bitmap`
};
BitopIndexedLayout bitop_indexed_layout(uint64_t n_words) {
    BitopIndexedLayout l;
    l.decoded_capacity = n_words + 1; // ceil(31 G / 32) is n_words or n_words + 1
    l.ws_c_bytes = wah_compress_workspace_bytes(n_words);
    l.bitmap = round256(wah::kCtlWords * sizeof(uint32_t));
    const uint64_t n_segments = seg_geometry(n_words).n_segments;
    l.runs_tiles = l.bitmap + round256(n_segments * sizeof(uint32_t));
    l.runs_temp = l.runs_tiles + round256((n_segments / 64 + 2) * sizeof(uint64_t));
    const size_t runs_end = l.runs_temp + round256((kRunsMaxWordsPerSeg * n_segments + 16) * sizeof(uint32_t));
    const size_t bitmap_end = l.bitmap + round256(l.decoded_capacity * sizeof(uint32_t));
    l.ws_c = runs_end > bitmap_end ? runs_end : bitmap_end;
    l.total = l.ws_c + round256(l.ws_c_bytes);
    return l;
}

// The run-merge route (wah_bitop_runs.hip) for operands of few words per segment: all operands together at most
// kRunsMaxWordsPerSeg words per segment on average -- the decode-based routes cost the same whatever the operands hold
// (about 0.25 ms per operand + 0.2 ms on a 1 GiB bitmap), a merge costs by the word (tools/bitop_density_time.py: two operands
// of 33 words per segment together 0.09 ms against 0.52, 63: 0.17, 122: 0.49-0.65 against 0.50-0.55; eight of 131 together:
// 1.1-1.3 against 1.6, of 250: 7.4).  false: not taken (the caller goes on with its own route); rc: what the call returns when taken.
bool bitop_runs_route(int op, uint64_t n_words, int n, const uint32_t *const *comp, const uint64_t *c_words, const uint64_t *const *offs,
                      uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, char *sc,
                      const BitopIndexedLayout &l, hipStream_t s, int *rc) {
    const SegGeometry g = seg_geometry(n_words);
    uint64_t total = 0;
    for (int j = 0; j < n; ++j) total += c_words[j];
    g_last_bitop_route = WAH_BITOP_ROUTE_GROUPS;
    const char *force = wah::experiment_env("WAH_BITOP_ROUTE"); // (experiment builds: "runs" / "groups", tools/bitop_density_time.py)
    const uint64_t temp_words = (l.ws_c - l.runs_temp) / sizeof(uint32_t);
    if (n_words == 0 || total + 16 > temp_words || (force ? force[0] != 'r' : total > kRunsMaxWordsPerSeg * g.n_segments)) return false;
    g_last_bitop_route = WAH_BITOP_ROUTE_RUNS;
    if (!d_out_words || !d_out) {
        *rc = refuse("null pointer", WAH_ERR_ARG);
        return true;
    }
    wah::BitopRunsArgs a = {};
    for (int j = 0; j < n; ++j) {
        a.comp[j] = comp[j];
        a.c_words[j] = c_words[j];
        a.offs[j] = offs[j];
    }
    a.n = n;
    a.op = op;
    a.groups = g.groups;
    a.n_segments = g.n_segments;
    a.seg_count = reinterpret_cast<uint32_t *>(sc + l.bitmap);
    a.tile_total = reinterpret_cast<uint64_t *>(sc + l.runs_tiles);
    a.temp = reinterpret_cast<uint32_t *>(sc + l.runs_temp);
    a.out = d_out;
    a.out_capacity = out_capacity_words;
    a.out_words = d_out_words;
    a.out_offsets = d_out_offsets;
    a.ctrl = reinterpret_cast<uint32_t *>(sc);
    // (both control blocks wah_bitop_indexed_status reads: this route's, and the compress workspace's, which it does not use)
    hipError_t e = wah::launch_clear(sc, wah::kCtlWords * sizeof(uint32_t), s);
    if (e == hipSuccess) e = wah::launch_clear(sc + l.ws_c, wah::kCtlWords * sizeof(uint32_t), s);
    if (e == hipSuccess) e = wah::launch_bitop_runs(a, s);
    *rc = e == hipSuccess ? WAH_OK : refuse("run-merge launch", WAH_ERR_HIP, e);
    return true;
}

// The road of every call that ends in the compress passes: the control words at the head of the scratch cleared (the call's
// *_status reads them), ONE kernel `launch` that writes decoded words into an area of the scratch, the compress passes over the
// `n_words` words at `decoded` with the workspace at `ws_c`.  One bitmap (combine_then_compress) or a matrix of slices
// (sweep_then_compress, further down): the compress passes take either.
extern "C++" template <class Args, class Launch>
int launch_then_compress(const Args &a, Launch launch, const char *label, const uint32_t *decoded, uint64_t n_words, uint32_t *d_out,
                         uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, char *sc, size_t ws_c,
                         size_t ws_c_bytes, void *stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = wah::launch_clear(sc, wah::kCtlWords * sizeof(uint32_t), s);
    if (e == hipSuccess) e = launch(a, s);
    if (e != hipSuccess) return refuse(label, WAH_ERR_HIP, e);
    return compress_device_impl(decoded, nullptr, 0, nullptr, n_words, d_out, out_capacity_words, d_out_words, d_out_offsets, sc + ws_c,
                                ws_c_bytes, stream, true);
}

// The calls that combine indexed operands into ONE decoded bitmap: the combining kernel runs over every segment into the scratch's
// bitmap area.  a: the kernel's arguments, its geometry a.g filled in here.  The bitmap area takes ceil(31 G / 32) words: n_words, or
// n_words + 1 when the last group has spare bits -- a negated clause, or a range with lo == 0, sets them, and they land in that
// one word more, which the area has room for and the compress passes, told n_words, never read.
extern "C++" template <class Args, class Launch>
int combine_then_compress(Args &a, Launch launch, const char *label, uint64_t n_words, uint32_t *d_out, uint64_t out_capacity_words,
                          uint64_t *d_out_words, uint64_t *d_out_offsets, char *sc, const BitopIndexedLayout &l, void *stream) {
    const SegGeometry g = seg_geometry(n_words);
    a.g.first_segment = 0;
    a.g.n_segments = g.n_segments;
    a.g.groups = g.groups;
    a.g.out_words = wah_decoded_words(g.groups);
    a.g.out = reinterpret_cast<uint32_t *>(sc + l.bitmap);
    a.g.ctrl = reinterpret_cast<uint32_t *>(sc);
    return launch_then_compress(a, launch, label, a.g.out, n_words, d_out, out_capacity_words, d_out_words, d_out_offsets, sc, l.ws_c,
                                l.ws_c_bytes, stream);
}

// The bits of `flags` that say which of two attributes comes with an existence bitmap, as the sweeps' arguments hold them
extern "C++" template <class Args>
void set_exists(Args &a, unsigned flags) {
    a.exists_a = (flags & WAH_BSI_EXISTS_A) ? 1u : 0u;
    a.exists_b = (flags & WAH_BSI_EXISTS_B) ? 1u : 0u;
}

// What the arguments of every kernel that walks whole bitmaps segment by segment hold: the bitmap's geometry and the control words
extern "C++" template <class Args>
void set_walk(Args &a, const SegGeometry &g, char *sc) {
    a.pad_bits = g.pad_bits;
    a.groups = g.groups;
    a.n_segments = g.n_segments;
    a.ctrl = reinterpret_cast<uint32_t *>(sc);
}
} // namespace

size_t wah_bitop_indexed_scratch_bytes(uint64_t n_words) { return bitop_indexed_layout(n_words).total; }

int wah_bitop_indexed_device(int op, uint64_t n_words, const uint32_t *d_a, uint64_t a_words, const uint64_t *d_a_offsets,
                             const uint32_t *d_b, uint64_t b_words, const uint64_t *d_b_offsets, uint32_t *d_out,
                             uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                             size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (op < WAH_OP_AND || op > WAH_OP_ANDNOT || !scratch_ok(d_scratch)) return refuse("bad operation or scratch pointer", WAH_ERR_ARG);
    if (!d_a_offsets || !d_b_offsets || (a_words && !d_a) || (b_words && !d_b) || n_words >= (1ull << 40) ||
        a_words >= (1ull << 40) || b_words >= (1ull << 40) || !aligned(d_a, 3) || !aligned(d_b, 3))
        return refuse("null or misaligned operand", WAH_ERR_ARG);
    const BitopIndexedLayout l = bitop_indexed_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    hipStream_t s = static_cast<hipStream_t>(stream);
    {
        const uint32_t *const comp[2] = {d_a, d_b};
        const uint64_t words[2] = {a_words, b_words};
        const uint64_t *const offs[2] = {d_a_offsets, d_b_offsets};
        int rc = WAH_OK;
        if (bitop_runs_route(op, n_words, 2, comp, words, offs, d_out, out_capacity_words, d_out_words, d_out_offsets, sc, l, s, &rc)) return rc;
    }
    // ONE kernel: both operands are walked segment by segment through their indexes, combined group by group in
    // registers, and the combined groups go straight into the compress passes -- no decoded bitmap is written or read
    // (the scratch's bitmap area stays unused on this route; the many-operand call still goes through it).
    hipError_t e = wah::launch_clear(sc, wah::kCtlWords * sizeof(uint32_t), s); // (read by wah_bitop_indexed_status)
    if (e != hipSuccess) return refuse("clearing the scratch", WAH_ERR_HIP, e);
    wah::BitopOperands ops;
    ops.comp_a = d_a;
    ops.comp_b = d_b;
    ops.c_words_a = a_words;
    ops.c_words_b = b_words;
    ops.offs_a = d_a_offsets;
    ops.offs_b = d_b_offsets;
    ops.groups = seg_geometry(n_words).groups;
    ops.op = (uint32_t)op;
    return compress_device_impl(nullptr, nullptr, 0, nullptr, n_words, d_out, out_capacity_words, d_out_words, d_out_offsets,
                                sc + l.ws_c, l.ws_c_bytes, stream, true, nullptr, &ops);
}

int wah_bitop_many_indexed_device(int op, uint64_t n_words, int n_operands, const uint32_t *const *d_streams,
                                  const uint64_t *stream_words, const uint64_t *const *d_offsets, uint32_t *d_out,
                                  uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                                  size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (op < WAH_OP_AND || op > WAH_OP_ANDNOT || !scratch_ok(d_scratch)) return refuse("bad operation or scratch pointer", WAH_ERR_ARG);
    if (n_operands < 1 || n_operands > wah::kMaxBitopOperands || !d_streams || !stream_words || !d_offsets ||
        n_words >= (1ull << 40))
        return refuse("between 1 and 8 operands, each with its stream, length and index", WAH_ERR_ARG);
    wah::BitopManyArgs a = {};
    for (int j = 0; j < n_operands; ++j) {
        if (!d_offsets[j] || (stream_words[j] && !d_streams[j]) || stream_words[j] >= (1ull << 40) || !aligned(d_streams[j], 3))
            return refuse("null or misaligned operand", WAH_ERR_ARG);
        a.comp[j] = d_streams[j];
        a.c_words[j] = stream_words[j];
        a.offs[j] = d_offsets[j];
    }
    const BitopIndexedLayout l = bitop_indexed_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    int rc = WAH_OK;
    if (bitop_runs_route(op, n_words, n_operands, d_streams, stream_words, d_offsets, d_out, out_capacity_words, d_out_words, d_out_offsets, sc,
                         l, static_cast<hipStream_t>(stream), &rc))
        return rc;
    a.n = n_operands;
    a.op = op;
    return combine_then_compress(a, wah::launch_bitop_many_segments, "combining pass launch", n_words, d_out, out_capacity_words, d_out_words,
                                 d_out_offsets, sc, l, stream);
}

int wah_bitop_indexed_status(void *d_scratch, uint64_t n_words, void *stream) {
    return scratch_status_then(bitop_indexed_layout(n_words).ws_c, d_scratch, stream); // (first: operands that are not segmented streams of n_words)
}

// Any number of operands, named by a table in device memory (wah_bitop_list.hip).  The scratch is that of the other indexed
// calls: control block, one decoded bitmap, compress workspace -- nothing of it goes with the number of operands.
static_assert(sizeof(wah_bitop_operand) == 24 && sizeof(wah::BitopListOperand) == sizeof(wah_bitop_operand), "the table's entries have no padding");
static_assert(WAH_BITOP_LIST_MAX_OPERANDS == wah::kMaxBitopListOperands, "one bound");
size_t wah_bitop_list_scratch_bytes(uint64_t n_words, uint64_t n_operands) {
    (void)n_operands;
    return bitop_indexed_layout(n_words).total;
}

int wah_bitop_list_indexed_device(int op, uint64_t n_words, uint64_t n_operands, const wah_bitop_operand *d_operands, uint32_t *d_out,
                                  uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                                  size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (op < WAH_OP_AND || op > WAH_OP_ANDNOT || !scratch_ok(d_scratch)) return refuse("bad operation or scratch pointer", WAH_ERR_ARG);
    if (!table_ok(n_operands, d_operands, n_words)) return refuse(kBadTable, WAH_ERR_ARG);
    if (!out_given(n_words, d_out, d_out_words)) return refuse("null pointer", WAH_ERR_ARG);
    const BitopIndexedLayout l = bitop_indexed_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    wah::BitopListArgs a = {};
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_operands);
    a.n = (uint32_t)n_operands;
    a.op = (uint32_t)op;
    return combine_then_compress(a, wah::launch_bitop_list_segments, "combining pass launch", n_words, d_out, out_capacity_words, d_out_words, d_out_offsets,
                                 static_cast<char *>(d_scratch), l, stream);
}

int wah_bitop_list_status(void *d_scratch, uint64_t n_words, uint64_t n_operands, void *stream) {
    (void)n_operands;
    return wah_bitop_indexed_status(d_scratch, n_words, stream);
}

// A conjunction of clauses, each the OR of its operands or the complement of it (wah_bitop_list.hip,
// bitop_clauses_segments_kernel).  Scratch and road as the list call's: one decoded bitmap, then the compress passes.
static_assert(WAH_CLAUSE_NEGATE == wah::kClauseNegate, "one flag");
size_t wah_bitop_clauses_scratch_bytes(uint64_t n_words, uint64_t n_operands, uint64_t n_clauses) {
    (void)n_operands;
    (void)n_clauses;
    return bitop_indexed_layout(n_words).total;
}

int wah_bitop_clauses_indexed_device(uint64_t n_words, uint64_t n_clauses, const uint64_t *d_clause_ends, uint64_t n_operands,
                                     const wah_bitop_operand *d_operands, uint32_t *d_out, uint64_t out_capacity_words,
                                     uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (!scratch_ok(d_scratch)) return refuse("bad scratch pointer", WAH_ERR_ARG);
    if (!table_ok(n_operands, d_operands, n_words)) return refuse(kBadTable, WAH_ERR_ARG);
    if (n_clauses < 1 || n_clauses > n_operands || !d_clause_ends || !aligned(d_clause_ends, 7))
        return refuse("between 1 and n_operands clauses in an 8-byte aligned table", WAH_ERR_ARG);
    if (!out_given(n_words, d_out, d_out_words)) return refuse("null pointer", WAH_ERR_ARG);
    const BitopIndexedLayout l = bitop_indexed_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    wah::BitopClausesArgs a = {};
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_operands);
    a.clause_ends = d_clause_ends;
    a.n = (uint32_t)n_operands;
    a.n_clauses = (uint32_t)n_clauses;
    return combine_then_compress(a, wah::launch_bitop_clauses_segments, "combining pass launch", n_words, d_out, out_capacity_words, d_out_words, d_out_offsets,
                                 static_cast<char *>(d_scratch), l, stream);
}

int wah_bitop_clauses_status(void *d_scratch, uint64_t n_words, uint64_t n_operands, uint64_t n_clauses, void *stream) {
    (void)n_operands;
    (void)n_clauses;
    return wah_bitop_indexed_status(d_scratch, n_words, stream);
}

// lo <= value <= hi over a bit-sliced attribute (wah_bitop_list.hip, bsi_range_segments_kernel).  Scratch and road as the
// clause call's: one decoded bitmap, then the compress passes.  The bounds stay in device memory: nothing here reads them.
static_assert(WAH_BSI_MAX_SLICES == wah::kMaxBsiSlices, "one bound");
size_t wah_bsi_range_scratch_bytes(uint64_t n_words, uint64_t n_slices) {
    (void)n_slices;
    return bitop_indexed_layout(n_words).total;
}

int wah_bsi_range_indexed_device(uint64_t n_words, uint64_t n_slices, const wah_bitop_operand *d_slices, const uint64_t *d_bounds,
                                 unsigned flags, uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words,
                                 uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_slices < 1 || n_slices > WAH_BSI_MAX_SLICES || (flags & ~WAH_BSI_EXISTS))
        return refuse("between 1 and 64 slices, no flag besides WAH_BSI_EXISTS", WAH_ERR_ARG);
    if (!d_slices || !aligned(d_slices, 7) || !d_bounds || !aligned(d_bounds, 7) || !scratch_ok(d_scratch))
        return refuse("null or misaligned slice table, bounds or scratch", WAH_ERR_ARG);
    if (!out_given(n_words, d_out, d_out_words) || n_words >= (1ull << 40)) return refuse("null output pointer, or 2^40 words or more", WAH_ERR_ARG);
    const BitopIndexedLayout l = bitop_indexed_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    wah::BsiRangeArgs a = {};
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_slices);
    a.bounds = d_bounds;
    a.n_slices = (uint32_t)n_slices;
    a.has_exists = (flags & WAH_BSI_EXISTS) ? 1u : 0u;
    return combine_then_compress(a, wah::launch_bsi_range_segments, "range sweep launch", n_words, d_out, out_capacity_words, d_out_words, d_out_offsets,
                                 static_cast<char *>(d_scratch), l, stream);
}

int wah_bsi_range_status(void *d_scratch, uint64_t n_words, uint64_t n_slices, void *stream) {
    (void)n_slices;
    return wah_bitop_indexed_status(d_scratch, n_words, stream);
}

// value IN (set) over a bit-sliced attribute (wah_member.hip, member_items_kernel behind member_check_kernel).  Scratch and road
// as the range call's: one decoded bitmap, then the compress passes.  The set and its count stay in device memory: nothing here
// reads them.
size_t wah_bsi_member_scratch_bytes(uint64_t n_words, uint64_t n_slices) {
    (void)n_slices;
    return bitop_indexed_layout(n_words).total;
}

int wah_bsi_member_indexed_device(uint64_t n_words, uint64_t n_slices, const wah_bitop_operand *d_slices, const void *d_set,
                                  uint64_t set_capacity, const uint64_t *d_set_count, unsigned flags, uint32_t *d_out,
                                  uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                                  size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_slices < 1 || n_slices > WAH_BSI_MAX_SLICES || (flags & ~(WAH_BSI_EXISTS | WAH_MEMBER_NEGATE | WAH_MEMBER_BITSET)))
        return refuse("between 1 and 64 slices, no flag besides WAH_BSI_EXISTS, WAH_MEMBER_NEGATE and WAH_MEMBER_BITSET", WAH_ERR_ARG);
    const bool bitset = (flags & WAH_MEMBER_BITSET) != 0;
    if (!d_slices || !aligned(d_slices, 7) || !scratch_ok(d_scratch)) return refuse("null or misaligned slice table or scratch", WAH_ERR_ARG);
    if (set_capacity >= (1ull << 40) || (set_capacity && !d_set) || !aligned(d_set, bitset ? 3 : 7) || !aligned(d_set_count, 7) ||
        (bitset && d_set_count))
        return refuse("a set of fewer than 2^40 entries or bits, aligned to its entries (8 bytes, a bit array's words: 4), a count only with a list", WAH_ERR_ARG);
    if (!out_given(n_words, d_out, d_out_words) || n_words >= (1ull << 40)) return refuse("null output pointer, or 2^40 words or more", WAH_ERR_ARG);
    const BitopIndexedLayout l = bitop_indexed_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    wah::MemberArgs a = {};
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_slices);
    a.set = d_set;
    a.set_capacity = set_capacity;
    a.set_count = d_set_count;
    a.n_slices = (uint32_t)n_slices;
    a.has_exists = (flags & WAH_BSI_EXISTS) ? 1u : 0u;
    a.negate = (flags & WAH_MEMBER_NEGATE) ? 1u : 0u;
    a.bitset = bitset ? 1u : 0u;
    a.n_items = seg_geometry(n_words).n_segments * (n_slices > 32 ? 2u : 1u);
    return combine_then_compress(a, wah::launch_member, "member launch", n_words, d_out, out_capacity_words, d_out_words, d_out_offsets,
                                 static_cast<char *>(d_scratch), l, stream);
}

int wah_bsi_member_status(void *d_scratch, uint64_t n_words, uint64_t n_slices, void *stream) {
    (void)n_slices;
    return wah_bitop_indexed_status(d_scratch, n_words, stream);
}

// A op B row by row over two bit-sliced attributes (wah_bitop_list.hip, bsi_compare_segments_kernel).  Scratch and road as the
// range call's: one decoded bitmap, then the compress passes.
static_assert(WAH_CMP_LT == wah::kCmpLT && WAH_CMP_LE == wah::kCmpLE && WAH_CMP_GT == wah::kCmpGT && WAH_CMP_GE == wah::kCmpGE &&
                  WAH_CMP_EQ == wah::kCmpEQ && WAH_CMP_NE == wah::kCmpNE,
              "the operators the sweep knows");
size_t wah_bsi_compare_scratch_bytes(uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b) {
    (void)n_slices_a;
    (void)n_slices_b;
    return bitop_indexed_layout(n_words).total;
}

int wah_bsi_compare_indexed_device(int op, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, const wah_bitop_operand *d_rows,
                                   unsigned flags, uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words,
                                   uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (op < WAH_CMP_LT || op > WAH_CMP_NE) return refuse("unknown comparison operator", WAH_ERR_ARG);
    if (n_slices_a < 1 || n_slices_a > WAH_BSI_MAX_SLICES || n_slices_b < 1 || n_slices_b > WAH_BSI_MAX_SLICES ||
        (flags & ~(WAH_BSI_EXISTS_A | WAH_BSI_EXISTS_B)))
        return refuse("between 1 and 64 slices per attribute, no flag besides WAH_BSI_EXISTS_A and WAH_BSI_EXISTS_B", WAH_ERR_ARG);
    if (!d_rows || !aligned(d_rows, 7) || !scratch_ok(d_scratch)) return refuse("null or misaligned row table or scratch", WAH_ERR_ARG);
    if (!out_given(n_words, d_out, d_out_words) || n_words >= (1ull << 40)) return refuse("null output pointer, or 2^40 words or more", WAH_ERR_ARG);
    const BitopIndexedLayout l = bitop_indexed_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    wah::BsiCompareArgs a = {};
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_rows);
    a.n_slices_a = (uint32_t)n_slices_a;
    a.n_slices_b = (uint32_t)n_slices_b;
    set_exists(a, flags);
    a.op = (uint32_t)op;
    return combine_then_compress(a, wah::launch_bsi_compare_segments, "compare sweep launch", n_words, d_out, out_capacity_words, d_out_words,
                                 d_out_offsets, static_cast<char *>(d_scratch), l, stream);
}

int wah_bsi_compare_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, void *stream) {
    (void)n_slices_a;
    (void)n_slices_b;
    return wah_bitop_indexed_status(d_scratch, n_words, stream);
}

// The value of a given rank over a bit-sliced attribute (wah_bitop_list.hip, bsi_kth_pass_kernel / bsi_kth_decide_kernel).  The
// scratch: control block, the decision state, then one histogram per pass and copy -- nothing of it goes with n_words.  The
// query stays in device memory: nothing here reads it.
static_assert(WAH_BSI_KTH_ASCENDING == 0 && WAH_BSI_KTH_DESCENDING == 1 && WAH_BSI_KTH_QUANTILE == 2, "the kinds the decide kernel knows");
static_assert(WAH_BSI_KTH_MAX_FILTERS == wah::kBsiKthMaxFilters, "one bound");
namespace {
// (the grouped call, further down, has the same scratch with one state and one set of histograms per select)
struct BsiKthLayout {
    uint32_t passes;
    size_t state, hist, total;
};
BsiKthLayout bsi_kth_layout(uint64_t n_slices, uint64_t selects, uint64_t copies) {
    BsiKthLayout l;
    if (n_slices < 1 || n_slices > WAH_BSI_MAX_SLICES) n_slices = WAH_BSI_MAX_SLICES; // (the size of a call that is refused anyway)
    l.passes = (uint32_t)ceil_div(n_slices, (uint64_t)wah::kBsiKthDigitBits);
    l.state = wah::kCtlWords * sizeof(uint32_t);
    l.hist = l.state + round256((size_t)selects * wah::kBsiKthStateWords * sizeof(uint64_t));
    l.total = l.hist + round256((size_t)l.passes * selects * copies * wah::kBsiKthBuckets * sizeof(uint64_t));
    return l;
}

// The road of both calls: everything cleared -- the control words (read by the call's *_status), the states, the histograms --
// then per digit a pass over the bitmaps and the decision on its histograms.  a: the kernels' arguments, the scratch's areas and
// the bitmaps' geometry filled in here.
extern "C++" template <class Args, class Launch>
int bsi_kth_passes(Args &a, Launch pass, Launch decide, const char *label, uint64_t n_words, char *sc, const BsiKthLayout &l, void *stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    a.state = reinterpret_cast<uint64_t *>(sc + l.state);
    a.hist = reinterpret_cast<uint64_t *>(sc + l.hist);
    set_walk(a, seg_geometry(n_words), sc);
    hipError_t e = wah::launch_clear(sc, l.total, s);
    for (uint32_t p = 0; p < l.passes && e == hipSuccess; ++p) {
        a.pass = p;
        e = pass(a, s);
        if (e == hipSuccess) e = decide(a, s);
    }
    if (e != hipSuccess) return refuse(label, WAH_ERR_HIP, e);
    return WAH_OK;
}
} // namespace

size_t wah_bsi_kth_scratch_bytes(uint64_t n_words, uint64_t n_slices) {
    (void)n_words;
    return bsi_kth_layout(n_slices, 1, wah::kBsiKthCopies).total;
}

int wah_bsi_kth_indexed_device(uint64_t n_words, uint64_t n_filters, uint64_t n_slices, const wah_bitop_operand *d_rows,
                               const uint64_t *d_query, uint64_t *d_result, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_slices < 1 || n_slices > WAH_BSI_MAX_SLICES || n_filters > WAH_BSI_KTH_MAX_FILTERS)
        return refuse("between 1 and 64 slices, at most 64 filters", WAH_ERR_ARG);
    if (!d_rows || !aligned(d_rows, 7) || !d_query || !aligned(d_query, 7) || !d_result || !aligned(d_result, 7) || !scratch_ok(d_scratch))
        return refuse("null or misaligned row table, query, result or scratch", WAH_ERR_ARG);
    if (n_words >= (1ull << 40)) return refuse("2^40 words or more", WAH_ERR_ARG);
    const BsiKthLayout l = bsi_kth_layout(n_slices, 1, wah::kBsiKthCopies);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    wah::BsiKthArgs a = {};
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_rows);
    a.query = d_query;
    a.result = d_result;
    a.n_filters = (uint32_t)n_filters;
    a.n_slices = (uint32_t)n_slices;
    return bsi_kth_passes(a, wah::launch_bsi_kth_pass, wah::launch_bsi_kth_decide, "radix select launch", n_words,
                          static_cast<char *>(d_scratch), l, stream);
}

int wah_bsi_kth_status(void *d_scratch, void *stream) { return scratch_status(d_scratch, stream); }

// The same for every (group, query) pair of a GROUP BY at once (wah_bitop_list.hip, bsi_kth_group_pass_kernel /
// bsi_kth_group_decide_kernel).  The scratch: control block, one decision state per select, then per pass and select its
// histograms -- nothing of it goes with n_words.  The queries stay in device memory.
static_assert(WAH_BSI_KTH_GROUPED_MAX_LANES == wah::kBsiKthGroupMaxSelects, "one bound");
namespace {
BsiKthLayout bsi_kth_group_layout(uint64_t n_slices, uint64_t n_groups, uint64_t n_queries) {
    const uint64_t most = wah::kBsiKthGroupMaxSelects; // (out of range: the size of a call that is refused anyway)
    const uint64_t selects = n_groups < 1 || n_queries < 1 || n_groups > most || n_queries > most || n_groups * n_queries > most ? most : n_groups * n_queries;
    return bsi_kth_layout(n_slices, selects, wah::kBsiKthGroupCopies);
}
} // namespace

size_t wah_bsi_kth_grouped_scratch_bytes(uint64_t n_words, uint64_t n_slices, uint64_t n_groups, uint64_t n_queries) {
    (void)n_words;
    return bsi_kth_group_layout(n_slices, n_groups, n_queries).total;
}

int wah_bsi_kth_grouped_indexed_device(uint64_t n_words, uint64_t n_filters, const wah_bitop_operand *d_filters, uint64_t n_groups,
                                       uint64_t rows_per_group, const wah_bitop_operand *d_groups, uint64_t n_slices,
                                       const wah_bitop_operand *d_slices, uint64_t n_queries, const uint64_t *d_queries,
                                       uint64_t *d_results, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_slices < 1 || n_slices > WAH_BSI_MAX_SLICES || n_filters > WAH_BSI_KTH_MAX_FILTERS)
        return refuse("between 1 and 64 slices, at most 64 filters", WAH_ERR_ARG);
    if (rows_per_group < 1 || rows_per_group > wah::kGroupMaxRows || n_groups < 1 || n_groups > wah::kBsiKthGroupMaxSelects || n_queries < 1 ||
        n_queries > wah::kBsiKthGroupMaxSelects || n_groups * n_queries > wah::kBsiKthGroupMaxSelects ||
        n_groups * rows_per_group > wah::kMaxBitopListOperands)
        return refuse("at least one group of 1 to 8 rows and one query, at most 4096 (group, query) pairs", WAH_ERR_ARG);
    if ((n_filters && !d_filters) || !aligned(d_filters, 7) || !d_groups || !aligned(d_groups, 7) || !d_slices || !aligned(d_slices, 7))
        return refuse("null or misaligned filter (null only when there is none), group or slice table", WAH_ERR_ARG);
    if (!d_queries || !aligned(d_queries, 7) || !d_results || !aligned(d_results, 7) || !scratch_ok(d_scratch))
        return refuse("null or misaligned queries, results or scratch", WAH_ERR_ARG);
    if (n_words >= (1ull << 40)) return refuse("2^40 words or more", WAH_ERR_ARG);
    const BsiKthLayout l = bsi_kth_group_layout(n_slices, n_groups, n_queries);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    wah::BsiKthGroupArgs a = {};
    a.filters = reinterpret_cast<const wah::BitopListOperand *>(d_filters);
    a.keys = reinterpret_cast<const wah::BitopListOperand *>(d_groups);
    a.slices = reinterpret_cast<const wah::BitopListOperand *>(d_slices);
    a.queries = d_queries;
    a.results = d_results;
    a.n_filters = (uint32_t)n_filters;
    a.rows_per_group = (uint32_t)rows_per_group;
    a.n_groups = (uint32_t)n_groups;
    a.n_queries = (uint32_t)n_queries;
    a.n_slices = (uint32_t)n_slices;
    return bsi_kth_passes(a, wah::launch_bsi_kth_group_pass, wah::launch_bsi_kth_group_decide, "grouped radix select launch", n_words,
                          static_cast<char *>(d_scratch), l, stream);
}

int wah_bsi_kth_grouped_status(void *d_scratch, void *stream) { return scratch_status(d_scratch, stream); }

// The values of listed rows (wah_bitop_list.hip, fetch_check_kernel / fetch_items_kernel).  The scratch: control block (with the
// item count), then the item list: one entry per 64 listed rows and one more per segment a list can change into -- it goes
// with the list, and with the bitmap only while the list is longer than the bitmap has segments.
static_assert(WAH_FETCH_BITS == wah::kFetchBits && WAH_FETCH_FIRST == wah::kFetchFirst, "the modes the items kernel knows");
namespace {
struct FetchLayout {
    SegGeometry g;
    uint64_t capacity;
    size_t items, total;
};
FetchLayout fetch_layout(uint64_t n_words, uint64_t n_rows) {
    FetchLayout l;
    const uint64_t most = 1ull << 40; // (the size of a call that is refused anyway)
    l.g = seg_geometry(n_words < most ? n_words : most);
    if (n_rows > most) n_rows = most;
    l.capacity = ceil_div(n_rows, 64) + (n_rows < l.g.n_segments ? n_rows : l.g.n_segments);
    l.items = wah::kCtlWords * sizeof(uint32_t);
    l.total = l.items + round256(l.capacity * sizeof(uint64_t));
    return l;
}
} // namespace

size_t wah_fetch_scratch_bytes(uint64_t n_words, uint64_t n_rows) { return fetch_layout(n_words, n_rows).total; }

int wah_fetch_indexed_device(unsigned mode, uint64_t n_words, uint64_t n_operands, const wah_bitop_operand *d_operands, const uint64_t *d_rows,
                             uint64_t n_rows, uint64_t *d_out, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (mode != WAH_FETCH_BITS && mode != WAH_FETCH_FIRST) return refuse("unknown mode", WAH_ERR_ARG);
    if (n_operands < 1 || n_operands > (mode == WAH_FETCH_BITS ? (uint64_t)WAH_BSI_MAX_SLICES : (uint64_t)WAH_BITOP_LIST_MAX_OPERANDS))
        return refuse("between 1 and 64 table rows (WAH_FETCH_BITS) or 2^24 (WAH_FETCH_FIRST)", WAH_ERR_ARG);
    if (n_rows && !n_words) return refuse("listed rows of an empty bitmap", WAH_ERR_ARG);
    if (n_words >= (1ull << 40) || n_rows >= (1ull << 40)) return refuse("2^40 words or listed rows, or more", WAH_ERR_ARG);
    if (!table_ok(n_operands, d_operands, n_words) || (n_rows && (!d_rows || !d_out)) || !aligned(d_rows, 7) || !aligned(d_out, 7) ||
        !scratch_ok(d_scratch))
        return refuse("null or misaligned table, rows, output or scratch", WAH_ERR_ARG);
    const FetchLayout l = fetch_layout(n_words, n_rows);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    hipStream_t s = static_cast<hipStream_t>(stream);
    wah::FetchArgs a = {};
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_operands);
    a.rows = d_rows;
    a.out = d_out;
    a.items = reinterpret_cast<uint64_t *>(sc + l.items);
    a.ctrl = reinterpret_cast<uint32_t *>(sc);
    a.n_rows = n_rows;
    a.n_bits = 32 * n_words;
    a.groups = l.g.groups;
    a.capacity = l.capacity;
    a.n_operands = (uint32_t)n_operands;
    hipError_t e = wah::launch_clear(sc, wah::kCtlWords * sizeof(uint32_t), s); // the error word (read by wah_fetch_status) and the item count
    if (e == hipSuccess) e = wah::launch_fetch_check(a, s);
    if (e == hipSuccess) e = wah::launch_fetch_items(a, mode, s);
    if (e != hipSuccess) return refuse("fetch launch", WAH_ERR_HIP, e);
    return WAH_OK;
}

int wah_fetch_status(void *d_scratch, void *stream) { return scratch_status(d_scratch, stream); }

// The values of a row range (wah_values.hip, values_items_kernel).  The scratch is the control block: the window is a host
// argument, so the items are known here and nothing is listed on the device.
size_t wah_values_scratch_bytes(uint64_t, uint64_t) { return round256(wah::kCtlWords * sizeof(uint32_t)); }

int wah_values_indexed_device(unsigned mode, uint64_t n_words, uint64_t n_operands, const wah_bitop_operand *d_operands, uint64_t first_row,
                              uint64_t n_rows, uint64_t *d_out, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (mode != WAH_FETCH_BITS && mode != WAH_FETCH_FIRST) return refuse("unknown mode", WAH_ERR_ARG);
    if (n_operands < 1 || n_operands > (mode == WAH_FETCH_BITS ? (uint64_t)WAH_BSI_MAX_SLICES : (uint64_t)WAH_BITOP_LIST_MAX_OPERANDS))
        return refuse("between 1 and 64 table rows (WAH_FETCH_BITS) or 2^24 (WAH_FETCH_FIRST)", WAH_ERR_ARG);
    if (n_words >= (1ull << 40)) return refuse("2^40 words or more", WAH_ERR_ARG);
    if (first_row > 32 * n_words || n_rows > 32 * n_words - first_row) return refuse("a window that leaves the bitmap's 32 n_words rows", WAH_ERR_ARG);
    if (!table_ok(n_operands, d_operands, n_words) || (n_rows && !d_out) || !aligned(d_out, 7) || !scratch_ok(d_scratch))
        return refuse("null or misaligned table, output or scratch", WAH_ERR_ARG);
    if (scratch_bytes < wah_values_scratch_bytes(n_words, n_operands)) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    wah::ValuesArgs a = {};
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_operands);
    a.out = d_out;
    a.ctrl = static_cast<uint32_t *>(d_scratch);
    a.first_row = first_row;
    a.n_rows = n_rows;
    a.groups = seg_geometry(n_words).groups;
    a.n_operands = (uint32_t)n_operands;
    if (n_rows) { // the segments the window overlaps
        constexpr uint64_t seg_rows = 31ull * wah::kSegGroups;
        a.first_segment = first_row / seg_rows;
        const uint64_t n_segments = (first_row + n_rows - 1) / seg_rows - a.first_segment + 1;
        a.n_items = n_segments * (mode == WAH_FETCH_BITS && n_operands > 32 ? 2u : 1u);
    }
    hipError_t e = wah::launch_clear(d_scratch, wah::kCtlWords * sizeof(uint32_t), s); // the error word (read by wah_values_status)
    if (e == hipSuccess) e = wah::launch_values_items(a, mode, s);
    if (e != hipSuccess) return refuse("values launch", WAH_ERR_HIP, e);
    return WAH_OK;
}

int wah_values_status(void *d_scratch, void *stream) { return scratch_status(d_scratch, stream); }

// COUNT and SUM per value of a bit-sliced key (wah_group_by.hip, group_by_items_kernel).  The scratch is the control block: the
// items are segments (and halves), known here.  The map, the tables and the outputs stay in device memory: nothing here reads them.
size_t wah_bsi_group_by_scratch_bytes(uint64_t) { return round256(wah::kCtlWords * sizeof(uint32_t)); }

int wah_bsi_group_by_indexed_device(uint64_t n_words, uint64_t n_rows, uint64_t n_filters, const wah_bitop_operand *d_filters,
                                    uint64_t n_slices_key, const wah_bitop_operand *d_key, uint64_t n_slices_val,
                                    const wah_bitop_operand *d_val, const uint32_t *d_map, uint64_t n_keys, uint64_t n_buckets,
                                    unsigned flags, uint64_t *d_counts, uint64_t *d_sums, void *d_scratch, size_t scratch_bytes,
                                    void *stream) {
    g_err[0] = 0;
    if (n_slices_key < 1 || n_slices_key > 32 || n_slices_val > 32 || (flags & ~(WAH_BSI_EXISTS | WAH_GROUP_BY_ACCUMULATE)) ||
        n_filters > wah::kGroupMaxFilters)
        return refuse("a key of 1 to 32 slices, a value of at most 32, no flag besides WAH_BSI_EXISTS and WAH_GROUP_BY_ACCUMULATE, at most 64 filter rows", WAH_ERR_ARG);
    if (!d_key || !aligned(d_key, 7) || !scratch_ok(d_scratch) || (n_slices_val != 0) != (d_val != nullptr) || !aligned(d_val, 7) ||
        (n_filters && !d_filters) || !aligned(d_filters, 7))
        return refuse("null or misaligned key table or scratch, a value table that does not go with n_slices_val, or a null or misaligned filter table", WAH_ERR_ARG);
    if ((n_keys != 0) != (d_map != nullptr) || !aligned(d_map, 3) || n_keys > (1ull << 32))
        return refuse("a 4-byte aligned map of 1 to 2^32 keys, or neither a map nor keys", WAH_ERR_ARG);
    if (n_buckets < 1 || n_buckets > WAH_GROUP_BY_MAX_BUCKETS || !d_counts || !aligned(d_counts, 7) ||
        (n_slices_val != 0) != (d_sums != nullptr) || !aligned(d_sums, 7))
        return refuse("between 1 and 2^30 buckets, null or misaligned counts, or sums that do not go with n_slices_val", WAH_ERR_ARG);
    if (n_words >= (1ull << 40) || n_rows > 32 * n_words) return refuse("2^40 words or more, or more rows than the bitmap's 32 n_words", WAH_ERR_ARG);
    if (scratch_bytes < wah_bsi_group_by_scratch_bytes(n_words)) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SegGeometry g = seg_geometry(n_words);
    wah::GroupByArgs a = {};
    a.filters = reinterpret_cast<const wah::BitopListOperand *>(d_filters);
    a.key = reinterpret_cast<const wah::BitopListOperand *>(d_key);
    a.val = reinterpret_cast<const wah::BitopListOperand *>(d_val);
    a.map = d_map;
    a.counts = d_counts;
    a.sums = d_sums;
    a.ctrl = static_cast<uint32_t *>(d_scratch);
    a.n_rows = n_rows;
    a.groups = g.groups;
    a.n_items = g.n_segments * (n_slices_val ? 2u : 1u);
    a.n_keys = n_keys;
    a.n_buckets = (uint32_t)n_buckets;
    a.n_filters = (uint32_t)n_filters;
    a.n_slices_key = (uint32_t)n_slices_key;
    a.n_slices_val = (uint32_t)n_slices_val;
    a.has_exists = (flags & WAH_BSI_EXISTS) ? 1u : 0u;
    hipError_t e = wah::launch_clear(d_scratch, wah::kCtlWords * sizeof(uint32_t), s); // the error word (read by wah_bsi_group_by_status)
    if (!(flags & WAH_GROUP_BY_ACCUMULATE)) {
        if (e == hipSuccess) e = wah::launch_clear(d_counts, (n_buckets + 1) * sizeof(uint64_t), s);
        if (e == hipSuccess && d_sums) e = wah::launch_clear(d_sums, 2 * (n_buckets + 1) * sizeof(uint64_t), s);
    }
    if (e == hipSuccess) e = wah::launch_group_by(a, s);
    if (e != hipSuccess) return refuse("group-by launch", WAH_ERR_HIP, e);
    return WAH_OK;
}

int wah_bsi_group_by_status(void *d_scratch, void *stream) { return scratch_status(d_scratch, stream); }

// Set bits counted and listed in the compressed domain (wah_select.hip).  The scratch: control block, then the positions
// call's rank table (one u64 per segment + 1) and the two upper levels of its scan (one u64 per 4096 entries of the level
// below) -- it goes with n_words / 992, not with the operands' number or their words.
namespace {
// the two upper levels of launch_select_rank_scan over `n_entries` u64, laid out from `at` on: one u64 per kRankChunk entries of
// the level below, each level rounded up to 256 bytes
struct ScanLevels {
    size_t level1, level2, end;
};
ScanLevels scan_levels(size_t at, uint64_t n_entries) {
    const uint64_t n1 = ceil_div(n_entries, (uint64_t)wah::kRankChunk), n2 = ceil_div(n1, (uint64_t)wah::kRankChunk);
    ScanLevels v;
    v.level1 = at;
    v.level2 = v.level1 + round256(n1 * sizeof(uint64_t));
    v.end = v.level2 + round256(n2 * sizeof(uint64_t));
    return v;
}

struct SelectLayout {
    SegGeometry g;
    size_t ranks, total;
    ScanLevels scan;
};
SelectLayout select_layout(uint64_t n_words) {
    SelectLayout l;
    l.g = seg_geometry(n_words);
    l.ranks = wah::kCtlWords * sizeof(uint32_t);
    l.scan = scan_levels(l.ranks + round256((l.g.n_segments + 1) * sizeof(uint64_t)), l.g.n_segments + 1);
    l.total = l.scan.end;
    return l;
}
} // namespace

size_t wah_select_scratch_bytes(uint64_t n_words, uint64_t n_operands) {
    (void)n_operands;
    return select_layout(n_words).total;
}

int wah_count_list_indexed_device(uint64_t n_words, uint64_t n_operands, const wah_bitop_operand *d_operands, uint64_t *d_counts,
                                  void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (!scratch_ok(d_scratch)) return refuse("bad scratch pointer", WAH_ERR_ARG);
    if (!table_ok(n_operands, d_operands, n_words)) return refuse(kBadTable, WAH_ERR_ARG);
    if (!d_counts || !aligned(d_counts, 7)) return refuse("null or misaligned counts", WAH_ERR_ARG);
    const SelectLayout l = select_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    hipStream_t s = static_cast<hipStream_t>(stream);
    wah::SelectCountArgs a = {};
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_operands);
    a.n_operands = (uint32_t)n_operands;
    a.counts = d_counts;
    set_walk(a, l.g, sc);
    hipError_t e = wah::launch_clear(sc, wah::kCtlWords * sizeof(uint32_t), s); // (read by wah_select_status)
    if (e == hipSuccess) e = wah::launch_clear(d_counts, n_operands * sizeof(uint64_t), s);
    if (e == hipSuccess) e = wah::launch_select_count(a, s);
    if (e != hipSuccess) return refuse("count pass launch", WAH_ERR_HIP, e);
    return WAH_OK;
}

int wah_count_masked_indexed_device(uint64_t n_words, uint64_t n_masks, const wah_bitop_operand *d_masks, uint64_t n_operands,
                                    const wah_bitop_operand *d_operands, uint64_t *d_counts, void *d_scratch, size_t scratch_bytes,
                                    void *stream) {
    g_err[0] = 0;
    if (!scratch_ok(d_scratch)) return refuse("bad scratch pointer", WAH_ERR_ARG);
    if (n_masks < 1 || n_masks > wah::kMaxBitopListOperands || n_operands < 1 || n_operands > wah::kMaxBitopListOperands ||
        n_masks * n_operands > wah::kMaxBitopListOperands || !d_masks || !aligned(d_masks, 7) || !d_operands ||
        !aligned(d_operands, 7) || n_words >= (1ull << 40))
        return refuse("at least one mask and one operand, at most 2^24 pairs, in 8-byte aligned tables, fewer than 2^40 words", WAH_ERR_ARG);
    if (!d_counts || !aligned(d_counts, 7)) return refuse("null or misaligned counts", WAH_ERR_ARG);
    const SelectLayout l = select_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    hipStream_t s = static_cast<hipStream_t>(stream);
    wah::CountMaskedArgs a = {};
    a.masks = reinterpret_cast<const wah::BitopListOperand *>(d_masks);
    a.operands = reinterpret_cast<const wah::BitopListOperand *>(d_operands);
    a.n_masks = (uint32_t)n_masks;
    a.n_operands = (uint32_t)n_operands;
    a.counts = d_counts;
    set_walk(a, l.g, sc);
    hipError_t e = wah::launch_clear(sc, wah::kCtlWords * sizeof(uint32_t), s); // (read by wah_select_status)
    if (e == hipSuccess) e = wah::launch_clear(d_counts, n_masks * n_operands * sizeof(uint64_t), s);
    if (e == hipSuccess) e = wah::launch_count_masked(a, s);
    if (e != hipSuccess) return refuse("masked count launch", WAH_ERR_HIP, e);
    return WAH_OK;
}

static_assert(WAH_GROUP_MAX_FILTERS == wah::kGroupMaxFilters && WAH_GROUP_MAX_ROWS == wah::kGroupMaxRows &&
                  WAH_GROUP_MAX_ATTRS == wah::kGroupMaxAttrs, "the limits the grouped count knows");

int wah_group_sum_indexed_device(uint64_t n_words, uint64_t n_filters, const wah_bitop_operand *d_filters, uint64_t n_groups,
                                 uint64_t rows_per_group, const wah_bitop_operand *d_groups, uint64_t n_operands,
                                 const wah_bitop_operand *d_operands, uint64_t n_attrs, const uint8_t *attr_bits, uint64_t *d_group_rows,
                                 uint64_t *d_counts, uint64_t *d_sums, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (!scratch_ok(d_scratch)) return refuse("bad scratch pointer", WAH_ERR_ARG);
    if (n_filters > wah::kGroupMaxFilters || (n_filters && !d_filters) || !aligned(d_filters, 7))
        return refuse("at most 64 filter rows in an 8-byte aligned table (null only when there is none)", WAH_ERR_ARG);
    if (rows_per_group < 1 || rows_per_group > wah::kGroupMaxRows || n_groups < 1 || n_groups > wah::kMaxBitopListOperands ||
        n_groups * rows_per_group > wah::kMaxBitopListOperands || n_operands < 1 || n_operands > wah::kMaxBitopListOperands ||
        n_groups * n_operands > wah::kMaxBitopListOperands || !d_groups || !aligned(d_groups, 7) || !d_operands ||
        !aligned(d_operands, 7) || n_words >= (1ull << 40))
        return refuse("at least one group of 1 to 8 rows and one operand, at most 2^24 group rows and 2^24 (group, operand) pairs, in "
                      "8-byte aligned tables, fewer than 2^40 words", WAH_ERR_ARG);
    if (n_attrs < 1 || n_attrs > wah::kGroupMaxAttrs || !attr_bits) return refuse("between 1 and 64 attributes and their widths", WAH_ERR_ARG);
    uint64_t slices = 0;
    for (uint64_t t = 0; t < n_attrs; ++t) {
        if (attr_bits[t] < 1 || attr_bits[t] > 64) return refuse("an attribute of no slice or of more than 64", WAH_ERR_ARG);
        slices += attr_bits[t];
    }
    if (slices != n_operands) return refuse("the attributes' widths do not add up to n_operands", WAH_ERR_ARG);
    if (!d_group_rows || !aligned(d_group_rows, 7) || !d_counts || !aligned(d_counts, 7) || !d_sums || !aligned(d_sums, 7))
        return refuse("null or misaligned group rows, counts or sums", WAH_ERR_ARG);
    const SelectLayout l = select_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    hipStream_t s = static_cast<hipStream_t>(stream);
    wah::GroupCountArgs a = {};
    a.filters = reinterpret_cast<const wah::BitopListOperand *>(d_filters);
    a.keys = reinterpret_cast<const wah::BitopListOperand *>(d_groups);
    a.operands = reinterpret_cast<const wah::BitopListOperand *>(d_operands);
    a.n_filters = (uint32_t)n_filters;
    a.rows_per_group = (uint32_t)rows_per_group;
    a.n_groups = (uint32_t)n_groups;
    a.n_operands = (uint32_t)n_operands;
    a.rows = d_group_rows;
    a.counts = d_counts;
    set_walk(a, l.g, sc);
    wah::GroupFoldArgs f = {};
    f.counts = d_counts;
    f.sums = d_sums;
    f.n_groups = a.n_groups;
    f.n_operands = a.n_operands;
    f.n_attrs = (uint32_t)n_attrs;
    for (uint64_t t = 0; t < n_attrs; ++t) f.bits[t] = attr_bits[t];
    hipError_t e = wah::launch_clear(sc, wah::kCtlWords * sizeof(uint32_t), s); // (read by wah_select_status)
    if (e == hipSuccess) e = wah::launch_clear(d_group_rows, n_groups * sizeof(uint64_t), s);
    if (e == hipSuccess) e = wah::launch_clear(d_counts, n_groups * n_operands * sizeof(uint64_t), s);
    if (e == hipSuccess) e = wah::launch_group_sum(a, f, s);
    if (e != hipSuccess) return refuse("grouped sum launch", WAH_ERR_HIP, e);
    return WAH_OK;
}

int wah_positions_indexed_device(uint64_t n_words, const uint32_t *d_stream, uint64_t stream_words, const uint64_t *d_offsets,
                                 uint64_t first_rank, uint64_t *d_out, uint64_t out_capacity, uint64_t *d_out_info, void *d_scratch,
                                 size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (!scratch_ok(d_scratch)) return refuse("bad scratch pointer", WAH_ERR_ARG);
    if (n_words >= (1ull << 40)) return refuse("fewer than 2^40 words", WAH_ERR_ARG);
    if (!d_out_info || !aligned(d_out_info, 7) || (out_capacity && !d_out) || !aligned(d_out, 7))
        return refuse("null or misaligned output", WAH_ERR_ARG);
    const SelectLayout l = select_layout(n_words);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint64_t *ranks = reinterpret_cast<uint64_t *>(sc + l.ranks);
    // the operand itself (a null or misaligned stream or index, a length of 2^40 or more) is judged where the table call's
    // rows are: on the device, before a pointer of it is followed
    wah::SelectCountArgs c = {};
    c.one.comp = d_stream;
    c.one.c_words = stream_words;
    c.one.offs = d_offsets;
    c.n_operands = 1;
    c.counts = ranks;
    set_walk(c, l.g, sc);
    wah::SelectEmitArgs a = {};
    a.g.comp = d_stream;
    a.g.c_words = stream_words;
    a.g.seg_offsets = d_offsets;
    a.g.n_segments = l.g.n_segments;
    a.g.groups = l.g.groups;
    a.g.ctrl = c.ctrl;
    a.ranks = ranks;
    a.first = first_rank;
    a.end = first_rank + out_capacity < first_rank ? ~0ull : first_rank + out_capacity;
    a.capacity = out_capacity;
    a.out = d_out;
    a.info = d_out_info;
    a.pad_bits = c.pad_bits;
    hipError_t e = wah::launch_clear(sc, wah::kCtlWords * sizeof(uint32_t), s); // (read by wah_select_status)
    if (e == hipSuccess) e = wah::launch_select_count(c, s);
    if (e == hipSuccess)
        e = wah::launch_select_rank_scan(ranks, l.g.n_segments, reinterpret_cast<uint64_t *>(sc + l.scan.level1), reinterpret_cast<uint64_t *>(sc + l.scan.level2), s);
    if (e == hipSuccess) e = wah::launch_select_emit(a, s);
    if (e != hipSuccess) return refuse("positions launch", WAH_ERR_HIP, e);
    return WAH_OK;
}

int wah_select_status(void *d_scratch, void *stream) { return scratch_status(d_scratch, stream); }

// Compressed bitmaps from sorted lists of row numbers (wah_from_positions.hip).  The scratch: control block, then the two upper
// levels of the prefix sum over the n_lists x S + 1 index entries (one u64 per 4096 entries of the level below); the scan itself
// runs in place in the caller's index.  The splice call, further down, has the same scratch with its n_pieces + 1 running starts
// between the control block and the levels, and takes the same road.
namespace {
struct StreamsLayout {
    SegGeometry g;
    uint64_t n_items; // (segment, bitmap) pairs: one index entry each, and one at the end
    size_t starts, total;
    ScanLevels scan;
};
StreamsLayout streams_layout(uint64_t n_words, uint64_t n_bitmaps, uint64_t n_starts) { // n_starts == 0: no such area, no bytes
    StreamsLayout l;
    l.g = seg_geometry(n_words);
    l.n_items = n_bitmaps * l.g.n_segments;
    l.starts = wah::kCtlWords * sizeof(uint32_t);
    l.scan = scan_levels(l.starts + round256(n_starts * sizeof(uint64_t)), l.n_items + 1);
    l.total = l.scan.end;
    return l;
}

// The road of the calls that write n_bitmaps streams back to back with their index: the control words cleared (read by the call's
// *_status), `check` over the call's lists, `segments` once to count every (segment, bitmap)'s words into the caller's index, the
// index scanned in place, `segments` again to emit.  a: the kernels' arguments, geometry and output filled in here.
extern "C++" template <class Args, class Check, class Segments>
int count_scan_emit(Args &a, Check check, Segments segments, const char *label, uint64_t n_words, uint32_t *d_out, uint64_t out_capacity_words,
                    uint64_t *d_out_words, uint64_t *d_out_offsets, char *sc, const StreamsLayout &l, void *stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    a.n_bits = 32u * n_words;
    a.groups = l.g.groups;
    a.n_segments = l.g.n_segments;
    a.out = d_out;
    a.out_capacity = out_capacity_words;
    a.out_words = d_out_words;
    a.offsets = d_out_offsets;
    a.ctrl = reinterpret_cast<uint32_t *>(sc);
    hipError_t e = wah::launch_clear(sc, wah::kCtlWords * sizeof(uint32_t), s);
    if (e == hipSuccess) e = check(a, s);
    if (e == hipSuccess) e = segments(a, false, s);
    if (e == hipSuccess)
        e = wah::launch_select_rank_scan(d_out_offsets, l.n_items, reinterpret_cast<uint64_t *>(sc + l.scan.level1), reinterpret_cast<uint64_t *>(sc + l.scan.level2), s);
    if (e == hipSuccess) e = segments(a, true, s);
    if (e != hipSuccess) return refuse(label, WAH_ERR_HIP, e);
    return WAH_OK;
}
} // namespace

uint64_t wah_from_positions_max_words(uint64_t n_words, uint64_t n_lists, uint64_t n_rows) {
    // (n_lists x G passes 2^64 for the longest bitmaps and the most lists)
    const SegGeometry g = seg_geometry(n_words);
    const unsigned __int128 groups = g.groups, segments = g.n_segments;
    const unsigned __int128 all_literals = (unsigned __int128)n_lists * groups;
    const unsigned __int128 by_rows = (unsigned __int128)n_lists * segments + 2 * (unsigned __int128)n_rows;
    const unsigned __int128 m = all_literals < by_rows ? all_literals : by_rows;
    return m > (unsigned __int128)~0ull ? ~0ull : (uint64_t)m;
}

size_t wah_from_positions_scratch_bytes(uint64_t n_words, uint64_t n_lists) { return streams_layout(n_words, n_lists, 0).total; }

int wah_from_positions_device(uint64_t n_words, uint64_t n_lists, const uint64_t *d_list_ends, const uint64_t *d_rows, uint64_t n_rows,
                              uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets,
                              void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_lists < 1 || n_lists > wah::kMaxBitopListOperands || n_words == 0 || n_words >= (1ull << 40) || n_rows >= (1ull << 40))
        return refuse("between 1 and 2^24 lists, between 1 and 2^40 - 1 words, fewer than 2^40 rows", WAH_ERR_ARG);
    const StreamsLayout l = streams_layout(n_words, n_lists, 0);
    if (l.n_items >= (1ull << 31)) return refuse("lists x segments of 992 words: fewer than 2^31", WAH_ERR_ARG);
    if (!scratch_ok(d_scratch)) return refuse("bad scratch pointer", WAH_ERR_ARG);
    if (!d_list_ends || !aligned(d_list_ends, 7) || (n_rows && !d_rows) || !aligned(d_rows, 7))
        return refuse("null or misaligned list ends or rows", WAH_ERR_ARG);
    if (!out_triple_ok(d_out, d_out_words, d_out_offsets)) return refuse("null or misaligned output", WAH_ERR_ARG);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    wah::FromPositionsArgs a = {};
    a.rows = d_rows;
    a.list_ends = d_list_ends;
    a.n_rows = n_rows;
    a.n_lists = n_lists;
    return count_scan_emit(a, wah::launch_from_positions_check, wah::launch_from_positions_segments, "from_positions launch", n_words, d_out,
                           out_capacity_words, d_out_words, d_out_offsets, static_cast<char *>(d_scratch), l, stream);
}

int wah_from_positions_status(void *d_scratch, void *stream) { return scratch_status(d_scratch, stream); }

// Row ranges of indexed bitmaps concatenated into new ones (splice_segments_kernel, wah_splice.hip).  The scratch: control
// block, the n_pieces + 1 running starts the check launch leaves, then the two upper levels of the prefix sum over the
// n_columns x S + 1 index entries: streams_layout, and its road.
static_assert(sizeof(wah_splice_piece) == 24 && sizeof(wah::SplicePiece) == 24 && WAH_SPLICE_MAX_PIECES == wah::kSpliceMaxPieces, "one piece, one bound");

uint64_t wah_splice_max_words(uint64_t n_words_out, uint64_t n_columns, uint64_t n_pieces, uint64_t source_words) {
    const SegGeometry g = seg_geometry(n_words_out);
    const unsigned __int128 columns = n_columns;
    const unsigned __int128 all_literals = columns * g.groups;
    const unsigned __int128 by_words = columns * (g.n_segments + 1) + 2 * columns * n_pieces + 2 * (unsigned __int128)source_words;
    const unsigned __int128 m = all_literals < by_words ? all_literals : by_words;
    return m > (unsigned __int128)~0ull ? ~0ull : (uint64_t)m;
}

size_t wah_splice_scratch_bytes(uint64_t n_words_out, uint64_t n_columns, uint64_t n_pieces) {
    return streams_layout(n_words_out, n_columns, n_pieces + 1).total;
}

int wah_splice_indexed_device(uint64_t n_words_out, uint64_t n_columns, uint64_t n_pieces, const wah_splice_piece *d_pieces,
                              const wah_bitop_operand *d_operands, uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words,
                              uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_columns < 1 || n_columns > wah::kMaxBitopListOperands || n_pieces < 1 || n_pieces > wah::kSpliceMaxPieces ||
        n_pieces * n_columns > wah::kMaxBitopListOperands || n_words_out == 0 || n_words_out >= (1ull << 40))
        return refuse("between 1 and 2^24 columns, between 1 and 2^16 pieces, at most 2^24 table entries, between 1 and 2^40 - 1 words",
                      WAH_ERR_ARG);
    const StreamsLayout l = streams_layout(n_words_out, n_columns, n_pieces + 1);
    if (l.n_items >= (1ull << 31)) return refuse("columns x segments of 992 words: fewer than 2^31", WAH_ERR_ARG);
    if (!scratch_ok(d_scratch)) return refuse("bad scratch pointer", WAH_ERR_ARG);
    if (!d_pieces || !aligned(d_pieces, 7) || !d_operands || !aligned(d_operands, 7))
        return refuse("null or misaligned pieces or operand table", WAH_ERR_ARG);
    if (!out_triple_ok(d_out, d_out_words, d_out_offsets)) return refuse("null or misaligned output", WAH_ERR_ARG);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    wah::SpliceArgs a = {};
    a.pieces = reinterpret_cast<const wah::SplicePiece *>(d_pieces);
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_operands);
    a.starts = reinterpret_cast<uint64_t *>(sc + l.starts);
    a.n_pieces = n_pieces;
    a.n_columns = n_columns;
    return count_scan_emit(a, wah::launch_splice_check, wah::launch_splice_segments, "splice launch", n_words_out, d_out, out_capacity_words,
                           d_out_words, d_out_offsets, sc, l, stream);
}

int wah_splice_status(void *d_scratch, void *stream) { return scratch_status(d_scratch, stream); }

// The rows a mask bitmap selects of every column of an index, moved together into new indexed bitmaps (wah_compact.hip).  The
// scratch: the splice call's, with the S_src + 1 running ranks of the mask's segments in the starts' place, then the two upper
// levels of the prefix sum over those ranks: streams_layout and its road, the rank pass being the road's check.
namespace {
struct CompactLayout {
    StreamsLayout s;
    SegGeometry src;
    ScanLevels ranks;
    size_t total;
};
CompactLayout compact_layout(uint64_t n_words, uint64_t n_words_out, uint64_t n_columns) {
    CompactLayout l;
    l.src = seg_geometry(n_words);
    l.s = streams_layout(n_words_out, n_columns, l.src.n_segments + 1);
    l.ranks = scan_levels(l.s.total, l.src.n_segments + 1);
    l.total = l.ranks.end;
    return l;
}
} // namespace

uint64_t wah_compact_max_words(uint64_t n_words_out, uint64_t n_columns, uint64_t source_words) {
    const SegGeometry g = seg_geometry(n_words_out);
    const unsigned __int128 columns = n_columns;
    const unsigned __int128 all_literals = columns * g.groups;
    const unsigned __int128 by_words = columns * (g.n_segments + 1) + 2 * (unsigned __int128)source_words;
    const unsigned __int128 m = all_literals < by_words ? all_literals : by_words;
    return m > (unsigned __int128)~0ull ? ~0ull : (uint64_t)m;
}

size_t wah_compact_scratch_bytes(uint64_t n_words, uint64_t n_words_out, uint64_t n_columns) {
    return compact_layout(n_words, n_words_out, n_columns).total;
}

int wah_compact_indexed_device(uint64_t n_words, uint64_t n_rows, uint32_t flags, const wah_bitop_operand *d_mask, uint64_t n_columns,
                               const wah_bitop_operand *d_operands, uint64_t n_words_out, uint32_t *d_out, uint64_t out_capacity_words,
                               uint64_t *d_out_words, uint64_t *d_out_offsets, uint64_t *d_out_rows, void *d_scratch, size_t scratch_bytes,
                               void *stream) {
    g_err[0] = 0;
    if (n_columns < 1 || n_columns > wah::kMaxBitopListOperands || n_words == 0 || n_words >= (1ull << 40) || n_words_out == 0 ||
        n_words_out >= (1ull << 40))
        return refuse("between 1 and 2^24 columns, between 1 and 2^40 - 1 words in and out", WAH_ERR_ARG);
    if (n_rows > 32u * n_words) return refuse("more rows than 32 * n_words", WAH_ERR_ARG);
    if ((flags & ~WAH_COMPACT_DELETE) != 0u) return refuse("unknown flag bits", WAH_ERR_ARG);
    const CompactLayout l = compact_layout(n_words, n_words_out, n_columns);
    if (l.s.n_items >= (1ull << 31)) return refuse("columns x segments of 992 words: fewer than 2^31", WAH_ERR_ARG);
    if (!scratch_ok(d_scratch)) return refuse("bad scratch pointer", WAH_ERR_ARG);
    if (!d_mask || !aligned(d_mask, 7) || !d_operands || !aligned(d_operands, 7)) return refuse("null or misaligned mask or operand table", WAH_ERR_ARG);
    if (!out_triple_ok(d_out, d_out_words, d_out_offsets) || !d_out_rows || !aligned(d_out_rows, 7))
        return refuse("null or misaligned output", WAH_ERR_ARG);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    wah::CompactArgs a = {};
    a.mask = reinterpret_cast<const wah::BitopListOperand *>(d_mask);
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_operands);
    a.starts = reinterpret_cast<uint64_t *>(sc + l.s.starts);
    a.level1 = reinterpret_cast<uint64_t *>(sc + l.ranks.level1);
    a.level2 = reinterpret_cast<uint64_t *>(sc + l.ranks.level2);
    a.out_rows = d_out_rows;
    a.n_columns = n_columns;
    a.src_rows = n_rows;
    a.src_groups = l.src.groups;
    a.src_segments = l.src.n_segments;
    a.del = (flags & WAH_COMPACT_DELETE) ? 1u : 0u;
    return count_scan_emit(a, wah::launch_compact_check, wah::launch_compact_segments, "compact launch", n_words_out, d_out, out_capacity_words,
                           d_out_words, d_out_offsets, sc, l.s, stream);
}

int wah_compact_status(void *d_scratch, void *stream) { return scratch_status(d_scratch, stream); }

// The rows a mask bitmap selects of every column of an index take the then column's bits, all others keep the else column's
// (wah_update.hip).  The scratch: the from-positions call's -- control block and the two upper levels of the prefix sum over the
// n_columns x S + 1 index entries; no ranks, no starts -- and its road, with a check step that launches nothing.
uint64_t wah_update_max_words(uint64_t n_words, uint64_t n_columns, uint64_t mask_words, uint64_t source_words) {
    const SegGeometry g = seg_geometry(n_words);
    const unsigned __int128 columns = n_columns;
    const unsigned __int128 all_literals = columns * g.groups;
    const unsigned __int128 by_words = (unsigned __int128)source_words + columns * ((unsigned __int128)mask_words + 3);
    const unsigned __int128 m = all_literals < by_words ? all_literals : by_words;
    return m > (unsigned __int128)~0ull ? ~0ull : (uint64_t)m;
}

size_t wah_update_scratch_bytes(uint64_t n_words, uint64_t n_columns) { return streams_layout(n_words, n_columns, 0).total; }

int wah_update_indexed_device(uint64_t n_words, uint64_t n_rows, const wah_bitop_operand *d_mask, uint64_t n_columns,
                              const wah_bitop_operand *d_else, const wah_bitop_operand *d_then, uint32_t *d_out,
                              uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                              size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_columns < 1 || n_columns > wah::kMaxBitopListOperands || n_words == 0 || n_words >= (1ull << 40))
        return refuse("between 1 and 2^24 columns, between 1 and 2^40 - 1 words", WAH_ERR_ARG);
    if (n_rows > 32u * n_words) return refuse("more rows than 32 * n_words", WAH_ERR_ARG);
    const StreamsLayout l = streams_layout(n_words, n_columns, 0);
    if (l.n_items >= (1ull << 31)) return refuse("columns x segments of 992 words: fewer than 2^31", WAH_ERR_ARG);
    if (!scratch_ok(d_scratch)) return refuse("bad scratch pointer", WAH_ERR_ARG);
    if (!d_mask || !aligned(d_mask, 7) || !d_else || !aligned(d_else, 7) || !d_then || !aligned(d_then, 7))
        return refuse("null or misaligned mask, else table or then table", WAH_ERR_ARG);
    if (!out_triple_ok(d_out, d_out_words, d_out_offsets)) return refuse("null or misaligned output", WAH_ERR_ARG);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    wah::UpdateArgs a = {};
    a.mask = reinterpret_cast<const wah::BitopListOperand *>(d_mask);
    a.else_table = reinterpret_cast<const wah::BitopListOperand *>(d_else);
    a.then_table = reinterpret_cast<const wah::BitopListOperand *>(d_then);
    a.n_columns = n_columns;
    a.n_rows = n_rows;
    return count_scan_emit(a, wah::launch_update_check, wah::launch_update_segments, "update launch", n_words, d_out, out_capacity_words,
                           d_out_words, d_out_offsets, static_cast<char *>(d_scratch), l, stream);
}

int wah_update_status(void *d_scratch, void *stream) { return scratch_status(d_scratch, stream); }

// A bit-sliced index from a column of values (wah_bsi_build.hip): the transpose writes the decoded slice matrix into the scratch,
// the compress passes run over it as over any column matrix.  The scratch: [control words][slice matrix][compress workspace] --
// the layout of every call that leaves a whole attribute (wah_bsi_arith_indexed_device below: its sweep writes the matrix).
namespace {
struct BsiBuildLayout {
    size_t matrix, ws_c, ws_c_bytes, total;
};
BsiBuildLayout bsi_build_layout(uint64_t n_words, uint64_t n_slices) { // n_slices: the matrix' rows, an existence row included
    BsiBuildLayout l;
    l.matrix = round256(wah::kCtlWords * sizeof(uint32_t));
    l.ws_c = l.matrix + round256(n_slices * n_words * sizeof(uint32_t));
    l.ws_c_bytes = wah_compress_workspace_bytes(n_slices * n_words);
    l.total = l.ws_c + round256(l.ws_c_bytes);
    return l;
}
inline uint32_t *bsi_matrix(char *sc, const BsiBuildLayout &l) { return reinterpret_cast<uint32_t *>(sc + l.matrix); }

// The road: launch_then_compress with a sweep that writes the decoded matrix of n_slices x n_words words
extern "C++" template <class Args, class Launch>
int sweep_then_compress(const Args &a, Launch launch, const char *label, uint64_t n_words, uint64_t n_slices, uint32_t *d_out,
                        uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, char *sc, const BsiBuildLayout &l, void *stream) {
    return launch_then_compress(a, launch, label, bsi_matrix(sc, l), n_slices * n_words, d_out, out_capacity_words, d_out_words, d_out_offsets,
                                sc, l.ws_c, l.ws_c_bytes, stream);
}
} // namespace

size_t wah_bsi_build_scratch_bytes(uint64_t n_words, uint64_t n_slices) { return bsi_build_layout(n_words, n_slices).total; }

int wah_bsi_build_device(uint64_t n_words, uint64_t n_bits, const uint64_t *d_values, uint64_t n_rows, const uint8_t *d_exists,
                         uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                         size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_bits < 1 || n_bits > 64) return refuse("between 1 and 64 bits", WAH_ERR_ARG);
    const uint64_t n_slices = n_bits + (d_exists ? 1u : 0u);
    if (n_words == 0 || n_words % wah::kSegWords || n_words >= (1ull << 40) || n_slices * n_words >= (1ull << 40))
        return refuse("slices of a multiple of 992 words, all slices together fewer than 2^40 words", WAH_ERR_ARG);
    if (n_rows > 32u * n_words) return refuse("more rows than a slice has bits", WAH_ERR_ARG);
    if ((n_rows && !d_values) || !aligned(d_values, 7)) return refuse("null or misaligned values", WAH_ERR_ARG);
    if (!out_triple_ok(d_out, d_out_words, d_out_offsets)) return refuse("null or misaligned output", WAH_ERR_ARG);
    if (!scratch_ok(d_scratch)) return refuse("bad scratch pointer", WAH_ERR_ARG);
    const BsiBuildLayout l = bsi_build_layout(n_words, n_slices);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    wah::BsiBuildArgs a = {};
    a.values = d_values;
    a.exists = d_exists;
    a.n_rows = n_rows;
    a.n_words = n_words;
    a.n_bits = (uint32_t)n_bits;
    a.out = bsi_matrix(sc, l);
    a.ctrl = reinterpret_cast<uint32_t *>(sc);
    return sweep_then_compress(a, wah::launch_bsi_slices, "slice transpose launch", n_words, n_slices, d_out, out_capacity_words, d_out_words,
                               d_out_offsets, sc, l, stream);
}

int wah_bsi_build_status(void *d_scratch, uint64_t n_words, uint64_t n_slices, void *stream) {
    return scratch_status_then(bsi_build_layout(n_words, n_slices).ws_c, d_scratch, stream); // (first the transpose: a value at or above 2^n_bits)
}

// A + B, A - B row by row over two bit-sliced attributes, as a new one (wah_bitop_list.hip, bsi_arith_segments_kernel).  The
// builder's scratch and its road: the sweep writes the result's decoded slice matrix, the compress passes run over it.
static_assert(WAH_ARITH_ADD == wah::kArithAdd && WAH_ARITH_SUB == wah::kArithSub, "the operations the sweep knows");
namespace {
constexpr unsigned kArithFlags = WAH_BSI_EXISTS_A | WAH_BSI_EXISTS_B;
// the result's matrix rows: its slices, and the AND of the existence bitmaps where there is one
inline uint64_t arith_rows_out(uint64_t n_slices_out, unsigned flags) { return n_slices_out + ((flags & kArithFlags) ? 1u : 0u); }
// the argument checks of the calls that compute a new attribute from two (arithmetic, multiplication, division): WAH_OK or the
// refusal.  rows_out: the result's matrix rows as the call counts them
int two_attribute_args(uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, uint64_t n_slices_out, uint64_t rows_out,
                       const wah_bitop_operand *d_rows, unsigned flags, const uint32_t *d_out, const uint64_t *d_out_words,
                       const uint64_t *d_out_offsets, const void *d_scratch) {
    if (n_slices_a < 1 || n_slices_a > WAH_BSI_MAX_SLICES || n_slices_b < 1 || n_slices_b > WAH_BSI_MAX_SLICES || n_slices_out < 1 ||
        n_slices_out > WAH_BSI_MAX_SLICES || (flags & ~kArithFlags))
        return refuse("between 1 and 64 slices per attribute and in the result, no flag besides WAH_BSI_EXISTS_A and WAH_BSI_EXISTS_B", WAH_ERR_ARG);
    if (n_words == 0 || n_words % wah::kSegWords || n_words >= (1ull << 40) || rows_out * n_words >= (1ull << 40))
        return refuse("slices of a multiple of 992 words, all slices of the result together fewer than 2^40 words", WAH_ERR_ARG);
    if (!d_rows || !aligned(d_rows, 7) || !scratch_ok(d_scratch)) return refuse("null or misaligned row table or scratch", WAH_ERR_ARG);
    if (!out_triple_ok(d_out, d_out_words, d_out_offsets)) return refuse("null or misaligned output", WAH_ERR_ARG);
    return WAH_OK;
}
// ... and what the arguments of the three sweeps hold
extern "C++" template <class Args>
void two_attribute_fill(Args &a, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, uint64_t n_slices_out, const wah_bitop_operand *d_rows,
                        unsigned flags, char *sc, const BsiBuildLayout &l) {
    const SegGeometry g = seg_geometry(n_words);
    a.table = reinterpret_cast<const wah::BitopListOperand *>(d_rows);
    a.matrix = bsi_matrix(sc, l);
    a.ctrl = reinterpret_cast<uint32_t *>(sc);
    a.n_words = n_words;
    a.groups = g.groups;
    a.n_segments = g.n_segments;
    a.n_slices_a = (uint32_t)n_slices_a;
    a.n_slices_b = (uint32_t)n_slices_b;
    a.n_slices_out = (uint32_t)n_slices_out;
    set_exists(a, flags);
}
} // namespace

size_t wah_bsi_arith_scratch_bytes(uint64_t n_words, uint64_t n_slices_out, unsigned flags) {
    return bsi_build_layout(n_words, arith_rows_out(n_slices_out, flags)).total;
}

int wah_bsi_arith_indexed_device(int op, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, uint64_t n_slices_out,
                                 const wah_bitop_operand *d_rows, unsigned flags, uint32_t *d_out, uint64_t out_capacity_words,
                                 uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (op != WAH_ARITH_ADD && op != WAH_ARITH_SUB) return refuse("unknown arithmetic operation", WAH_ERR_ARG);
    const uint64_t rows_out = arith_rows_out(n_slices_out, flags);
    if (const int rc = two_attribute_args(n_words, n_slices_a, n_slices_b, n_slices_out, rows_out, d_rows, flags, d_out, d_out_words, d_out_offsets, d_scratch))
        return rc;
    const BsiBuildLayout l = bsi_build_layout(n_words, rows_out);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    wah::BsiArithArgs a = {};
    two_attribute_fill(a, n_words, n_slices_a, n_slices_b, n_slices_out, d_rows, flags, sc, l);
    a.sub = op == WAH_ARITH_SUB ? 1u : 0u;
    return sweep_then_compress(a, wah::launch_bsi_arith_segments, "arithmetic sweep launch", n_words, rows_out, d_out, out_capacity_words,
                               d_out_words, d_out_offsets, sc, l, stream);
}

int wah_bsi_arith_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_out, unsigned flags, void *stream) {
    // (first the sweep: everything the list call refuses in an operand)
    return scratch_status_then(bsi_build_layout(n_words, arith_rows_out(n_slices_out, flags)).ws_c, d_scratch, stream);
}

// A * B row by row over two bit-sliced attributes, as a new one (wah_bitop_list.hip, bsi_mul_segments_kernel).  The arithmetic
// call's scratch and road, and behind them the sweep's working area: per segment A's image and the accumulator in group form,
// n_slices_a + n_slices_out slices of 1024 groups, which needs no initialisation.
namespace {
inline size_t mul_work_bytes(uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_out) {
    return (size_t)(n_words / wah::kSegWords) * (size_t)(n_slices_a + n_slices_out) * wah::kSegGroups * sizeof(uint32_t);
}
} // namespace

size_t wah_bsi_mul_scratch_bytes(uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_out, unsigned flags) {
    return bsi_build_layout(n_words, arith_rows_out(n_slices_out, flags)).total + mul_work_bytes(n_words, n_slices_a, n_slices_out);
}

int wah_bsi_mul_indexed_device(uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, uint64_t n_slices_out,
                               const wah_bitop_operand *d_rows, unsigned flags, uint32_t *d_out, uint64_t out_capacity_words,
                               uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    const uint64_t rows_out = arith_rows_out(n_slices_out, flags);
    if (const int rc = two_attribute_args(n_words, n_slices_a, n_slices_b, n_slices_out, rows_out, d_rows, flags, d_out, d_out_words, d_out_offsets, d_scratch))
        return rc;
    const BsiBuildLayout l = bsi_build_layout(n_words, rows_out);
    if (scratch_bytes < l.total + mul_work_bytes(n_words, n_slices_a, n_slices_out)) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    wah::BsiMulArgs a = {};
    two_attribute_fill(a, n_words, n_slices_a, n_slices_b, n_slices_out, d_rows, flags, sc, l);
    a.work = reinterpret_cast<uint32_t *>(sc + l.total); // (a multiple of 256 bytes: the quads are aligned)
    return sweep_then_compress(a, wah::launch_bsi_mul_segments, "multiplication sweep launch", n_words, rows_out, d_out, out_capacity_words,
                               d_out_words, d_out_offsets, sc, l, stream);
}

int wah_bsi_mul_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_out, unsigned flags, void *stream) {
    (void)n_slices_a; // (the working area lies behind everything the status reads)
    return wah_bsi_arith_status(d_scratch, n_words, n_slices_out, flags, stream);
}

// floor(A / B), A mod B row by row over two bit-sliced attributes, as a new one (wah_bitop_list.hip, bsi_div_segments_kernel).
// The arithmetic call's scratch and road for n_slices_out + 1 rows -- the existence row, which holds B != 0, is always there --
// and behind them the sweep's working area: per segment B's image and two remainder buffers of n_slices_b + 1 slices in group
// form, which needs no initialisation.
static_assert(WAH_DIV_QUOTIENT == wah::kDivQuotient && WAH_DIV_REMAINDER == wah::kDivRemainder, "the results the sweep knows");
namespace {
inline size_t div_work_bytes(uint64_t n_words, uint64_t n_slices_b) {
    return (size_t)(n_words / wah::kSegWords) * (size_t)(3u * n_slices_b + 2u) * wah::kSegGroups * sizeof(uint32_t);
}
} // namespace

size_t wah_bsi_div_scratch_bytes(uint64_t n_words, uint64_t n_slices_b, uint64_t n_slices_out, unsigned flags) {
    (void)flags; // (the result has its existence row whatever the flags)
    return bsi_build_layout(n_words, n_slices_out + 1u).total + div_work_bytes(n_words, n_slices_b);
}

int wah_bsi_div_indexed_device(int what, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, uint64_t n_slices_out,
                               const wah_bitop_operand *d_rows, unsigned flags, uint32_t *d_out, uint64_t out_capacity_words,
                               uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (what != WAH_DIV_QUOTIENT && what != WAH_DIV_REMAINDER) return refuse("unknown division result", WAH_ERR_ARG);
    const uint64_t rows_out = n_slices_out + 1u;
    if (const int rc = two_attribute_args(n_words, n_slices_a, n_slices_b, n_slices_out, rows_out, d_rows, flags, d_out, d_out_words, d_out_offsets, d_scratch))
        return rc;
    const BsiBuildLayout l = bsi_build_layout(n_words, rows_out);
    if (scratch_bytes < l.total + div_work_bytes(n_words, n_slices_b)) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    wah::BsiDivArgs a = {};
    two_attribute_fill(a, n_words, n_slices_a, n_slices_b, n_slices_out, d_rows, flags, sc, l);
    a.work = reinterpret_cast<uint32_t *>(sc + l.total); // (a multiple of 256 bytes: the quads are aligned)
    a.remainder = what == WAH_DIV_REMAINDER ? 1u : 0u;
    return sweep_then_compress(a, wah::launch_bsi_div_segments, "division sweep launch", n_words, rows_out, d_out, out_capacity_words,
                               d_out_words, d_out_offsets, sc, l, stream);
}

int wah_bsi_div_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_b, uint64_t n_slices_out, unsigned flags, void *stream) {
    (void)n_slices_b; // (the working area lies behind everything the status reads)
    (void)flags;
    return scratch_status_then(bsi_build_layout(n_words, n_slices_out + 1u).ws_c, d_scratch, stream);
}

// A bit-sliced key through a lookup table key -> value, as a new bit-sliced attribute (wah_map.hip, bsi_map_segments_kernel).  The
// builder's scratch and its road: the kernel writes the result's decoded slice matrix, the compress passes run over it.  The map
// and the key table stay in device memory: nothing here reads them.
static_assert(WAH_MAP_PARTIAL != WAH_BSI_EXISTS, "a flag bit of its own");
namespace {
constexpr unsigned kMapFlags = WAH_BSI_EXISTS | WAH_MAP_PARTIAL;
// the result's matrix rows: its slices, and the rows that have a value where either flag is set
inline uint64_t map_rows_out(uint64_t n_slices_out, unsigned flags) { return n_slices_out + ((flags & kMapFlags) ? 1u : 0u); }
} // namespace

size_t wah_bsi_map_scratch_bytes(uint64_t n_words, uint64_t n_slices_out, unsigned flags) {
    return bsi_build_layout(n_words, map_rows_out(n_slices_out, flags)).total;
}

int wah_bsi_map_indexed_device(uint64_t n_words, uint64_t n_rows, uint64_t n_slices_key, const wah_bitop_operand *d_key,
                               const uint32_t *d_map, uint64_t n_keys, uint64_t n_slices_out, unsigned flags, uint32_t *d_out,
                               uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                               size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_slices_key < 1 || n_slices_key > 32 || n_slices_out < 1 || n_slices_out > 32 || (flags & ~kMapFlags))
        return refuse("a key of 1 to 32 slices, a result of 1 to 32, no flag besides WAH_BSI_EXISTS and WAH_MAP_PARTIAL", WAH_ERR_ARG);
    if (!d_key || !aligned(d_key, 7) || !scratch_ok(d_scratch) || !out_triple_ok(d_out, d_out_words, d_out_offsets))
        return refuse("null or misaligned key table, scratch or output", WAH_ERR_ARG);
    if (!d_map || !aligned(d_map, 3) || n_keys < 1 || n_keys > (1ull << 32)) return refuse("a 4-byte aligned map of 1 to 2^32 keys", WAH_ERR_ARG);
    const uint64_t rows_out = map_rows_out(n_slices_out, flags);
    if (n_words == 0 || n_words % wah::kSegWords || n_words >= (1ull << 40) || rows_out * n_words >= (1ull << 40) || n_rows > 32 * n_words)
        return refuse("slices of a multiple of 992 words, all slices of the result together fewer than 2^40 words, at most 32 n_words rows", WAH_ERR_ARG);
    const BsiBuildLayout l = bsi_build_layout(n_words, rows_out);
    if (scratch_bytes < l.total) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    const SegGeometry g = seg_geometry(n_words);
    wah::BsiMapArgs a = {};
    a.key = reinterpret_cast<const wah::BitopListOperand *>(d_key);
    a.map = d_map;
    a.matrix = bsi_matrix(sc, l);
    a.ctrl = reinterpret_cast<uint32_t *>(sc);
    a.n_rows = n_rows;
    a.n_words = n_words;
    a.groups = g.groups;
    a.n_segments = g.n_segments;
    a.n_keys = n_keys;
    a.n_slices_key = (uint32_t)n_slices_key;
    a.n_slices_out = (uint32_t)n_slices_out;
    a.has_exists = (flags & WAH_BSI_EXISTS) ? 1u : 0u;
    a.out_exists = (flags & kMapFlags) ? 1u : 0u;
    a.partial = (flags & WAH_MAP_PARTIAL) ? 1u : 0u;
    return sweep_then_compress(a, wah::launch_bsi_map, "map launch", n_words, rows_out, d_out, out_capacity_words, d_out_words, d_out_offsets, sc, l,
                               stream);
}

int wah_bsi_map_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_out, unsigned flags, void *stream) {
    // (first the kernel: a bad key operand, a miss without WAH_MAP_PARTIAL, an entry too wide for the result)
    return scratch_status_then(bsi_build_layout(n_words, map_rows_out(n_slices_out, flags)).ws_c, d_scratch, stream);
}

// The running sum of a bit-sliced value over the selected rows, as a new bit-sliced attribute (wah_cumsum.hip).  The builder's
// scratch and its road, and behind them one u64 per segment: the segments' totals, scanned in place into their bases.  The
// kernels write the result's decoded slice matrix, the compress passes run over it.  The tables stay in device memory: nothing
// here reads them.
static_assert(WAH_CUMSUM_EXCLUSIVE != WAH_BSI_EXISTS && WAH_CUMSUM_ALL_ROWS != WAH_BSI_EXISTS && WAH_CUMSUM_EXCLUSIVE != WAH_CUMSUM_ALL_ROWS,
              "flag bits of their own");
namespace {
constexpr unsigned kCumsumFlags = WAH_BSI_EXISTS | WAH_CUMSUM_EXCLUSIVE | WAH_CUMSUM_ALL_ROWS;
// the result's matrix rows: its slices, and the selection unless every row holds a value
inline uint64_t cumsum_rows_out(uint64_t n_slices_out, unsigned flags) { return n_slices_out + ((flags & WAH_CUMSUM_ALL_ROWS) ? 0u : 1u); }
inline size_t cumsum_totals_bytes(uint64_t n_words) { return round256((size_t)(n_words / wah::kSegWords) * sizeof(uint64_t)); }
} // namespace

size_t wah_bsi_cumsum_scratch_bytes(uint64_t n_words, uint64_t n_slices_out, unsigned flags) {
    return bsi_build_layout(n_words, cumsum_rows_out(n_slices_out, flags)).total + cumsum_totals_bytes(n_words);
}

int wah_bsi_cumsum_indexed_device(uint64_t n_words, uint64_t n_rows, uint64_t n_filters, const wah_bitop_operand *d_filters,
                                  uint64_t n_slices_val, const wah_bitop_operand *d_val, uint64_t n_slices_out, unsigned flags,
                                  uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets,
                                  void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_slices_val > 32 || n_slices_out < 1 || n_slices_out > WAH_BSI_MAX_SLICES || (flags & ~kCumsumFlags) || n_filters > wah::kGroupMaxFilters)
        return refuse("a value of at most 32 slices, a result of 1 to 64, no flag besides WAH_BSI_EXISTS, WAH_CUMSUM_EXCLUSIVE and WAH_CUMSUM_ALL_ROWS, at most 64 filter rows", WAH_ERR_ARG);
    const bool has_val = n_slices_val != 0 || (flags & WAH_BSI_EXISTS);
    if (!scratch_ok(d_scratch) || !out_triple_ok(d_out, d_out_words, d_out_offsets) || has_val != (d_val != nullptr) || !aligned(d_val, 7) ||
        (n_filters && !d_filters) || !aligned(d_filters, 7))
        return refuse("null or misaligned scratch or output, a value table that does not go with n_slices_val and WAH_BSI_EXISTS, or a null or misaligned filter table", WAH_ERR_ARG);
    const uint64_t rows_out = cumsum_rows_out(n_slices_out, flags);
    if (n_words == 0 || n_words % wah::kSegWords || n_words >= (1ull << 40) || rows_out * n_words >= (1ull << 40) || n_rows > 32 * n_words)
        return refuse("slices of a multiple of 992 words, all slices of the result together fewer than 2^40 words, at most 32 n_words rows", WAH_ERR_ARG);
    const BsiBuildLayout l = bsi_build_layout(n_words, rows_out);
    if (scratch_bytes < l.total + cumsum_totals_bytes(n_words)) return refuse("scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    const SegGeometry g = seg_geometry(n_words);
    wah::BsiCumsumArgs a = {};
    a.filters = reinterpret_cast<const wah::BitopListOperand *>(d_filters);
    a.val = reinterpret_cast<const wah::BitopListOperand *>(d_val);
    a.totals = reinterpret_cast<uint64_t *>(sc + l.total); // (a multiple of 256 bytes)
    a.matrix = bsi_matrix(sc, l);
    a.ctrl = reinterpret_cast<uint32_t *>(sc);
    a.n_rows = n_rows;
    a.n_words = n_words;
    a.groups = g.groups;
    a.n_segments = g.n_segments;
    a.n_filters = (uint32_t)n_filters;
    a.n_slices_val = (uint32_t)n_slices_val;
    a.n_slices_out = (uint32_t)n_slices_out;
    a.has_exists = (flags & WAH_BSI_EXISTS) ? 1u : 0u;
    a.exclusive = (flags & WAH_CUMSUM_EXCLUSIVE) ? 1u : 0u;
    a.all_rows = (flags & WAH_CUMSUM_ALL_ROWS) ? 1u : 0u;
    return sweep_then_compress(a, wah::launch_bsi_cumsum, "running sum launch", n_words, rows_out, d_out, out_capacity_words, d_out_words,
                               d_out_offsets, sc, l, stream);
}

int wah_bsi_cumsum_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_out, unsigned flags, void *stream) {
    // (first the kernels: everything the list call refuses in a row of the filter table or the value table)
    return scratch_status_then(bsi_build_layout(n_words, cumsum_rows_out(n_slices_out, flags)).ws_c, d_scratch, stream);
}

// The running sum that starts again at every row of a starts bitmap (wah_cumsum.hip).  The road above, one more operand row, and
// behind the builder's layout one record of 16 bytes per segment: (tail sum, has_start), the sums scanned in place.
namespace {
inline size_t cumsum_parts_records_bytes(uint64_t n_words) { return round256((size_t)(n_words / wah::kSegWords) * sizeof(wah::BsiCumsumPartsRecord)); }
} // namespace

size_t wah_bsi_cumsum_parts_scratch_bytes(uint64_t n_words, uint64_t n_slices_out, unsigned flags) {
    return bsi_build_layout(n_words, cumsum_rows_out(n_slices_out, flags)).total + cumsum_parts_records_bytes(n_words);
}

int wah_bsi_cumsum_parts_indexed_device(uint64_t n_words, uint64_t n_rows, uint64_t n_filters, const wah_bitop_operand *d_filters,
                                        uint64_t n_slices_val, const wah_bitop_operand *d_val, const wah_bitop_operand *d_starts,
                                        uint64_t n_slices_out, unsigned flags, uint32_t *d_out, uint64_t out_capacity_words,
                                        uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_slices_val > 32 || n_slices_out < 1 || n_slices_out > WAH_BSI_MAX_SLICES || (flags & ~kCumsumFlags) || n_filters > wah::kGroupMaxFilters)
        return refuse("partitioned running sum: a value of at most 32 slices, a result of 1 to 64, no flag besides WAH_BSI_EXISTS, WAH_CUMSUM_EXCLUSIVE and WAH_CUMSUM_ALL_ROWS, at most 64 filter rows", WAH_ERR_ARG);
    const bool has_val = n_slices_val != 0 || (flags & WAH_BSI_EXISTS);
    if (!scratch_ok(d_scratch) || !out_triple_ok(d_out, d_out_words, d_out_offsets) || has_val != (d_val != nullptr) || !aligned(d_val, 7) ||
        (n_filters && !d_filters) || !aligned(d_filters, 7) || !d_starts || !aligned(d_starts, 7))
        return refuse("partitioned running sum: null or misaligned scratch or output, a value table that does not go with n_slices_val and WAH_BSI_EXISTS, a null or misaligned filter table, or a null or misaligned starts row", WAH_ERR_ARG);
    const uint64_t rows_out = cumsum_rows_out(n_slices_out, flags);
    if (n_words == 0 || n_words % wah::kSegWords || n_words >= (1ull << 40) || rows_out * n_words >= (1ull << 40) || n_rows > 32 * n_words)
        return refuse("partitioned running sum: slices of a multiple of 992 words, all slices of the result together fewer than 2^40 words, at most 32 n_words rows", WAH_ERR_ARG);
    const BsiBuildLayout l = bsi_build_layout(n_words, rows_out);
    if (scratch_bytes < l.total + cumsum_parts_records_bytes(n_words)) return refuse("partitioned running sum: scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    const SegGeometry g = seg_geometry(n_words);
    wah::BsiCumsumPartsArgs a = {};
    a.c.filters = reinterpret_cast<const wah::BitopListOperand *>(d_filters);
    a.c.val = reinterpret_cast<const wah::BitopListOperand *>(d_val);
    a.starts = reinterpret_cast<const wah::BitopListOperand *>(d_starts);
    a.records = reinterpret_cast<wah::BsiCumsumPartsRecord *>(sc + l.total); // (a multiple of 256 bytes)
    a.c.matrix = bsi_matrix(sc, l);
    a.c.ctrl = reinterpret_cast<uint32_t *>(sc);
    a.c.n_rows = n_rows;
    a.c.n_words = n_words;
    a.c.groups = g.groups;
    a.c.n_segments = g.n_segments;
    a.c.n_filters = (uint32_t)n_filters;
    a.c.n_slices_val = (uint32_t)n_slices_val;
    a.c.n_slices_out = (uint32_t)n_slices_out;
    a.c.has_exists = (flags & WAH_BSI_EXISTS) ? 1u : 0u;
    a.c.exclusive = (flags & WAH_CUMSUM_EXCLUSIVE) ? 1u : 0u;
    a.c.all_rows = (flags & WAH_CUMSUM_ALL_ROWS) ? 1u : 0u;
    return sweep_then_compress(a, wah::launch_bsi_cumsum_parts, "partitioned running sum launch", n_words, rows_out, d_out, out_capacity_words,
                               d_out_words, d_out_offsets, sc, l, stream);
}

int wah_bsi_cumsum_parts_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_out, unsigned flags, void *stream) {
    // (first the kernels: everything the list call refuses in a row of the filter table, the value table or the starts row)
    return scratch_status_then(bsi_build_layout(n_words, cumsum_rows_out(n_slices_out, flags)).ws_c, d_scratch, stream);
}

// The partition's total in every one of its rows (wah_cumsum.hip).  The road above with records of 24 bytes per segment:
// (head, tail, has_start), head and tail scanned in place from behind and from the front.  No WAH_CUMSUM_EXCLUSIVE.
namespace {
constexpr unsigned kTotalPartsFlags = WAH_BSI_EXISTS | WAH_CUMSUM_ALL_ROWS;
inline size_t total_parts_records_bytes(uint64_t n_words) { return round256((size_t)(n_words / wah::kSegWords) * sizeof(wah::BsiTotalPartsRecord)); }
} // namespace

size_t wah_bsi_total_parts_scratch_bytes(uint64_t n_words, uint64_t n_slices_out, unsigned flags) {
    return bsi_build_layout(n_words, cumsum_rows_out(n_slices_out, flags)).total + total_parts_records_bytes(n_words);
}

int wah_bsi_total_parts_indexed_device(uint64_t n_words, uint64_t n_rows, uint64_t n_filters, const wah_bitop_operand *d_filters,
                                       uint64_t n_slices_val, const wah_bitop_operand *d_val, const wah_bitop_operand *d_starts,
                                       uint64_t n_slices_out, unsigned flags, uint32_t *d_out, uint64_t out_capacity_words,
                                       uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream) {
    g_err[0] = 0;
    if (n_slices_val > 32 || n_slices_out < 1 || n_slices_out > WAH_BSI_MAX_SLICES || (flags & ~kTotalPartsFlags) || n_filters > wah::kGroupMaxFilters)
        return refuse("partition totals: a value of at most 32 slices, a result of 1 to 64, no flag besides WAH_BSI_EXISTS and WAH_CUMSUM_ALL_ROWS, at most 64 filter rows", WAH_ERR_ARG);
    const bool has_val = n_slices_val != 0 || (flags & WAH_BSI_EXISTS);
    if (!scratch_ok(d_scratch) || !out_triple_ok(d_out, d_out_words, d_out_offsets) || has_val != (d_val != nullptr) || !aligned(d_val, 7) ||
        (n_filters && !d_filters) || !aligned(d_filters, 7) || !d_starts || !aligned(d_starts, 7))
        return refuse("partition totals: null or misaligned scratch or output, a value table that does not go with n_slices_val and WAH_BSI_EXISTS, a null or misaligned filter table, or a null or misaligned starts row", WAH_ERR_ARG);
    const uint64_t rows_out = cumsum_rows_out(n_slices_out, flags);
    if (n_words == 0 || n_words % wah::kSegWords || n_words >= (1ull << 40) || rows_out * n_words >= (1ull << 40) || n_rows > 32 * n_words)
        return refuse("partition totals: slices of a multiple of 992 words, all slices of the result together fewer than 2^40 words, at most 32 n_words rows", WAH_ERR_ARG);
    const BsiBuildLayout l = bsi_build_layout(n_words, rows_out);
    if (scratch_bytes < l.total + total_parts_records_bytes(n_words)) return refuse("partition totals: scratch too small", WAH_ERR_WORKSPACE);
    char *sc = static_cast<char *>(d_scratch);
    const SegGeometry g = seg_geometry(n_words);
    wah::BsiTotalPartsArgs a = {};
    wah::BsiCumsumArgs &c = a.p.c;
    c.filters = reinterpret_cast<const wah::BitopListOperand *>(d_filters);
    c.val = reinterpret_cast<const wah::BitopListOperand *>(d_val);
    a.p.starts = reinterpret_cast<const wah::BitopListOperand *>(d_starts);
    a.records = reinterpret_cast<wah::BsiTotalPartsRecord *>(sc + l.total); // (a multiple of 256 bytes)
    c.matrix = bsi_matrix(sc, l);
    c.ctrl = reinterpret_cast<uint32_t *>(sc);
    c.n_rows = n_rows;
    c.n_words = n_words;
    c.groups = g.groups;
    c.n_segments = g.n_segments;
    c.n_filters = (uint32_t)n_filters;
    c.n_slices_val = (uint32_t)n_slices_val;
    c.n_slices_out = (uint32_t)n_slices_out;
    c.has_exists = (flags & WAH_BSI_EXISTS) ? 1u : 0u;
    c.all_rows = (flags & WAH_CUMSUM_ALL_ROWS) ? 1u : 0u;
    return sweep_then_compress(a, wah::launch_bsi_total_parts, "partition totals launch", n_words, rows_out, d_out, out_capacity_words, d_out_words,
                               d_out_offsets, sc, l, stream);
}

int wah_bsi_total_parts_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_out, unsigned flags, void *stream) {
    // (first the kernels: everything the list call refuses in a row of the filter table, the value table or the starts row)
    return scratch_status_then(bsi_build_layout(n_words, cumsum_rows_out(n_slices_out, flags)).ws_c, d_scratch, stream);
}

// ---------------------------------------------------------------------------
// host-pointer entry points (the reference's API)
// ---------------------------------------------------------------------------
uint32_t *wah_compress(const uint32_t *data_host, uint64_t n_words, uint64_t *out_words, float *t_to_device_ms,
                       float *t_device_ms, float *t_from_device_ms) {
    g_err[0] = 0;
    if (n_words && !data_host) {
        set_err("null input");
        std::fprintf(stderr, "wah: compress() called with a null input\n");
        return nullptr;
    }
    HostCall hc;
    if (!hc.init()) {
        set_err("hipEventCreate failed (no usable GPU?)");
        std::fprintf(stderr, "wah: %s\n", g_err);
        return nullptr;
    }
    float t_in = 0.f, t_dev = 0.f, t_out = 0.f;

    // phase 1: allocate + H2D (compress.cu:57-120)
    hc.start();
    const uint64_t cap = wah_max_compressed_words(n_words);
    void *d_in = nullptr, *d_out = nullptr, *d_ws = nullptr;
    // (one word more than the data: the buffer is decompress()'s output buffer next, and a bitmap whose length is not a
    //  multiple of 31 decodes to one padding word more, decompress.cu:84-93)
    if (!hc.alloc(0, &d_in, (n_words + 1) * sizeof(uint32_t), "space for the data")) return nullptr;
    if (!hc.alloc(1, &d_out, cap * sizeof(uint32_t), "space for the compressed output")) return nullptr;
    bool fresh_ws = false;
    if (!hc.alloc(2, &d_ws, wah_compress_workspace_bytes(n_words), "workspace", &fresh_ws)) return nullptr;
    // a kept workspace is named with ITS size, call after call, whatever this call needs of it: where a launch keeps its
    // entries follows from the size it is given (include/wah.h), and entries that moved with the input's size would let
    // one call's tables be read as another call's published entries
    const size_t ws_bytes = hc.cache.cap[2];
    // the compress workspace is zeroed once; from then on the kernel keeps it up itself (launch epochs)
    if (fresh_ws && wah_workspace_init_device(d_ws, ws_bytes, nullptr) != WAH_OK) return nullptr;
    uint64_t *d_cnt = reinterpret_cast<uint64_t *>(static_cast<uint32_t *>(d_ws) + wah::kCtlResult); // beside the error word
    if (n_words && !hip_ok(hipMemcpy(d_in, data_host, n_words * sizeof(uint32_t), hipMemcpyHostToDevice), "copy input"))
        return nullptr;
    t_in = hc.stop();

    // phase 2: device work (compress.cu:125-172)
    hc.start();
    uint64_t *const host_result = reinterpret_cast<uint64_t *>(hc.cache.pinned) + 4; // behind the copy's landing area
    host_result[0] = 0;
    int rc = compress_device_impl(static_cast<uint32_t *>(d_in), nullptr, 0, nullptr, n_words, static_cast<uint32_t *>(d_out), cap, d_cnt,
                                  nullptr, d_ws, ws_bytes, nullptr, false, n_words ? host_result : nullptr);
    hc.mark();
    uint64_t c = 0;
    if (rc == WAH_OK) rc = wait_host_result(host_result, d_ws, hc.cache.pinned, &c, 1); // status + size: one wait, no copy
    if (rc == WAH_OK && test_timeout_hook()) rc = WAH_ERR_TIMEOUT;
    if (rc == WAH_ERR_TIMEOUT) {
        // A bounded wait inside the kernel expired: a workgroup this launch depended on did not get to run in time (a GPU
        // shared in a way the arrival tickets do not cover, a preempted queue).  The no-wait route has no such
        // dependency: three launches, the bitmap read twice, the same stream.
        std::fprintf(stderr, "wah: compress: in-kernel wait expired, taking the no-wait route\n");
        host_result[0] = 0;
        rc = compress_device_impl(static_cast<uint32_t *>(d_in), nullptr, 0, nullptr, n_words, static_cast<uint32_t *>(d_out), cap, d_cnt,
                                  nullptr, d_ws, ws_bytes, nullptr, false, host_result, nullptr, false, true);
        hc.mark(); // the device phase ends with this route's last launch
        if (rc == WAH_OK) rc = wait_host_result(host_result, d_ws, hc.cache.pinned, &c, 1);
        // (the abandoned launch left its tickets and its epoch half way: the next call starts from a fresh workspace,
        //  whatever became of this one)
        if (wah_workspace_init_device(d_ws, ws_bytes, nullptr) != WAH_OK && rc == WAH_OK) rc = WAH_ERR_HIP;
    }
    if (rc != WAH_OK) {
        std::fprintf(stderr, "wah: compress failed: %s\n", g_err);
        return nullptr;
    }
    t_dev = hc.since_mark();

    // phase 3: D2H + free (compress.cu:177-202)
    hc.start();
    bool huge = false;
    uint32_t *host = static_cast<uint32_t *>(host_result_alloc(c * sizeof(uint32_t), &huge));
    if (!host) {
        set_err("host malloc failed");
        return nullptr;
    }
    if (c && !copy_to_fresh_host(host, d_out, c * sizeof(uint32_t), huge, "copy final output")) {
        std::free(host);
        return nullptr;
    }
    hc.release();
    t_out = hc.stop();

    if (out_words) *out_words = c;
    if (t_to_device_ms) *t_to_device_ms = t_in;
    if (t_device_ms) *t_device_ms = t_dev;
    if (t_from_device_ms) *t_from_device_ms = t_out;
    return host;
}

uint32_t *wah_decompress(const uint32_t *comp_host, uint64_t c_words, uint64_t *out_words, float *t_to_device_ms,
                         float *t_device_ms, float *t_from_device_ms) {
    g_err[0] = 0;
    if (c_words && !comp_host) {
        set_err("null input");
        std::fprintf(stderr, "wah: decompress() called with a null input\n");
        return nullptr;
    }
    HostCall hc;
    if (!hc.init()) {
        set_err("hipEventCreate failed (no usable GPU?)");
        std::fprintf(stderr, "wah: %s\n", g_err);
        return nullptr;
    }
    float t_in = 0.f, t_dev = 0.f, t_out = 0.f;

    // phase 1: allocate + H2D (decompress.cu:34-54)
    hc.start();
    void *d_comp = nullptr, *d_ws0 = nullptr;
    if (!hc.alloc(1, &d_comp, c_words * sizeof(uint32_t), "space for the compressed data")) return nullptr;
    bool fresh_ws = false;
    if (!hc.alloc(4, &d_ws0, wah_decompress_workspace_bytes(c_words, 0), "scan workspace", &fresh_ws)) return nullptr;
    const size_t ws0 = hc.cache.cap[4]; // (named with its own size every time: see wah_compress)
    // zeroed once; from then on the sums kernel keeps it up itself (launch epochs)
    if (fresh_ws && wah_workspace_init_device(d_ws0, ws0, nullptr) != WAH_OK) return nullptr;
    uint64_t *d_info = reinterpret_cast<uint64_t *>(static_cast<uint32_t *>(d_ws0) + wah::kCtlResult); // beside the error word
    // which decoder: a look at the stream itself, which lies in host memory -- the group counts of up to 65 536 words spread
    // evenly over it.  One pass up to 7 groups per word; the two launches from there to 128 (tools/report.py, 992 MiB, device
    // phase: one bit in 2^11 = 32 groups per word 0.248 ms in one pass against 0.223, 2^12 0.223 / 0.210, 2^14 0.209 / 0.203 --
    // through this boundary the one-pass kernel's longer workgroups show on a stream of a few megabytes); above: the same.
    // (BEFORE the copy: a device left idle for the millisecond this takes starts its next kernel slower)
    // The same sample says how large the bitmap will be, to a percent or so (exactly, for a stream of up to 65 536 words): see
    // phase 2.
    int route = 1;
    uint64_t expect_words = 0; // decoded words the sample predicts (0: no prediction)
    if (c_words) {
        uint64_t sampled = 0, sample_groups = 0;
        const uint64_t stride = c_words > 65536 ? c_words / 65536 : 1;
        for (uint64_t i = 0; i < c_words; i += stride, ++sampled)
            sample_groups += (comp_host[i] & wah::kFillZero) ? (comp_host[i] & wah::kCountMask) : 1u;
        const uint64_t per_word = sample_groups / (sampled ? sampled : 1);
        route = (per_word <= 7 || per_word >= 128) ? 1 : 2;
        const unsigned __int128 groups = (unsigned __int128)sample_groups * c_words / (sampled ? sampled : 1);
        if (groups < ((unsigned __int128)1 << 40)) expect_words = ((uint64_t)groups * 31u + 31u) / 32u;
    }
    if (c_words && !hip_ok(hipMemcpy(d_comp, comp_host, c_words * sizeof(uint32_t), hipMemcpyHostToDevice), "copy input"))
        return nullptr;
    t_in = hc.stop();

    // phase 2: device work (decompress.cu:56-122): size scan, allocate, scan + expand
    hc.start();
    uint64_t info[2] = {0, 0};
    void *d_out = nullptr;
    int rc = WAH_OK;
    bool expanded = false, no_wait = false;
    // An output buffer kept from an earlier call (the reference's callers decompress in loops, source.cpp:70): expand
    // right behind the scan, into what is there -- the expand kernel compares the decoded size with the capacity on the
    // device and writes nothing if it does not fit.  One host round trip for the whole phase instead of two.
    // Without one -- a process's first call, a bitmap larger than any before -- the reference's order (scan, read the size back,
    // allocate, expand: decompress.cu:72-100) would read the stream twice and wait for the device twice: instead a buffer of
    // the size the SAMPLE predicts, plus a sixteenth (+ 64 Ki words: a sample of 65 536 words is good to about a percent), and
    // the same single pass.  A prediction that was too small costs what a kept buffer that is too small costs: the decoder
    // reports WAH_ERR_CAPACITY and the call goes by the book below; a buffer the device cannot give: by the book, too.
    size_t kept_words = hc.cache.buf[0] ? hc.cache.cap[0] / sizeof(uint32_t) : 0;
    if (c_words && expect_words && kept_words < expect_words) {
        const uint64_t want = expect_words + expect_words / 16u + 65536u;
        void *grown = nullptr;
        if (hc.alloc(0, &grown, want * sizeof(uint32_t), "space for the result", nullptr, true)) kept_words = want;
        else kept_words = 0; // (alloc has dropped the smaller buffer)
    }
    if (c_words && kept_words) {
        rc = decode_common(static_cast<uint32_t *>(d_comp), c_words, static_cast<uint32_t *>(hc.cache.buf[0]), kept_words, d_info, d_ws0,
                           ws0, nullptr, true, true, false, nullptr, false, route);
        hc.mark();
        if (rc == WAH_OK) rc = read_status_packed(d_ws0, hc.cache.pinned, info, 2); // status + sizes in one copy
        if (rc == WAH_OK && test_timeout_hook()) rc = WAH_ERR_TIMEOUT;
        if (rc == WAH_OK) {
            d_out = hc.cache.buf[0];
            expanded = true;
        } else if (rc == WAH_ERR_TIMEOUT) {
            no_wait = true; // (by the book below, without waits)
        } else if (rc != WAH_ERR_CAPACITY) {
            std::fprintf(stderr, "wah: decompress failed: %s\n", g_err);
            return nullptr;
        } // (too small: by the book below)
    }
    if (!expanded) {
        uint64_t *const host_result = reinterpret_cast<uint64_t *>(hc.cache.pinned) + 4; // behind the copy's landing area
        host_result[0] = 0;
        rc = decode_common(static_cast<uint32_t *>(d_comp), c_words, nullptr, 0, d_info, d_ws0, ws0, nullptr, true, false, false,
                           c_words ? host_result : nullptr, no_wait);
        if (rc == WAH_OK) rc = wait_host_result(host_result, d_ws0, hc.cache.pinned, info, 2); // status + sizes: one wait, no copy
        if (rc == WAH_OK && !no_wait && test_timeout_hook()) rc = WAH_ERR_TIMEOUT;
        if (rc == WAH_ERR_TIMEOUT && !no_wait) {
            // A bounded wait inside the sums kernel expired (see wah_compress): the no-wait route has no such dependency --
            // per-tile totals, then one scan launch, the reference's own shape (decompress.cu:66-80).
            std::fprintf(stderr, "wah: decompress: in-kernel wait expired, taking the no-wait route\n");
            no_wait = true;
            host_result[0] = 0;
            rc = decode_common(static_cast<uint32_t *>(d_comp), c_words, nullptr, 0, d_info, d_ws0, ws0, nullptr, true, false, false,
                               c_words ? host_result : nullptr, true);
            if (rc == WAH_OK) rc = wait_host_result(host_result, d_ws0, hc.cache.pinned, info, 2);
        }
        if (rc != WAH_OK) {
            std::fprintf(stderr, "wah: decompress failed: %s\n", g_err);
            return nullptr;
        }
        if (!hc.alloc(0, &d_out, info[0] * sizeof(uint32_t), "space for the result")) return nullptr;
        // the tile bases of the scan are still in the workspace: expand only
        rc = wah_decompress_expand_device(static_cast<uint32_t *>(d_comp), c_words, static_cast<uint32_t *>(d_out), info[0], d_info,
                                          d_ws0, ws0, nullptr);
        hc.mark();
        if (rc == WAH_OK) rc = read_status_packed(d_ws0, hc.cache.pinned, nullptr, 0);
        if (rc != WAH_OK) {
            std::fprintf(stderr, "wah: decompress failed: %s\n", g_err);
            return nullptr;
        }
    }
    const uint64_t n_out = info[0], groups = info[1];
    t_dev = hc.since_mark();
    // (after a timeout the abandoned launch left its tickets and its epoch half way: the next call starts from a fresh workspace)
    if (no_wait && wah_workspace_init_device(d_ws0, ws0, nullptr) != WAH_OK) return nullptr;

    // phase 3: D2H + free (decompress.cu:124-131).  The reference hands back a buffer of G words
    // (one per group) of which ceil(31 G / 32) are meaningful; we keep the size and zero the rest.
    hc.start();
    bool huge = false;
    uint32_t *host = static_cast<uint32_t *>(host_result_alloc(groups * sizeof(uint32_t), &huge));
    if (!host) {
        set_err("host malloc failed");
        return nullptr;
    }
    if (groups > n_out) std::memset(host + n_out, 0, (groups - n_out) * sizeof(uint32_t));
    if (groups == 0) host[0] = 0;
    if (n_out && !copy_to_fresh_host(host, d_out, n_out * sizeof(uint32_t), huge, "copy final output")) {
        std::free(host);
        return nullptr;
    }
    hc.release();
    t_out = hc.stop();

    if (out_words) *out_words = n_out;
    if (t_to_device_ms) *t_to_device_ms = t_in;
    if (t_device_ms) *t_device_ms = t_dev;
    if (t_from_device_ms) *t_from_device_ms = t_out;
    return host;
}

} // extern "C"

// ---------------------------------------------------------------------------
// The reference's own symbols, C++ linkage (compress.h:12-18, decompress.h:11-17):
// _Z8compressPjyPyPfS1_S1_ and _Z10decompressPjyPyPfS1_S1_.
// ---------------------------------------------------------------------------
unsigned int *compress(unsigned int *data_cpu, unsigned long long int dataSize, unsigned long long int *outputSize,
                       float *pTransferToDeviceTime, float *pCompressionTime, float *ptranserFromDeviceTime) {
    uint64_t c = 0;
    uint32_t *r = wah_compress(data_cpu, dataSize, &c, pTransferToDeviceTime, pCompressionTime, ptranserFromDeviceTime);
    if (r && outputSize) *outputSize = c;
    return r;
}

unsigned int *decompress(unsigned int *data, unsigned long long int dataSize, unsigned long long int *outSize,
                         float *pTransferToDeviceTime, float *pCompressionTime, float *ptranserFromDeviceTime) {
    uint64_t n = 0;
    uint32_t *r = wah_decompress(data, dataSize, &n, pTransferToDeviceTime, pCompressionTime, ptranserFromDeviceTime);
    if (r && outSize) *outSize = n;
    return r;
}
