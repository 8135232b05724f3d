/*
 * wah.h -- C ABI of the MI355X-native WAH bitmap compressor / decompressor.
 *
 * This is the drop-in boundary for the reference's hot path.  Every entry point
 * is `extern "C"`, takes plain pointers and sizes, and names the reference
 * interface it replaces.  The reference's own two symbols have C++ linkage
 * (compress.h:12-18, decompress.h:11-17 carry no extern "C"); the library also
 * exports those, declared in include/compress.h and include/decompress.h, so
 * the reference's source.cpp / tests.cpp link against libwah_hip.so unchanged.
 *
 * Units: all sizes are in 32-bit words unless a name says bytes
 * (compress.cu:35-36, decompress.cu:12-13).  Sizes, word indices and offsets are
 * 64-bit throughout; a bitmap or a stream of 2^40 words (4 TiB) or more is
 * refused with WAH_ERR_ARG (the reference: int indices, dataSize < 2^31,
 * kernels.cu:51).  Tested on the GPU up to one launch of 4 362 072 000 words
 * (130 columns of 128 MiB: tests/test_gpu_parity.py).
 *
 * Wire format (reference const.h:3-16, kernels.cu:79,244-249,298-354):
 * 31-bit groups of the LSB-first bit stream; literal = group (bit31 = 0);
 * fill = 0x80000000 | bit<<30 | count; fills are maximal inside a segment of
 * 1024 groups (= 992 input words) and never cross a segment boundary.
 */
#ifndef WAH_H_
#define WAH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: what this header declares (and the reference's two C++ symbols of
 * compress.h / decompress.h) is ALL it exports (tests/test_abi.py checks the dynamic symbol table) */
#pragma GCC visibility push(default)

#define WAH_SEGMENT_WORDS 992u   /* compress.cu:62  blockCount = dataSize / (31*32) */
#define WAH_SEGMENT_GROUPS 1024u /* kernels.cu:68   one (32,32) CUDA block          */

/* status codes of the device-pointer API (0 = success) */
#define WAH_OK 0
#define WAH_ERR_ARG (-1)      /* null / misaligned pointer, size out of range        */
#define WAH_ERR_WORKSPACE (-2) /* workspace too small, or never initialised           */
#define WAH_ERR_HIP (-3)      /* a HIP runtime call failed (see wah_last_error())    */
#define WAH_ERR_CAPACITY (-4) /* output buffer too small (reported by wah_*_status)  */
#define WAH_ERR_TIMEOUT (-5)  /* an in-kernel bounded wait expired                   */
#define WAH_ERR_STREAM (-6)   /* malformed compressed stream                         */

/* ------------------------------------------------------------------------- *
 * Host-pointer entry points: the reference's API.
 * ------------------------------------------------------------------------- */

/* Replaces compress() -- compress.h:12-18, compress.cu:41-209.
 * data_host: caller-owned host memory, read only, n_words words.
 * Returns a malloc()ed host buffer of *out_words compressed words (release
 * with free() or wah_free()), or NULL on error (message on stderr;
 * compress.cu:89-114 prints and returns NULL).  out_words and the three
 * timing pointers may be NULL (timeMeasuring.h:27-28).  Timings are
 * milliseconds from device events: (alloc + H2D), (device work), (D2H + free)
 * -- compress.cu:117-120,169-172,199-202. */
uint32_t *wah_compress(const uint32_t *data_host, uint64_t n_words, uint64_t *out_words, float *t_to_device_ms,
                       float *t_device_ms, float *t_from_device_ms);

/* Replaces decompress() -- decompress.h:11-17, decompress.cu:18-141.
 * comp_host: c_words compressed words.  Returns a malloc()ed buffer holding G
 * words (G = number of 31-bit groups, decompress.cu:127) of which the first
 * *out_words = ceil(31*G/32) are the bitmap (decompress.cu:84-93); the rest
 * are zero.  NULL on error. */
uint32_t *wah_decompress(const uint32_t *comp_host, uint64_t c_words, uint64_t *out_words, float *t_to_device_ms,
                         float *t_device_ms, float *t_from_device_ms);

/* free() for buffers returned above (source.cpp:108-109, tests.h:22 use free()). */
void wah_free(void *p);

/* The two entry points above keep their device buffers between calls (grow-only, one set per device; calls
 * from several threads take turns), where the reference allocates and frees inside every call
 * (compress.cu:57-114,177-202; decompress.cu:34-54,124-131).  This returns them to the device now; setting
 * WAH_HOST_CACHE=0 in the environment restores allocate-and-free per call.
 * decompress() does not know the decoded size before it has scanned the stream (nor does the reference,
 * decompress.cu:72-97).  With a kept buffer that is large enough -- the one a compress() or decompress() of this
 * process left behind: the reference's callers run them in turn on one size, source.cpp:70-103 -- it decodes into it in
 * ONE pass, one host round trip; without one (a process's first call, a larger bitmap than any before) it sizes one
 * from a sample of the stream in host memory (the group counts of 65 536 words spread evenly over it, plus a
 * sixteenth) and does the same.  Only when that prediction was too small (a foreign stream whose long fills the sample
 * missed) does it go by the reference's order: scan the stream, read the size back, allocate, expand -- two passes
 * over the stream, two round trips.
 *
 * Environment read by the library (nothing else is; the one experiment switch, WAH_BITOP_ROUTE, exists only in builds
 * made with -DWAH_EXPERIMENTS): WAH_HOST_CACHE=0 (above); WAH_FORCE_FALLBACK=1 (every launch by its no-wait route, below);
 * WAH_FAULT_INJECT=timeout -- fault injection: compress() / decompress() treat their first launch as if a bounded
 * in-kernel wait had expired and take the no-wait route by themselves, as they would on a GPU shared in a way that
 * starves the waits (the reference has no failure handling to compare with, compress.cu:89-114). */
void wah_host_cache_release(void);

/* ------------------------------------------------------------------------- *
 * Sizes.
 * ------------------------------------------------------------------------- */

/* ceil(32*n/31): number of 31-bit groups == worst-case compressed size
 * (compress.cu:74-81 maxExpectedSize). */
uint64_t wah_max_compressed_words(uint64_t n_words);

/* ceil(31*G/32): words a stream of G groups decodes to (decompress.cu:84-93). */
uint64_t wah_decoded_words(uint64_t n_groups);

/* Scratch the device-pointer calls need (bytes; 256-byte aligned pointer). */
size_t wah_compress_workspace_bytes(uint64_t n_words);
size_t wah_decompress_workspace_bytes(uint64_t c_words, uint64_t out_capacity_words);

/* ------------------------------------------------------------------------- *
 * Device-pointer entry points (inputs and outputs resident in HBM, caller's
 * stream, no allocation, no host synchronisation -- graph capturable).  These
 * replace the kernel + scan sections of the reference hosts:
 *   compress.cu:129-166  compressData -> exclusive_scan -> moveData
 *   decompress.cu:66-115 getCounts -> exclusive_scan -> decompressWords -> mergeWords
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).
 * ------------------------------------------------------------------------- */

/* A workspace (compress, decompress, merge_fills) is initialised ONCE (all zero bytes: this call, or any memset) and
 * then keeps itself up: every launch stamps what it leaves there with a launch epoch, so nothing is cleared between
 * launches, and one workspace may serve inputs of different sizes (up to the one it was sized for) in turn -- but only
 * one launch at a time.  A workspace that is neither zeroed nor left by an earlier launch is reported as
 * WAH_ERR_WORKSPACE by the status calls (checked: the magic word, the launch epoch, and every tile number drawn from
 * the ticket counter, before anything is indexed with it).  Where a launch keeps its entries depends on the workspace's
 * size only, so pass the SAME workspace_bytes with a workspace every time.  (The `scratch` of the wah_bitop_* calls
 * needs no initialisation.)  Asynchronous on `stream`. */
int wah_workspace_init_device(void *d_workspace, size_t workspace_bytes, void *stream);

/* d_in: n_words words, 16-byte aligned (a pointer that is only 4-byte aligned is accepted and takes slower loads).
 * d_out: room for out_capacity_words (wah_max_compressed_words(n) always suffices; exactly C is enough), 4-byte aligned:
 * every store of the output goes through a descriptor that starts at a word of its own and ends with the capacity, so
 * the output may start at any word and nothing is written in front of it or behind it.  d_out_words: one device
 * uint64 that receives C.  d_workspace: wah_compress_workspace_bytes(n_words) bytes or more, initialised as above.
 * Result status is left in the workspace; read it with wah_compress_status() after the stream has been synchronised.
 * One kernel launch, nothing else: no clearing pass, no residency requirement (the kernel's workgroups are short-lived
 * and only ever wait for workgroups dispatched before them), so it shares the GPU with other work like any kernel. */
int wah_compress_device(const uint32_t *d_in, uint64_t n_words, uint32_t *d_out, uint64_t out_capacity_words,
                        uint64_t *d_out_words, void *d_workspace, size_t workspace_bytes, void *stream);

/* The same with flags.  WAH_UNSEGMENTED: classic WAH straight out of the encoder -- a fill may cross the 1024-group
 * segment cut of the reference (kernels.cu:68,188-229; never a multiple of 2^29 groups, so that every count fits 30
 * bits): exactly the stream wah_merge_fills_device makes of wah_compress_device's, in the one pass.  It
 * decodes to the same bitmap with wah_decompress*; it is not what the reference's encoder emits and has no segment
 * index. */
#define WAH_UNSEGMENTED 1u
/* WAH_NO_WAIT: the same stream as wah_compress_device by a route in which no workgroup ever waits for another: three
 * launches -- count (every tile's word count to a table), one exclusive scan of the table, place (every tile again,
 * its words to their place) -- and the bitmap is read twice (about 1.6 x the time).  The one-launch kernel resolves its
 * offsets with bounded in-kernel waits on workgroups that started earlier (reference: thrust::exclusive_scan between two
 * kernels, compress.cu:129-166); should such a wait ever expire the launch reports WAH_ERR_TIMEOUT, and this is the
 * route to take instead: compress() does so by itself, a caller of the device API passes the flag (or sets
 * WAH_FORCE_FALLBACK=1 in the environment, which sends every plain compress launch this way).  Combined with
 * WAH_UNSEGMENTED: the unsegmented stream by the same three launches.  The route itself reads nothing of the workspace's earlier content; before the one-launch kernel is used
 * again after a WAH_ERR_TIMEOUT the workspace must be initialised again (wah_workspace_init_device). */
#define WAH_NO_WAIT 2u
int wah_compress_device_ex(const uint32_t *d_in, uint64_t n_words, uint32_t *d_out, uint64_t out_capacity_words,
                           uint64_t *d_out_words, unsigned flags, void *d_workspace, size_t workspace_bytes, void *stream);

/* Optional side output: when d_segment_offsets != NULL it receives, for every
 * 992-word segment s, the index of its first compressed word
 * (n_segments + 1 entries, the last one = C).  This is the reference's scanned
 * blockCounts array (compress.cu:146) kept instead of thrown away. */
int wah_compress_device_indexed(const uint32_t *d_in, uint64_t n_words, uint32_t *d_out, uint64_t out_capacity_words,
                                uint64_t *d_out_words, uint64_t *d_segment_offsets, void *d_workspace,
                                size_t workspace_bytes, void *stream);

/* Synchronises `stream`, returns WAH_OK or the error a compress launch recorded. */
int wah_compress_status(void *d_workspace, void *stream);

/* Column shards over several GPUs of a node (the reference is one device, default stream:
 * compress.cu:129,166).  Columns are independent bitmaps, so there is nothing to exchange: every shard is the column
 * matrix one device owns (n_columns columns of n_words_per_column words, back to back in that device's memory, every
 * column a whole number of 992-word segments so that no fill crosses a column), compressed by ONE launch on a stream of
 * its own by a host thread of its own that makes `device` current -- no collective, no peer access, no RCCL.  All the
 * other entry points of this header work on the device that is current in the calling thread; this one names its
 * devices.  Per shard: d_out receives the columns' streams back to back (capacity out_capacity_words;
 * wah_max_compressed_words(n_columns * n_words_per_column) always suffices), d_out_words their total,
 * d_segment_offsets (n_columns * n_words_per_column / 992 + 1 entries) the first word of every segment -- column c of
 * the shard starts at entry c * n_words_per_column / 992 --, d_workspace an initialised workspace of
 * wah_compress_workspace_bytes(n_columns * n_words_per_column) bytes on that device.  Returns when every shard has
 * finished: WAH_OK, or the first error (shard order); status[i], if status != NULL, receives shard i's own code.
 * The launches run on streams of the call's own: inputs and workspaces must be complete when it is made (synchronise
 * whatever other stream wrote them), and the outputs are complete when it returns.
 * Several shards may name the same device (they then share it like any two streams). */
typedef struct {
    int device;                 /* HIP device ordinal of this shard */
    uint64_t n_columns;
    const uint32_t *d_in;       /* n_columns * n_words_per_column words on `device`, 16-byte aligned */
    uint32_t *d_out;
    uint64_t out_capacity_words;
    uint64_t *d_out_words;      /* one uint64 on `device` */
    uint64_t *d_segment_offsets; /* may be NULL */
    void *d_workspace;
    size_t workspace_bytes;
} wah_column_shard;
int wah_compress_columns_multi_device(int n_shards, const wah_column_shard *shards, uint64_t n_words_per_column, int *status);

/* d_comp: c_words compressed words, 16-byte aligned (4-byte aligned is accepted: see below).  d_out: room for
 * out_capacity_words decoded words, 4-byte aligned (as for wah_compress_device; the same for the d_out of
 * wah_decompress_device_ex, wah_decompress_expand_device and wah_decompress_segments_device).  d_out_info: two device uint64:
 * [0] = ceil(31*G/32) decoded words, [1] = G groups.
 * Two decoders, the same words out of both.  ONE PASS over the stream (decode_tile_kernel): it decides tile by tile
 * (8192 words), from the tile's own words, whether the workgroup that holds the tile expands it (up to about 7 groups
 * per word) or puts it on a list that a second launch shares out in work items of about 32 output segments (a highly
 * compressed stream: every tile; a long fill inside incompressible data: that tile) -- correct for every stream,
 * the faster one up to about 7 groups per word (by 13-19 %: the stream is read once) and from about 200 on (3-6 %).
 * TWO LAUNCHES (a scan of the stream + an expansion pass, as _scan_device + _expand_device): about 20 % faster between 8
 * and 30 groups per word, where the one pass finds out tile by tile that everything goes onto its list, and within 1.5 %
 * from there to 200.  Without a pass over the
 * stream the library cannot know which it holds, so the DEFAULT goes by what out_capacity_words allows it to be: at most
 * 7 words of output per word of stream, or more than 40: one pass; between: two launches.  A caller who knows the
 * stream passes WAH_ONE_PASS or WAH_TWO_LAUNCHES (wah_decompress_device_ex); decompress(), which has the stream in
 * host memory, samples it (one pass up to 7 groups per word and from 128 on).  A stream that is only 4-byte aligned and WAH_NO_WAIT: always the two launches.
 * wah_last_decode_route() says which one the calling thread's last call launched.
 * On ANY status other than WAH_OK the content of d_out is undefined: on WAH_ERR_CAPACITY the one-pass decoder has
 * written the part that fits (it learns the size while it writes; nothing is ever written behind out_capacity_words),
 * the two-launch routes nothing; on WAH_ERR_TIMEOUT / WAH_ERR_STREAM segments may have been written at positions
 * derived from an unresolved count, inside the capacity. */
int wah_decompress_device(const uint32_t *d_comp, uint64_t c_words, uint32_t *d_out, uint64_t out_capacity_words,
                          uint64_t *d_out_info, void *d_workspace, size_t workspace_bytes, void *stream);

/* The same with flags.  WAH_NO_WAIT: the scan of the stream by a route in which no workgroup waits for another (and the
 * two-launch form of the decoder, whatever the stream) -- every 4096-word
 * tile's group total to a table, then one scan launch over the table (the reference's getCounts ->
 * thrust::exclusive_scan, decompress.cu:66-80, with one entry per tile instead of one per word); the expand pass never
 * waits anyway.  It is what decompress() takes by itself when a bounded wait of the one-launch sums kernel has expired
 * (WAH_ERR_TIMEOUT), and what WAH_FORCE_FALLBACK=1 in the environment selects for every call.  The route reads nothing
 * of the workspace's earlier content; before the scan route is used again after a WAH_ERR_TIMEOUT the workspace must be
 * initialised again (wah_workspace_init_device). */
/* WAH_TWO_LAUNCHES: the scan of the stream (decode_sums_kernel) and the expansion (decode_expand_kernel) as two launches
 * with waits, as _scan_device + _expand_device: the stream is read twice.  WAH_ONE_PASS: decode_tile_kernel + the launch
 * over its list, whatever the capacity suggests.  (Not both.) */
#define WAH_TWO_LAUNCHES 4u
#define WAH_ONE_PASS 8u
int wah_decompress_device_ex(const uint32_t *d_comp, uint64_t c_words, uint32_t *d_out, uint64_t out_capacity_words,
                             uint64_t *d_out_info, unsigned flags, void *d_workspace, size_t workspace_bytes, void *stream);

/* Which decoder the calling thread's last wah_decompress* call launched: 0 none (an argument error), WAH_ROUTE_ONE_PASS,
 * WAH_ROUTE_TWO_LAUNCHES, WAH_ROUTE_NO_WAIT. */
#define WAH_ROUTE_ONE_PASS 1
#define WAH_ROUTE_TWO_LAUNCHES 2
#define WAH_ROUTE_NO_WAIT 3
int wah_last_decode_route(void);

/* Decoding through the segment index of wah_compress_device_indexed(): segments [first_segment, first_segment +
 * n_segments) of the bitmap (992 words each, the bitmap's last one shorter) are written to d_out[0 ..).  A stream of
 * compress() never lets a fill cross a segment (compress.cu:129-146: one block per 992 words, fills merged inside
 * it), so with the index every segment is an independent job: no scan of the stream (the getCounts + scan half of
 * decompress.cu:56-83 is what the index already holds), one pass, any sub-range.  n_words: length of the ORIGINAL
 * bitmap; the whole bitmap decodes to wah_decoded_words(wah_max_compressed_words(n_words)) words like
 * wah_decompress_device.  Only for streams of this library's (= the reference's) compress(): a range whose words do
 * not make up exactly its segment, or an empty fill word, is reported as WAH_ERR_STREAM by wah_decompress_status().
 * Workspace: wah_decompress_segments_workspace_bytes(), 256-byte aligned. */
size_t wah_decompress_segments_workspace_bytes(void);
int wah_decompress_segments_device(const uint32_t *d_comp, uint64_t c_words, const uint64_t *d_segment_offsets, uint64_t n_words,
                                   uint64_t first_segment, uint64_t n_segments, uint32_t *d_out, uint64_t out_capacity_words,
                                   void *d_workspace, size_t workspace_bytes, void *stream);

/* The segment index of a stream that came WITHOUT one (written by the reference, read from storage, ...):
 * d_segment_offsets receives ceil(G / 1024) + 1 entries, exactly what wah_compress_device_indexed() would have
 * written beside the stream, so that wah_decompress_segments_device / wah_bitop_indexed_device can be used on it from
 * then on.  One scan of the stream (as wah_decompress_scan_device: d_out_info = [decoded words, groups]) + one pass
 * that places every word.  A stream in which a fill crosses a 1024-group boundary, or that contains an empty fill,
 * has no such index: WAH_ERR_STREAM from wah_decompress_status(); too few entries: WAH_ERR_CAPACITY.
 * Nothing else is asked of the stream: an indexed call accepts EXACTLY the streams that have an index, whatever the
 * maximality of their fills -- fills that could have been longer, neighbouring fills of one kind, literals 0 / 0x7FFFFFFF
 * that could have been fills, a whole segment written as 1024 one-group words, a last group whose pad bits are set (what
 * wah_validate_device counts in [3] and [5]).  See "Operands of the indexed calls" at wah_bitop_indexed_device.
 * Workspace: wah_decompress_workspace_bytes(c_words, 0). */
int wah_build_index_device(const uint32_t *d_comp, uint64_t c_words, uint64_t *d_segment_offsets, uint64_t offsets_capacity,
                           uint64_t *d_out_info, void *d_workspace, size_t workspace_bytes, void *stream);

/* First half of the above only (getCounts + scan): fills d_out_info so a
 * caller that does not know the decoded size can allocate, then call
 * wah_decompress_device (which repeats the scan) or _expand_device. */
int wah_decompress_scan_device(const uint32_t *d_comp, uint64_t c_words, uint64_t *d_out_info, void *d_workspace,
                               size_t workspace_bytes, void *stream);
int wah_decompress_expand_device(const uint32_t *d_comp, uint64_t c_words, uint32_t *d_out,
                                 uint64_t out_capacity_words, uint64_t *d_out_info, void *d_workspace,
                                 size_t workspace_bytes, void *stream);

int wah_decompress_status(void *d_workspace, void *stream);

/* Stream checker.  The reference decoder accepts ANY sequence of words
 * (kernels.cu:332-354): fills of count 0, literals that should have been fills, fills that run across the
 * 1024-group segments the reference's encoder never crosses (kernels.cu:68, tests.cpp:166-172), adjacent fills it
 * would have merged.  wah_validate_device says what a stream contains, without decoding it.
 * d_report: 8 x uint64 in device memory:
 *   [0] groups the stream expands to          [1] decoded words = ceil(31 * groups / 32)
 *   [2] fill words of count 0                 [3] literal words equal to 0 or 0x7FFFFFFF
 *   [4] fills crossing a 1024-group boundary  [5] adjacent fills of the same kind inside one segment
 *   [6] 1 if [2], [3], [4] and [5] are all zero, else 0
 *   [7] reserved (0)
 * [6] == 1 exactly when the stream is what compress() of this library / of the reference emits for some bitmap
 * ("segment-canonical"): every check above clean.  Workspace: wah_decompress_workspace_bytes(c_words, 0).
 * Asynchronous on `stream`; errors are reported as for wah_decompress_device. */
#define WAH_REPORT_WORDS 8
int wah_validate_device(const uint32_t *d_comp, uint64_t c_words, uint64_t *d_report, void *d_workspace,
                        size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 * Unsegmented ("canonical") WAH.  compress() never lets a fill cross a 1024-group segment
 * (the reference's block structure, kernels.cu:68, tests.cpp:166-172): a long run costs one word per segment.
 * wah_merge_fills_device rewrites a stream with adjacent fills of the same kind merged into one word (and fills of
 * count 0 dropped), which turns the output of compress() into the classic unsegmented WAH form; the result decodes
 * to the same bitmap with wah_decompress* (whose decoder takes fills of any length), but it is no longer what the
 * reference's encoder would emit.  Runs are not merged across multiples of 2^29 groups, so every count fits 30 bits.
 *   d_out: capacity c_words is always enough.  Workspace: wah_merge_fills_workspace_bytes(c_words), 256-byte aligned.
 *   d_out_words: device uint64.  Errors are read back with wah_decompress_status(d_workspace, stream).
 * ------------------------------------------------------------------------- */
size_t wah_merge_fills_workspace_bytes(uint64_t c_words);
int wah_merge_fills_device(const uint32_t *d_comp, uint64_t c_words, uint32_t *d_out, uint64_t out_capacity_words,
                           uint64_t *d_out_words, void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 * Bitwise operations on two compressed bitmaps (not in the reference, whose README.md:10
 * names them as the reason bitmap indexes use WAH).  Both streams must describe bitmaps of n_words words.  The
 * result is what compress() gives for (A op B): decode A, decode B (decode_sums + decode_expand each) into scratch,
 * then ONE pass of the compress kernel that combines the two bitmaps while it stages them -- three streaming passes
 * at HBM speed, nothing leaves the device.
 *   d_scratch: wah_bitop_scratch_bytes(n_words, a_words, b_words) bytes, 256-byte aligned.
 *   Errors that only the device sees (a stream that does not expand to n_words words, output capacity) are read
 *   back by wah_bitop_status(), which synchronises the stream.
 * ------------------------------------------------------------------------- */
#define WAH_OP_AND 0
#define WAH_OP_OR 1
#define WAH_OP_XOR 2
#define WAH_OP_ANDNOT 3 /* A & ~B */
size_t wah_bitop_scratch_bytes(uint64_t n_words, uint64_t a_words, uint64_t b_words);
int wah_bitop_device(int op, uint64_t n_words, const uint32_t *d_a, uint64_t a_words, const uint32_t *d_b,
                     uint64_t b_words, uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words,
                     void *d_scratch, size_t scratch_bytes, void *stream);
int wah_bitop_status(void *d_scratch, uint64_t n_words, uint64_t a_words, uint64_t b_words, void *stream);

/* The same for operands that come with their segment index (wah_compress_device_indexed): the two streams are walked
 * segment by segment through their indexes, combined group by group in registers, and ONE decoded bitmap is written,
 * which the compress kernel then reads -- no scan of the operands, no second read of them, half the intermediate
 * traffic of wah_bitop_device.  d_out_offsets (may be NULL) receives the result's own segment index, so results can
 * be combined further.
 * Operands of the indexed calls (this one and every call below that takes a stream with its segment index, or a table of
 * such): an operand is accepted exactly when it has an index for a bitmap of n_words words -- every segment's words
 * (offsets[s] .. offsets[s + 1]) make up exactly the segment's groups, 1024 or what is left in the last one, and no fill is
 * empty; anything else is WAH_ERR_STREAM from the call's status function.  That is what compress() writes and what
 * wah_build_index_device accepts, and no more: fills need not be maximal, neighbouring fills may be of one kind, a zero or
 * all-ones group may be a literal, a segment may be 1024 one-group words.  A result that is a compressed bitmap is always in
 * compress()'s form, word for word, whatever form the operands had.  Pad bits never matter, on any route: the 31 G - 32 n_words
 * bits of the last group that lie behind the bitmap may be set in an operand (a last literal, a fill of ones that runs over
 * the group); they are not part of the bitmap, are never counted, listed or fetched, and are clear in every result.
 *   d_scratch: wah_bitop_indexed_scratch_bytes(n_words) bytes, 256-byte aligned. */
size_t wah_bitop_indexed_scratch_bytes(uint64_t n_words);
int wah_bitop_indexed_device(int op, uint64_t n_words, const uint32_t *d_a, uint64_t a_words, const uint64_t *d_a_offsets,
                             const uint32_t *d_b, uint64_t b_words, const uint64_t *d_b_offsets, uint32_t *d_out,
                             uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                             size_t scratch_bytes, void *stream);
int wah_bitop_indexed_status(void *d_scratch, uint64_t n_words, void *stream);

/* Two routes, the same words out of both (the library chooses by the operands' lengths; wah_last_bitop_route() says which
 * the calling thread's last wah_bitop_indexed_device / wah_bitop_many_indexed_device call took):
 * WAH_BITOP_ROUTE_RUNS -- all operands together hold at most 112 words per 1024-group segment on average (sparse or
 * clustered bitmaps, what a bitmap index mostly holds): their run lists are MERGED in the compressed domain, one lane per
 * segment, the way WAH operations are done on a CPU; nothing is decoded, nothing of bitmap size is written, the cost goes
 * with the operands' words (count pass, scan of 1/256 of the segment counts, write pass: the operands are read twice).
 * WAH_BITOP_ROUTE_GROUPS -- anything else: every segment decoded into its 1024 groups, combined in registers and
 * compressed again (the description above); the cost goes with the bitmap's length. */
#define WAH_BITOP_ROUTE_RUNS 1
#define WAH_BITOP_ROUTE_GROUPS 2
int wah_last_bitop_route(void);

/* The same for up to 8 operands in ONE combining pass, left to right: A op B op C ... (WAH_OP_ANDNOT: A and not B
 * and not C ...) -- the conjunction of several predicates of a bitmap index in one go.  d_streams / stream_words /
 * d_offsets: HOST arrays of n_operands device pointers / lengths / index pointers.  Scratch and status as for
 * wah_bitop_indexed_device (wah_bitop_indexed_scratch_bytes, wah_bitop_indexed_status). */
int wah_bitop_many_indexed_device(int op, uint64_t n_words, int n_operands, const uint32_t *const *d_streams,
                                  const uint64_t *stream_words, const uint64_t *const *d_offsets, uint32_t *d_out,
                                  uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                                  size_t scratch_bytes, void *stream);

/* The same for ANY number of operands, named by a table in DEVICE memory: the query an equality-encoded bitmap index
 * exists for -- `value IN (...)`, `lo <= value <= hi` are the OR of as many bitmaps as the list or the range has bins.
 * Semantics as above, word for word: left to right, A op B op C ... (WAH_OP_ANDNOT: A and not B and not C ...); the result
 * is what compress() emits for the combined bitmap of n_words words (ragged ends included; n_words == 0: an empty stream);
 * d_out_offsets (may be NULL) receives the result's own segment index, so results chain into every indexed call.
 *   d_operands: n_operands entries, 8-byte aligned, 1 <= n_operands <= WAH_BITOP_LIST_MAX_OPERANDS.  An operand may appear
 *   more than once (OR is idempotent, XOR cancels).  An entry may be a WINDOW into a longer stream, which is what a column
 *   of a column matrix is (wah_compress_columns_multi_device, one launch over back-to-back columns): d_offsets then
 *   points into the matrix index at the column's first segment, its entries count from the start of the whole stream, and
 *   stream_words is the whole stream's length -- which is why an entry carries pointers, not a column number.
 * The library never reads the table on the host: the call is asynchronous on `stream`, allocates nothing, never
 * synchronises, and a captured graph replayed after the table was overwritten in place combines the NEW selection.  For
 * the same reason there is one route whatever the operands hold (their lengths are only bounds, known to the device): one
 * wavefront per segment applies every operand's words to the segment's 1024 groups where they lie -- a fill that is the
 * operation's identity costs its load only, so the cost goes with the operands' words plus the fills that change the
 * result, not with n_operands x n_words -- and the compress passes run over the one decoded bitmap that leaves.
 *   d_scratch: wah_bitop_list_scratch_bytes(n_words, n_operands) bytes, 256-byte aligned, no initialisation; it EQUALS
 *   wah_bitop_indexed_scratch_bytes(n_words) for every n_operands (nothing in it goes with the operands' number).
 * Errors the host can see come back before any HIP call: a bad op, n_operands out of range, a null or misaligned scratch or
 * table, null outputs, n_words >= 2^40: WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE.  Everything only the device
 * sees is reported by wah_bitop_list_status(), which synchronises the stream: WAH_ERR_STREAM for an entry with a null or
 * misaligned index or stream or a length of 2^40 or more, an index range that is not inside stream_words, a segment whose
 * words do not make up exactly its groups, an empty fill; WAH_ERR_CAPACITY for too small an output (nothing is written behind
 * out_capacity_words).  An entry is checked before a pointer of it is followed, an index range before the stream is read
 * through it, and EVERY operand's every segment is checked: nothing stops early, so the verdict does not depend on the data. */
typedef struct {
    const uint32_t *d_stream;  /* the operand's words, 4-byte aligned                         */
    uint64_t stream_words;     /* its length, or a capacity that bounds it                    */
    const uint64_t *d_offsets; /* its segment index: n_segments + 1 entries, into d_stream    */
} wah_bitop_operand;           /* 24 bytes, no padding */
#define WAH_BITOP_LIST_MAX_OPERANDS (1u << 24)
size_t wah_bitop_list_scratch_bytes(uint64_t n_words, uint64_t n_operands);
int wah_bitop_list_indexed_device(int op, uint64_t n_words, uint64_t n_operands, const wah_bitop_operand *d_operands,
                                  uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets,
                                  void *d_scratch, size_t scratch_bytes, void *stream);
int wah_bitop_list_status(void *d_scratch, uint64_t n_words, uint64_t n_operands, void *stream);

/* A whole conjunction of IN / NOT IN lists in ONE call -- `city IN (...) AND age BETWEEN 30 AND 39 AND status NOT IN (...)`:
 *     result = AND over clauses i of ( negate_i ? NOT (OR of clause i's operands) : (OR of clause i's operands) )
 * over bitmaps of n_words words, NOT over the bitmap's 32 * n_words bits.  The result is what compress() emits for that
 * bitmap (ragged ends included; n_words == 0: an empty stream); d_out_offsets (may be NULL) receives its segment index, so
 * results chain into every indexed call.  Word for word: one clause, not negated, is the list call's WAH_OP_OR; clauses of one
 * operand each, none negated, its WAH_OP_AND; one positive clause {A} and negated clauses its WAH_OP_ANDNOT with A first; one
 * negated clause of one operand the complement of a compressed bitmap.
 *   d_operands: the operands of all clauses back to back, clause 0 first: n_operands entries as for the list call (8-byte
 *   aligned, 1 <= n_operands <= WAH_BITOP_LIST_MAX_OPERANDS, windows into column matrices allowed, operands may repeat).
 *   d_clause_ends: n_clauses entries (1 <= n_clauses <= n_operands) in DEVICE memory, 8-byte aligned: the low bits of entry i
 *   are the index one past clause i's last operand in d_operands (clause 0 starts at 0), bit 63 is WAH_CLAUSE_NEGATE.  The
 *   ends are strictly increasing (no empty clause) and the last one equals n_operands.
 * Like the list call it never reads a table on the host, is asynchronous on `stream`, allocates nothing and never
 * synchronises: a captured graph replayed after BOTH tables were overwritten in place (same counts; other boundaries, flags,
 * operands) answers the NEW query.  One route: one wavefront per segment ORs the current clause's operands as the list call
 * does and folds the clause into the running AND, which it keeps in registers, when the walk over the flattened table crosses
 * the clause's end; one decoded bitmap leaves, and the compress passes run over it.  No intermediate per clause exists.
 *   d_scratch: wah_bitop_clauses_scratch_bytes(n_words, n_operands, n_clauses) bytes, 256-byte aligned, no initialisation;
 *   it EQUALS wah_bitop_indexed_scratch_bytes(n_words) for every n_operands and n_clauses.
 * Errors the host can see come back before any HIP call: n_clauses < 1 or > n_operands, n_operands out of range, a null or
 * misaligned scratch or table, null outputs, n_words >= 2^40: WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE (the
 * argument checks come first).  Everything only the device sees is reported by wah_bitop_clauses_status(), which synchronises
 * the stream: WAH_ERR_STREAM for everything the list call refuses in an operand, and for a clause table that is not strictly
 * increasing, has bits set besides the index and WAH_CLAUSE_NEGATE, or does not end at n_operands; WAH_ERR_CAPACITY for too
 * small an output.  A clause end is checked before it steers anything, and EVERY operand's every segment is checked: a result
 * that has already become all zeros skips nothing, so the verdict does not depend on the data. */
#define WAH_CLAUSE_NEGATE (1ull << 63)
size_t wah_bitop_clauses_scratch_bytes(uint64_t n_words, uint64_t n_operands, uint64_t n_clauses);
int wah_bitop_clauses_indexed_device(uint64_t n_words, uint64_t n_clauses, const uint64_t *d_clause_ends, uint64_t n_operands,
                                     const wah_bitop_operand *d_operands, uint32_t *d_out, uint64_t out_capacity_words,
                                     uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes,
                                     void *stream);
int wah_bitop_clauses_status(void *d_scratch, uint64_t n_words, uint64_t n_operands, uint64_t n_clauses, void *stream);

/* `lo <= value <= hi` over a BIT-SLICED attribute in ONE call (O'Neil & Quass): an attribute of many distinct values -- a
 * price, a timestamp, an id -- is stored as one bitmap per BIT of the value, n_slices of them, not one per value, and a range
 * predicate is one most-significant-bit-first sweep over them.
 *   d_slices: n_slices rows (1 <= n_slices <= WAH_BSI_MAX_SLICES), plus ONE more with WAH_BSI_EXISTS in flags, entries as for
 *   the list call (8-byte aligned, windows into column matrices allowed, the length may be a capacity, a row may name the
 *   not-yet-checked output of an earlier call on the stream).  The table is in sweep order: the value of row p (position
 *   32 * word + bit) is the unsigned integer whose bit n_slices - 1 - i is bit p of table row i -- row 0 is the MOST
 *   significant slice.  With WAH_BSI_EXISTS table row n_slices is the existence bitmap: the rows that have a value at all.
 *   d_bounds: lo = d_bounds[0], hi = d_bounds[1], two uint64 in DEVICE memory, 8-byte aligned.
 * The result is the bitmap of the rows with lo <= value <= hi, both inclusive, ANDed with the existence bitmap where there is
 * one: word for word what compress() emits for that bitmap of n_words words (ragged ends included, pad bits never matter;
 * n_words == 0: an empty stream); d_out_offsets (may be NULL) receives its segment index, so the result goes into the
 * clause call as one more operand.  <, <=, >, >=, = are all ranges; != is = put through a negated clause of the clause call.
 * Bounds are data, never errors: lo > hi gives all zeros; for n_slices < 64, hi >= 2^n_slices behaves as 2^n_slices - 1 and
 * lo >= 2^n_slices gives all zeros.  WITHOUT an existence bitmap the rows of the bitmap beyond the caller's own row count
 * (up to 32 * n_words) have the value 0 like any other row whose slices are all zero: they MATCH when lo == 0.
 * Bounds and table are read by the device only: the call is asynchronous on `stream`, allocates nothing, never synchronises,
 * and a captured graph replayed after d_bounds (and / or the table) was overwritten in place answers the NEW query.  One
 * route: one wavefront per segment ORs a slice into an LDS image as the list call does, folds it into the sweep's state,
 * which it keeps in registers, when the walk crosses to the next row, and the compress passes run over the one decoded
 * bitmap that leaves.
 *   d_scratch: wah_bsi_range_scratch_bytes(n_words, n_slices) bytes, 256-byte aligned, no initialisation; it EQUALS
 *   wah_bitop_indexed_scratch_bytes(n_words) for every n_slices.
 * Errors the host can see come back before any HIP call, the argument checks first: n_slices outside 1 .. 64, unknown flag
 * bits, a null or misaligned table, bounds (8 B) or scratch (256 B), a null d_out_words, a null d_out with n_words > 0,
 * n_words >= 2^40: WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE.  Everything only the device sees is reported by
 * wah_bsi_range_status(), which synchronises the stream: WAH_ERR_STREAM for everything the list call refuses in an operand,
 * WAH_ERR_CAPACITY for too small an output.  EVERY row's every segment is checked: an empty range, or a result that has
 * become all zeros, skips nothing, so the verdict depends neither on the data nor on the bounds. */
#define WAH_BSI_MAX_SLICES 64u
#define WAH_BSI_EXISTS 1u /* flags: the table has one more row behind the slices, the existence bitmap */
size_t wah_bsi_range_scratch_bytes(uint64_t n_words, uint64_t n_slices);
int wah_bsi_range_indexed_device(uint64_t n_words, uint64_t n_slices, const wah_bitop_operand *d_slices, const uint64_t *d_bounds,
                                 unsigned flags, uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words,
                                 uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream);
int wah_bsi_range_status(void *d_scratch, uint64_t n_words, uint64_t n_slices, void *stream);

/* `value IN (set)` / `value NOT IN (set)` over a BIT-SLICED attribute in ONE call: an IN list of constants, or a SEMI-JOIN --
 * `WHERE fk IN (SELECT id FROM dim WHERE ...)`, the probe side of a star join -- without the value column in global memory.
 *   d_slices: exactly the range call's table: n_slices rows (1 .. WAH_BSI_MAX_SLICES), most significant slice first, plus ONE
 *   more with WAH_BSI_EXISTS, the existence bitmap; windows into column matrices, capacities as lengths and the not-yet-checked
 *   output of an earlier call on the stream are allowed.
 *   The set as a SORTED LIST (no WAH_MEMBER_BITSET): d_set is set_capacity uint64 in DEVICE memory, 8-byte aligned; its first
 *   *d_set_count entries are the set, in NON-DECREASING order -- duplicates are allowed, so the torch.sort of a value column
 *   is a set.  d_set_count is one uint64 in device memory, read by the device only; NULL: the count is set_capacity.
 *   set_capacity == 0 is an empty set (d_set may then be NULL).  An entry at or above 2^n_slices matches nothing: entries
 *   are data, never errors.
 *   The set as a BIT ARRAY (WAH_MEMBER_BITSET): d_set is ceil(set_capacity / 32) uint32 words, 4-byte aligned; value v is in the
 *   set iff v < set_capacity and bit v % 32 of word v / 32 is set -- the layout of a DECODED bitmap, so the decoded filter of a
 *   dimension table is the set for the fact table's foreign key.  Bits of the last word at or behind set_capacity are never
 *   looked at; d_set_count must be NULL; set_capacity may be anything below 2^40.
 * The result is the bitmap of the rows whose value is in the set, with WAH_MEMBER_NEGATE of those whose value is NOT, either
 * ANDed with the existence bitmap where there is one (NOT IN over an attribute with NULLs is one call): word for word what
 * compress() emits for that bitmap of n_words words (ragged ends included; n_words == 0: an empty stream); d_out_offsets (may
 * be NULL) receives its segment index.  WITHOUT an existence bitmap the rows beyond the caller's own row count have the value 0,
 * as in the range call: they match when 0 is in the set, and under NEGATE when it is not.
 * Set, count and table are read by the device only: the call is asynchronous on `stream`, allocates nothing, never
 * synchronises, and a captured graph replayed after any of them was overwritten in place answers the NEW query.  One check
 * launch over the list, then one launch of one workgroup per segment (per half segment above 32 slices) that folds the slices
 * into one word (two) per row in LDS and probes the set per row -- about log2(count) dependent 8-byte loads a row for a list,
 * one 4-byte load for a bit array; then the compress passes over the one decoded bitmap that leaves.
 *   d_scratch: wah_bsi_member_scratch_bytes(n_words, n_slices) bytes, 256-byte aligned, no initialisation; it EQUALS
 *   wah_bitop_indexed_scratch_bytes(n_words) for every n_slices.
 * Errors the host can see come back before any HIP call, in this order: n_slices outside 1 .. 64 or unknown flag bits; a null
 * or misaligned table (8 B) or scratch (256 B); set_capacity >= 2^40, a null d_set with set_capacity > 0, a misaligned set (8 B
 * for a list, 4 B for a bit array) or count (8 B), a count with WAH_MEMBER_BITSET; a null d_out_words, a null d_out with
 * n_words > 0, n_words >= 2^40 -- all WAH_ERR_ARG; then too small a scratch: WAH_ERR_WORKSPACE.  Everything only the device
 * sees is reported by wah_bsi_member_status(), which synchronises the stream: WAH_ERR_STREAM for everything the list call
 * refuses in an operand, for *d_set_count > set_capacity (nothing is read behind the capacity) and for a list that is not
 * non-decreasing within its count (what lies behind the count is never looked at); then WAH_ERR_CAPACITY for too small an
 * output, and nothing is written behind out_capacity_words.  The set is checked whole and every table row's every segment is
 * walked: the verdict depends neither on the attribute's data nor on which values match. */
#define WAH_MEMBER_NEGATE 2u /* NOT IN: the rows (that exist) whose value is not in the set */
#define WAH_MEMBER_BITSET 4u /* the set is a bit array over the value domain, not a sorted list */
size_t wah_bsi_member_scratch_bytes(uint64_t n_words, uint64_t n_slices);
int wah_bsi_member_indexed_device(uint64_t n_words, uint64_t n_slices, const wah_bitop_operand *d_slices, const void *d_set,
                                  uint64_t set_capacity, const uint64_t *d_set_count, unsigned flags, uint32_t *d_out,
                                  uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                                  size_t scratch_bytes, void *stream);
int wah_bsi_member_status(void *d_scratch, uint64_t n_words, uint64_t n_slices, void *stream);

/* `A op B` ROW BY ROW over TWO bit-sliced attributes in ONE call -- `ship_date > commit_date`, `price < cost`, `a == b`: the
 * range call's sweep with the constant's bit replaced by the other attribute's slice.  A has n_slices_a slices and B has
 * n_slices_b, each 1 .. WAH_BSI_MAX_SLICES and possibly different; the narrower one counts as zero above its width.  BOTH
 * values are read as UNSIGNED integers.
 *   op: WAH_CMP_LT, _LE, _GT, _GE, _EQ or _NE.
 *   d_rows: n_slices_a + n_slices_b rows, plus one for each of WAH_BSI_EXISTS_A and WAH_BSI_EXISTS_B in flags, entries as
 *   for the list call (8-byte aligned, windows into column matrices allowed, the length may be a capacity, a row may name the
 *   not-yet-checked output of an earlier call on the stream).  TABLE ORDER: the two attributes' slices interleaved by
 *   significance, most significant first -- for sig = max(n_slices_a, n_slices_b) - 1 down to 0: A's slice of significance sig
 *   if sig < n_slices_a, then B's if sig < n_slices_b; then A's existence bitmap with WAH_BSI_EXISTS_A; then B's with
 *   WAH_BSI_EXISTS_B.  (For 3 and 2 slices: A2, A1, B1, A0, B0.)  Nothing else describes the table.
 * The result is the bitmap of the rows where A op B holds, ANDed with every existence bitmap there is: word for word what
 * compress() emits for that bitmap of n_words words (ragged ends included, pad bits never matter; n_words == 0: an empty
 * stream); d_out_offsets (may be NULL) receives its segment index, so the result goes into the clause call as one more
 * operand.  WITHOUT an existence bitmap the rows of the bitmap behind the caller's own row count (up to 32 * n_words) hold 0
 * in BOTH attributes like any other row whose slices are all zero: they MATCH ==, <= and >=.
 * The table is read by the device only: the call is asynchronous on `stream`, allocates nothing, never synchronises, and a
 * captured graph replayed after the table was overwritten in place compares the NEW rows (the slice counts, the flags and
 * the operator are host arguments and stay as captured).  One route: one wavefront per segment ORs a row into an LDS image
 * as the list call does, folds it into the sweep's state (rows still equal, rows already greater, A's slice of the current
 * significance), which it keeps in registers, when the walk crosses to the next row, and the compress passes run over the one
 * decoded bitmap that leaves.
 *   d_scratch: wah_bsi_compare_scratch_bytes(n_words, n_slices_a, n_slices_b) bytes, 256-byte aligned, no initialisation; it
 *   EQUALS wah_bitop_indexed_scratch_bytes(n_words) for every pair of widths.
 * Errors the host can see come back before any HIP call, the argument checks first: op outside 0 .. 5, a slice count outside
 * 1 .. 64, unknown flag bits, a null or misaligned table (8 B) or scratch (256 B), a null d_out_words, a null d_out with
 * n_words > 0, n_words >= 2^40: WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE.  Everything only the device sees is
 * reported by wah_bsi_compare_status(), which synchronises the stream: WAH_ERR_STREAM for everything the list call refuses
 * in an operand, WAH_ERR_CAPACITY for too small an output.  EVERY row's every segment is checked whatever the operator and
 * whatever the result has become, so the verdict depends neither on the data nor on the operator. */
#define WAH_BSI_EXISTS_A 1u /* flags: A's existence bitmap is a row behind the slices */
#define WAH_BSI_EXISTS_B 2u /* flags: B's existence bitmap is a row behind the slices (behind A's) */
#define WAH_CMP_LT 0
#define WAH_CMP_LE 1
#define WAH_CMP_GT 2
#define WAH_CMP_GE 3
#define WAH_CMP_EQ 4
#define WAH_CMP_NE 5
size_t wah_bsi_compare_scratch_bytes(uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b);
int wah_bsi_compare_indexed_device(int op, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, const wah_bitop_operand *d_rows,
                                   unsigned flags, uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words,
                                   uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream);
int wah_bsi_compare_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, void *stream);

/* `A + B` and `A - B` ROW BY ROW over TWO bit-sliced attributes in ONE call, as a NEW bit-sliced attribute -- `ship_date -
 * order_date <= 30`, `price + tax > limit`, `MAX(end - start) WHERE ...`, `ORDER BY a + b LIMIT k`: a ripple carry over the
 * slices, least significant first (O'Neil & Quass).  The result is an attribute like any other, so the range, compare, k-th,
 * count and fetch calls, and a further call of this one, take it.  Not in the reference.
 *   op: WAH_ARITH_ADD or WAH_ARITH_SUB.
 *   A has n_slices_a slices and B has n_slices_b, each 1 .. WAH_BSI_MAX_SLICES and possibly different; BOTH are read as UNSIGNED
 *   integers and the narrower one counts as zero above its width.
 *   The result is (A op B) mod 2^n_slices_out, n_slices_out 1 .. 64 and the caller's choice.  max(n_slices_a, n_slices_b) + 1
 *   never loses a carry; for SUB that top slice is the borrow, the sign of the two's-complement difference: it is set exactly
 *   where A < B.  A smaller n_slices_out truncates; a larger one zero-extends for ADD and sign-extends for SUB.
 *   flags: WAH_BSI_EXISTS_A | WAH_BSI_EXISTS_B.  With either one the result has an existence bitmap, the AND of those present: it
 *   is the LAST row of the output, as in wah_bsi_build_device, and every output slice is ANDed with it -- a row that does not
 *   exist is stored as value 0, as the builder stores it.  rows_out = n_slices_out + (flags ? 1 : 0).
 *   d_rows: n_slices_a + n_slices_b rows, plus one for each flag, entries as for the list call (8-byte aligned, windows into
 *   column matrices allowed, the length may be a capacity, a row may name the not-yet-checked output of an earlier call on the
 *   stream).  TABLE ORDER: LEAST significant first, because the carry runs that way, and the existence bitmaps in FRONT, because
 *   the first sum slice leaves before the sweep ends -- A's existence bitmap with WAH_BSI_EXISTS_A; then B's with
 *   WAH_BSI_EXISTS_B; then for sig = 0 up to max(n_slices_a, n_slices_b) - 1: A's slice of significance sig if sig < n_slices_a,
 *   then B's if sig < n_slices_b.  (For 3 and 2 slices with both flags: XA, XB, A0, B0, A1, B1, A2.)  Nothing else describes the
 *   table.
 *   n_words: the words of ONE slice, a non-zero multiple of 992 with rows_out * n_words < 2^40, as for the builder: the output
 *   is a column matrix, whose rows start on segment boundaries.
 * d_out, d_out_words and d_out_offsets receive exactly what wah_bsi_build_device leaves for the result's value column: the
 * slices' compress() streams back to back, MOST significant slice first, the existence bitmap last; rows_out * (n_words / 992)
 * + 1 index entries, entry i * (n_words / 992) + s the first word of segment s of output row i, the last one the total, which
 * d_out_words receives too.  out_capacity_words = wah_max_compressed_words(rows_out * n_words) always suffices.  The operands may
 * not overlap d_out or the scratch.
 * The table is read by the device only: the call is asynchronous on `stream`, allocates nothing, never synchronises, and a
 * captured graph replayed after the table was overwritten in place computes the NEW rows (the widths, op and the flags are host
 * arguments and stay as captured).  One route: one wavefront per segment ORs a row into an LDS image as the list call does
 * and, when the walk crosses to the next row, folds it into the sweep's state (the existence mask, the carry, A's slice of the
 * current significance), which it keeps in registers; at the second slice of a significance the sum slice leaves as the
 * segment's 992 decoded words of the result's slice matrix in the scratch -- every word of it is written once, it needs no
 * clearing -- and the one-launch compressor runs over the matrix.  The operands' words are read once; 4 * rows_out * n_words
 * bytes are written once and read once.
 *   d_scratch: wah_bsi_arith_scratch_bytes(n_words, n_slices_out, flags) bytes, 256-byte aligned, no initialisation; it EQUALS
 *   wah_bsi_build_scratch_bytes(n_words, rows_out):
 *       1024 + round256(4 * rows_out * n_words) + round256(wah_compress_workspace_bytes(rows_out * n_words)).
 * Errors the host can see come back before any HIP call, the argument checks first: an unknown op, a slice count (of A, of B
 * or of the result) outside 1 .. 64, unknown flag bits, n_words == 0 or not a multiple of 992, rows_out * n_words >= 2^40, a
 * null or misaligned table (8 B), scratch (256 B), d_out (4 B), d_out_words or d_out_offsets (8 B): WAH_ERR_ARG; too small a
 * scratch: WAH_ERR_WORKSPACE.  Everything only the device sees is reported by wah_bsi_arith_status(), which synchronises the
 * stream and reads the sweep's control words, then the compressor's: WAH_ERR_STREAM for everything the list call refuses in an
 * operand, WAH_ERR_CAPACITY for too small an output (nothing is written at or behind d_out[out_capacity_words]).  EVERY row's
 * every segment is walked and checked, the slices at or above n_slices_out that contribute nothing included, so the verdict
 * depends neither on the data nor on n_slices_out.  The output of a refused call is unspecified.
 * wah_bsi_arith_status(NULL, ...): WAH_ERR_ARG. */
#define WAH_ARITH_ADD 0
#define WAH_ARITH_SUB 1
size_t wah_bsi_arith_scratch_bytes(uint64_t n_words, uint64_t n_slices_out, unsigned flags);
int wah_bsi_arith_indexed_device(int op, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, uint64_t n_slices_out,
                                 const wah_bitop_operand *d_rows, unsigned flags, uint32_t *d_out, uint64_t out_capacity_words,
                                 uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream);
int wah_bsi_arith_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_out, unsigned flags, void *stream);

/* `A * B` ROW BY ROW over TWO bit-sliced attributes in ONE call, as a NEW bit-sliced attribute -- `price * qty > limit`, `ORDER
 * BY price * qty DESC LIMIT k`, `SUM(extended_price * discount) WHERE ...`: schoolbook shift-and-add over the slices.  The
 * result is an attribute like any other, as that of wah_bsi_arith_indexed_device, whose contract this one follows word for word
 * except where stated here.  Not in the reference.
 *   The result is (A * B) mod 2^n_slices_out, BOTH operands read as UNSIGNED, n_slices_out 1 .. 64 and the caller's choice:
 *   n_slices_a + n_slices_b slices lose nothing (that sum may reach 128: beyond 64 the call truncates), fewer truncate, more
 *   zero-extend.
 *   flags: WAH_BSI_EXISTS_A | WAH_BSI_EXISTS_B, as there: the AND of the bitmaps present is the LAST row of the output, and every
 *   output slice is ANDed with it.  rows_out = n_slices_out + (flags ? 1 : 0).
 *   d_rows: n_slices_a + n_slices_b rows, plus one for each flag, entries as for the list call.  TABLE ORDER: A's existence
 *   bitmap with WAH_BSI_EXISTS_A; then B's with WAH_BSI_EXISTS_B; then ALL of A's slices, least significant first; then ALL of B's
 *   slices, least significant first.  There is NO interleaving: every slice of B meets every slice of A, so A has to be complete
 *   before the first slice of B arrives.  (For 3 and 2 slices with both flags: XA, XB, A0, A1, A2, B0, B1.)  Nothing else
 *   describes the table.  The operation is commutative and the call takes the operands as given; the narrower one as A keeps
 *   the scratch small.
 *   n_words, d_out, d_out_words, d_out_offsets, out_capacity_words: exactly those of wah_bsi_arith_indexed_device -- slices MOST
 *   significant first, the existence bitmap last, rows_out * (n_words / 992) + 1 index entries, n_words a non-zero multiple of
 *   992 with rows_out * n_words < 2^40.
 * Asynchronous on `stream`, allocates nothing, never synchronises; the table is read by the device only, so a captured graph
 * replayed after the table was overwritten in place computes the NEW rows.  One route: one wavefront per segment walks the
 * table as the arithmetic call does; the fold of a slice of A puts the segment's 1024 groups into the wave's own area of the
 * scratch, the fold of slice j of B adds (A & B_j) << j into an accumulator of n_slices_out slices that lies there too, one
 * ripple carry over A's slices whose carry leaves into a slice no earlier step has written -- nothing is cleared.  A slice of B
 * that is all zero in a segment skips that addition (a constant multiplier costs its set bits only) but is walked and checked
 * like any other.  Behind the sweep the accumulator leaves as the result's decoded slice matrix and the one-launch compressor
 * runs over it.
 *   d_scratch: wah_bsi_mul_scratch_bytes(n_words, n_slices_a, n_slices_out, flags) bytes, 256-byte aligned, no initialisation:
 *       wah_bsi_arith_scratch_bytes(n_words, n_slices_out, flags) + 4096 * (n_words / 992) * (n_slices_a + n_slices_out),
 *   that is 1024 + round256(4 * rows_out * n_words) + round256(wah_compress_workspace_bytes(rows_out * n_words)) and 4 KiB per
 *   segment for each slice of A and of the result.
 * Errors the host can see come back before any HIP call, the argument checks first: a slice count (of A, of B or of the
 * result) outside 1 .. 64, unknown flag bits, n_words == 0 or not a multiple of 992, rows_out * n_words >= 2^40, a null or
 * misaligned table (8 B), scratch (256 B), d_out (4 B), d_out_words or d_out_offsets (8 B): WAH_ERR_ARG; too small a scratch:
 * WAH_ERR_WORKSPACE.  Everything only the device sees is reported by wah_bsi_mul_status(), which synchronises the stream and
 * reads the sweep's control words, then the compressor's: WAH_ERR_STREAM for everything the list call refuses in an operand,
 * WAH_ERR_CAPACITY for too small an output (nothing is written at or behind d_out[out_capacity_words]).  EVERY row's every
 * segment is walked and checked, the slices that contribute nothing -- above n_slices_out, or where the other operand is zero --
 * included, so the verdict depends neither on the data nor on n_slices_out.  The output of a refused call is unspecified.
 * wah_bsi_mul_status(NULL, ...): WAH_ERR_ARG. */
size_t wah_bsi_mul_scratch_bytes(uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_out, unsigned flags);
int wah_bsi_mul_indexed_device(uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, uint64_t n_slices_out,
                               const wah_bitop_operand *d_rows, unsigned flags, uint32_t *d_out, uint64_t out_capacity_words,
                               uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream);
int wah_bsi_mul_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_out, unsigned flags, void *stream);

/* `A / B` and `A % B` ROW BY ROW over TWO bit-sliced attributes in ONE call, as a NEW bit-sliced attribute -- `revenue / qty`,
 * `elapsed / 60`, `id % 1024`, `ORDER BY clicks * 1000 / views DESC LIMIT k`, `WHERE a % b = 0`: restoring long division over
 * the slices, most significant slice of the dividend first.  The result is an attribute like any other, as that of
 * wah_bsi_mul_indexed_device, whose contract this one follows word for word except where stated here.  Not in the reference.
 *   BOTH operands are read as UNSIGNED, n_slices_a and n_slices_b 1 .. 64 each, n_slices_out 1 .. 64 and the caller's choice.
 *   what = WAH_DIV_QUOTIENT: floor(A / B) mod 2^n_slices_out -- n_slices_a slices lose nothing, fewer truncate, more zero-extend.
 *   what = WAH_DIV_REMAINDER: (A mod B) mod 2^n_slices_out -- min(n_slices_a, n_slices_b) slices lose nothing.  One result per
 *   call: a caller who wants both calls twice.
 *   DIVISION BY ZERO IS NULL.  The result ALWAYS has an existence bitmap as the LAST row of its output, whatever the flags:
 *   rows_out = n_slices_out + 1.  It is (A's existence bitmap with WAH_BSI_EXISTS_A) AND (B's with WAH_BSI_EXISTS_B) AND
 *   (B != 0), and every output slice is ANDed with it: a row that does not exist is stored as value 0, as the builder stores it.
 *   n_words is a multiple of 992, so the last group has no pad bits; rows of a column behind the caller's own row count hold
 *   B = 0 and fall out by themselves.
 *   d_rows: n_slices_a + n_slices_b rows, plus one for each flag, entries as for the list call.  TABLE ORDER: A's existence
 *   bitmap with WAH_BSI_EXISTS_A; then B's with WAH_BSI_EXISTS_B; then ALL of B's slices, LEAST significant first; then ALL of A's
 *   slices, MOST significant first.  B has to be complete, and with it the existence mask, before the first quotient slice
 *   leaves, and long division consumes the dividend from the top.  (For 3 and 2 slices with both flags:
 *   XA, XB, B0, B1, A2, A1, A0.)  Nothing else describes the table.
 *   n_words, d_out, d_out_words, d_out_offsets, out_capacity_words: exactly those of wah_bsi_mul_indexed_device with THIS call's
 *   rows_out -- slices MOST significant first, the existence bitmap last, rows_out * (n_words / 992) + 1 index entries, n_words
 *   a non-zero multiple of 992 with rows_out * n_words < 2^40.
 * Asynchronous on `stream`, allocates nothing, never synchronises; the table is read by the device only, so a captured graph
 * replayed after the table was overwritten in place computes the NEW rows (what, the widths and the flags are host arguments
 * and stay as captured).  One route: one wavefront per segment walks the table as the multiplication call does; the fold of a
 * slice of B puts the segment's 1024 groups into the wave's own area of the scratch and ORs them into the mask B != 0; the
 * fold of slice i of A shifts the remainder up by one with A_i below it (R) and subtracts B from it by one ripple borrow over
 * n_slices_b + 1 slices (T); the quotient bit q is set where nothing is borrowed, and the next step reads the remainder as
 * q ? T : R -- nothing is moved, nothing is cleared.  While every slice of A so far was all zero in a segment the step is
 * skipped, and the slices of B above its last one that is not all zero in a segment are left out of every ripple there (values
 * far below their declared width cost their real width), but every row is walked and checked like any other.
 * Behind the sweep the one-launch compressor runs over the result's decoded slice matrix.
 *   d_scratch: wah_bsi_div_scratch_bytes(n_words, n_slices_b, n_slices_out, flags) bytes, 256-byte aligned, no initialisation:
 *       wah_bsi_build_scratch_bytes(n_words, n_slices_out + 1) + 4096 * (n_words / 992) * (3 * n_slices_b + 2),
 *   that is 1024 + round256(4 * rows_out * n_words) + round256(wah_compress_workspace_bytes(rows_out * n_words)) and 4 KiB per
 *   segment for each slice of B's image and of the two remainder buffers of n_slices_b + 1 slices.
 * Errors the host can see come back before any HIP call, the argument checks first and in this order: an unknown `what`; a
 * slice count (of A, of B or of the result) outside 1 .. 64 or unknown flag bits; n_words == 0, not a multiple of 992 or
 * rows_out * n_words >= 2^40; a null or misaligned table (8 B) or scratch (256 B); a null or misaligned d_out (4 B), d_out_words
 * or d_out_offsets (8 B): WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE.  Everything only the device sees is reported by
 * wah_bsi_div_status(), which synchronises the stream and reads the sweep's control words, then the compressor's:
 * WAH_ERR_STREAM for everything the list call refuses in an operand, WAH_ERR_CAPACITY for too small an output (nothing is
 * written at or behind d_out[out_capacity_words]).  EVERY row's every segment is walked and checked, so the verdict depends
 * neither on the data, nor on `what`, nor on n_slices_out.  The output of a refused call is unspecified.
 * wah_bsi_div_status(NULL, ...): WAH_ERR_ARG. */
#define WAH_DIV_QUOTIENT 0
#define WAH_DIV_REMAINDER 1
size_t wah_bsi_div_scratch_bytes(uint64_t n_words, uint64_t n_slices_b, uint64_t n_slices_out, unsigned flags);
int wah_bsi_div_indexed_device(int what, uint64_t n_words, uint64_t n_slices_a, uint64_t n_slices_b, uint64_t n_slices_out,
                               const wah_bitop_operand *d_rows, unsigned flags, uint32_t *d_out, uint64_t out_capacity_words,
                               uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream);
int wah_bsi_div_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_b, uint64_t n_slices_out, unsigned flags, void *stream);

/* The ORDER statistics of a bit-sliced attribute in ONE call -- `MIN(price) WHERE ...`, MAX, the median or any percentile, the
 * k-th largest, the threshold of `ORDER BY price DESC LIMIT k`: the value of a given rank among the rows that a set of filter
 * bitmaps selects (O'Neil & Quass; Rinfret, O'Neil & O'Neil).  It is a radix select over the slices, most significant first, all
 * of it on the device, and nothing of bitmap size is written.
 *   d_rows: n_filters + n_slices entries as for the list call (8-byte aligned, windows into column matrices allowed, the
 *   length may be a capacity, a row may name the not-yet-checked output of an earlier call on the stream).  The FILTERS come
 *   first, 0 <= n_filters <= WAH_BSI_KTH_MAX_FILTERS: bitmaps that are ANDed -- the attribute's existence bitmap, the result of
 *   a clause or range call.  The slices follow in sweep order, exactly as for the range call: the first slice row is the MOST
 *   significant, 1 <= n_slices <= WAH_BSI_MAX_SLICES.  The SELECTED rows are the positions p < 32 * n_words set in every
 *   filter; the pad bits of the last group are never selected, whichever stream sets them.  With n_filters == 0 all
 *   32 * n_words positions are selected: rows behind the caller's own row count then count with the value 0, as the range
 *   call documents.
 *   d_query: three uint64 in DEVICE memory, 8-byte aligned: {kind, a, b}.  WAH_BSI_KTH_ASCENDING: the value of rank a from
 *   the bottom, 0-based (a = 0: MIN); WAH_BSI_KTH_DESCENDING: rank a from the top (a = 0: MAX; a = k - 1: the threshold of a
 *   top-k); WAH_BSI_KTH_QUANTILE: rank floor(a * (total - 1) / b) from the bottom, the product taken in 128 bits, for b > 0
 *   and a <= b -- 0/1 is MIN, 1/1 is MAX, 1/2 the lower median.  b is not read by the other two kinds.
 *   d_result: five uint64, 8-byte aligned: {found, value, total, less, equal}.  total is the number of selected rows, less
 *   the number of selected rows whose value is below `value`, equal the number with exactly `value` (so the rows of `value`
 *   have the ranks less .. less + equal - 1 from the bottom).  The query is data, never an error: a rank at or beyond total,
 *   total == 0, an unknown kind, b == 0 or a > b give found = 0, and value, less and equal are then 0; total is still right,
 *   and everything is still walked and checked.  n_words == 0: total = 0.
 * Table and query are read by the device only: the call is asynchronous on `stream`, allocates nothing, never synchronises,
 * and a captured graph replayed after d_query (and / or the table) was overwritten in place answers the NEW query.  The value
 * is resolved in digits of four slices (the last digit may be shorter): per digit one launch in which one wavefront per
 * segment walks the filter rows and the slices down to the digit's end as the range call does, keeps the rows that still
 * match the bits decided so far in registers, and adds the segment's count of every pattern of the digit into a histogram;
 * and a one-wave launch that picks the bucket holding the rank.  No workgroup waits for another: the order of the launches is
 * the only synchronisation -- 2 * ceil(n_slices / 4) launches and the scratch clear.  The cost goes with the words of the
 * rows walked: the filters once per digit, slice i once per digit from its own on; no decoded bitmap exists at any point.
 *   d_scratch: wah_bsi_kth_scratch_bytes(n_words, n_slices) bytes, 256-byte aligned, no initialisation: the control words,
 *   the decision state and the histograms.  A multiple of 256, never 0; nothing in it goes with n_words or n_filters.
 * Errors the host can see come back before any HIP call, the argument checks first: n_slices outside 1 .. 64, n_filters
 * above 64, a null or misaligned table, query, result (8 B) or scratch (256 B), n_words >= 2^40: WAH_ERR_ARG; too small a
 * scratch: WAH_ERR_WORKSPACE.  Everything only the device sees is reported by wah_bsi_kth_status(), which synchronises the
 * stream: WAH_ERR_STREAM for everything the list call refuses in an operand.  EVERY row's every segment is checked in every
 * launch that walks it, and the last digit's launch walks them all: the verdict depends neither on the data nor on the
 * query.  The result of a refused call is unspecified.  wah_bsi_kth_status(NULL, ...): WAH_ERR_ARG. */
#define WAH_BSI_KTH_MAX_FILTERS 64u
#define WAH_BSI_KTH_ASCENDING 0u
#define WAH_BSI_KTH_DESCENDING 1u
#define WAH_BSI_KTH_QUANTILE 2u
size_t wah_bsi_kth_scratch_bytes(uint64_t n_words, uint64_t n_slices);
int wah_bsi_kth_indexed_device(uint64_t n_words, uint64_t n_filters, uint64_t n_slices, const wah_bitop_operand *d_rows,
                               const uint64_t *d_query, uint64_t *d_result, void *d_scratch, size_t scratch_bytes, void *stream);
int wah_bsi_kth_status(void *d_scratch, void *stream);

/* The VALUES of listed rows in ONE call, without decoding a bitmap -- the last step of `SELECT price, city FROM t WHERE ...
 * LIMIT 100`: the positions call gives the 100 row numbers, this call says what an attribute holds in them.  It is the inverse of
 * the two ways into the index (a bit-sliced attribute, an equality-encoded one): values -> index -> values.
 *   d_operands: a table exactly as for the list call (8-byte aligned, windows into column matrices allowed, rows may repeat, the
 *   length may be a capacity, an entry may name the not-yet-checked output of an earlier call on the stream).
 *   d_rows: n_rows positions p = 32 * word + bit in DEVICE memory, 8-byte aligned, NON-DESCENDING (duplicates are allowed and
 *   each gets its own output), each below 32 * n_words -- so a pad bit can never be asked for, and pad bits never matter.
 *   d_out: n_rows uint64, 8-byte aligned; entry i belongs to d_rows[i].
 *   WAH_FETCH_BITS: out[i] = the unsigned value whose bit n_operands - 1 - j is bit d_rows[i] of table row j (row 0 is the MOST
 *   significant, the sweep order of the range call): a bit-sliced attribute, 1 <= n_operands <= WAH_BSI_MAX_SLICES.  With the
 *   existence bitmap as row 0 in front of up to 63 slices the top bit of the output says whether the row has a value.
 *   WAH_FETCH_FIRST: out[i] = the lowest j whose bitmap has bit d_rows[i] set, UINT64_MAX if none has: the key of an
 *   equality-encoded attribute, 1 <= n_operands <= WAH_BITOP_LIST_MAX_OPERANDS.
 * Table and rows are read by the device only: the call is asynchronous on `stream`, allocates nothing, never synchronises, and a
 * captured graph replayed after d_rows and / or the table were overwritten in place, with the same counts, fetches the NEW rows.
 * Two launches and the clear of the control words; no workgroup waits for another.  The first checks every listed row and cuts
 * the list into items of at most 64 consecutive listed rows of one segment; the second is a grid of fixed size whose wavefronts
 * stride over the items: each walks the table for its segment as the range call does, and every lane picks the one bit of its
 * own listed row out of the segment's image whenever the walk crosses to another table row.
 * UNLIKE THE OTHER INDEXED CALLS, ONLY THE SEGMENTS THAT HOLD A LISTED ROW ARE READ AND CHECKED: the cost goes with the listed
 * rows and the words the table's rows hold in the segments they touch, not with the index -- so the verdict depends on WHICH
 * rows are listed (a malformed segment that no listed row lies in is never seen), and not on the data in them.  A segment with
 * R listed rows is walked at least ceil(R / 64) times: for a list that approaches every row, decoding the slices is the better
 * tool -- and wah_values_indexed_device (below) is that tool as one call, for a row RANGE.
 *   d_scratch: wah_fetch_scratch_bytes(n_words, n_rows) bytes, 256-byte aligned, no initialisation: the control words and the
 *   item list, ceil(n_rows / 64) + min(n_rows, segments) entries.  A multiple of 256, never 0, monotone in n_rows.
 * n_rows == 0 is WAH_OK (d_rows and d_out may be null) and wah_fetch_status() then reports WAH_OK.  Errors the host can see come
 * back before any HIP call, the argument checks first: an unknown mode, n_operands == 0 or above 64 (BITS) or above
 * WAH_BITOP_LIST_MAX_OPERANDS (FIRST), n_words == 0 with n_rows > 0, n_words >= 2^40 or n_rows >= 2^40, a null or misaligned
 * table, rows, out (8 B) or scratch (256 B): WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE.  Everything only the device
 * sees is reported by wah_fetch_status(), which synchronises the stream: WAH_ERR_STREAM for a row at or beyond 32 * n_words, a
 * row smaller than its predecessor, and everything the list call refuses in an operand, in the segments that are read.  EVERY
 * listed row is checked, and before it steers a read: after a refused row the second launch reads no stream at all.  The output
 * of a refused call is unspecified.  wah_fetch_status(NULL, ...): WAH_ERR_ARG. */
#define WAH_FETCH_BITS 0u
#define WAH_FETCH_FIRST 1u
size_t wah_fetch_scratch_bytes(uint64_t n_words, uint64_t n_rows);
int wah_fetch_indexed_device(unsigned mode, uint64_t n_words, uint64_t n_operands, const wah_bitop_operand *d_operands,
                             const uint64_t *d_rows, uint64_t n_rows, uint64_t *d_out, void *d_scratch, size_t scratch_bytes,
                             void *stream);
int wah_fetch_status(void *d_scratch, void *stream);

/* The values of a ROW RANGE in ONE call, without a decoded slice in global memory: a whole attribute read back out of the index --
 * exporting it, handing it to other code as a column, ORDER BY / DISTINCT / GROUP BY over all rows, a join probe, reordering a
 * table by a sort key.  It is the inverse of wah_bsi_build_device (WAH_FETCH_BITS) and of an equality-encoded index
 * (WAH_FETCH_FIRST) at column scale, as wah_fetch_indexed_device is for a short list of rows.
 *   d_out[i], for i in 0 .. n_rows - 1, is exactly what wah_fetch_indexed_device gives for the listed row first_row + i, with
 *   the same table and the same mode:
 *   WAH_FETCH_BITS: the unsigned value whose bit n_operands - 1 - j is that row's bit in table row j (row 0 is the MOST
 *   significant; an existence bitmap in front of up to 63 slices becomes the top bit), 1 <= n_operands <= WAH_BSI_MAX_SLICES.
 *   WAH_FETCH_FIRST: the lowest j whose bitmap has the row set, UINT64_MAX if none has, 1 <= n_operands <=
 *   WAH_BITOP_LIST_MAX_OPERANDS.
 *   d_operands: a table exactly as for the list call (8-byte aligned, windows into column matrices allowed, rows may repeat, the
 *   length may be a capacity, an entry may name the not-yet-checked output of an earlier call on the stream).
 *   first_row, n_rows: HOST arguments, first_row + n_rows <= 32 * n_words -- so a pad bit can never be asked for.
 *   d_out: n_rows uint64, 8-byte aligned.
 * The table is read by the device only: the call is asynchronous on `stream`, allocates nothing, never synchronises, and a
 * captured graph replayed after the table was overwritten in place reads the NEW attribute; the window stays as captured.
 * One launch and the clear of the control words; no workgroup waits for another.  One workgroup per item, a grid of capped size
 * striding over the items.  An item is a segment that overlaps the window; for WAH_FETCH_BITS with more than 32 table rows it is
 * a segment and a HALF of the value -- the table rows of significance 0 .. 31 (the table's last 32 rows) or 32 .. 63 (the rows in
 * front of them) -- and owns that 4-byte half of every output element of its segment, so no two items touch the same byte.  The
 * workgroup keeps 32 bits per row of the segment in LDS, its wavefronts walk the item's table rows as the list call does and fold
 * each into them, and the rows leave 64 consecutive rows per wavefront store, clipped to the window.
 * AS WITH FETCH, ONLY THE SEGMENTS THAT OVERLAP THE WINDOW ARE READ AND CHECKED; in those segments every table row is walked and
 * checked, so the verdict depends on the window and not on the data.
 * Every byte of d_out[0 .. n_rows) is written exactly once: no clearing pass, no read-modify-write of global memory, no atomics on
 * the output; nothing is written in front of d_out[0] or at or behind d_out[n_rows].
 *   d_scratch: wah_values_scratch_bytes(n_words, n_operands) bytes, 256-byte aligned, no initialisation: the control words only.
 *   A multiple of 256, never 0.
 * n_rows == 0 is WAH_OK (d_out may be null) and wah_values_status() then reports WAH_OK.  Errors the host can see come back
 * before any HIP call, the argument checks first: an unknown mode, n_operands == 0 or above 64 (BITS) or above
 * WAH_BITOP_LIST_MAX_OPERANDS (FIRST), n_words >= 2^40, a window that leaves 32 * n_words (overflow of first_row + n_rows
 * included), a null or misaligned table, out (8 B) or scratch (256 B): WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE.
 * Everything only the device sees is reported by wah_values_status(), which synchronises the stream: WAH_ERR_STREAM for
 * everything the list call refuses in an operand, in the segments that are read.  The output of a refused call is unspecified.
 * wah_values_status(NULL, ...): WAH_ERR_ARG. */
size_t wah_values_scratch_bytes(uint64_t n_words, uint64_t n_operands);
int wah_values_indexed_device(unsigned mode, uint64_t n_words, uint64_t n_operands, const wah_bitop_operand *d_operands,
                              uint64_t first_row, uint64_t n_rows, uint64_t *d_out, void *d_scratch, size_t scratch_bytes,
                              void *stream);
int wah_values_status(void *d_scratch, void *stream);

/* What a query wants from a result bitmap, WITHOUT decoding it: how many bits it has set (COUNT(*)) and which ones (row
 * numbers, with LIMIT / OFFSET).  A bitmap of n_words words has its bits at positions p = 32 * word + bit, LSB first; group g,
 * bit j, of its stream is position 31 * g + j.  "Set bits" are the positions p < 32 * n_words whose bit is 1: the 0 to 30 pad
 * bits of the last group (31 * G - 32 * n_words, G = wah_max_compressed_words(n_words)) are never counted or listed, even in a
 * hand-built stream that sets them -- by a last literal with pad bits, or by a one-fill that covers the last group
 * (compress() never sets them).  So a count equals the popcount of the first n_words decoded words, for every accepted stream.
 * Operands are indexed streams of compress() for bitmaps of n_words words, exactly as for wah_bitop_list_indexed_device, and
 * the same things are refused with WAH_ERR_STREAM, reported by wah_select_status(), which synchronises the stream: a null or
 * misaligned stream or index, a length of 2^40 or more, an index range outside stream_words, a segment whose words do not make
 * up exactly its groups, an empty fill.  An entry is checked before a pointer of it is followed, an index range before the
 * stream is read through it, and EVERY segment of every operand is checked, so the verdict does not depend on the data.
 *
 * wah_count_list_indexed_device: d_counts receives n_operands uint64, the set bits of each operand; entry i belongs to table
 * row i.  Over the columns of an equality-encoded attribute that is the GROUP BY histogram, over results of the clause call a
 * batch of COUNT(*)s.  d_operands as for the list call (8-byte aligned, 1 <= n_operands <= WAH_BITOP_LIST_MAX_OPERANDS,
 * operands may repeat, windows into column matrices allowed).  The call clears d_counts itself.  The table is read only by the
 * device: the call is asynchronous on `stream`, allocates nothing and never synchronises, and a captured graph replayed after
 * the table was overwritten in place counts the NEW selection.  n_words == 0: all counts 0.  Work is shared out by (operand,
 * segment) -- one operand of a long bitmap and thousands of short ones both fill the chip --; words are counted where they lie (a literal: its popcount; a one-fill: 31 bits per group; a
 * zero-fill: nothing), so the cost goes with the operands' words, not with n_operands x n_words.  A refused operand's count
 * is unspecified.
 *
 * wah_positions_indexed_device: ONE operand, given by host arguments (a window into a column matrix: d_offsets points into the
 * matrix index at the column's first segment, stream_words is the whole stream's length).  Writes the positions of the set
 * bits of ranks [first_rank, first_rank + out_capacity) to d_out[0 ..), ascending, as uint64; d_out_info[0] receives the total
 * of set bits, d_out_info[1] the number written, min(max(total - first_rank, 0), out_capacity).  A window that is too small is
 * not an error (LIMIT / OFFSET); nothing is written at or behind d_out[out_capacity].  out_capacity == 0 with a null d_out is
 * allowed and gives the total only.  Three steps, none of which waits for another workgroup: the count pass above with one
 * count per segment, a multi-level prefix sum of those, and one wavefront per segment that returns at once when its ranks miss
 * the window and otherwise stages its bits' positions in LDS and stores them 64 consecutive entries at a time.  A refused
 * stream writes nothing to d_out and zeros to d_out_info.
 *
 * wah_count_masked_indexed_device: the histogram of the rows a filter selects -- `SELECT b, COUNT(*) WHERE <conjunction> GROUP BY
 * b`, the cross-tab `GROUP BY a, b`, SUM over a bit-sliced attribute.  d_counts receives n_masks * n_operands uint64, row-major:
 * d_counts[i * n_operands + j] is the number of positions p < 32 * n_words set in BOTH mask i and operand j -- the popcount of the
 * AND of the first n_words decoded words of the two streams, for every accepted pair; the pad bits are never counted, whichever
 * of the two streams sets them.  d_masks and d_operands are two tables as for the list call (8-byte aligned, windows into column
 * matrices allowed, rows may repeat, a stream may be a mask and an operand); 1 <= n_masks, 1 <= n_operands, n_masks * n_operands
 * <= WAH_BITOP_LIST_MAX_OPERANDS.  A mask row may name the output buffer and index of a clause or list call enqueued before it on
 * the stream and not yet checked: stream_words is then the buffer's capacity, and the index bounds the words that are read.  The
 * call clears d_counts itself.  The tables are read only by the device: the call is asynchronous on `stream`, allocates nothing
 * and never synchronises, and a captured graph replayed after a table was overwritten in place counts the NEW selection.
 * n_words == 0: all counts 0.  Work is shared out by (mask, chunk of up to 64 consecutive operands, segment); no operand is decoded
 * and no bitmap written: the mask's segment is expanded ONCE per chunk into its 1024 groups and the prefix sums of their popcounts
 * in LDS, and the words of the chunk's operands are counted against them where they lie (a literal: one AND and a popcount; a
 * one-fill: a difference of two prefix sums; a zero-fill: nothing), so the cost goes with the operands' words.  A mask segment that is one fill needs no expansion: under zeros the
 * operand's segment is checked and counts nothing, under ones it is counted as by the call above.  EVERY segment of every mask
 * and of every operand is checked, also under an empty mask segment; a mask row is refused for what an operand row is refused for.
 * Counts of a refused call are unspecified.
 *
 * wah_group_sum_indexed_device: the grouped aggregate under a filter -- `SELECT g, h, COUNT(*), SUM(x), SUM(y) WHERE <filter>
 * GROUP BY g, h` over bit-sliced attributes x, y -- in one call, nothing read back and no bitmap written.  The mask of group g is
 * a CONJUNCTION: the AND of the n_filters rows of d_filters (0 <= n_filters <= WAH_GROUP_MAX_FILTERS; d_filters may be NULL when
 * there is none) and of rows g * rows_per_group .. (g + 1) * rows_per_group - 1 of d_groups (1 <= rows_per_group <=
 * WAH_GROUP_MAX_ROWS: one row per grouping attribute; n_groups * rows_per_group <= WAH_BITOP_LIST_MAX_OPERANDS).  d_operands are
 * the slices of n_attrs attributes back to back (1 <= n_attrs <= WAH_GROUP_MAX_ATTRS), attribute t's attr_bits[t] slices (1 .. 64)
 * most significant first; attr_bits is a HOST array, copied by the call, and its entries add up to n_operands.  1 <= n_groups,
 * 1 <= n_operands, n_groups * n_operands <= WAH_BITOP_LIST_MAX_OPERANDS.  All three tables are as for the list call (8-byte aligned,
 * windows into column matrices allowed, rows may repeat, a stream may stand in several tables; a filter row may name the output of
 * a clause or list call enqueued before it, as a mask row above).  Three outputs:
 *   d_group_rows[g]: the positions p < 32 * n_words set in every row of group g's conjunction -- COUNT(*) of the group;
 *   d_counts[g * n_operands + j]: those of them that are set in operand j as well, as the call above writes them;
 *   d_sums[(g * n_attrs + t) * 2 + {0, 1}]: the low and the high 64 bits of the sum over attribute t's slices i of
 *     d_counts[g][first_t + i] << (attr_bits[t] - 1 - i) -- SUM(x) over the group's rows.  A count is below 2^45, a sum below 2^109.
 * The pad bits are never counted, whichever stream sets them, in d_group_rows as little as in d_counts.  The call clears its
 * outputs itself.  The tables are read only by the device: the call is asynchronous on `stream`, allocates nothing and never
 * synchronises, and a captured graph replayed after a table was overwritten in place sums the NEW selection.  n_words == 0: all
 * zeros.  Work is shared out by (group, chunk of up to 64 consecutive operands, segment); the conjunction's segment is built ONCE
 * per chunk in LDS, row after row -- the first row's 1024 groups stored, every later row's ANDed into them, the prefix sums of the
 * popcounts behind the last one -- and the chunk's operands are counted against it as above; a second launch on the same stream
 * folds the counts into the sums.  A row whose segment is one one-fill changes nothing and is not expanded; one whose segment is
 * one zero-fill leaves nothing to count; if every row's is a one-fill the operands are counted as by the count call.  EVERY
 * segment of every filter row, group row and operand is checked under each of these short cuts; a filter row and a group row are
 * refused for what an operand row is refused for.  The outputs of a refused call are unspecified.
 *
 *   d_scratch: wah_select_scratch_bytes(n_words, n_operands) bytes, 256-byte aligned, no initialisation.  The size is a
 *   multiple of 256, never 0, and grows with n_words only: the control words, one uint64 per segment of 992 words + 1 (the
 *   positions call's rank table), and one uint64 per 4096 of those for each of the two upper levels of its prefix sum.
 *   Nothing in it goes with n_operands, n_masks or n_groups; one scratch serves all four calls.
 * Errors the host can see come back before any HIP call, argument checks first: a null or misaligned scratch (256 B), table,
 * d_counts, d_group_rows, d_sums, d_out or d_out_info (8 B; a null d_filters only with n_filters == 0), n_operands, n_masks,
 * n_groups or their products out of range, n_filters > WAH_GROUP_MAX_FILTERS, rows_per_group outside 1 .. WAH_GROUP_MAX_ROWS,
 * n_attrs outside 1 .. WAH_GROUP_MAX_ATTRS, a null attr_bits, a width of 0 or above 64, widths that do not add up to n_operands,
 * n_words >= 2^40: WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE.  wah_select_status(NULL, ...): WAH_ERR_ARG. */
#define WAH_GROUP_MAX_FILTERS 64u
#define WAH_GROUP_MAX_ROWS 8u /* rows ANDed per group: GROUP BY up to 8 attributes */
#define WAH_GROUP_MAX_ATTRS 64u
size_t wah_select_scratch_bytes(uint64_t n_words, uint64_t n_operands);
int wah_count_list_indexed_device(uint64_t n_words, uint64_t n_operands, const wah_bitop_operand *d_operands,
                                  uint64_t *d_counts, void *d_scratch, size_t scratch_bytes, void *stream);
int wah_count_masked_indexed_device(uint64_t n_words, uint64_t n_masks, const wah_bitop_operand *d_masks,
                                    uint64_t n_operands, const wah_bitop_operand *d_operands, uint64_t *d_counts,
                                    void *d_scratch, size_t scratch_bytes, void *stream);
int wah_group_sum_indexed_device(uint64_t n_words, uint64_t n_filters, const wah_bitop_operand *d_filters,
                                 uint64_t n_groups, uint64_t rows_per_group, const wah_bitop_operand *d_groups,
                                 uint64_t n_operands, const wah_bitop_operand *d_operands, uint64_t n_attrs,
                                 const uint8_t *attr_bits, uint64_t *d_group_rows, uint64_t *d_counts, uint64_t *d_sums,
                                 void *d_scratch, size_t scratch_bytes, void *stream);
int wah_positions_indexed_device(uint64_t n_words, const uint32_t *d_stream, uint64_t stream_words,
                                 const uint64_t *d_offsets, uint64_t first_rank, uint64_t *d_out,
                                 uint64_t out_capacity, uint64_t *d_out_info, void *d_scratch,
                                 size_t scratch_bytes, void *stream);
int wah_select_status(void *d_scratch, void *stream);

/* GROUP BY a BIT-SLICED key in ONE call -- `SELECT custkey, COUNT(*), SUM(revenue) WHERE <filters> GROUP BY custkey`, and with
 * a lookup table in front of the add the star join's GROUP BY: `SELECT d.year, SUM(f.revenue) FROM f JOIN d ON f.datekey = d.key
 * WHERE <d filter> GROUP BY d.year`.  The grouped calls above take one BITMAP per group; this one takes the grouping attribute
 * as slices, so a key of a million values is one table of twenty rows.  No value column, no decoded filter, no row list is
 * written.
 *   SELECTION: a row p < n_rows is selected if it is set in every row of d_filters (0 <= n_filters <= WAH_GROUP_MAX_FILTERS;
 *   d_filters may be NULL when there is none) and, with WAH_BSI_EXISTS in flags, in the key's existence bitmap, which is ONE more
 *   row behind the key's slices in d_key.  n_rows <= 32 n_words; rows at or behind n_rows and pad bits are never counted.
 *   KEY AND BUCKET: the key k of a selected row is the unsigned value of the key's n_slices_key slices (1 .. 32, most significant
 *   first).  With d_map (n_keys uint32 in DEVICE memory, 4-byte aligned, 1 <= n_keys <= 2^32) the row's bucket is b = d_map[k]
 *   when k < n_keys; without one (d_map NULL and n_keys == 0) b = k.  A row with k >= n_keys (with a map) or b >= n_buckets goes
 *   to the bucket "other", index n_buckets.  Keys and map entries are data, never errors, and nothing is read behind n_keys: a
 *   map entry of 0xFFFFFFFF drops a key, so a dimension's filter can ride in the map.
 *   OUTPUTS: d_counts is n_buckets + 1 uint64, bucket b the number of selected rows that map to b; d_sums is 2 (n_buckets + 1)
 *   uint64, per bucket the LOW then the HIGH word of the sum of the value attribute over those rows.  The value attribute is
 *   n_slices_val slices (1 .. 32, most significant first) WITHOUT an existence row: rows outside an existence bitmap were stored
 *   as 0 and add nothing.  n_slices_val == 0 is count only: d_val and d_sums must then be NULL.  The call clears both outputs
 *   itself unless WAH_GROUP_BY_ACCUMULATE is set; with the flag it ADDS into what is there, the carry from the low sum word
 *   going into the high one -- partitions of a table, or batches, land in one histogram.
 * Tables are 8-byte aligned; windows into column matrices, capacities as lengths and the not-yet-checked output of an earlier
 * call on the stream are allowed.  Tables and map are read by the device only: the call is asynchronous on `stream`, allocates
 * nothing, never synchronises, and a captured graph replayed after the map or a table was overwritten in place answers the NEW
 * query.  n_words == 0: all zeros, or under ACCUMULATE nothing added.  One launch of one workgroup per segment (two per segment
 * with a value attribute: each walks the segment and owns half of its groups, so a value attribute doubles the operand reads)
 * that folds the slices into one word per row in LDS and adds per row -- runs of equal consecutive buckets of a lane merged
 * first -- into buckets in LDS while n_buckets + 1 <= 2048, else into the outputs with 64-bit atomics.
 *   d_scratch: the control words only, 256-byte aligned, no initialisation:
 *   wah_bsi_group_by_scratch_bytes(n_words) = 1024 for every n_words (a multiple of 256, never 0).
 * Errors the host can see come back before any HIP call, in this order: (1) n_slices_key outside 1 .. 32, n_slices_val above 32,
 * unknown flag bits, n_filters above the cap; (2) a null or misaligned key table or scratch, a value table that does not go
 * with n_slices_val, a null filter table with n_filters > 0; (3) a map that does not go with n_keys or is misaligned, n_keys >
 * 2^32; (4) n_buckets outside 1 .. WAH_GROUP_BY_MAX_BUCKETS, null or misaligned d_counts, a d_sums that does not go with
 * n_slices_val; (5) n_words >= 2^40 or n_rows > 32 n_words -- all WAH_ERR_ARG; then too small a scratch: WAH_ERR_WORKSPACE.
 * Everything only the device sees is reported by wah_bsi_group_by_status(), which synchronises the stream: WAH_ERR_STREAM for
 * everything the list call refuses in an operand of any of the three tables.  EVERY row's every segment is walked and checked:
 * the verdict depends neither on the data nor on which rows are selected.  A key of more than 32 slices is refused -- a dense
 * array of buckets over such a domain does not exist: bucket its low slices, or group after a subtraction or a range. */
#define WAH_GROUP_BY_ACCUMULATE 2u /* add into the outputs instead of clearing them first */
#define WAH_GROUP_BY_MAX_BUCKETS (1u << 30)
size_t wah_bsi_group_by_scratch_bytes(uint64_t n_words);
int wah_bsi_group_by_indexed_device(uint64_t n_words, uint64_t n_rows, uint64_t n_filters, const wah_bitop_operand *d_filters,
                                    uint64_t n_slices_key, const wah_bitop_operand *d_key, uint64_t n_slices_val,
                                    const wah_bitop_operand *d_val, const uint32_t *d_map, uint64_t n_keys, uint64_t n_buckets,
                                    unsigned flags, uint64_t *d_counts, uint64_t *d_sums, void *d_scratch, size_t scratch_bytes,
                                    void *stream);
int wah_bsi_group_by_status(void *d_scratch, void *stream);

/* A BIT-SLICED key pushed through a lookup table in ONE call, the looked-up value leaving as a NEW bit-sliced attribute that
 * every call here takes -- the star join's PROJECTION, `SELECT d.unit_price FROM f JOIN d ON f.fk = d.rowid` as an attribute of f
 * (then compared, multiplied, ranked); a unary function of a small-domain key tabulated once (`EXTRACT(year FROM date_key)`,
 * `price / 10`, a CASE, histogram bins); a dictionary recoding.  The group-by call above pushes a key through the same kind of
 * table and leaves a histogram; this one leaves the column.  No value column is written and read again.
 *   KEY: d_key is the key's table, n_slices_key rows (1 .. 32, most significant slice first); with WAH_BSI_EXISTS in flags the
 *   key's existence bitmap follows as ONE more row.  n_rows <= 32 n_words.
 *   MAP: d_map is n_keys uint32 in DEVICE memory (4-byte aligned, 1 <= n_keys <= 2^32), key -> value.  An entry of WAH_MAP_NULL
 *   (0xFFFFFFFF) means "no value"; n_slices_out is 1 .. 32, so THE VALUE 2^32 - 1 IS NOT STORABLE: it is the null entry.
 *   WHICH ROWS HAVE A VALUE: a row p has one when p < n_rows, p exists in the key, its key k < n_keys and d_map[k] is not
 *   WAH_MAP_NULL; every other row is 0 in every result slice.  A MISS is an existing row in front of n_rows whose key is at or
 *   behind n_keys or whose entry is WAH_MAP_NULL.  With WAH_MAP_PARTIAL in flags a miss is simply a row without a value -- a
 *   dimension's filter rides in the map as null entries.  Without the flag a miss sets the sticky WAH_ERR_STREAM that
 *   wah_bsi_map_status reports, as a value at or above 2^n_bits does in wah_bsi_build_device.  In both modes an entry other
 *   than WAH_MAP_NULL with a bit at or above n_slices_out, loaded for a row, is WAH_ERR_STREAM.  Nothing is read at or behind
 *   n_keys, and nothing is loaded for a row that is not selected.
 *   RESULT: n_slices_out slices, most significant first, and an existence row as the LAST row exactly when
 *   flags & (WAH_BSI_EXISTS | WAH_MAP_PARTIAL): the rows that have a value (rows at or behind n_rows never do).  d_out,
 *   d_out_words and d_out_offsets receive exactly what wah_bsi_build_device leaves for the resulting value column: the
 *   compress() of the result's slice matrix [rows_out, n_words] as ONE bitmap and its whole segment index, rows_out * (n_words /
 *   992) + 1 entries, rows_out = n_slices_out (+ 1 with an existence row).
 * n_words is a non-zero multiple of 992 below 2^40, and rows_out * n_words stays below 2^40, as in the arithmetic call.  The
 * table and the map are read by the device only: the call is asynchronous on `stream`, allocates nothing, never synchronises and
 * reads nothing back, and a captured graph replayed after the map or the table was overwritten in place computes the NEW
 * attribute.  One launch of one workgroup per segment that folds the key's slices into one word per row in LDS, looks every
 * selected row up with many loads in flight per lane and transposes the values in registers into slice words by ballots; then
 * the compress passes.
 *   d_scratch: the builder's layout, 256-byte aligned, no initialisation:
 *   wah_bsi_map_scratch_bytes(n_words, n_slices_out, flags) = wah_bsi_build_scratch_bytes(n_words, rows_out).
 * Errors the host can see come back before any HIP call, in this order: (1) n_slices_key or n_slices_out outside 1 .. 32,
 * unknown flag bits; (2) a null or misaligned key table, scratch or output; (3) a null or misaligned map, n_keys outside 1 ..
 * 2^32; (4) n_words 0, no multiple of 992 or >= 2^40, rows_out * n_words >= 2^40, n_rows > 32 n_words -- all WAH_ERR_ARG; then
 * too small a scratch: WAH_ERR_WORKSPACE.  Everything only the device sees is reported by wah_bsi_map_status(), which
 * synchronises the stream: WAH_ERR_STREAM for everything the list call refuses in a row of the key table, for a miss without
 * WAH_MAP_PARTIAL and for an entry too wide for the result; then the compress passes' verdict (WAH_ERR_CAPACITY: nothing is
 * written at or behind d_out[out_capacity_words]).  A miss in a row that does not exist, or at or behind n_rows, is no miss.  The
 * output of a refused call is unspecified.  wah_bsi_map_status(NULL, ...): WAH_ERR_ARG. */
#define WAH_MAP_PARTIAL 2u /* flags: a miss is a row without a value, and the result has an existence row */
#define WAH_MAP_NULL 0xFFFFFFFFu /* a map entry without a value */
size_t wah_bsi_map_scratch_bytes(uint64_t n_words, uint64_t n_slices_out, unsigned flags);
int wah_bsi_map_indexed_device(uint64_t n_words, uint64_t n_rows, uint64_t n_slices_key, const wah_bitop_operand *d_key,
                               const uint32_t *d_map, uint64_t n_keys, uint64_t n_slices_out, unsigned flags, uint32_t *d_out,
                               uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                               size_t scratch_bytes, void *stream);
int wah_bsi_map_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_out, unsigned flags, void *stream);

/* The RUNNING SUM of a bit-sliced value over the rows a conjunction of filters selects, in ONE call, leaving as a NEW bit-sliced
 * attribute that every call here takes -- `SELECT SUM(x) OVER (ORDER BY rowid) FROM t WHERE f`, and without value slices the
 * running COUNT: ROW_NUMBER() over the selected rows, the cumulative distribution behind "the first row at which the running
 * revenue passes L", the rank of any row among the selected ones.  It is the one call here whose answer for row p depends on the
 * rows in front of p.  No value column is written and read again.
 *   SELECTION: as in the group-by call.  A row p < n_rows is selected if it is set in every row of d_filters (0 <= n_filters <=
 *   WAH_GROUP_MAX_FILTERS; d_filters may be NULL when there is none) and, with WAH_BSI_EXISTS in flags, in the value's existence
 *   bitmap, which is ONE more row behind the slices in d_val.  n_rows <= 32 n_words; rows at or behind n_rows and pad bits are
 *   never selected.
 *   VALUE: d_val is the value's table, n_slices_val rows (0 .. 32, most significant slice first), unsigned.  n_slices_val == 0:
 *   every selected row counts 1; d_val is then NULL unless WAH_BSI_EXISTS is set, and with the flag holds just the existence row.
 *   RESULT: R[p] = (the sum of the values of the selected rows q <= p) mod 2^n_slices_out, with WAH_CUMSUM_EXCLUSIVE over q < p;
 *   n_slices_out is 1 .. WAH_BSI_MAX_SLICES, most significant slice first.  The sum is carried in 64 bits everywhere and cut only
 *   where it is stored: a result narrower than the true sum holds its low bits.  By default only SELECTED rows hold a value, every
 *   other row is 0 in every slice, and the result's LAST row is its existence row, equal to the selection.  With
 *   WAH_CUMSUM_ALL_ROWS every row in front of n_rows holds the running value -- an unselected row carries it forward: the rank of
 *   row p among the selected rows, for any p -- and the result has NO existence row.  rows_out = n_slices_out + (ALL_ROWS ? 0 : 1).
 *   d_out, d_out_words and d_out_offsets receive exactly what wah_bsi_build_device leaves for a value column of rows_out rows:
 *   the compress() of the result's slice matrix [rows_out, n_words] as ONE bitmap and its whole segment index, rows_out *
 *   (n_words / 992) + 1 entries.
 * n_words is a non-zero multiple of 992 below 2^40, and rows_out * n_words stays below 2^40, as in the map call.  Tables are
 * 8-byte aligned; windows into column matrices, capacities as lengths and the not-yet-checked output of an earlier call on the
 * stream are allowed.  The tables are read by the device only: the call is asynchronous on `stream`, allocates nothing, never
 * synchronises and reads nothing back, and a captured graph replayed after a table was overwritten in place computes the NEW
 * result.  Three launches, no workgroup of which waits for another -- one workgroup per segment adds popcount(slice AND
 * selection) << significance into one total per segment; one workgroup scans the totals; one workgroup per segment folds the
 * slices into one word per row in LDS, scans the rows 64 at a time with the carry of the steps, blocks and segments in front, and
 * transposes the sums in registers into slice words by ballots -- then the compress passes.
 *   d_scratch: the builder's layout and one uint64 per segment behind it, 256-byte aligned, no initialisation:
 *   wah_bsi_cumsum_scratch_bytes(n_words, n_slices_out, flags) = wah_bsi_build_scratch_bytes(n_words, rows_out) + 8 (n_words /
 *   992) rounded up to a multiple of 256.
 * Errors the host can see come back before any HIP call, in this order: (1) n_slices_val above 32, n_slices_out outside 1 .. 64,
 * unknown flag bits, n_filters above the cap; (2) a null or misaligned scratch or output, a d_val that does not go with
 * n_slices_val and the flags, a null filter table with n_filters > 0; (3) n_words 0, no multiple of 992 or >= 2^40, rows_out *
 * n_words >= 2^40, n_rows > 32 n_words -- all WAH_ERR_ARG; then too small a scratch: WAH_ERR_WORKSPACE.  Everything only the
 * device sees is reported by wah_bsi_cumsum_status(), which synchronises the stream: WAH_ERR_STREAM for everything the list call
 * refuses in a row of either table, EVERY row's every segment being walked whatever is selected; then the compress passes'
 * verdict (WAH_ERR_CAPACITY: nothing is written at or behind d_out[out_capacity_words]).  The output of a refused call is
 * unspecified.  wah_bsi_cumsum_status(NULL, ...): WAH_ERR_ARG.  Not here: signed values, values above 32 slices.  (Sums that
 * start again per partition: wah_bsi_cumsum_parts_indexed_device, below; a partition's total in every one of its rows:
 * wah_bsi_total_parts_indexed_device, below that.) */
#define WAH_CUMSUM_EXCLUSIVE 2u /* flags: the sum runs over the rows in front of a row, not up to it */
#define WAH_CUMSUM_ALL_ROWS 4u  /* flags: unselected rows carry the sum forward, and the result has no existence row */
size_t wah_bsi_cumsum_scratch_bytes(uint64_t n_words, uint64_t n_slices_out, unsigned flags);
int wah_bsi_cumsum_indexed_device(uint64_t n_words, uint64_t n_rows, uint64_t n_filters, const wah_bitop_operand *d_filters,
                                  uint64_t n_slices_val, const wah_bitop_operand *d_val, uint64_t n_slices_out, unsigned flags,
                                  uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets,
                                  void *d_scratch, size_t scratch_bytes, void *stream);
int wah_bsi_cumsum_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_out, unsigned flags, void *stream);

/* The RUNNING SUM PER PARTITION: wah_bsi_cumsum_indexed_device with a sum that starts again at every row of a bitmap of partition
 * starts -- `SELECT SUM(x) OVER (PARTITION BY g ORDER BY rowid) FROM t WHERE f` on a table clustered by g, without value slices
 * `ROW_NUMBER() OVER (PARTITION BY g)`, and with the starts the complement of the filter the length of the current streak of
 * selected rows.  Selection, value, flags (WAH_BSI_EXISTS, WAH_CUMSUM_EXCLUSIVE, WAH_CUMSUM_ALL_ROWS), the result's layout,
 * rows_out, the compress road and the status call's behaviour are those of wah_bsi_cumsum_indexed_device.
 *   STARTS: d_starts names ONE indexed bitmap of n_words words in device memory, in the operand form of a filter row, 8-byte
 *   aligned.  Row p STARTS A PARTITION if its bit is set and p < n_rows -- whether or not p is selected.  Bits at or behind n_rows
 *   and pad bits have no effect.
 *   RESULT: let s(p) be the largest start row <= p, or 0 if there is none; R[p] = (the sum of the values of the selected rows q
 *   with s(p) <= q <= p) mod 2^n_slices_out, with WAH_CUMSUM_EXCLUSIVE over s(p) <= q < p.  A selected start row holds its own
 *   value, under EXCLUSIVE 0.  With WAH_CUMSUM_ALL_ROWS an unselected row carries its partition's running value forward, and an
 *   unselected start row holds 0.  Without value slices the result is the running COUNT within the partition.  A starts bitmap
 *   with no bit set gives, word for word, what wah_bsi_cumsum_indexed_device gives.  The sum is carried in 64 bits and cut only
 *   where it is stored.
 * The same three launches, none of which waits for another workgroup, with the segmented operator on pairs (has_start, sum),
 * (f1, s1) o (f2, s2) = (f1 | f2, f2 ? s2 : s1 + s2), in the place of addition: per segment whether it holds a start and the sum of
 * the selected values at or behind its last one (popcounts under a "rows at or behind the last start" mask); one workgroup scans
 * the pairs into what flows into each segment; the rows kernel folds block pairs the same way and, in a step of 64 rows that
 * holds a start, subtracts from the ordinary scan its exclusive value at the lane's own head lane.
 *   d_scratch: the builder's layout and one record of 16 bytes per segment behind it, 256-byte aligned, no initialisation:
 *   wah_bsi_cumsum_parts_scratch_bytes(n_words, n_slices_out, flags) = wah_bsi_build_scratch_bytes(n_words, rows_out) + 16
 *   (n_words / 992) rounded up to a multiple of 256.
 * Errors the host can see come back before any HIP call, in the order of wah_bsi_cumsum_indexed_device, with texts of this call's
 * own: (1) n_slices_val above 32, n_slices_out outside 1 .. 64, unknown flag bits, n_filters above the cap; (2) a null or
 * misaligned scratch or output, a d_val that does not go with n_slices_val and the flags, a null filter table with n_filters > 0,
 * a null or misaligned d_starts; (3) n_words 0, no multiple of 992 or >= 2^40, rows_out * n_words >= 2^40, n_rows > 32 n_words --
 * all WAH_ERR_ARG; then too small a scratch: WAH_ERR_WORKSPACE.  Everything only the device sees is reported by
 * wah_bsi_cumsum_parts_status(), which synchronises the stream: WAH_ERR_STREAM for everything the list call refuses in a row of
 * either table or in the starts row, EVERY row's every segment being walked; then the compress passes' verdict.  Nothing is read
 * back: the call is asynchronous on `stream`, allocates nothing and can be captured in a graph.  The output of a refused call is
 * unspecified.  wah_bsi_cumsum_parts_status(NULL, ...): WAH_ERR_ARG.  Not here: signed values, values above 32 slices.  (Partition
 * totals broadcast to every row: wah_bsi_total_parts_indexed_device, below.) */
size_t wah_bsi_cumsum_parts_scratch_bytes(uint64_t n_words, uint64_t n_slices_out, unsigned flags);
int wah_bsi_cumsum_parts_indexed_device(uint64_t n_words, uint64_t n_rows, uint64_t n_filters, const wah_bitop_operand *d_filters,
                                        uint64_t n_slices_val, const wah_bitop_operand *d_val, const wah_bitop_operand *d_starts,
                                        uint64_t n_slices_out, unsigned flags, uint32_t *d_out, uint64_t out_capacity_words,
                                        uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes,
                                        void *stream);
int wah_bsi_cumsum_parts_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_out, unsigned flags, void *stream);

/* The PARTITION'S TOTAL IN EVERY ROW: `SELECT SUM(x) OVER (PARTITION BY g) FROM t WHERE f` on a table clustered by g -- the window
 * aggregate without ORDER BY, for a share of total (x / SUM(x) OVER ...), without value slices `COUNT(*) OVER (PARTITION BY g)`,
 * the size of a row's group, both divided the group mean, and compared with a bound the rows of the groups that a HAVING keeps.
 * Selection, value, starts, widths, alignment, limits, the result's layout, rows_out, the compress road and the status call's
 * behaviour are those of wah_bsi_cumsum_parts_indexed_device.
 *   RESULT: let s(p) be the largest start row <= p, or 0 if there is none, and e(p) the smallest start row > p, minus 1, or
 *   n_rows - 1 if there is none; T[p] = (the sum of the values of the selected rows q with s(p) <= q <= e(p)) mod 2^n_slices_out.
 *   By default only selected rows hold T, every other row is 0 in every slice, and the result's last row is its existence row,
 *   the selection.  With WAH_CUMSUM_ALL_ROWS every row in front of n_rows holds its partition's total, a partition without a
 *   selected row 0, and there is no existence row.  Without value slices T is the number of selected rows of the partition.  A
 *   starts bitmap with no bit set puts the grand total into every row.  The sum is carried in 64 bits and cut only where it is
 *   stored.  T[p] is what wah_bsi_cumsum_parts_indexed_device with WAH_CUMSUM_ALL_ROWS holds at row e(p).
 *   FLAGS: WAH_BSI_EXISTS and WAH_CUMSUM_ALL_ROWS.  WAH_CUMSUM_EXCLUSIVE has no meaning here and is refused with the unknown bits.
 * The same three launches, none of which waits for another workgroup, with TWO sums per item beside has_start: its head, the
 * selected values in front of its first start, and its tail, those at or behind its last one (both the whole item where it holds
 * no start).  Per segment a record from popcounts under the two masks; one workgroup scans the records in both directions, the
 * tails from the front with the operator above, the heads from the end with its mirror -- what flows in from behind a segment is
 * the heads of the segments behind it up to and including the first that holds a start; the rows kernel folds block triples the
 * same way, runs the partitioned call's inclusive step forward over a block and then walks the steps backward: a row's total is
 * the running sum at the lane in front of the next start behind it in its step of 64 rows (one ds_bpermute per word), and where
 * the step holds none behind it a wave-uniform value carried from step to step.
 *   d_scratch: the builder's layout and one record of 24 bytes per segment behind it, 256-byte aligned, no initialisation:
 *   wah_bsi_total_parts_scratch_bytes(n_words, n_slices_out, flags) = wah_bsi_build_scratch_bytes(n_words, rows_out) + 24
 *   (n_words / 992) rounded up to a multiple of 256.
 * Errors the host can see come back before any HIP call, in the groups and the order of wah_bsi_cumsum_parts_indexed_device, with
 * texts of this call's own: (1) n_slices_val above 32, n_slices_out outside 1 .. 64, unknown flag bits -- WAH_CUMSUM_EXCLUSIVE
 * among them --, n_filters above the cap; (2) a null or misaligned scratch or output, a d_val that does not go with n_slices_val
 * and the flags, a null filter table with n_filters > 0, a null or misaligned d_starts; (3) n_words 0, no multiple of 992 or
 * >= 2^40, rows_out * n_words >= 2^40, n_rows > 32 n_words -- all WAH_ERR_ARG; then too small a scratch: WAH_ERR_WORKSPACE.
 * Everything only the device sees is reported by wah_bsi_total_parts_status(), which synchronises the stream: WAH_ERR_STREAM for
 * everything the list call refuses in a row of either table or in the starts row, EVERY row's every segment being walked; then
 * the compress passes' verdict.  Nothing is read back: the call is asynchronous on `stream`, allocates nothing and can be
 * captured in a graph.  The output of a refused call is unspecified.  wah_bsi_total_parts_status(NULL, ...): WAH_ERR_ARG.  Not
 * here: MIN / MAX per partition in every row, frames (ROWS BETWEEN), signed values, values above 32 slices. */
size_t wah_bsi_total_parts_scratch_bytes(uint64_t n_words, uint64_t n_slices_out, unsigned flags);
int wah_bsi_total_parts_indexed_device(uint64_t n_words, uint64_t n_rows, uint64_t n_filters, const wah_bitop_operand *d_filters,
                                       uint64_t n_slices_val, const wah_bitop_operand *d_val, const wah_bitop_operand *d_starts,
                                       uint64_t n_slices_out, unsigned flags, uint32_t *d_out, uint64_t out_capacity_words,
                                       uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes,
                                       void *stream);
int wah_bsi_total_parts_status(void *d_scratch, uint64_t n_words, uint64_t n_slices_out, unsigned flags, void *stream);

/* The order statistics PER GROUP in ONE call -- `SELECT g, h, MIN(x), MAX(x), median(x) WHERE <filter> GROUP BY g, h`: for every
 * group g and every query q the value of rank q among the rows that `filters AND group g's rows` select, over ONE bit-sliced
 * attribute.  It is wah_bsi_kth_indexed_device's radix select for L = n_groups * n_queries selects ("lanes") at once.
 *   d_filters, d_groups, d_slices: three tables as for the list call (8-byte aligned, windows into column matrices allowed, rows
 *   may repeat, a stream may stand in several tables, the length may be a capacity, a filter row may name the not-yet-checked
 *   output of an earlier call on the stream).  0 <= n_filters <= WAH_BSI_KTH_MAX_FILTERS (d_filters may be NULL only when there
 *   is none); 1 <= rows_per_group <= WAH_GROUP_MAX_ROWS and group g's rows are rows g * rows_per_group .. of d_groups, exactly as
 *   for wah_group_sum_indexed_device; 1 <= n_slices <= WAH_BSI_MAX_SLICES, the MOST significant slice first.  Group g SELECTS the
 *   positions p < 32 * n_words set in every filter row and in every one of its rows; the pad bits of the last group are never
 *   selected, whichever stream sets them.  Groups may overlap and may be empty.
 *   d_queries: n_queries x {kind, a, b} uint64 in DEVICE memory, 8-byte aligned, each exactly as d_query of the ungrouped call;
 *   every group is asked the same n_queries queries.
 *   d_results: five uint64 per (group, query), 8-byte aligned: d_results[(g * n_queries + q) * 5 + {0 .. 4}] = {found, value,
 *   total, less, equal}, each meaning exactly what it means in the ungrouped call.  A query is data, never an error: a rank at or
 *   beyond total, an unknown kind, b == 0 or a > b give found = 0 and value = less = equal = 0, total is still right.  n_words ==
 *   0: total = 0 and found = 0 everywhere.  The call writes every result row itself.
 * Bounds: 1 <= n_groups, 1 <= n_queries, n_groups * n_queries <= WAH_BSI_KTH_GROUPED_MAX_LANES, n_groups * rows_per_group <=
 * WAH_BITOP_LIST_MAX_OPERANDS.  The lane bound is 4096 because the scratch goes with it: sixteen passes of a 64-bit attribute
 * are 2 KiB of histograms a lane, 8.5 MiB at 4096 lanes, cleared by every call; and 64 groups x 64 queries is more than a
 * GROUP BY with percentiles asks for.
 * Tables and queries are read by the device only: the call is asynchronous on `stream`, allocates nothing, reads nothing back,
 * writes nothing of bitmap size, and a captured graph replayed after the queries and / or a table were overwritten in place
 * answers the NEW question.  Per digit of four slices ONE launch serves all lanes and one more decides for all of them:
 * 2 * ceil(n_slices / 4) launches and the scratch clear, whatever n_groups and n_queries are.  The work items of a pass are
 * (segment, lane) pairs, the lane running fastest; an item ANDs the filter rows and its group's rows of that segment, and, if
 * they select anything there, walks the slices down to the digit's end and counts as the ungrouped call does.  With keys that
 * are clustered in row order nearly every item ends behind its group's rows.
 *   d_scratch: wah_bsi_kth_grouped_scratch_bytes(n_words, n_slices, n_groups, n_queries) bytes, 256-byte aligned, no
 *   initialisation.  With L = n_groups * n_queries and P = ceil(n_slices / 4) it is
 *       1024 + round256(L * 128) + round256(P * L * 128)
 *   bytes (round256: up to a multiple of 256): the control words, a decision state of 16 uint64 per lane, and per pass and lane
 *   one histogram of 16 uint64.  A multiple of 256, never 0; nothing in it goes with n_words, n_filters or rows_per_group.
 * Errors the host can see come back before any HIP call, the argument checks first: n_slices outside 1 .. 64, n_filters above
 * 64, rows_per_group outside 1 .. WAH_GROUP_MAX_ROWS, n_groups or n_queries 0 or their product above the lane bound, a null or
 * misaligned table (a null d_filters only with n_filters == 0), queries, results (8 B) or scratch (256 B), n_words >= 2^40:
 * WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE.  Everything only the device sees is reported by
 * wah_bsi_kth_grouped_status(), which synchronises the stream: WAH_ERR_STREAM for everything the list call refuses in an operand.
 * The verdict depends neither on the data nor on the queries, but HOW is weaker here than "every launch checks every row it
 * walks": every segment of every filter row and of every group's rows is walked and checked by that group's items in every
 * pass; every segment of every SLICE is walked and checked once per call, by the items of lane 0 in the LAST pass (which walks
 * all slices), whether or not lane 0 selects anything there.  The other items skip the slices of a segment in which they select
 * nothing, so a malformed slice segment is always refused, but not by every launch.  The results of a refused call are
 * unspecified.  wah_bsi_kth_grouped_status(NULL, ...): WAH_ERR_ARG. */
#define WAH_BSI_KTH_GROUPED_MAX_LANES 4096u
size_t wah_bsi_kth_grouped_scratch_bytes(uint64_t n_words, uint64_t n_slices, uint64_t n_groups, uint64_t n_queries);
int wah_bsi_kth_grouped_indexed_device(uint64_t n_words, uint64_t n_filters, const wah_bitop_operand *d_filters,
                                       uint64_t n_groups, uint64_t rows_per_group, const wah_bitop_operand *d_groups,
                                       uint64_t n_slices, const wah_bitop_operand *d_slices, uint64_t n_queries,
                                       const uint64_t *d_queries, uint64_t *d_results, void *d_scratch, size_t scratch_bytes,
                                       void *stream);
int wah_bsi_kth_grouped_status(void *d_scratch, void *stream);

/* The way INTO the index that does not go through a decoded bitmap: compressed bitmaps straight from sorted lists of row numbers
 * -- the rows of every value of a key column (one stable sort groups them), the row ids a join returns, a tombstone list.  The
 * reverse of wah_positions_indexed_device; not in the reference, whose compress() takes the decoded bitmap (compress.cu:41-209).
 *   d_rows: n_rows positions p = 32 * word + bit, the lists back to back.  d_list_ends: n_lists entries in DEVICE memory: list c
 *   is d_rows[end(c - 1) .. end(c)) with end(-1) = 0.  Inside a list the positions ascend strictly and are below 32 * n_words; a
 *   list may be empty; the ends never decrease and the last one equals n_rows.  n_rows == 0 with a null d_rows is allowed.
 * d_out receives the streams of all lists back to back, list 0 first, each word for word what compress() emits for the bitmap of
 * n_words words that has exactly those bits set (ragged n_words included: the pad bits of the last group stay zero).
 * d_out_offsets (required) receives n_lists * S + 1 entries, S = ceil(G / 1024), G = wah_max_compressed_words(n_words): entry
 * c * S + s is the first word of segment s of list c, counted from d_out[0]; the last entry is the total, which d_out_words
 * receives too.  For n_words % 992 == 0 the pair is exactly the (stream, whole index) of a column matrix compressed in one launch
 * (wah_compress_device_indexed over back-to-back columns), so every indexed call takes it unchanged; for any n_words a
 * wah_bitop_operand with d_offsets = d_out_offsets + c * S is list c.
 *   wah_from_positions_max_words: an out_capacity_words that always suffices: min(n_lists * G, n_lists * S + 2 * n_rows) -- a
 *   segment with r rows has at most r literal or one-fill words and r + 1 gaps.
 *   d_scratch: wah_from_positions_scratch_bytes(n_words, n_lists) bytes, 256-byte aligned, no initialisation: the control words
 *   and the two upper levels (one uint64 per 4096 entries of the level below) of the prefix sum over the index entries, which
 *   itself runs in place in d_out_offsets.  A multiple of 256, never 0.
 * The lists are read only by the device: the call is asynchronous on `stream`, allocates nothing and never synchronises, and a
 * captured graph replayed after d_rows and d_list_ends were overwritten in place (same n_rows, same n_lists) builds the NEW
 * lists.  Three steps, none of which waits for another workgroup: a pass that checks every end and every row; one wavefront per
 * (list, segment) that finds its slice of the list by searching for the segment's bit range and counts the segment's words -- no
 * row: one zero-fill; up to 64 rows: in registers, a row per lane; more: through an image of the segment's 1024 groups in LDS --;
 * the prefix sum of the counts; and the same wavefronts again, which now store the words, 64 consecutive ones at a time.  No
 * decoded bitmap exists at any point: the cost goes with n_rows and n_lists * S.
 * Errors the host can see come back before any HIP call, argument checks first: n_lists < 1 or > WAH_BITOP_LIST_MAX_OPERANDS,
 * n_lists * S >= 2^31, n_words == 0 or >= 2^40, n_rows >= 2^40, a null or misaligned d_list_ends, d_out_offsets, d_out_words
 * (8 B), d_out (4 B) or scratch (256 B), a null d_rows with n_rows > 0: WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE.
 * Everything only the device sees is reported by wah_from_positions_status(), which synchronises the stream: WAH_ERR_STREAM for a
 * row at or beyond 32 * n_words, two neighbours of one list that do not ascend strictly (duplicates included), ends that
 * decrease, a last end that is not n_rows -- a descent across a list boundary is legal --; WAH_ERR_CAPACITY for too small an
 * output (nothing is written at or behind d_out[out_capacity_words]).  EVERY row and every end is checked, so the verdict does not
 * depend on the data, and an end is checked before it bounds a read of d_rows.  Rows that do not ascend are refused, not
 * sorted; the output of a refused call is unspecified.  wah_from_positions_status(NULL, ...): WAH_ERR_ARG. */
uint64_t wah_from_positions_max_words(uint64_t n_words, uint64_t n_lists, uint64_t n_rows);
size_t wah_from_positions_scratch_bytes(uint64_t n_words, uint64_t n_lists);
int wah_from_positions_device(uint64_t n_words, uint64_t n_lists, const uint64_t *d_list_ends, const uint64_t *d_rows,
                              uint64_t n_rows, uint32_t *d_out, uint64_t out_capacity_words, uint64_t *d_out_words,
                              uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream);
int wah_from_positions_status(void *d_scratch, void *stream);

/* The call that changes the ROWS of an index: row ranges ("pieces") of indexed bitmaps concatenated into new indexed bitmaps, at
 * any bit offset, for all columns of an index at once -- INSERT of a batch (the index, then the batch), the rollover of a time
 * partition (drop the oldest range, append the newest), a [first, first + n) window of every column of an attribute, the split of
 * an index by row ranges over the GPUs of a node.  Not in the reference.
 *   d_pieces: n_pieces entries in DEVICE memory, 8-byte aligned.  d_operands: n_pieces * n_columns entries, piece-major: entry
 *   p * n_columns + c is column c of piece p, an indexed bitmap of d_pieces[p].n_words words as for the list call (windows into
 *   column matrices allowed, the length may be a capacity, streams compress() never emits are legal).
 * With start(p) the sum of n_rows of the pieces before p and T the sum over all pieces, output bitmap c has n_words_out words;
 * its position start(p) + i is position first_row(p) + i of operand (p, c) for i < n_rows(p), and every position at or behind T is
 * zero, the pad bits of the last group included.  A piece of no rows is legal: its operands are not followed and may be null.
 * The output is laid out as wah_from_positions_device's: d_out receives the n_columns compress() streams back to back, word for
 * word, whatever form the sources had; d_out_offsets (required) receives n_columns * S + 1 entries counted from d_out[0],
 * S = ceil(G / 1024), G = wah_max_compressed_words(n_words_out); d_out_words receives the total, also when it exceeds the capacity.
 * For n_words_out % 992 == 0 the pair is a column matrix's (stream, whole index); for any n_words_out a wah_bitop_operand with
 * d_offsets = d_out_offsets + c * S is column c.
 *   wah_splice_max_words: an out_capacity_words that always suffices:
 *   min(n_columns * G, n_columns * (S + 1) + 2 * n_pieces * n_columns + 2 * source_words), saturating at UINT64_MAX.  source_words
 *   is any upper bound the caller has on the words of the source segments that are touched; the operands' whole streams are one.
 *   Why it holds: a literal source word meets at most two output groups (2 * source_words); a fill leaves one fill word, and at
 *   most one group where it ends inside an output group is charged to it (the other 1 of its 2); a piece has two ends in every
 *   column, each of which may cut a run in two (2 * n_pieces * n_columns); every output segment cuts at most one run, and the zeros
 *   behind T are one more run (n_columns * (S + 1)).
 *   d_scratch: wah_splice_scratch_bytes(n_words_out, n_columns, n_pieces) bytes, 256-byte aligned, no initialisation:
 *   1024 (the control words) + round256(8 * (n_pieces + 1)) (the running starts) + round256(8 * ceil(E / 4096)) +
 *   round256(8 * ceil(ceil(E / 4096) / 4096)) with E = n_columns * S + 1 (the two upper levels of the prefix sum over the index,
 *   which itself runs in place in d_out_offsets) and round256 rounding up to a multiple of 256.  A multiple of 256, never 0.
 * Pieces and table are read only by the device: the call is asynchronous on `stream`, allocates nothing and never synchronises,
 * and a captured graph replayed after d_pieces and d_operands were overwritten in place, with the same counts, splices the NEW
 * pieces.  Four steps, none of which waits for another workgroup: a launch that checks every piece and leaves start(0 .. n_pieces)
 * in the scratch; one wavefront per (column, output segment) that searches the starts for the pieces overlapping its 31 744 bits,
 * walks for each of them the one or two source segments that hold its rows into an image of 1024 groups in LDS, moves the bits
 * onto the output's group grid in a second image and counts the words of that; the prefix sum of the counts; the same wavefronts
 * again, which now store the words, 64 consecutive ones at a time.  No decoded bitmap exists at any point.  Like the fetch call
 * and unlike the others, ONLY the source segments that hold a spliced row are read and checked: the verdict depends on the
 * pieces, not on the data.
 * Errors the host can see come back before any HIP call, argument checks first: n_columns < 1 or > WAH_BITOP_LIST_MAX_OPERANDS,
 * n_pieces < 1 or > WAH_SPLICE_MAX_PIECES, n_pieces * n_columns > 2^24, n_columns * S >= 2^31, n_words_out == 0 or >= 2^40, a null
 * or misaligned d_pieces, d_operands, d_out_offsets, d_out_words (8 B), d_out (4 B) or scratch (256 B): WAH_ERR_ARG; too small a
 * scratch: WAH_ERR_WORKSPACE.  Everything only the device sees is reported by wah_splice_status(), which synchronises the
 * stream: WAH_ERR_STREAM for a piece with n_rows > 0 and n_words == 0 or >= 2^40, for first_row + n_rows > 32 * n_words (checked
 * without wrapping), for an n_rows above 32 * n_words_out or T > 32 * n_words_out, and for everything the list call refuses in
 * an operand, in the source segments that are read; WAH_ERR_CAPACITY for too small an output (nothing is written at or behind
 * d_out[out_capacity_words]).  Every piece is checked before it steers a read, and after a refused piece the later launches read
 * no stream.  The output of a refused call is unspecified.  wah_splice_status(NULL, ...): WAH_ERR_ARG. */
typedef struct {
    uint64_t n_words;   /* the words of ONE bitmap of this piece's operands          */
    uint64_t first_row; /* first position (32 * word + bit) taken from each of them  */
    uint64_t n_rows;    /* how many consecutive positions; 0 is legal                */
} wah_splice_piece;     /* 24 bytes, no padding */
#define WAH_SPLICE_MAX_PIECES (1u << 16)
uint64_t wah_splice_max_words(uint64_t n_words_out, uint64_t n_columns, uint64_t n_pieces, uint64_t source_words);
size_t wah_splice_scratch_bytes(uint64_t n_words_out, uint64_t n_columns, uint64_t n_pieces);
int wah_splice_indexed_device(uint64_t n_words_out, uint64_t n_columns, uint64_t n_pieces, const wah_splice_piece *d_pieces,
                              const wah_bitop_operand *d_operands, uint32_t *d_out, uint64_t out_capacity_words,
                              uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch, size_t scratch_bytes, void *stream);
int wah_splice_status(void *d_scratch, void *stream);

/* The call that changes an index by a PREDICATE: the rows a mask bitmap selects of every column of an index, moved together into
 * new indexed bitmaps -- DELETE FROM t WHERE ... (WAH_COMPACT_DELETE: the rows the mask does NOT name survive), CREATE TABLE s AS
 * SELECT * FROM t WHERE ..., a sample, the drop of tomb-stoned rows, "the next twenty queries on the rows the first filter kept".
 * The splice call moves row RANGES the host knows; this one moves scattered rows only the device knows.  Not in the reference.
 *   d_mask: ONE wah_bitop_operand in DEVICE memory, 8-byte aligned; d_operands: n_columns of them.  All are indexed bitmaps of
 *   n_words words as for the list call (windows into column matrices allowed, stream_words may be a capacity, streams compress()
 *   never emits are legal).  The mask may be the output of a clause, list or range call enqueued before this one on the same
 *   stream and not yet checked.
 * Only positions p < n_rows are rows, n_rows <= 32 * n_words: a position at or behind n_rows is never selected and never carried,
 * whatever the mask or a column holds there, the pad bits of the last group included.  A row is selected where the mask bit is 1
 * (flags == 0) or where it is 0 (WAH_COMPACT_DELETE).  With T the number of selected rows, output bitmap c has n_words_out words;
 * its position k is column c's bit at the k-th selected row for k < T, and every position at or behind T is zero.  *d_out_rows
 * receives T.  The output is laid out exactly as wah_splice_indexed_device's: d_out receives the n_columns compress() streams
 * back to back, word for word, whatever form the sources had; d_out_offsets (required) receives n_columns * S_out + 1 entries
 * counted from d_out[0], S_out = ceil(G_out / 1024), G_out = wah_max_compressed_words(n_words_out); d_out_words receives the
 * total, also when it exceeds the capacity.
 *   wah_compact_max_words: an out_capacity_words that always suffices:
 *   min(n_columns * G_out, n_columns * (S_out + 1) + 2 * source_words), saturating at UINT64_MAX.  source_words is any upper bound
 *   the caller has on the words of the column segments that are read; the columns' whole streams are one.
 *   Why it holds: the surviving bits of a source word are consecutive in the output.  Those of a literal (at most 31) meet at most
 *   two output groups; those of a fill are one run, which leaves one fill word and at most one group where it ends inside an
 *   output group -- the group where it begins is the one where its predecessor ended, and is charged there (2 * source_words).
 *   Removing rows between two runs only merges them.  Every output segment cuts at most one run, and the zeros behind T are one
 *   more run (n_columns * (S_out + 1)).
 *   d_scratch: wah_compact_scratch_bytes(n_words, n_words_out, n_columns) bytes, 256-byte aligned, no initialisation:
 *   1024 (the control words) + round256(8 * R) (the running ranks: the selected rows in front of every source segment, then T)
 *   + L(E) + L(R), with R = S_src + 1, S_src = ceil(wah_max_compressed_words(n_words) / 1024), E = n_columns * S_out + 1 and
 *   L(x) = round256(8 * ceil(x / 4096)) + round256(8 * ceil(ceil(x / 4096) / 4096)) the two upper levels of a prefix sum over x
 *   entries (the one over the index runs in place in d_out_offsets, the one over the ranks in place in the scratch); round256
 *   rounds up to a multiple of 256.  A multiple of 256, never 0.
 * Mask and table are read only by the device: the call is asynchronous on `stream`, allocates nothing, reads nothing back and
 * never synchronises; it can be captured in a graph, and a replay after the mask's stream or the tables were overwritten in place
 * compacts the NEW selection.  The steps, none of which waits for another workgroup: a rank pass, one wavefront per mask segment,
 * that walks the segment into an image of 1024 groups in LDS and counts its selected rows (a mask segment that is one fill word
 * selecting nothing costs no image); the prefix sum of the counts; one wavefront per (column, output segment) that searches the
 * ranks for the source segments whose survivors lie in its 31 744 bits, walks the mask segment and the column segment into two
 * images, moves the column's bits under the mask together, 64 groups per step, and deposits them on the output's group grid in a
 * third image, whose words it counts; the prefix sum of the counts; the same wavefronts again, which now store the words, 64
 * consecutive ones at a time.  No decoded bitmap exists at any point; ranks, rows and offsets are 64-bit throughout.
 * The mask is read and checked in EVERY segment.  A column, as in the splice and fetch calls, is read and checked ONLY in the
 * source segments that hold a selected row: whether a broken column segment is refused depends on the mask.  After a refused
 * mask no column is read.
 * Errors the host can see come back before any HIP call, argument checks first: n_columns < 1 or > WAH_BITOP_LIST_MAX_OPERANDS,
 * n_words or n_words_out == 0 or >= 2^40, n_rows > 32 * n_words, unknown flag bits, n_columns * S_out >= 2^31, a null or misaligned
 * d_mask, d_operands, d_out_offsets, d_out_words, d_out_rows (8 B), d_out (4 B) or scratch (256 B): WAH_ERR_ARG; too small a
 * scratch: WAH_ERR_WORKSPACE.  Everything only the device sees is reported by wah_compact_status(), which synchronises the
 * stream: WAH_ERR_STREAM for T > 32 * n_words_out and for everything the list call refuses in an operand, in the mask and in the
 * column segments that are read; WAH_ERR_CAPACITY for too small an output (nothing is written at or behind
 * d_out[out_capacity_words]).  The output of a refused call is unspecified.  wah_compact_status(NULL, ...): WAH_ERR_ARG. */
#define WAH_COMPACT_DELETE 1u
uint64_t wah_compact_max_words(uint64_t n_words_out, uint64_t n_columns, uint64_t source_words);
size_t wah_compact_scratch_bytes(uint64_t n_words, uint64_t n_words_out, uint64_t n_columns);
int wah_compact_indexed_device(uint64_t n_words, uint64_t n_rows, uint32_t flags, const wah_bitop_operand *d_mask,
                               uint64_t n_columns, const wah_bitop_operand *d_operands, uint64_t n_words_out, uint32_t *d_out,
                               uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, uint64_t *d_out_rows,
                               void *d_scratch, size_t scratch_bytes, void *stream);
int wah_compact_status(void *d_scratch, void *stream);

/* The call that changes the VALUES of an index by a predicate: the rows a mask bitmap selects take a new value in every column,
 * all other rows keep theirs -- UPDATE t SET x = 5 WHERE ..., UPDATE t SET city = 'X' WHERE ..., the MERGE of a corrected batch
 * into the rows it corrects, CASE WHEN p THEN a ELSE b END.  The compact call moves the selected rows together; this one leaves
 * every row where it is.  Not in the reference.
 *   d_mask: ONE wah_bitop_operand in DEVICE memory, 8-byte aligned; d_else and d_then: n_columns of them each.  All are indexed
 *   bitmaps of n_words words as for the list call (windows into column matrices allowed, stream_words may be a capacity, streams
 *   compress() never emits are legal).  The mask may be the output of a clause, list, range or compare call enqueued before this
 *   one on the same stream and not yet checked.
 *   An entry of d_else or d_then whose d_stream AND d_offsets are both NULL is a CONSTANT: stream_words == 0 means every position
 *   is 0, stream_words == 1 means every position is 1; nothing is read for it.  The mask cannot be a constant.
 * For every column c and every position p < 32 * n_words: output c at p is then_c(p) where p < n_rows and the mask bit is 1, and
 * else_c(p) everywhere else, n_rows <= 32 * n_words.  What the mask holds at or behind n_rows selects nothing.  The pad bits of
 * the last group are zero in the output whatever the sources hold there.  Output bitmap c is, word for word, what compress()
 * emits for that bitmap, whatever form the sources had.  The output is laid out exactly as wah_compact_indexed_device's with
 * n_words_out == n_words: d_out receives the n_columns streams back to back; d_out_offsets (required) receives n_columns * S + 1
 * entries counted from d_out[0], S = ceil(G / 1024), G = wah_max_compressed_words(n_words); d_out_words receives the total, also
 * when it exceeds the capacity.  The output must not overlap an input (not checked): the result is a NEW index, as in the splice
 * and compact calls.
 *   wah_update_max_words: an out_capacity_words that always suffices:
 *   min(n_columns * G, source_words + n_columns * (mask_words + 3)), saturating at UINT64_MAX.  source_words is any upper bound the
 *   caller has on the words of all else and then entries that are no constants together, mask_words one on the mask's words; the
 *   whole streams are one.
 *   Why it holds: inside a segment an output word can begin only at a group where a word of the mask, of the else or of the then
 *   stream begins -- between two such groups all three streams are inside fills, the selection and both sources are constant from
 *   group to group, and so the output is one run.  Each source word is charged once (source_words), each mask word once per
 *   column (n_columns * mask_words).  A constant begins a word only at a segment's first group, which every stream shares: it is
 *   charged to the mask's word there.  Clipping the mask at n_rows makes the selection change inside one group and again at the
 *   next: two more groups where a word may begin; clearing the pad bits sets the last group apart: one more (n_columns * 3).
 *   d_scratch: wah_update_scratch_bytes(n_words, n_columns) bytes, 256-byte aligned, no initialisation: 1024 (the control words)
 *   + L(n_columns * S + 1), L as for the compact call: the two upper levels of the prefix sum over the index, which runs in place
 *   in d_out_offsets.  No ranks, no starts: the same as wah_from_positions_scratch_bytes(n_words, n_columns).  A multiple of 256,
 *   never 0.
 * Mask and tables are read only by the device: the call is asynchronous on `stream`, allocates nothing, reads nothing back and
 * never synchronises; it can be captured in a graph, and a replay after the mask's stream or either table was overwritten in
 * place applies the NEW update.  The steps, none of which waits for another workgroup: one wavefront per (segment, column) item,
 * the items shared out in contiguous runs and enumerated segment by segment, so that a wavefront walks a mask segment into its
 * image of 1024 groups in LDS once and keeps it across the columns (a mask segment that is one zero fill costs no image pass); per
 * column the else entry is walked into a second image, where the clipped mask selects a row of the segment the then entry into a
 * third, every lane blends its groups, (else & ~sel) | (then & sel), the pad bits are cleared and the image's words are counted;
 * the prefix sum of the counts; the same wavefronts again, which now store the words, 64 consecutive ones at a time.  No decoded
 * bitmap exists at any point.
 * The mask and every else entry that is no constant are read and checked in EVERY segment.  A then entry that is no constant is
 * read and checked ONLY in the segments where the mask, clipped at n_rows, selects a row: whether a broken then segment is
 * refused depends on the mask, as in the compact and fetch calls.  After a refused mask segment the item reads no column.
 * Errors the host can see come back before any HIP call, argument checks first: n_columns < 1 or > WAH_BITOP_LIST_MAX_OPERANDS,
 * n_words == 0 or >= 2^40, n_rows > 32 * n_words, n_columns * S >= 2^31, a null or misaligned scratch (256 B), d_mask, d_else,
 * d_then, d_out_offsets, d_out_words (8 B) or d_out (4 B): WAH_ERR_ARG; too small a scratch: WAH_ERR_WORKSPACE.  Everything only
 * the device sees is reported by wah_update_status(), which synchronises the stream: WAH_ERR_STREAM for everything the list call
 * refuses in an operand, in the segments that are read, for an entry with exactly one of d_stream and d_offsets NULL, for a
 * constant with stream_words > 1 and for a constant mask; WAH_ERR_CAPACITY for too small an output (nothing is written at or
 * behind d_out[out_capacity_words]).  The output of a refused call is unspecified.  wah_update_status(NULL, ...): WAH_ERR_ARG. */
uint64_t wah_update_max_words(uint64_t n_words, uint64_t n_columns, uint64_t mask_words, uint64_t source_words);
size_t wah_update_scratch_bytes(uint64_t n_words, uint64_t n_columns);
int wah_update_indexed_device(uint64_t n_words, uint64_t n_rows, const wah_bitop_operand *d_mask, uint64_t n_columns,
                              const wah_bitop_operand *d_else, const wah_bitop_operand *d_then, uint32_t *d_out,
                              uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets, void *d_scratch,
                              size_t scratch_bytes, void *stream);
int wah_update_status(void *d_scratch, void *stream);

/* The way into the BIT-SLICED index: a column of values in, the index of its slices out, in one call -- what
 * wah_bsi_range_indexed_device, wah_bsi_kth_indexed_device and wah_fetch_indexed_device read.  Not in the reference.
 *   d_values: n_rows unsigned 64-bit values below 2^n_bits, n_bits 1 .. 64 (a negative int64 is a value of 2^63 or more).
 *   d_exists: n_rows bytes in DEVICE memory, 0 = the row has no value (it is stored as value 0), anything else = it has one; NULL:
 *   every row has one, and there is no existence bitmap.  n_slices = n_bits + (d_exists ? 1 : 0).
 *   n_words: the words of ONE slice, a multiple of 992 with n_rows <= 32 * n_words; the rows behind n_rows are not loaded and count
 *   as value 0, not existing.  n_rows == 0 with a null d_values is allowed: all-zero slices.
 * The decoded slice matrix [n_slices, n_words] -- row i holds bit n_bits - 1 - i of every value, so row 0 is the MOST significant
 * bit, the existence bitmap is the last row; table row p is word p / 32, bit p % 32 (LSB first) of every matrix row -- is written
 * into the scratch and compressed there as ONE bitmap: d_out and d_out_offsets receive exactly what wah_compress_device_indexed
 * leaves for it, the slices' compress() streams back to back (slice 0 first) and n_slices * (n_words / 992) + 1 index entries, entry
 * i * (n_words / 992) + s the first word of segment s of slice i, the last one the total, which d_out_words receives too.  Every
 * indexed call takes the pair unchanged: a wah_bitop_operand with d_offsets = d_out_offsets + i * (n_words / 992) is slice i.
 * out_capacity_words = wah_max_compressed_words(n_slices * n_words) always suffices.
 *   d_scratch: wah_bsi_build_scratch_bytes(n_words, n_slices) bytes, 256-byte aligned, no initialisation:
 *       1024 + round256(4 * n_slices * n_words) + round256(wah_compress_workspace_bytes(n_slices * n_words))
 *   -- the control words, the slice matrix, the compress workspace (round256: up to a multiple of 256).
 * The values are read only by the device: the call is asynchronous on `stream`, allocates nothing and never synchronises, and a
 * captured graph replayed after d_values and d_exists were overwritten in place builds the NEW index.  Two steps.  The transpose,
 * in which no workgroup waits for another: a wavefront owns 2048 consecutive rows, reads each value once, 512 contiguous bytes per
 * load, and for every slice writes 64 words made of 32 ballots with one 256-byte store; every word of the matrix is written, so it
 * needs no clearing.  Then the one-launch compressor over the matrix (slices are mostly incompressible: 4 * n_slices * n_words
 * bytes written once and read once: n_bits / 8 bytes per row, never more than the values themselves).
 * Errors the host can see come back before any HIP call, argument checks first: n_bits outside 1 .. 64, n_words == 0 or not a
 * multiple of 992, n_slices * n_words >= 2^40, n_rows > 32 * n_words, a null d_values with n_rows > 0, a misaligned d_values (8 B),
 * a null or misaligned d_out (4 B), d_out_words, d_out_offsets (8 B) or scratch (256 B): WAH_ERR_ARG; too small a scratch:
 * WAH_ERR_WORKSPACE.  Everything only the device sees is reported by wah_bsi_build_status(), which synchronises the stream:
 * WAH_ERR_STREAM for a value at or above 2^n_bits -- EVERY row below n_rows is checked, whatever its existence byte says, so the
 * verdict does not depend on which rows exist --; WAH_ERR_CAPACITY for too small an output (nothing is written at or behind
 * d_out[out_capacity_words]).  The output of a refused call is unspecified.  wah_bsi_build_status(NULL, ...): WAH_ERR_ARG. */
size_t wah_bsi_build_scratch_bytes(uint64_t n_words, uint64_t n_slices);
int wah_bsi_build_device(uint64_t n_words, uint64_t n_bits, const uint64_t *d_values, uint64_t n_rows,
                         const uint8_t *d_exists /* NULL: every row exists */, uint32_t *d_out,
                         uint64_t out_capacity_words, uint64_t *d_out_words, uint64_t *d_out_offsets,
                         void *d_scratch, size_t scratch_bytes, void *stream);
int wah_bsi_build_status(void *d_scratch, uint64_t n_words, uint64_t n_slices, void *stream);

/* ------------------------------------------------------------------------- *
 * Benchmark support: synthetic bitmaps generated in HBM (include/wah_gen.h
 * states the bit-exact definition; replaces tests.cpp:42-64), and a plain
 * 16-byte-per-lane copy used as the on-box HBM ceiling.
 * ------------------------------------------------------------------------- */
int wah_gen_uniform_device(uint32_t *d_out, uint64_t n_words, uint64_t seed, uint64_t threshold, void *stream);
int wah_gen_clustered_device(uint32_t *d_out, uint64_t n_words, uint64_t seed, uint64_t threshold, void *stream);
int wah_copy_device(const uint32_t *d_in, uint32_t *d_out, uint64_t n_words, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *wah_last_error(void);

/* Library / build identification, e.g. "wah-mi355x 0.1 gfx950". */
const char *wah_version(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* WAH_H_ */
